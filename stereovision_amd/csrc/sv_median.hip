// sv_median.hip — the 5x5 median and the reference's post-processing (gfx950).
//
//  * k_median_i16  medianBlur(disparity, 5) on the int16 x16 map, fused with the
//                  reference's post-processing (depth_map.py:909-937 or
//                  fused_depth_map.py:1004-1029) so the filtered map never round-trips HBM;
//                  <1|2, *> carry Harris bands (sv_harris_wave.h) in extra blocks
//  * k_median_f32  medianBlur(f32, 5) for arbitrary float input (the public sv_median5_f32)
//  * k_post_m16    the post-processing alone on an int16 x16 median map
//  * k_post        the post-processing alone on an f32 disparity
//  * k_post_lut    the post-processing as a table of the int16 x16 median value
// All are HBM-bound stencils: LDS tiles with halos, one read and one write per pixel.
// Built with -ffp-contract=off so every f32 operation rounds exactly like NumPy's.
#include <type_traits>
#include "sv_harris_wave.h"
#include "sv_median_net.h"

namespace sv {
namespace {

// ---------------------------------------------------------------------------------------
// Post-processing of one f32 disparity value (shared by the median kernels and k_post).
struct PostVals { float a, b; uint8_t u; };

__device__ __forceinline__ PostVals post_vals(const PostParams& pp, float d) {
    PostVals o{0.0f, 0.0f, 0};
    if (pp.mode == POST_DEPTH) {
        // depth_map.py:925-936 — NumPy-2 keeps float32 throughout
        const float fxb = (float)(700 * 0.08);
        const float den = d + (float)1e-6;
        const float depth = fxb / den;
        float dc = depth < pp.minf ? pp.minf : depth;
        dc = dc > pp.maxf ? pp.maxf : dc;
        const bool valid = (d > pp.min_disp_global) && (dc >= pp.minf) && (dc <= pp.maxf);
        o.a = valid ? dc : 0.0f;
        float t = dc - pp.minf;
        t = t / pp.rangef;
        t = t * 255.0f;
        o.u = (uint8_t)(int)t;
    } else if (pp.mode == POST_SCALED) {
        // fused_depth_map.py:1010-1024
        const float lo = (float)pp.min_disp, hi = (float)(pp.min_disp + pp.num_disp - 1);
        float c = d < lo ? lo : d;
        c = c > hi ? hi : c;
        float t = c - lo;
        t = t / (float)pp.num_disp;
        t = t * 255.0f;
        o.u = (uint8_t)(int)t;
        o.a = (float)o.u;
        o.b = (d > (float)(pp.min_disp + 1) && d < hi) ? 1.0f : 0.0f;
    }
    return o;
}

// Element i of a frame-based array through a 32-bit byte offset from a uniform base, so
// loads and stores take the saddr + 32-bit voffset form (no 64-bit address arithmetic per
// access; launch_median_i16 bounds a frame to < 2^30 elements).
template <typename T>
__device__ __forceinline__ T& at(T* base, uint32_t i) {
    using B = typename std::conditional<std::is_const<T>::value, const char, char>::type;
    return *reinterpret_cast<T*>(reinterpret_cast<B*>(base) + (uint32_t)(i * (uint32_t)sizeof(T)));
}
// ... and through a 64-bit index, for arrays without that bound
template <typename T>
__device__ __forceinline__ T& at(T* base, size_t i) { return base[i]; }

// One pixel's post outputs to element i (uint32_t: the 32-bit offset form, size_t: plain).
template <typename I>
__device__ __forceinline__ void store_post(const PostParams& pp, I i, const PostVals& o) {
    at(pp.out_a, i) = o.a;
    at(pp.out_u8, i) = o.u;
    if (pp.mode == POST_SCALED) at(pp.out_b, i) = o.b;
}

// ... and its stores (k_post, k_post_lut).
__device__ __forceinline__ void post_one(const PostParams& pp, size_t i, float d) {
    if (pp.mode == POST_NONE) return;
    store_post(pp, i, post_vals(pp, d));
}

// Median-of-25 for the int16 map, 2 columns x 4 rows per lane.
// Two vertically adjacent 5x5 windows (rows y, y+1) share 20 of their 25 values (rows
// y-1..y+2): 5 columns of 4, each read by 5 horizontally adjacent windows, so every column
// is sorted once (5 comparators, in LDS).  Two horizontally adjacent windows (x, x+1) then
// share 4 of those sorted columns: the 13th of 25 has rank 3..12 among the common 16 (9
// values lie outside them), so SEL16H (41 comparators, 76 ops) takes the sorted ranks 3..12
// once per column pair and each window merges its own column in (MRG14: 20 comparators, 32
// ops) to the sorted ranks 4..9 of its 14 — the same 6 candidates C as SEL20S's ranks 7..12
// of 20 (59 comparators, 104 ops per window, the round-3 form).  Each window's unique row is
// sorted with its neighbour's (4 shared values sorted once, 1 inserted each), and the median
// is the 6th smallest of (6 sorted + 5 sorted) = min_i max(C_i, U_{4-i}) (10 ops).  Each
// lane packs two row pairs (rows y,y+1 | y+2,y+3) into short2 halves, so one
// v_pk_min/max_i16 serves both: ~34 network ops per output (46 for the SEL20S form, 113 for
// the plain 25-input network); round 4: 77 -> 68 us per 16 1080p frames.
typedef short s2 __attribute__((ext_vector_type(2)));
constexpr int MT_W = 64, MT_H = 8;        // k_median_f32 tile
constexpr int MQ_W = 128, MQ_H = 16;      // k_median_i16: 128 columns x 16 rows per block

__device__ __forceinline__ s2 as_s2(uint32_t u) { return __builtin_bit_cast(s2, u); }

// A comparator network of sv_median_net.h over v: each row (a, b[, use]) leaves min(v[a], v[b])
// in v[a] and the max in v[b]; a selection network's `use` bits say which of the two is still
// read (1: the min, 2: the max), a sorting network (two columns) keeps both.
__device__ __forceinline__ s2 net_min(s2 a, s2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ s2 net_max(s2 a, s2 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ float net_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float net_max(float a, float b) { return fmaxf(a, b); }
template <typename T, int N, int M>
__device__ __forceinline__ void apply_net(T* v, const unsigned char (&net)[N][M]) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int a = net[c][0], b = net[c][1], use = M == 3 ? net[c][M - 1] : 3;
        const T lo = net_min(v[a], v[b]), hi = net_max(v[a], v[b]);
        if (use & 1) v[a] = lo;
        if (use & 2) v[b] = hi;
    }
}

// The post-processing table's entry li (built by launch_post_lut).
__device__ __forceinline__ PostVals lut_entry(const PostParams& pp, uint32_t li) {
    PostVals o;
    o.a = at(pp.lut_a, li);
    o.u = at(pp.lut_u8, li);
    o.b = pp.mode == POST_SCALED ? at(pp.lut_b, li) : 0.0f;
    return o;
}
__device__ __forceinline__ PostVals post_median(const PostParams& pp, int mv) {
    const uint32_t dm = (uint32_t)(mv - pp.lut_m0);
    const uint32_t li = dm >> pp.lut_shift;
    // the whole-disparity table (lut_shift 4) holds multiples of 16 only: any other median (a
    // sub-pixel map passed through these entry points) takes the exact path below
    if (li < (uint32_t)pp.lut_n && (dm & ((1u << pp.lut_shift) - 1u)) == 0) return lut_entry(pp, li);   // (exact)
    return post_vals(pp, (float)mv / 16.0f);
}
// ... of a map whose values are all entries of the whole-disparity table (PostParams::
// lut_unchecked): no range or multiple test and no exact path beside the lookup.  The index
// keeps 12 bits (one v_bfe_u32 in the shift's place) and the host allocates the table for
// kLutWholeSpan entries, so a map that breaks the promise reads unset entries, never memory
// outside the table.
__device__ __forceinline__ PostVals post_median_whole(const PostParams& pp, int mv) {
    return lut_entry(pp, ((uint32_t)(mv - pp.lut_m0) >> 4) & (uint32_t)(kLutWholeSpan - 1));
}

// Post-processing of an int16 x16 median map (the value OpenCV's fixed-point disparity holds
// after medianBlur, depth_map.py:909-912) into create_depth_map's outputs (depth_map.py:
// 915-936) or the scaled app's (fused_depth_map.py:1010-1024): the median kernel's epilogue
// as a pass of its own, for maps that crossed xGMI as 2 B/px (multi-GPU gathers).  8 pixels
// per thread: one 16-B load, 2 x 16-B f32 stores per output, one 8-B u8 store; table lookup
// as in the median epilogue (bit-identical).  Algorithmic bytes: 2 in + 9 out (DEPTH).
__global__ __launch_bounds__(256) void k_post_m16(const int16_t* __restrict__ in, long long n,
                                                  float* __restrict__ disp, PostParams pp) {
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= n) return;
    const bool vec = i0 + 8 <= n && ((((uintptr_t)in) & 15) | (((uintptr_t)disp | (uintptr_t)pp.out_a |
                                                                  (uintptr_t)pp.out_b) & 15) |
                                     ((uintptr_t)pp.out_u8 & 7)) == 0;
    if (vec) {
        const uint4 raw = *reinterpret_cast<const uint4*>(in + i0);
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
        int mv[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            mv[2 * q] = (int)(int16_t)(w[q] & 0xFFFFu);
            mv[2 * q + 1] = (int)(int16_t)(w[q] >> 16);
        }
        if (disp) {
            float4* d = reinterpret_cast<float4*>(disp + i0);
            d[0] = make_float4((float)mv[0] / 16.0f, (float)mv[1] / 16.0f, (float)mv[2] / 16.0f, (float)mv[3] / 16.0f);
            d[1] = make_float4((float)mv[4] / 16.0f, (float)mv[5] / 16.0f, (float)mv[6] / 16.0f, (float)mv[7] / 16.0f);
        }
        if (pp.mode == POST_NONE) return;
        PostVals o[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) o[q] = post_median(pp, mv[q]);
        float4* a = reinterpret_cast<float4*>(pp.out_a + i0);
        a[0] = make_float4(o[0].a, o[1].a, o[2].a, o[3].a);
        a[1] = make_float4(o[4].a, o[5].a, o[6].a, o[7].a);
        uint32_t u[2] = {0u, 0u};
#pragma unroll
        for (int q = 0; q < 8; ++q) u[q >> 2] |= (uint32_t)o[q].u << (8 * (q & 3));
        *reinterpret_cast<uint2*>(pp.out_u8 + i0) = make_uint2(u[0], u[1]);
        if (pp.mode == POST_SCALED) {
            float4* b = reinterpret_cast<float4*>(pp.out_b + i0);
            b[0] = make_float4(o[0].b, o[1].b, o[2].b, o[3].b);
            b[1] = make_float4(o[4].b, o[5].b, o[6].b, o[7].b);
        }
        return;
    }
    for (long long i = i0; i < i0 + 8 && i < n; ++i) {
        const int mv = (int)in[i];
        if (disp) disp[i] = (float)mv / 16.0f;
        if (pp.mode == POST_NONE) continue;
        store_post(pp, (size_t)i, post_median(pp, mv));
    }
}

// HF: the Harris blocks this instance carries (0 none, 1 60-column waves, 2 248-column waves):
// the 248-column form needs 81 VGPRs, which would cost the plain median (36) its occupancy
// WH: the epilogue's table lookups are unchecked (PostParams::lut_unchecked)
template <int HF, bool WH>
__global__ __launch_bounds__(256) void k_median_i16(const int16_t* __restrict__ in, int H, int W,
                                                    int row0, int row1, float* __restrict__ disp,
                                                    PostParams pp, long long fs_in, long long fs_out,
                                                    HarrisParams hp) {
    // Harris blocks (hp.g != nullptr): blockIdx.x >= hp.mbx; each wave one DPP band of 60
    // columns x 16 rows of the frame's left image (harris_wave, the k_harris_dpp form), so
    // C2's Harris response rides in the median launch instead of a launch of its own
    if (HF != 0 && (int)blockIdx.x >= hp.mbx) {
        const int w = (int)(blockIdx.x - hp.mbx) * 4 + (int)(threadIdx.x >> 6);
        const int y0 = row0 + (int)blockIdx.y * MQ_H;
        if constexpr (HF == 2) {   // 248 columns per wave, one dword per lane-row (W >= 256)
            const int x0 = w * 248;
            if (x0 < W && y0 < row1)
                harris_wave4<MQ_H, 4>(hp.g + blockIdx.z * hp.fs_in, H, W, hp.pitch, hp.out + blockIdx.z * hp.fs_out,
                                      x0, y0, threadIdx.x & 63);
        } else {
            const int x0 = w * 60;
            if (x0 < W && y0 < row1)
                harris_wave<MQ_H, 4>(hp.g + blockIdx.z * hp.fs_in, H, W, hp.pitch, hp.out + blockIdx.z * hp.fs_out,
                                     x0, y0, threadIdx.x & 63);
        }
        return;
    }
    // t2[r][c] = (tile row r, tile row r+2) of column x0-2+c; tile row r = image row y0-2+r
    constexpr int TC = MQ_W + 4, TR = MQ_H + 2;
    __shared__ uint32_t t2[TR][TC];
    // srt[g][i][c]: rank i of column c over the shared pair rows 4g+1..4g+4 of t2
    __shared__ __attribute__((aligned(8))) uint32_t srt[MQ_H / 4][4][TC];
    if (blockIdx.z) {   // frame batch
        in += blockIdx.z * fs_in;
        const long long o = blockIdx.z * fs_out;
        if (disp) disp += o;   // nullable (an int16-only median pass): keep it null
        if (pp.out_a) pp.out_a += o;
        if (pp.out_u8) pp.out_u8 += o;
        if (pp.out_b) pp.out_b += o;
        if (pp.out_bgr) pp.out_bgr += 3 * o;
        if (pp.out_m16) pp.out_m16 += o;
        if (pp.out_d8) pp.out_d8 += o;
    }
    const int x0 = blockIdx.x * MQ_W, y0 = row0 + blockIdx.y * MQ_H;
    {   // thread -> tile column t % 128 (clamped once), rows t / 128, +2, ...; the 4 columns
        // past 128 (72 entries) go to the first 72 threads
        const int c = (int)(threadIdx.x & (MQ_W - 1)), g = (int)(threadIdx.x / MQ_W);
        constexpr int G = 256 / MQ_W;
        static_assert(TR % G == 0, "row groups must tile the pair rows");
        const uint32_t cx = (uint32_t)clampi(x0 - 2 + c, 0, W - 1);
        if (y0 >= 2 && y0 + TR - 1 <= H - 1) {   // interior rows (uniform): no row clamps
            uint32_t off = (uint32_t)(y0 - 2 + g) * W + cx;
            const uint32_t two = 2u * (uint32_t)W, step = (uint32_t)G * W;
#pragma unroll
            for (int k = 0; k < TR / G; ++k) {
                const uint16_t a = (uint16_t)at(in, off);
                const uint16_t b = (uint16_t)at(in, off + two);
                t2[g + G * k][c] = (uint32_t)a | ((uint32_t)b << 16);
                off += step;
            }
        } else {
#pragma unroll
            for (int k = 0; k < TR / G; ++k) {
                const int r = g + G * k;
                const uint16_t a = (uint16_t)at(in, (uint32_t)clampi(y0 - 2 + r, 0, H - 1) * W + cx);
                const uint16_t b = (uint16_t)at(in, (uint32_t)clampi(y0 + r, 0, H - 1) * W + cx);
                t2[r][c] = (uint32_t)a | ((uint32_t)b << 16);
            }
        }
        if (threadIdx.x < 4 * TR) {
            const int r = (int)(threadIdx.x >> 2), ce = MQ_W + (int)(threadIdx.x & 3);
            const uint32_t cxe = (uint32_t)clampi(x0 - 2 + ce, 0, W - 1);
            const uint16_t a = (uint16_t)at(in, (uint32_t)clampi(y0 - 2 + r, 0, H - 1) * W + cxe);
            const uint16_t b = (uint16_t)at(in, (uint32_t)clampi(y0 + r, 0, H - 1) * W + cxe);
            t2[r][ce] = (uint32_t)a | ((uint32_t)b << 16);
        }
    }
    __syncthreads();
    // every thread computes (the tile is clamped, so columns/rows past the edge read valid
    // data); only in-range pixels are written, after the LDS transpose below.  Thread (tb, tx)
    // owns output columns tx, tx+1 (tile columns tx .. tx+5) of rows tb .. tb+3.
    const int tx = 2 * (int)(threadIdx.x & 63), tb = 4 * (int)(threadIdx.x >> 6);
    {   // sort each column of the 4 shared pair rows once (5 comparators); the 5 windows
        // that read a column share the sort.  The 4 columns past 128 of each row group go to
        // the first 16 lanes of wave 0
        auto sort_col = [&](int g4, int c) {
            s2 w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = as_s2(t2[g4 + 1 + i][c]);
            apply_net(w, SV_SORT4_NET);
#pragma unroll
            for (int i = 0; i < 4; ++i) srt[g4 >> 2][i][c] = __builtin_bit_cast(uint32_t, w[i]);
        };
        sort_col(tb, tx);
        sort_col(tb, tx + 1);
        if (threadIdx.x < 16) sort_col(4 * (threadIdx.x >> 2), MQ_W + (threadIdx.x & 3));
    }
    __syncthreads();

    // the two windows share tile columns tx+1 .. tx+4: SEL16H once (their sorted ranks 3..12),
    // then each window merges its own column (MRG14) -> the 6 candidates C of SEL20S
    s2 cm[16], own[2][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint2 p0 = *reinterpret_cast<const uint2*>(&srt[tb >> 2][i][tx]);
        const uint2 p1 = *reinterpret_cast<const uint2*>(&srt[tb >> 2][i][tx + 2]);
        const uint2 p2 = *reinterpret_cast<const uint2*>(&srt[tb >> 2][i][tx + 4]);
        own[0][i] = as_s2(p0.x);
        cm[0 * 4 + i] = as_s2(p0.y);
        cm[1 * 4 + i] = as_s2(p1.x);
        cm[2 * 4 + i] = as_s2(p1.y);
        cm[3 * 4 + i] = as_s2(p2.x);
        own[1][i] = as_s2(p2.y);
    }
    apply_net(cm, SV_SEL16H_NET);
    s2 cw[2][6];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        s2 z[14];
#pragma unroll
        for (int k = 0; k < 10; ++k) z[k] = cm[SV_SEL16H_OUT[k]];
#pragma unroll
        for (int k = 0; k < 4; ++k) z[10 + k] = own[w][k];
        apply_net(z, SV_MRG14_NET);
#pragma unroll
        for (int k = 0; k < 6; ++k) cw[w][k] = z[SV_MRG14_OUT[k]];
    }
    // unique rows (tile rows tb, tb+5): the two windows share 4 of their 5 values, sorted once
    // (5 comparators), each inserts its own (4); median = 6th of (C: 6 sorted, U: 5 sorted)
    uint32_t mp[4];   // (column tx | column tx+1) of rows tb, tb+1, tb+2, tb+3
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        s2 q[6];
        {
            const uint2 p0 = *reinterpret_cast<const uint2*>(&t2[tb + 5 * h][tx]);
            const uint2 p1 = *reinterpret_cast<const uint2*>(&t2[tb + 5 * h][tx + 2]);
            const uint2 p2 = *reinterpret_cast<const uint2*>(&t2[tb + 5 * h][tx + 4]);
            q[0] = as_s2(p0.x); q[1] = as_s2(p0.y); q[2] = as_s2(p1.x);
            q[3] = as_s2(p1.y); q[4] = as_s2(p2.x); q[5] = as_s2(p2.y);
        }
        s2 sc[4] = {q[1], q[2], q[3], q[4]};
        apply_net(sc, SV_SORT4_NET);
        s2 m[2];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            s2 u[5] = {sc[0], sc[1], sc[2], sc[3], w ? q[5] : q[0]};
#pragma unroll
            for (int k = 3; k >= 0; --k) {   // insertion of u[4]
                const s2 lo = __builtin_elementwise_min(u[k], u[k + 1]);
                u[k + 1] = __builtin_elementwise_max(u[k], u[k + 1]);
                u[k] = lo;
            }
            s2 r = cw[w][5];
#pragma unroll
            for (int i = 0; i < 5; ++i) r = __builtin_elementwise_min(r, __builtin_elementwise_max(cw[w][i], u[4 - i]));
            m[w] = r;
        }
        // h = 0: (row tb, row tb+2), h = 1: (row tb+1, row tb+3); halves x = rows, w = columns
        const uint32_t a0 = __builtin_bit_cast(uint32_t, m[0]), a1 = __builtin_bit_cast(uint32_t, m[1]);
        mp[h] = (a0 & 0xFFFFu) | (a1 << 16);
        mp[h + 2] = (a0 >> 16) | (a1 & 0xFFFF0000u);
    }
    // park the medians in LDS, then re-read them as 4 consecutive columns of one row per
    // thread so the outputs leave as 16-byte (f32) and 4-byte (u8) stores.  med aliases srt
    // (every wave has read its ranks by the barrier): 17.9 KB of LDS, 8 blocks per CU
    static_assert(sizeof(srt) >= MQ_H * (MQ_W / 2) * sizeof(uint32_t), "med must fit in srt");
    auto med = reinterpret_cast<uint32_t (*)[MQ_W / 2]>(&srt[0][0][0]);
    __syncthreads();
    med[tb][tx >> 1] = mp[0];
    med[tb + 1][tx >> 1] = mp[1];
    med[tb + 2][tx >> 1] = mp[2];
    med[tb + 3][tx >> 1] = mp[3];
    __syncthreads();
    auto post = [&](int mv) { return WH ? post_median_whole(pp, mv) : post_median(pp, mv); };
    // the outputs allow 4-pixel stores (uniform; with W % 4 == 0 a thread's 4 columns are all
    // inside the row or all outside)
    const bool vec = (W & 3) == 0 &&
                     (((uintptr_t)disp | (uintptr_t)pp.out_a | (uintptr_t)pp.out_b) & 15) == 0 &&
                     (((uintptr_t)pp.out_u8 | (uintptr_t)pp.out_bgr | (uintptr_t)pp.out_d8) & 3) == 0 &&
                     ((uintptr_t)pp.out_m16 & 7) == 0;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int r = (int)(threadIdx.x >> 5) + 8 * pass, c4 = (int)(threadIdx.x & 31) * 4;
        const int y = y0 + r, x = x0 + c4;
        if (y >= row1 || x >= W) continue;
        const uint2 raw = *reinterpret_cast<const uint2*>(&med[r][c4 >> 1]);
        const int mv[4] = {(int)(int16_t)(raw.x & 0xFFFF), (int)(int16_t)(raw.x >> 16),
                           (int)(int16_t)(raw.y & 0xFFFF), (int)(int16_t)(raw.y >> 16)};
        const uint32_t i = (uint32_t)y * W + x;
        if (vec) {
            if (disp)
                at(reinterpret_cast<float4*>(disp), i >> 2) =
                    make_float4((float)mv[0] / 16.0f, (float)mv[1] / 16.0f, (float)mv[2] / 16.0f, (float)mv[3] / 16.0f);
            if (pp.out_m16) at(reinterpret_cast<uint2*>(pp.out_m16), i >> 2) = raw;
            if (pp.out_d8)
                at(reinterpret_cast<uint32_t*>(pp.out_d8), i >> 2) =
                    (uint32_t)(uint8_t)((mv[0] >> 4) - pp.d8_base) | ((uint32_t)(uint8_t)((mv[1] >> 4) - pp.d8_base) << 8) |
                    ((uint32_t)(uint8_t)((mv[2] >> 4) - pp.d8_base) << 16) |
                    ((uint32_t)(uint8_t)((mv[3] >> 4) - pp.d8_base) << 24);
            if (pp.mode == POST_NONE) continue;
            PostVals o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = post(mv[q]);
            at(reinterpret_cast<float4*>(pp.out_a), i >> 2) = make_float4(o[0].a, o[1].a, o[2].a, o[3].a);
            at(reinterpret_cast<uint32_t*>(pp.out_u8), i >> 2) =
                (uint32_t)o[0].u | ((uint32_t)o[1].u << 8) | ((uint32_t)o[2].u << 16) | ((uint32_t)o[3].u << 24);
            if (pp.mode == POST_SCALED)
                at(reinterpret_cast<float4*>(pp.out_b), i >> 2) = make_float4(o[0].b, o[1].b, o[2].b, o[3].b);
            if (pp.out_bgr) {   // 4 pixels = 12 bytes = 3 dwords (byte offset 3i, i % 4 == 0)
                const uint32_t c0 = pp.cmap[o[0].u], c1 = pp.cmap[o[1].u], c2 = pp.cmap[o[2].u],
                               c3 = pp.cmap[o[3].u];
                uint32_t* d = &at(reinterpret_cast<uint32_t*>(pp.out_bgr), 3 * (i >> 2));
                d[0] = c0 | (c1 << 24);
                d[1] = (c1 >> 8) | (c2 << 16);
                d[2] = (c2 >> 16) | (c3 << 8);
            }
            continue;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (x + q >= W) break;
            if (disp) at(disp, i + q) = (float)mv[q] / 16.0f;
            if (pp.out_m16) at(pp.out_m16, i + q) = (int16_t)mv[q];
            if (pp.out_d8) at(pp.out_d8, i + q) = (uint8_t)((mv[q] >> 4) - pp.d8_base);
            if (pp.mode == POST_NONE) continue;
            const PostVals o = post(mv[q]);
            store_post(pp, i + q, o);
            if (pp.out_bgr) {
                const uint32_t c = pp.cmap[o.u];
                uint8_t* d = &at(pp.out_bgr, 3 * (i + q));
                d[0] = (uint8_t)c;
                d[1] = (uint8_t)(c >> 8);
                d[2] = (uint8_t)(c >> 16);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_median_f32(const float* __restrict__ in, int H, int W,
                                                    float* __restrict__ out) {
    __shared__ float tile[MT_H + 4][MT_W + 4];
    const int x0 = blockIdx.x * MT_W, y0 = blockIdx.y * MT_H;
    for (int i = threadIdx.x; i < (MT_H + 4) * (MT_W + 4); i += 256) {
        const int ty = i / (MT_W + 4), tx = i % (MT_W + 4);
        tile[ty][tx] = in[(size_t)clampi(y0 - 2 + ty, 0, H - 1) * W + clampi(x0 - 2 + tx, 0, W - 1)];
    }
    __syncthreads();
    const int tx = threadIdx.x % MT_W, pr = threadIdx.x / MT_W;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float v[25];
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int i = 0; i < 5; ++i) v[j * 5 + i] = tile[2 * pr + h + j][tx + i];
        apply_net(v, SV_MED25_NET);
        const int x = x0 + tx, y = y0 + 2 * pr + h;
        if (x < W && y < H) out[(size_t)y * W + x] = v[SV_MED25_OUT];
    }
}

__global__ void k_post(const float* __restrict__ disp, int n, PostParams pp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) post_one(pp, (size_t)i, disp[i]);
}

__global__ void k_post_lut(PostParams pp, int m0, int n, int step) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) post_one(pp, (size_t)i, (float)(m0 + i * step) / 16.0f);
}

}  // namespace

int launch_median_i16(const int16_t* in, int H, int W, int row0, int row1, float* disp,
                      const PostParams& pp, hipStream_t s, int nf, long long fs_in, long long fs_out,
                      const HarrisParams* harris) {
    if (row1 <= row0 || nf <= 0) return 0;
    if ((long long)H * W >= (1LL << 30)) return (int)hipErrorInvalidValue;   // 32-bit offsets
    HarrisParams hp{};
    int hbx = 0;
    if (harris && harris->g) {   // Harris of rows [row0, row1): 4 waves of 60 (248) columns per block
        hp = *harris;
        // 248-column waves (k_harris_dpp4's form) from W >= 256: a quarter of the waves and one
        // dword load per lane-row where the band is interior (C2, 640x480 with 3 streams: 238k ->
        // 254-256k frames/s on one box).  SV_HARRIS_MED4=0 (A/B): 60-column waves everywhere
        static const bool med4 = env_flag("SV_HARRIS_MED4", true);
        hp.form = (med4 && W >= 256) ? 1 : 0;
        hbx = hp.form ? ((W + 247) / 248 + 3) / 4 : ((W + 59) / 60 + 3) / 4;
    }
    hp.mbx = (W + MQ_W - 1) / MQ_W;
    // unchecked lookups only with the whole-disparity table attached, and only if each of its
    // planes may be read for the kLutWholeSpan entries a 12-bit index can reach: anything else
    // takes the checked form
    const bool wh = pp.lut_unchecked && pp.mode != POST_NONE && pp.lut_shift == 4 && pp.lut_n > 0 &&
                    pp.lut_cap >= kLutWholeSpan;
    void (*fn)(const int16_t*, int, int, int, int, float*, PostParams, long long, long long, HarrisParams) =
        wh ? (hbx == 0 ? k_median_i16<0, true> : hp.form ? k_median_i16<2, true> : k_median_i16<1, true>)
           : (hbx == 0 ? k_median_i16<0, false> : hp.form ? k_median_i16<2, false> : k_median_i16<1, false>);
    hipLaunchKernelGGL(fn, dim3(hp.mbx + hbx, (row1 - row0 + MQ_H - 1) / MQ_H, nf),
                       dim3(256), 0, s, in, H, W, row0, row1, disp, pp, fs_in, fs_out, hp);
    return (int)hipGetLastError();
}

int launch_post_m16(const int16_t* in, long long n, float* disp, const PostParams& pp, hipStream_t s) {
    if (n <= 0) return 0;
    const long long blocks = (n + 8 * 256 - 1) / (8 * 256);
    if (blocks > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_post_m16, dim3((unsigned)blocks), dim3(256), 0, s, in, n, disp, pp);
    return (int)hipGetLastError();
}

int launch_median_f32(const float* in, int H, int W, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_median_f32, dim3((W + MT_W - 1) / MT_W, (H + MT_H - 1) / MT_H), dim3(256),
                       0, s, in, H, W, out);
    return (int)hipGetLastError();
}

int launch_post_lut(const PostParams& pp, int m0, int n, int step, float* lut_a, uint8_t* lut_u8,
                    float* lut_b, hipStream_t s) {
    if (n <= 0 || pp.mode == POST_NONE) return 0;
    PostParams q = pp;
    q.out_a = lut_a;
    q.out_u8 = lut_u8;
    q.out_b = lut_b;
    q.out_bgr = nullptr;
    q.out_m16 = nullptr;
    q.lut_n = 0;
    hipLaunchKernelGGL(k_post_lut, dim3((n + 255) / 256), dim3(256), 0, s, q, m0, n, step);
    return (int)hipGetLastError();
}

int launch_post(const float* disp, int n, const PostParams& pp, hipStream_t s) {
    if (n <= 0 || pp.mode == POST_NONE) return 0;
    hipLaunchKernelGGL(k_post, dim3((n + 255) / 256), dim3(256), 0, s, disp, n, pp);
    return (int)hipGetLastError();
}

}  // namespace sv
