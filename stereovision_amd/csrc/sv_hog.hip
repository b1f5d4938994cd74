// sv_hog.hip — HOG window histograms: per-pixel 9-bin gradient orientation + the sums over
// the matching window (north_star), in two forms with identical outputs (gfx950):
//  * k_hog_hist_cr  column runs, 4 columns per lane (the default)
//  * k_hog_hist     64x16 tiles (records over 2 GB, SV_HOG_STRIP=0)
#include "sv_stencil.h"

namespace sv {
namespace {

// ---------------------------------------------------------------------------------------
// HOG window histograms: 64x16 output tile, window radius r <= 7.
constexpr int GT_W = 64, GT_H = 16, GR_MAX = 7;
constexpr int GX_MAX = GT_W + 2 * GR_MAX, GY_MAX = GT_H + 2 * GR_MAX;
// bin boundaries at 20°·(k+1): round(16384·cos), round(16384·sin); cos[7-k] = -cos[k] and
// sin[7-k] = sin[k], so the 8 tests need only 4 products pairs: boundary k is
// cos·gy >= sin·gx, boundary 7-k is -cos·gy >= sin·gx.
constexpr int kHogCos[4] = {15396, 12551, 8192, 2845};
constexpr int kHogSin[4] = {5604, 10531, 14189, 16135};

template <int r>   // window radius: compile-time, so the tile loops index by constants
__global__ __launch_bounds__(256) void k_hog_hist(const uint8_t* __restrict__ g, int H, int W,
                                                  int pitch, int row0, int row1,
                                                  uint16_t* __restrict__ hist) {
    __shared__ uint8_t simg[GY_MAX + 2][GX_MAX + 2];
    __shared__ uint16_t sbm[GY_MAX][GX_MAX];             // (bin << 8) | magnitude
    // window-sum records: bins 2k, 2k+1 as the u16 halves of dword k (dword 4's high half
    // is the zero pad bin 9).  Sums stay below 2^16 (<= 15*15*191 = 42,975: the magnitude
    // (|gx| + |gy|) >> 3 is at most 1530 >> 3), so packed adds and subtracts never carry or
    // borrow between halves.
    __shared__ uint32_t vrec[GT_H][GX_MAX][5];
    const int x0 = blockIdx.x * GT_W, y0 = row0 + blockIdx.y * GT_H;
    constexpr int nx = GT_W + 2 * r, ny = GT_H + 2 * r;
    // stage the image bytes once (all loads independent): rows y0-r-1 .. y0+GT_H+r and
    // columns x0-r-1 .. x0+GT_W+r, clamped; every pixel the gradients below read (the
    // replicate-clamped window positions and their reflect-101 neighbours) lies inside
    const int sy0 = y0 - r - 1, sx0 = x0 - r - 1;
    // rows below row1 + r feed only outputs at or past row1 (never stored): clamp the staging
    // there too, so a band-only input buffer (rows [row0 - r - 1, row1 + r] + SV_BAND_MARGIN)
    // is never read past its end when row1 - row0 is not a multiple of the tile height
    const int ylast = min(H - 1, row1 + r);
    for (int i = threadIdx.x; i < (ny + 2) * (nx + 2); i += 256) {
        const int ty = i / (nx + 2), tx = i - ty * (nx + 2);
        simg[ty][tx] = g[(size_t)clampi(sy0 + ty, 0, ylast) * pitch + clampi(sx0 + tx, 0, W - 1)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nx * ny; i += 256) {
        const int ty = i / nx, tx = i % nx;
        const int yy = clampi(y0 - r + ty, 0, H - 1);
        const int xx = clampi(x0 - r + tx, 0, W - 1);
        const int ym = refl101(yy - 1, H) - sy0, yc = yy - sy0, yp = refl101(yy + 1, H) - sy0;
        const int xm = refl101(xx - 1, W) - sx0, xc = xx - sx0, xp = refl101(xx + 1, W) - sx0;
        int gx, gy;
        sobel_tile(simg, ym, yc, yp, xm, xc, xp, gx, gy);
        const int m = (abs(gx) + abs(gy)) >> 3;
        if (gy < 0 || (gy == 0 && gx < 0)) { gx = -gx; gy = -gy; }
        int b = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int cy = kHogCos[k] * gy, sx = kHogSin[k] * gx;   // |products| < 2^24
            b += (cy >= sx) + (-cy >= sx);
        }
        sbm[ty][tx] = (uint16_t)((b << 8) | m);
    }
    __syncthreads();
    // vertical window sums: task = (column, half of the tile's rows), one packed record
    auto acc = [](uint32_t (&v)[5], uint32_t code, bool add) {
        const int k = (int)(code >> 9);                                  // bin / 2
        const uint32_t val = (code & 0xFFu) << ((code & 0x100u) ? 16 : 0);
#pragma unroll
        for (int kk = 0; kk < 5; ++kk) {
            const uint32_t t = kk == k ? val : 0u;
            v[kk] = add ? v[kk] + t : v[kk] - t;
        }
    };
    for (int task = threadIdx.x; task < nx * 2; task += 256) {
        const int tx = task >> 1, oy0 = (task & 1) * (GT_H / 2);
        uint32_t v[5] = {0u, 0u, 0u, 0u, 0u};
        for (int j = 0; j <= 2 * r; ++j) acc(v, sbm[oy0 + j][tx], true);
#pragma unroll
        for (int kk = 0; kk < 5; ++kk) vrec[oy0][tx][kk] = v[kk];
        for (int oy = oy0 + 1; oy < oy0 + GT_H / 2; ++oy) {
            acc(v, sbm[oy + 2 * r][tx], true);
            acc(v, sbm[oy - 1][tx], false);
#pragma unroll
            for (int kk = 0; kk < 5; ++kk) vrec[oy][tx][kk] = v[kk];
        }
    }
    __syncthreads();
    // horizontal window sums: task = (row, run of 4 columns): 256 running sums of 4 steps,
    // each thread storing its 4 records (80 contiguous bytes) straight to HBM
    {
        const int oy = threadIdx.x >> 4, c0 = (threadIdx.x & 15) * 4;
        const int y = y0 + oy, x = x0 + c0;
        uint32_t o[4][5];
        uint32_t v[5] = {0u, 0u, 0u, 0u, 0u};
        for (int i = 0; i <= 2 * r; ++i)
#pragma unroll
            for (int kk = 0; kk < 5; ++kk) v[kk] += vrec[oy][c0 + i][kk];
#pragma unroll
        for (int kk = 0; kk < 5; ++kk) o[0][kk] = v[kk];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
#pragma unroll
            for (int kk = 0; kk < 5; ++kk) {
                v[kk] += vrec[oy][c0 + q + 2 * r][kk] - vrec[oy][c0 + q - 1][kk];
                o[q][kk] = v[kk];
            }
        }
        if (y < row1 && x < W) {
            uint32_t* dst = reinterpret_cast<uint32_t*>(hist + ((size_t)y * W + x) * 10);
            if (x + 3 < W && ((uintptr_t)dst & 15) == 0) {
                const uint32_t* f = &o[0][0];
                uint4* d4 = reinterpret_cast<uint4*>(dst);
#pragma unroll
                for (int k = 0; k < 5; ++k) d4[k] = make_uint4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
            } else {
                for (int q = 0; q < 4 && x + q < W; ++q)
#pragma unroll
                    for (int kk = 0; kk < 5; ++kk) dst[q * 5 + kk] = o[q][kk];
            }
        }
    }
}

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------
// HOG window histograms, column-run form (round 5): lane L owns K = 4 CONSECUTIVE columns,
// so the horizontal window sum is a running sum inside the lane over the vertical sums of its
// K columns and of the r columns either side, which belong to the HL = ceil(r / K) neighbour
// lanes on each side (read from LDS) — instead of a 64-lane prefix scan per row; lanes
// HL .. 63-HL emit, the HL lanes at each end are the halo.  Per step (one image row) a lane
// loads the K + 2 bytes of the one new Sobel row, forms the K Sobel pairs as packed u16
// (S = a0 + 2a1 + a2, D = a2 - a0), the magnitudes packed, and each bin with 4 v_dot2 on the
// sign-normalised (gx, gy) pair (the 8 boundary tests of k_hog_hist folded into 4: below).
// Vertical window sums: 5 packed dwords per column in LDS, one ds_add / ds_sub per code; the
// last 2r+1 codes per column in a register ring of packed u16 (slot = step mod 2r+1 through
// s_set_gpr_idx, so the body is not unrolled 2r+1 times).  Records are staged in LDS and
// leave as coalesced 16-byte stores.  118 VGPRs and 9.9 KB of LDS at r = 7 (4 waves per
// SIMD); 4K r = 7, 4 images per launch: 205 us (round 4's 64-lane strips: 249).
// Bins: with (gx', gy') sign-normalised (gy' > 0, or gy' = 0 and gx' >= 0) and F_k =
// cos_k gy' - sin_k |gx'|, k_hog_hist's b = sum_k [cos_k gy' >= sin_k gx'] + [-cos_k gy' >=
// sin_k gx'] is 4 - #{F_k < 0} for gx' >= 0 and 8 - #{F_k > 0} for gx' < 0 (cos_k, sin_k > 0:
// one of each pair of tests is decided by the sign of gx'), i.e. base - #{G_k < 0} with G_k =
// dot2((gx', gx' < 0 ? -gy' : gy'), (-sin_k, cos_k)) — except for gx' = gy' = 0, where the
// magnitude is 0 and the bin never matters.
constexpr int HC_K = 4, HC_ROWS = 24;
template <int r, int K>
struct HogCr {
    static constexpr int HL = (r + K - 1) / K;        // halo lanes per side (a window reaches HL lanes)
    static constexpr int NOUT = (64 - 2 * HL) * K;     // columns a wave emits
    static constexpr int NP = K / 2 + 1;               // packed byte pairs per image row and lane
    static constexpr int NCH = (NOUT * 20 / 16 + 63) / 64;   // 16-byte chunks per lane and row
};

typedef short v2i16 __attribute__((ext_vector_type(2)));
typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2u16 as_u2(uint32_t v) { return __builtin_bit_cast(v2u16, v); }
__device__ __forceinline__ v2i16 as_i2(uint32_t v) { return __builtin_bit_cast(v2i16, v); }
__device__ __forceinline__ uint32_t u2_as(v2u16 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t i2_as(v2i16 v) { return __builtin_bit_cast(uint32_t, v); }

template <int r, int K>
__global__ __launch_bounds__(64) void k_hog_hist_cr(const uint8_t* __restrict__ g, int H, int W, int pitch,
                                                     int row0, int row1, uint16_t* __restrict__ hist, int hs_rows,
                                                     const uint8_t* __restrict__ g1, uint16_t* __restrict__ hist1,
                                                     long long fs_in, long long fs_hist) {
    using C = HogCr<r, K>;
    constexpr int HL = C::HL, NOUT = C::NOUT, NP = C::NP;
    if (blockIdx.z) {   // image pairs: z = 2 * frame + (0 left, 1 right)
        const int f = blockIdx.z >> 1;
        if (blockIdx.z & 1) {
            g = g1;
            hist = hist1;
        }
        g += f * fs_in;
        hist += f * fs_hist;
    }
    constexpr int W2 = 2 * r + 1;
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * NOUT;
    const int xs = x0 + (lane - HL) * K;   // this lane's first column (< 0 or >= W: halo / past the edge)
    const int ys = row0 + blockIdx.y * hs_rows;
    const int ye = min(ys + hs_rows, row1);
    const int nsteps = ye - ys + 2 * r;
    const auto gsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(g), 0, 0x7FFFFFFF, 0x00020000);
    const auto hdst = __builtin_amdgcn_make_buffer_rsrc(hist, 0, 0x7FFFFFFF, 0x00020000);

    // the K + 2 byte columns xs-1 .. xs+K: reflect-101 (the neighbours of columns 0 and W-1),
    // then clamped (columns past the edge read something valid; their codes are replaced below)
    int bcol[K + 2];
#pragma unroll
    for (int i = 0; i < K + 2; ++i) bcol[i] = clampi(refl101(xs - 1 + i, W), 0, W - 1);
    auto load_row = [&](int row, int (&b)[K + 2]) {
#pragma unroll
        for (int i = 0; i < K + 2; ++i) b[i] = (int)__builtin_amdgcn_raw_buffer_load_b8(gsrc, bcol[i], row * pitch, 0);
    };
    auto pack_row = [&](const int (&b)[K + 2], uint32_t (&p)[NP]) {
#pragma unroll
        for (int m = 0; m < NP; ++m) p[m] = (uint32_t)b[2 * m] | ((uint32_t)b[2 * m + 1] << 16);
    };
    auto crow = [&](int t) { return clampi(ys - r + t, 0, H - 1); };

    // vertical window sums, [bin pair][column j][lane] (conflict-free: lane-consecutive)
    __shared__ uint32_t vs[5 * K * 64];
#pragma unroll
    for (int i = 0; i < 5 * K; ++i) vs[i * 64 + lane] = 0u;

    uint32_t R0[NP], R1[NP], R2[NP];
    int nb[K + 2];
    {
        const int c = crow(0);
        load_row(refl101(c - 1, H), nb);
        pack_row(nb, R0);
        load_row(c, nb);
        pack_row(nb, R1);
        load_row(refl101(c + 1, H), nb);
        pack_row(nb, R2);
    }

    // the code ring: K/2 packed dwords (K u16 codes) per slot, slot = step mod 2r+1 (uniform:
    // s_set_gpr_idx-relative moves, no per-slot copy of the loop body)
    typedef uint32_t v16u __attribute__((ext_vector_type(16)));
    v16u ring[K / 2];
#pragma unroll
    for (int q = 0; q < K / 2; ++q) ring[q] = (v16u)(0u);   // code 0: adds nothing

    // a row's records (NOUT of them, contiguous in HBM) are staged in LDS and leave as 16-byte
    // chunks over all 64 lanes: the same NCH + 3 stores per row on every path (a chunk past the
    // row's end rewrites the last whole chunk's bytes, a tail dword past it the last dword's,
    // both with the same values), so the next step's wait for its prefetched row counts them
    // and never waits on them.  (Dropping such stores by an offset past num_records did not
    // work: the stores landed 2 GB past the buffer.)
    __shared__ __attribute__((aligned(16))) uint32_t stage[NOUT * 5];
    const int nbytes = 20 * min(NOUT, W - x0);   // >= 20
    const int last16 = (nbytes & ~15) - 16, tb = nbytes & ~15, owner = (tb >> 4) & 63;

    const bool first_wave = x0 == 0;
    const bool last_wave = x0 + (64 - HL) * K > W;   // some column of this wave is >= W
    const int jw = (W - 1 - x0) % K, lw = (W - 1 - x0) / K + HL;   // column W-1: lane lw, j jw
    uint32_t code[K];
    int cprev = -1;
    int slot = 0;
    uint32_t Rn[NP];   // the packed row the next advancing step brings in
    // one row of codes: Sobel, bins, the edge columns, the ring and the vertical sums
    auto step = [&](int t) {
        const int c = crow(t);
        if (c != cprev) {   // uniform: a new Sobel centre row (clamped rows repeat the codes)
            if (cprev >= 0) {
#pragma unroll
                for (int m = 0; m < NP; ++m) {
                    R0[m] = R1[m];
                    R1[m] = R2[m];
                    R2[m] = Rn[m];
                }
            }
            cprev = c;
            uint32_t S[NP], D[NP];
#pragma unroll
            for (int m = 0; m < NP; ++m) {
                S[m] = u2_as(as_u2(R0[m]) + (as_u2(R1[m]) << (unsigned short)1) + as_u2(R2[m]));
                D[m] = u2_as(as_u2(R2[m]) - as_u2(R0[m]));
            }
#pragma unroll
            for (int q = 0; q < K / 2; ++q) {
                const v2i16 gx = as_i2(u2_as(as_u2(S[q + 1]) - as_u2(S[q])));
                const uint32_t dmid = __builtin_amdgcn_alignbyte(D[q + 1], D[q], 2);   // (D[2q+1], D[2q+2])
                const v2i16 gy = as_i2(u2_as(as_u2(D[q]) + (as_u2(dmid) << (unsigned short)1) + as_u2(D[q + 1])));
                const v2i16 ax = __builtin_elementwise_max(gx, -gx), ay = __builtin_elementwise_max(gy, -gy);
                const uint32_t mm = u2_as((as_u2(i2_as(ax)) + as_u2(i2_as(ay))) >> (unsigned short)3);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    // p = (gy << 16) | gx, then sign-normalised: flip iff (gy, gx) < (0, 0)
                    const uint32_t p = __builtin_amdgcn_perm(i2_as(gy), i2_as(gx), h ? 0x07060302u : 0x05040100u);
                    const int vkey = (int)p - (int)((p & 0x8000u) << 1);   // gy * 65536 + gx
                    const uint32_t fm = (uint32_t)(vkey >> 31);
                    const uint32_t pn = u2_as(as_u2(p ^ fm) - as_u2(fm));
                    const uint32_t gm = (uint32_t)((int)(pn << 16) >> 31);    // gx' < 0
                    const uint32_t hm = gm & 0xFFFF0000u;
                    const v2i16 qv = as_i2(u2_as(as_u2(pn ^ hm) - as_u2(hm)));
                    uint32_t nneg = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const v2i16 w = {(short)-kHogSin[k], (short)kHogCos[k]};
                        nneg += (uint32_t)__builtin_amdgcn_sdot2(qv, w, 0, false) >> 31;
                    }
                    const uint32_t b = 4u + (gm & 4u) - nneg;
                    const uint32_t m = h ? mm >> 16 : mm & 0xFFFFu;
                    code[2 * q + h] = (b << 8) | m;
                }
            }
            // columns past the image edge take the edge column's code (clamped positions)
            if (first_wave) {
                const uint32_t c0 = __builtin_amdgcn_readlane(code[0], HL);
                if (lane < HL)
#pragma unroll
                    for (int j = 0; j < K; ++j) code[j] = c0;
            }
            if (last_wave) {
                uint32_t cw = code[0];
#pragma unroll
                for (int j = 1; j < K; ++j) cw = jw == j ? code[j] : cw;
                const uint32_t cwb = __builtin_amdgcn_readlane(cw, lw);
#pragma unroll
                for (int j = 0; j < K; ++j) code[j] = xs + j >= W ? cwb : code[j];
            }
        }
#pragma unroll
        for (int q = 0; q < K / 2; ++q) {
            const uint32_t nc = code[2 * q] | (code[2 * q + 1] << 16), oc = ring[q][slot];
            ring[q][slot] = nc;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = 2 * q + h;
                const uint32_t cn = code[j], co = h ? oc >> 16 : oc & 0xFFFFu;
                __hip_atomic_fetch_add(&vs[((cn >> 9) * K + j) * 64 + lane], (cn & 0xFFu) << ((cn >> 4) & 16u),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_sub(&vs[((co >> 9) * K + j) * 64 + lane], (co & 0xFFu) << ((co >> 4) & 16u),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
        }
        slot = slot + 1 == W2 ? 0 : slot + 1;
    };
    // each iteration loads the row step t + 1 brings in if it advances (unconditionally, at its
    // top) and packs it at its end, after the stores: no loaded register lives across the
    // back edge (a copy there would wait for the load), and the wait counts the stores
    auto prefetch = [&](int t) { load_row(refl101(crow(min(t + 1, nsteps - 1)) + 1, H), nb); };
    for (int t = 0; t < 2 * r && t < nsteps; ++t) {   // warm-up: the vertical window only
        prefetch(t);
        step(t);
        pack_row(nb, Rn);
    }
    const bool own = lane >= HL && lane < 64 - HL;
    uint32_t* srec = &stage[(own ? lane - HL : 0) * 5 * K];
    for (int t = 2 * r; t < nsteps; ++t) {
        prefetch(t);
        step(t);
        // the neighbour lanes' vertical sums of this step, just updated by their wavefront-scope
        // atomics, are read below: an acquire-release fence at wavefront scope orders the two
        // for the compiler (no instruction on gfx950: a wave's LDS ops complete in order); the
        // next step's atomics come after the barriers below
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // horizontal window: a running sum over columns -r .. K-1+r, the outer ones the
        // neighbour lanes' vertical sums (read from LDS; LDS ops of a wave complete in order);
        // each plane's K sums go straight to the row's staging area
#pragma unroll
        for (int p = 0; p < 5; ++p) {
            uint32_t v[K + 2 * r];
#pragma unroll
            for (int i = 0; i < K + 2 * r; ++i) {
                const int col = i - r;
                const int dl = col >= 0 ? col / K : -((K - 1 - col) / K);   // source lane offset
                const int sl = min(max(lane + dl, 0), 63);
                v[i] = vs[(p * K + (col - dl * K)) * 64 + sl];
            }
            uint32_t h = v[0];
#pragma unroll
            for (int i = 1; i <= 2 * r; ++i) h += v[i];
            if (own) srec[p] = h;
#pragma unroll
            for (int j = 1; j < K; ++j) {
                h += v[j + 2 * r] - v[j - 1];
                if (own) srec[5 * j + p] = h;
            }
        }
        __syncthreads();   // (one wave: orders the staging, fences the compiler)
        const int soff = ((ys + t - 2 * r) * W + x0) * 20;
#pragma unroll
        for (int k = 0; k < C::NCH; ++k) {
            int b0 = 16 * (lane + 64 * k);
            b0 = b0 + 16 <= nbytes ? b0 : last16;
            const v4u q = *reinterpret_cast<const v4u*>(&stage[b0 >> 2]);
            __builtin_amdgcn_raw_buffer_store_b128(q, hdst, b0, soff, 0);
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {   // the tail chunk (nbytes is a multiple of 4, not always of 16)
            int o = tb + 4 * d;
            o = lane == owner && o < nbytes ? o : nbytes - 4;
            __builtin_amdgcn_raw_buffer_store_b32(stage[o >> 2], hdst, o, soff, 0);
        }
        pack_row(nb, Rn);
        __syncthreads();
    }
}

// Whether the column-run kernel serves an H x W image: SV_HOG_STRIP=0 (A/B) turns it off, and
// it addresses through 32-bit buffer offsets (stores below 0x7FFFFFF0).
bool hog_strips_ok(int H, int W, int pitch) {
    static const bool strip = env_flag("SV_HOG_STRIP", true);
    return strip && (long long)H * W * 20 < (1LL << 31) - (1LL << 20) && (long long)H * pitch < (1LL << 31);
}

// The column-run kernel over nz images (nz = 1: g0 / h0; else z = 2 * frame + side).
// SV_HOG_CR_ROWS: rows per strip wave (A/B; 24 by default: 4K, 4 images per launch, 16 / 24 /
// 32 / 48 rows measured 1,552 / 1,572 / 1,564 / 1,558 C5 HOG frames/s).
int launch_hog_strips(const uint8_t* g0, const uint8_t* g1, int H, int W, int pitch, int r, int row0,
                      int row1, uint16_t* h0, uint16_t* h1, int nz, long long fs_in, long long fs_hist,
                      hipStream_t s) {
    static const int hc_rows = [] {
        const int x = env_int("SV_HOG_CR_ROWS", 4, 4096);
        return x ? x : HC_ROWS;
    }();
    switch (r) {
#define SV_HOG_C(R)                                                                                              \
    case R: {                                                                                                   \
        constexpr int NOUT = HogCr<R, HC_K>::NOUT;                                                              \
        const dim3 grid((W + NOUT - 1) / NOUT, (row1 - row0 + hc_rows - 1) / hc_rows, nz);                      \
        hipLaunchKernelGGL((k_hog_hist_cr<R, HC_K>), grid, dim3(64), 0, s, g0, H, W, pitch, row0, row1, h0,     \
                           hc_rows, g1, h1, fs_in, fs_hist);                                                    \
    } break;
        SV_HOG_C(0) SV_HOG_C(1) SV_HOG_C(2) SV_HOG_C(3) SV_HOG_C(4) SV_HOG_C(5) SV_HOG_C(6) SV_HOG_C(7)
#undef SV_HOG_C
    }
    return (int)hipGetLastError();
}

}  // namespace

int launch_hog_hist(const uint8_t* g, int H, int W, int pitch, int win, int row0, int row1,
                    uint16_t* hist, hipStream_t s) {
    const int r = win / 2;
    if (r > GR_MAX) return (int)hipErrorInvalidValue;
    if (row0 < 0) row0 = 0;
    if (row1 > H) row1 = H;
    if (row1 <= row0) return 0;
    if (hog_strips_ok(H, W, pitch)) return launch_hog_strips(g, g, H, W, pitch, r, row0, row1, hist, hist, 1, 0, 0, s);
    const dim3 grid((W + GT_W - 1) / GT_W, (row1 - row0 + GT_H - 1) / GT_H);
    switch (r) {
#define SV_HOG_R(R) case R: hipLaunchKernelGGL(k_hog_hist<R>, grid, dim3(256), 0, s, g, H, W, pitch, row0, row1, hist); break;
        SV_HOG_R(0) SV_HOG_R(1) SV_HOG_R(2) SV_HOG_R(3) SV_HOG_R(4) SV_HOG_R(5) SV_HOG_R(6) SV_HOG_R(7)
#undef SV_HOG_R
    }
    return (int)hipGetLastError();
}

int launch_hog_hist_pairs(const uint8_t* g0, const uint8_t* g1, int H, int W, int pitch, int win, int row0,
                          int row1, uint16_t* h0, uint16_t* h1, int nf, long long fs_in, long long fs_hist,
                          hipStream_t s) {
    const int r = win / 2;
    if (r > GR_MAX || nf <= 0) return (int)hipErrorInvalidValue;
    if (row0 < 0) row0 = 0;
    if (row1 > H) row1 = H;
    if (row1 <= row0) return 0;
    if (!hog_strips_ok(H, W, pitch)) {
        for (int z = 0; z < nf; ++z) {   // the tile kernel: image by image
            int e = launch_hog_hist(g0 + z * fs_in, H, W, pitch, win, row0, row1, h0 + z * fs_hist, s);
            if (!e) e = launch_hog_hist(g1 + z * fs_in, H, W, pitch, win, row0, row1, h1 + z * fs_hist, s);
            if (e) return e;
        }
        return 0;
    }
    return launch_hog_strips(g0, g1, H, W, pitch, r, row0, row1, h0, h1, 2 * nf, fs_in, fs_hist, s);
}

}  // namespace sv
