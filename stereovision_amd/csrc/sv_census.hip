// sv_census.hip — the census / Hamming matching cost:
//  * k_census        the 9 x 7 census transform: one 62-bit code per pixel, both images of every
//                    frame pair in one launch (grid.z)
//  * k_census_match  the fused winner-take-all matcher over two code planes: Hamming distances,
//                    the win x win box sum and the first argmin, no cost volume in HBM
#include "sv_internal.h"

namespace sv {
namespace {

// ---------------------------------------------------------------------------------------
// Census transform.  Bit k of C(x, y), k = 0..61 over dy = -3..3 (outer), dx = -4..4 (inner)
// without (0, 0), is Ip(x + dx, y + dy) < I(x, y) on the replicate-clamped image.
constexpr int CN_RX = 4, CN_RY = 3;
constexpr int CT_W = 64, CT_H = 16;   // output tile of a 256-thread block
constexpr int CT_LW = CT_W + 2 * CN_RX, CT_LH = CT_H + 2 * CN_RY;

__global__ __launch_bounds__(256) void k_census(CensusArgs a) {
    __shared__ uint8_t tile[CT_LH][CT_LW];
    const int z = blockIdx.z;   // image pairs: z = 2 * frame + (0 left, 1 right)
    const uint8_t* g = ((z & 1) ? a.g1 : a.g0) + (long long)(z >> 1) * a.fs_in;
    uint64_t* out = ((z & 1) ? a.c1 : a.c0) + (long long)(z >> 1) * a.fs_codes;
    const int x0 = blockIdx.x * CT_W, y0 = a.y0 + blockIdx.y * CT_H;
    // rows: the frame's clamp for every code row written; tile rows past y1 feed no stored code
    // and are clamped to the last row a stored code reads, so a band-only input buffer is never
    // read beyond [y0 - 3, y1 + 3) of the launch
    const int rlo = max(0, a.y0 - CN_RY), rhi = min(a.H - 1, a.y1 - 1 + CN_RY);
    for (int i = threadIdx.x; i < CT_LH * CT_LW; i += 256) {
        const int ty = i / CT_LW, tx = i - ty * CT_LW;
        tile[ty][tx] = g[(size_t)clampi(y0 - CN_RY + ty, rlo, rhi) * a.pitch + clampi(x0 - CN_RX + tx, 0, a.W - 1)];
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, x = x0 + tx;
    for (int ty = threadIdx.x >> 6; ty < CT_H; ty += 4) {
        const int y = y0 + ty;
        const uint32_t c = tile[ty + CN_RY][tx + CN_RX];
        uint32_t lo = 0u, hi = 0u;
#pragma unroll
        for (int dy = 0; dy <= 2 * CN_RY; ++dy) {
#pragma unroll
            for (int dx = 0; dx <= 2 * CN_RX; ++dx) {
                if (dy == CN_RY && dx == CN_RX) continue;
                const int k = dy * (2 * CN_RX + 1) + dx - (dy > CN_RY || (dy == CN_RY && dx > CN_RX) ? 1 : 0);
                const uint32_t bit = (uint32_t)tile[ty + dy][tx + dx] < c ? 1u : 0u;
                if (k < 32) lo |= bit << k;
                else hi |= bit << (k - 32);
            }
        }
        if (x < a.W && y < a.y1)   // one 8-byte vector store per code (little-endian: lo first)
            *reinterpret_cast<uint2*>(out + (size_t)y * a.cpitch + x) = make_uint2(lo, hi);
    }
}

// ---------------------------------------------------------------------------------------
// Fused Hamming matcher.  A block owns NOUT = 64 - 2r output columns and a strip of up to CM_RS
// rows; lane l of every wave is column x0 - r + l (r halo lanes per side).  The disparities are
// cut into chunks of CM_DC; the block's waves take chunks in turn.  For one chunk a wave marches
// down the strip: the lane keeps the CM_DC vertical sums (over the window's rows) of its column's
// Hamming distances in registers, adds the entering row's distances and removes the leaving
// row's (recomputed), then the horizontal window sum runs across lanes through LDS as packed
// u16 (four disparities per 8-byte slot, lane-consecutive slots: conflict-free ds_read_b64) and
// the lane's best (cost << 9 | index) key goes into the strip's key plane with an LDS minimum.
// Bounds: a distance <= 64, a vertical sum <= 64 * 15 = 960, a window cost <= 14400 < 2^14, so
// the packed halves never carry and a key fits 23 bits.  Smaller index wins a tie: first argmin.
constexpr int CM_DC = 16;                  // disparities per chunk
constexpr int CM_RS = 32;                  // most rows of a strip
constexpr int CM_NW = 4;                   // most waves of a block
constexpr int CM_STRIP = 64 + CM_DC;       // right codes a row of a chunk reaches: 64 + CM_DC - 1
constexpr int CM_HS = 64 + 2 * 7 + 2;      // the exchange row: 64 lanes + the widest halo
constexpr int CM_DBITS = 9;
constexpr uint32_t CM_NOKEY = 0xFFFFFFFFu;

struct CmWave {
    uint2 sE[CM_STRIP];            // right codes of the entering row, [0] at column `base`
    uint2 sL[CM_STRIP];            // ... of the leaving row
    uint2 hs[CM_DC / 4][CM_HS];    // packed vertical sums: lane l's at [r + l]
};

// Orders a wave's LDS stores before its later LDS loads of other lanes' slots (and loads before
// later stores) for the compiler; the hardware completes one wave's LDS operations in order
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t hamming_acc(uint2 p, uint2 q, uint32_t acc) {
    acc += (uint32_t)__builtin_popcount(p.x ^ q.x);   // v_xor + accumulating v_bcnt_u32_b32
    acc += (uint32_t)__builtin_popcount(p.y ^ q.y);
    return acc;
}

template <int R>
__global__ __launch_bounds__(64 * CM_NW) void k_census_match(CensusMatchArgs a, int rs) {
    constexpr int NOUT = 64 - 2 * R, W2 = 2 * R + 1;
    __shared__ uint32_t skey[CM_RS][64];
    __shared__ CmWave swave[CM_NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const uint64_t* CL = a.CL + (long long)blockIdx.z * a.fs_codes;
    const uint64_t* CR = a.CR + (long long)blockIdx.z * a.fs_codes;
    int16_t* out = a.out + (long long)blockIdx.z * a.fs_out;
    const int x0 = blockIdx.x * NOUT;
    const int ys = a.row0 + blockIdx.y * rs;
    const int nrows = min(ys + rs, a.row1) - ys;
    // (uniform) some column of the block lies in the matched band: else only the invalid value
    const bool banded = a.X1 > a.X0 && x0 < a.X1 && x0 + NOUT > a.X0;
    if (banded) {
        for (int i = threadIdx.x; i < nrows * 64; i += blockDim.x) (&skey[0][0])[i] = CM_NOKEY;
        __syncthreads();
        CmWave& w = swave[wave];
        const int xl = x0 - R + lane;
        const int xlc = clampi(xl, 0, a.W - 1);
        const int nsteps = nrows + 2 * R;
        const int nch = (a.D + CM_DC - 1) / CM_DC;
        // step t brings in row ys - R + t and, past the warm-up, drops the row W2 steps before
        auto row_e = [&](int t) { return clampi(ys - R + t, 0, a.H - 1); };
        auto row_l = [&](int t) { return clampi(ys - R + max(t - W2, 0), 0, a.H - 1); };
        for (int c = wave; c < nch; c += nw) {
            const int c0 = c * CM_DC;
            // strip slot i holds the right code at column base + i (clamped): lane l and the
            // chunk's disparity k read slot l + CM_DC - 1 - k = column xl - (minD + c0 + k)
            const int base = x0 - R - a.minD - c0 - (CM_DC - 1);
            const int col0 = clampi(base + lane, 0, a.W - 1), col1 = clampi(base + 64 + lane, 0, a.W - 1);
            uint32_t v[CM_DC];
#pragma unroll
            for (int k = 0; k < CM_DC; ++k) v[k] = 0u;
            uint2 nle, nll, nre0, nre1 = make_uint2(0u, 0u), nrl0, nrl1 = make_uint2(0u, 0u);
            auto load = [&](int t) {   // the codes step t needs, into registers
                const uint2* le = reinterpret_cast<const uint2*>(CL + (size_t)row_e(t) * a.cpitch);
                const uint2* ll = reinterpret_cast<const uint2*>(CL + (size_t)row_l(t) * a.cpitch);
                const uint2* re = reinterpret_cast<const uint2*>(CR + (size_t)row_e(t) * a.cpitch);
                const uint2* rl = reinterpret_cast<const uint2*>(CR + (size_t)row_l(t) * a.cpitch);
                nle = le[xlc];
                nll = ll[xlc];
                nre0 = re[col0];
                nrl0 = rl[col0];
                if (lane < CM_DC) {
                    nre1 = re[col1];
                    nrl1 = rl[col1];
                }
            };
            load(0);
            for (int t = 0; t < nsteps; ++t) {
                const uint2 le = nle, ll = nll;
                w.sE[lane] = nre0;
                w.sL[lane] = nrl0;
                if (lane < CM_DC) {
                    w.sE[64 + lane] = nre1;
                    w.sL[64 + lane] = nrl1;
                }
                wave_lds_fence();
                load(min(t + 1, nsteps - 1));   // the next step's codes arrive behind this step's work
#pragma unroll
                for (int k = 0; k < CM_DC; ++k) v[k] = hamming_acc(le, w.sE[lane + CM_DC - 1 - k], v[k]);
                if (t >= W2) {
#pragma unroll
                    for (int k = 0; k < CM_DC; ++k) v[k] -= hamming_acc(ll, w.sL[lane + CM_DC - 1 - k], 0u);
                }
                if (t >= 2 * R) {
#pragma unroll
                    for (int p = 0; p < CM_DC / 4; ++p)
                        w.hs[p][R + lane] = make_uint2(v[4 * p] | (v[4 * p + 1] << 16), v[4 * p + 2] | (v[4 * p + 3] << 16));
                    wave_lds_fence();
                    uint32_t best = CM_NOKEY;
#pragma unroll
                    for (int p = 0; p < CM_DC / 4; ++p) {
                        uint32_t s0 = 0u, s1 = 0u;   // (halo lanes sum slots nobody wrote: never emitted)
#pragma unroll
                        for (int i = 0; i < W2; ++i) {
                            const uint2 q = w.hs[p][lane + i];
                            s0 += q.x;
                            s1 += q.y;
                        }
                        const uint32_t cost[4] = {s0 & 0xFFFFu, s0 >> 16, s1 & 0xFFFFu, s1 >> 16};
#pragma unroll
                        for (int h = 0; h < 4; ++h) {
                            const int idx = c0 + 4 * p + h;
                            if (idx < a.D) best = min(best, (cost[h] << CM_DBITS) | (uint32_t)idx);
                        }
                    }
                    __hip_atomic_fetch_min(&skey[t - 2 * R][lane], best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                wave_lds_fence();
            }
        }
        __syncthreads();
    }
    const int16_t inv = (int16_t)((a.minD - 1) * 16);
    for (int i = threadIdx.x; i < nrows * 64; i += blockDim.x) {
        const int row = i >> 6, l = i & 63, x = x0 - R + l;
        if (l < R || l >= 64 - R || x >= a.W) continue;
        int16_t val = inv;
        if (x >= a.X0 && x < a.X1) val = (int16_t)((a.minD + (int)(skey[row][l] & ((1u << CM_DBITS) - 1u))) * 16);
        out[(size_t)(ys + row) * a.opitch + x] = val;
    }
}

}  // namespace

int launch_census(const CensusArgs& a, hipStream_t s) {
    if (a.nz <= 0 || a.y1 <= a.y0) return 0;
    const dim3 grid((a.W + CT_W - 1) / CT_W, (a.y1 - a.y0 + CT_H - 1) / CT_H, a.nz);
    hipLaunchKernelGGL(k_census, grid, dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_census_match(const CensusMatchArgs& a, hipStream_t s) {
    if (a.r < 0 || a.r > 7 || a.D < 1 || a.D > (1 << CM_DBITS)) return (int)hipErrorInvalidValue;
    if (a.row1 <= a.row0 || a.nf <= 0) return 0;
    const int nout = 64 - 2 * a.r, gx = (a.W + nout - 1) / nout, rows = a.row1 - a.row0;
    // shorter strips for small launches (more blocks; each strip pays 2r warm-up rows per chunk)
    int rs = CM_RS;
    while (rs > 8 && (long long)gx * ((rows + rs - 1) / rs) * a.nf < 1024) rs >>= 1;
    const int nch = (a.D + CM_DC - 1) / CM_DC;
    const dim3 grid(gx, (rows + rs - 1) / rs, a.nf), block(64 * std::min(nch, CM_NW));
    switch (a.r) {
#define SV_CM_R(R) case R: hipLaunchKernelGGL(k_census_match<R>, grid, block, 0, s, a, rs); break;
        SV_CM_R(0) SV_CM_R(1) SV_CM_R(2) SV_CM_R(3) SV_CM_R(4) SV_CM_R(5) SV_CM_R(6) SV_CM_R(7)
#undef SV_CM_R
    }
    return (int)hipGetLastError();
}

}  // namespace sv
