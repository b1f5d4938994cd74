// sv_refine.hip — refinement of the winner-take-all maps: the column mirror
// around the right-referenced match (k_flip_rows) and the left-right check, curvature test
// and parabolic sub-pixel step in one pass per output tile (k_refine).  Semantics:
// tests/sv_refine_oracle.py.  gfx950 (wave64).
#include "sv_internal.h"

namespace sv {
namespace {

constexpr int kTW = 64, kTH = 4;   // output tile: one wave per row, 256 threads

template <class T>
__global__ __launch_bounds__(256) void k_flip_rows(const T* __restrict__ s0, const T* __restrict__ s1,
                                                   T* __restrict__ d0, T* __restrict__ d1, int W, int spitch,
                                                   int dpitch) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const T* s = blockIdx.z ? s1 : s0;
    T* d = blockIdx.z ? d1 : d0;
    d[(size_t)y * dpitch + x] = s[(size_t)y * spitch + (W - 1 - x)];
}

// Strip geometry of a tile at column x0: the L rows hold image columns x0 - r .. x0 + kTW - 1 + r,
// the R strip columns x0 - (minD + D) - r .. x0 + kTW - 1 - minD + 1 + r (every column a window
// at d - 1, d or d + 1 can touch for d in the sweep), both replicate-clamped while staging, over
// rows y0 - r .. y0 + kTH - 1 + r.  Static: no per-tile bounding box.
__host__ __device__ inline int strip_lw(int r) { return kTW + 2 * r; }
__host__ __device__ inline int strip_rw(int D, int r) { return kTW + D + 2 * r + 1; }

template <int COST>
__device__ __forceinline__ uint32_t tap(int l, int s) {
    const int df = l - s;
    return COST == COST_SSD ? (uint32_t)(df * df) : (uint32_t)(df < 0 ? -df : df);
}

// COSTS: the launch needs the window costs (min_curv > 0 or subpixel); LDS: staged form.
template <int COST, bool COSTS, bool LDS>
__global__ __launch_bounds__(256) void k_refine(RefineArgs a) {
    extern __shared__ uint8_t smem[];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int x = x0 + tx, y = y0 + ty;
    const int r = a.r, W = a.W, H = a.H;
    const int lw = strip_lw(r), rw = strip_rw(a.D, r), rows = kTH + 2 * r;
    const int rbase = x0 - (a.minD + a.D) - r;   // image column of the R strip's column 0
    uint8_t* sl = smem;
    uint8_t* sr = smem + rows * lw;
    if (COSTS && LDS) {
        for (int i = threadIdx.x; i < rows * lw; i += 256) {
            const int j = i / lw, k = i - j * lw;
            sl[i] = a.L[(size_t)clampi(y0 - r + j, 0, H - 1) * a.pitch + clampi(x0 - r + k, 0, W - 1)];
        }
        for (int i = threadIdx.x; i < rows * rw; i += 256) {
            const int j = i / rw, k = i - j * rw;
            sr[i] = a.R[(size_t)clampi(y0 - r + j, 0, H - 1) * a.pitch + clampi(rbase + k, 0, W - 1)];
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const int inv = (a.minD - 1) * 16;
    const size_t o = (size_t)y * a.mpitch + x;
    const int v = a.dl[o];
    const int d = v >> 4;
    if ((v & 15) != 0 || d < a.minD || d > a.minD + a.D - 1) {   // step 0
        a.out[o] = (int16_t)inv;
        return;
    }
    if (a.dr && a.lr_max_diff >= 0) {                             // step 1
        const int xr = x - d;
        if (xr >= 0 && xr < W) {
            const int vr = a.dr[(size_t)y * a.mpitch + xr];
            const int df = vr - 16 * d;
            if (vr != inv && (df < 0 ? -df : df) > 16 * a.lr_max_diff) {
                a.out[o] = (int16_t)inv;
                return;
            }
        }
    }
    int res = d * 16;
    if (COSTS) {                                                  // step 2
        uint32_t c0 = 0, cm = 0, cp = 0;
        const int rc0 = x - d - r - 1;   // image column of the window row's R strip: win + 2 bytes
        for (int j = 0; j <= 2 * r; ++j) {
            const uint8_t* lrow;
            const uint8_t* rrow;
            if (LDS) {
                lrow = sl + (ty + j) * lw + tx;
                rrow = sr + (ty + j) * rw + (rc0 - rbase);
            } else {
                const size_t yo = (size_t)clampi(y - r + j, 0, H - 1) * a.pitch;
                lrow = a.L + yo;
                rrow = a.R + yo;
            }
            auto lv = [&](int i) -> int { return LDS ? lrow[i] : lrow[clampi(x - r + i, 0, W - 1)]; };
            auto rv = [&](int k) -> int { return LDS ? rrow[k] : rrow[clampi(rc0 + k, 0, W - 1)]; };
            int s_lo = rv(0), s_mid = rv(1);   // R at d + 1 and d for the window's first column
            for (int i = 0; i <= 2 * r; ++i) {
                const int s_hi = rv(i + 2);    // R at d - 1
                const int l = lv(i);
                cp += tap<COST>(l, s_lo);
                c0 += tap<COST>(l, s_mid);
                cm += tap<COST>(l, s_hi);
                s_lo = s_mid;
                s_mid = s_hi;
            }
        }
        if (a.D == 1) cm = cp = c0;
        else if (d == a.minD) cm = cp;
        else if (d == a.minD + a.D - 1) cp = cm;
        // SSD: each cost <= 15^2 * 255^2 = 14.6M, so the sums below stay inside int32
        const int curv = (int)cm + (int)cp - 2 * (int)c0;         // step 3
        if (a.min_curv > 0 && curv < a.min_curv) {
            a.out[o] = (int16_t)inv;
            return;
        }
        if (a.subpixel) {                                         // step 4
            const int dcm = (int)cm - (int)cp;
            const int den = curv + (dcm < 0 ? -dcm : dcm);
            int q = 0;
            // (cm - cp) * 256 reaches 3.7e9 for SSD at win 15: the quotient alone is 64-bit
            if (c0 <= cm && c0 <= cp && den > 0) q = (int)(((long long)dcm * 256) / den);
            res = (d * 256 + q + 15) >> 4;
        }
    }
    a.out[o] = (int16_t)res;
}

template <int COST, bool COSTS>
int launch_form(const RefineArgs& a, bool lds, dim3 grid, size_t bytes, hipStream_t s) {
    if (lds) hipLaunchKernelGGL((k_refine<COST, COSTS, true>), grid, dim3(256), bytes, s, a);
    else hipLaunchKernelGGL((k_refine<COST, COSTS, false>), grid, dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace

size_t refine_lds_bytes(int num_disp, int win) {
    const int r = win / 2;
    return (size_t)(kTH + 2 * r) * (strip_lw(r) + strip_rw(num_disp, r));
}

int launch_refine(const RefineArgs& a, int cost, hipStream_t s) {
    const dim3 grid((a.W + kTW - 1) / kTW, (a.H + kTH - 1) / kTH);
    const bool costs = a.min_curv > 0 || a.subpixel;
    if (!costs) return launch_form<COST_SAD, false>(a, false, grid, 0, s);
    const int win = 2 * a.r + 1;
    const bool lds = refine_lds_form(a.D, win);
    const size_t bytes = refine_lds_bytes(a.D, win);
    if (cost == COST_SSD) return launch_form<COST_SSD, true>(a, lds, grid, bytes, s);
    return launch_form<COST_SAD, true>(a, lds, grid, bytes, s);
}

int launch_flip_u8(const uint8_t* s0, const uint8_t* s1, uint8_t* d0, uint8_t* d1, int H, int W, int spitch,
                   int dpitch, hipStream_t s) {
    hipLaunchKernelGGL((k_flip_rows<uint8_t>), dim3((W + 255) / 256, H, 2), dim3(256), 0, s, s0, s1, d0, d1, W, spitch,
                       dpitch);
    return (int)hipGetLastError();
}

int launch_flip_i16(const int16_t* src, int16_t* dst, int H, int W, int spitch, int dpitch, hipStream_t s) {
    hipLaunchKernelGGL((k_flip_rows<int16_t>), dim3((W + 255) / 256, H, 1), dim3(256), 0, s, src, src, dst, dst, W,
                       spitch, dpitch);
    return (int)hipGetLastError();
}

}  // namespace sv
