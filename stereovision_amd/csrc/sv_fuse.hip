// sv_fuse.hip — the fusion step of the reference's loop (fused_depth_map.py:1560-1718) and
// the two float32 image filters it is built on, for gfx950.
//
//  * k_fuse_blend     stereo base, MiDaS fill (Gaussian-blurred fill weight) and flow fill of
//                     fuse_depth_maps (:1603-1684) in one launch, with the range of the blended
//                     map and the two fill counts folded per block
//  * k_gauss_f32      cv2.GaussianBlur(x, (k, k), 0) on a float32 map (:1638), stand-alone
//  * k_bilateral_f32  cv2.bilateralFilter on a float32 map (:1688, :2769, :1403), optionally
//                     with the quantisation epilogue of :1696-1700 (clip, u8, colormap, range)
//  * k_fuse_quant     that epilogue alone (the "max <= 10" branch of :1687)
//
// Semantics: every f32 operation is rounded on its own (-ffp-contract=off), in
// the order the NumPy restatement of the tests uses; every exp is evaluated on the host in
// float64 and arrives as a float32 table, so the results are bit-identical to that
// restatement.  Borders are BORDER_REFLECT_101; the callers guarantee H, W > radius.
//
// One block of 256 threads owns a 16 x 64 output tile: wave w, lane l computes the pixels
// (w + 4 j, l), j = 0..3.  Four independent pixels per lane hide the serial tap sums, and a
// lane's taps of one (dy, dx) are 64 consecutive LDS words per wave (no bank conflicts on
// the tile; the colour-table lookups are data-dependent gathers and take what they get).
#include "sv_fold.h"
#include "sv_stencil.h"

namespace sv {
namespace {

constexpr int kTH = 16, kTW = 64, kPix = 4;
constexpr int kGaussR = 15;                    // ksize <= 31
constexpr int kBilPitch = kTW + 2 * kBilateralMaxR + 1;

struct GaussTile {
    float in[kTH + 2 * kGaussR][kTW + 2 * kGaussR + 1];
    float row[kTH + 2 * kGaussR][kTW];
};

// The separable blur of one tile at (y0, x0): out[j] = the blurred value at (y0 + w + 4 j,
// x0 + l).  FW: the staged value is the fill weight (1 - conf) * mfw of :1637 (src == nullptr:
// conf = 1).  c[0] is the centre coefficient.  Rows first, f32 intermediate; each pass is
// s = c0 x0, then s = s + c_i (x_-i + x_+i) for i = 1..r.
template <bool FW>
__device__ __forceinline__ void gauss_tile(GaussTile& t, const float* __restrict__ src, int H, int W, int y0,
                                           int x0, int r, const float* c, float mfw, float out[kPix]) {
    const int tid = threadIdx.x;
    const int rows = kTH + 2 * r, cols = kTW + 2 * r;
    for (int i = tid; i < rows * cols; i += 256) {
        const int ly = i / cols, lx = i - ly * cols;
        // reflect at the image borders; rows and columns past a partial tile are never used
        const int gy = clampi(refl101(y0 - r + ly, H), 0, H - 1);
        const int gx = clampi(refl101(x0 - r + lx, W), 0, W - 1);
        float v = src ? src[(size_t)gy * W + gx] : 1.0f;
        if (FW) v = (1.0f - v) * mfw;
        t.in[ly][lx] = v;
    }
    __syncthreads();
    for (int i = tid; i < rows * kTW; i += 256) {
        const int ly = i >> 6, lx = i & 63;
        const float* p = &t.in[ly][lx + r];
        float s = c[0] * p[0];
        for (int k = 1; k <= r; ++k) s = s + c[k] * (p[-k] + p[k]);
        t.row[ly][lx] = s;
    }
    __syncthreads();
    const int tx = tid & 63, ty = tid >> 6;
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const float* p = &t.row[ty + 4 * j + r][tx];
        float s = c[0] * p[0];
        for (int k = 1; k <= r; ++k) s = s + c[k] * (p[-k * kTW] + p[k * kTW]);
        out[j] = s;
    }
}

__global__ __launch_bounds__(256) void k_gauss_f32(GaussArgs a) {
    __shared__ GaussTile t;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    float o[kPix];
    gauss_tile<false>(t, a.src, a.H, a.W, y0, x0, a.r, a.c, 0.f, o);
    const int x = x0 + (threadIdx.x & 63), ty = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const int y = y0 + ty + 4 * j;
        if (y < a.H && x < a.W) a.dst[(size_t)y * a.W + x] = o[j];
    }
}

__global__ __launch_bounds__(256) void k_fuse_blend(FuseBlendArgs a) {
    __shared__ GaussTile t;
    __shared__ uint32_t red[4][4];
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    float fw[kPix] = {0.f, 0.f, 0.f, 0.f};
    if (a.midas_fill) gauss_tile<true>(t, a.conf, a.H, a.W, y0, x0, a.r, a.c, a.mfw, fw);
    const int x = x0 + (threadIdx.x & 63), ty = threadIdx.x >> 6;
    uint32_t kmin_inv = 0, kmax = 0, n_midas = 0, n_hole = 0;
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const int y = y0 + ty + 4 * j;
        if (y >= a.H || x >= a.W) continue;
        const size_t i = (size_t)y * a.W + x;
        float f;
        if (a.base == FUSE_BASE_STEREO) f = a.stereo[i] * a.sw;          // :1626-1628
        else if (a.base == FUSE_BASE_MIDAS) f = a.midas[i];              // :1666
        else f = a.flow[i];                                              // :1682
        if (a.midas_fill) {                                              // :1632-1649
            const float w = fminf(fmaxf(fw[j], 0.0f), 1.0f);
            const float conf = a.conf ? a.conf[i] : 1.0f;
            if (conf < a.thr && w > 0.1f) {
                f = f * (1.0f - w) + a.midas[i] * w;
                ++n_midas;
            }
        }
        if (a.flow_fill && (f < a.hthr || f == 0.0f)) {                  // :1653-1660, :1671-1676
            f = f * a.k1 + a.flow[i] * a.k2;
            ++n_hole;
        }
        a.fused[i] = f;
        const uint32_t k = fkey(f);
        kmin_inv = max(kmin_inv, ~k);
        kmax = max(kmax, k);
    }
    fold_stats(kmin_inv, kmax, n_midas, n_hole, red, a.stats);
}

// :1696-1700 for one pixel: np.clip(v, 0, 255), astype(uint8), the colormap, and the range of
// the clipped map.  The unclipped value goes to dst_f32 (the stand-alone filter's output).
template <bool QUANT>
__device__ __forceinline__ void bil_store(const BilateralArgs& a, size_t i, float v, uint32_t& kmin_inv,
                                          uint32_t& kmax) {
    if (a.dst_f32) a.dst_f32[i] = v;
    if (QUANT) {
        float q = v > 0.0f ? v : 0.0f;
        q = q < 255.0f ? q : 255.0f;
        const uint32_t u = (uint32_t)(int)q;
        if (a.dst_u8) a.dst_u8[i] = (uint8_t)u;
        if (a.dst_bgr) {
            const uint32_t c = a.cmap[u];
            a.dst_bgr[3 * i] = (uint8_t)c;
            a.dst_bgr[3 * i + 1] = (uint8_t)(c >> 8);
            a.dst_bgr[3 * i + 2] = (uint8_t)(c >> 16);
        }
        const uint32_t k = fkey(q);
        kmin_inv = max(kmin_inv, ~k);
        kmax = max(kmax, k);
    }
}

struct BilTile {
    float px[kTH + 2 * kBilateralMaxR][kBilPitch];
    float lut[kBilateralLut];
};

template <bool QUANT>
__global__ __launch_bounds__(256) void k_bilateral_f32(BilateralArgs a) {
    __shared__ BilTile t;
    __shared__ uint32_t red[4][4];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int r = a.r, rows = kTH + 2 * r, cols = kTW + 2 * r;
    for (int i = tid; i < rows * cols; i += 256) {
        const int ly = i / cols, lx = i - ly * cols;
        const int gy = clampi(refl101(y0 - r + ly, a.H), 0, a.H - 1);
        const int gx = clampi(refl101(x0 - r + lx, a.W), 0, a.W - 1);
        t.px[ly][lx] = a.src[(size_t)gy * a.W + gx];
    }
    for (int i = tid; i < kBilateralLut; i += 256) t.lut[i] = a.lut[i];
    __syncthreads();
    const int tx = tid & 63, ty = tid >> 6;
    const float* base[kPix];
    float c[kPix], sum[kPix], wsum[kPix];
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        base[j] = &t.px[ty + 4 * j + r][tx + r];
        c[j] = base[j][0];
        sum[j] = 0.0f;
        wsum[j] = 0.0f;
    }
    // fixed tap order (dy outer, dx inner): the sums are order-dependent by definition
    for (int k = 0; k < a.ntaps; ++k) {
        const float sw = a.sw[k];
        const int off = a.off[k];
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            const float v = base[j][off];
            float d = fabsf(v - c[j]) * a.scale;
            // in contract idx <= 4096; the clamp only keeps a stray value inside the table
            const int idx = clampi((int)d, 0, kBilateralLut - 2);
            d = d - (float)idx;
            const float l0 = t.lut[idx], l1 = t.lut[idx + 1];
            const float w = sw * (l0 + d * (l1 - l0));
            sum[j] = sum[j] + v * w;
            wsum[j] = wsum[j] + w;
        }
    }
    uint32_t kmin_inv = 0, kmax = 0;
    const int x = x0 + tx;
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const int y = y0 + ty + 4 * j;
        if (y < a.H && x < a.W)
            bil_store<QUANT>(a, (size_t)y * a.W + x, (sum[j] + c[j]) / (wsum[j] + 1.0f), kmin_inv, kmax);
    }
    if (QUANT) fold_stats(kmin_inv, kmax, 0, 0, red, a.stats);
}

__global__ __launch_bounds__(256) void k_fuse_quant(BilateralArgs a) {
    __shared__ uint32_t red[4][4];
    const size_t n = (size_t)a.H * a.W, stride = (size_t)gridDim.x * 256;
    uint32_t kmin_inv = 0, kmax = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        bil_store<true>(a, i, a.src[i], kmin_inv, kmax);
    fold_stats(kmin_inv, kmax, 0, 0, red, a.stats);
}

__global__ __launch_bounds__(256) void k_copy_f32(const float* __restrict__ src, float* __restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}

dim3 tile_grid(int H, int W) { return dim3((W + kTW - 1) / kTW, (H + kTH - 1) / kTH); }

int flat_blocks(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 4096); }

}  // namespace

int bilateral_taps(int r, int* dy, int* dx) {
    int n = 0;
    for (int y = -r; y <= r; ++y)
        for (int x = -r; x <= r; ++x) {
            if (y * y + x * x > r * r || (y == 0 && x == 0)) continue;
            if (dy) dy[n] = y;
            if (dx) dx[n] = x;
            ++n;
        }
    return n;
}

int launch_gauss_f32(const GaussArgs& a, hipStream_t s) {
    if (a.r < 1 || a.r > kGaussR || a.H <= a.r || a.W <= a.r) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gauss_f32, tile_grid(a.H, a.W), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_fuse_blend(const FuseBlendArgs& a, hipStream_t s) {
    if (a.H <= 0 || a.W <= 0) return (int)hipErrorInvalidValue;
    if (a.midas_fill && (a.r < 1 || a.r > kGaussR || a.H <= a.r || a.W <= a.r)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fuse_blend, tile_grid(a.H, a.W), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_bilateral_f32(BilateralArgs a, const float* space_w, hipStream_t s) {
    if (a.H <= 0 || a.W <= 0 || a.r < 0 || a.r > kBilateralMaxR) return (int)hipErrorInvalidValue;
    const bool quant = a.stats != nullptr;   // the quantised outputs come with the range fold
    if (!a.src || ((a.dst_u8 || a.dst_bgr) && !quant) || (a.dst_bgr && !a.cmap)) return (int)hipErrorInvalidValue;
    if (a.r == 0) {   // no filter: the epilogue (or a plain copy) elementwise
        const size_t n = (size_t)a.H * a.W;
        if (quant) hipLaunchKernelGGL(k_fuse_quant, dim3(flat_blocks(n)), dim3(256), 0, s, a);
        else if (a.dst_f32) hipLaunchKernelGGL(k_copy_f32, dim3(flat_blocks(n)), dim3(256), 0, s, a.src, a.dst_f32, n);
        return (int)hipGetLastError();
    }
    if (a.H <= a.r || a.W <= a.r || !space_w || !a.lut) return (int)hipErrorInvalidValue;
    int dy[kBilateralMaxTaps], dx[kBilateralMaxTaps];
    a.ntaps = bilateral_taps(a.r, dy, dx);
    for (int k = 0; k < a.ntaps; ++k) {
        a.sw[k] = space_w[k];
        a.off[k] = (short)(dy[k] * kBilPitch + dx[k]);
    }
    if (quant) hipLaunchKernelGGL(k_bilateral_f32<true>, tile_grid(a.H, a.W), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_bilateral_f32<false>, tile_grid(a.H, a.W), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace sv
