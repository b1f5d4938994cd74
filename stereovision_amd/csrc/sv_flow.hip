// sv_flow.hip — cv2.calcOpticalFlowFarneback (flags = 0) and the residual-flow depth of the
// reference's OpticalFlowDepthEstimator (fused_depth_map.py:1263-1501), for gfx950.
//
//  * k_fb_u8_f32            the u8 -> f32 source of the pyramid's Gaussian blur
//  * k_fb_polyexp           FarnebackPolyExp: separable (2n+1)^2 polynomial expansion, five planes
//  * k_fb_update_matrices   FarnebackUpdateMatrices: bilinear gather of the second frame's
//                           coefficients at x + flow, the five products of M
//  * k_fb_blur_solve        FarnebackUpdateFlow_Blur: winsize^2 box sums of M and the 2x2 solve
//  * k_fb_scale             the 1 / pyr_scale factor on an upsampled flow plane
//  * k_flow_depth           expected flow of a homography, residual, 1 / (|r| + 0.5), the
//                           exponential average and the range of the depth map
//
// Semantics: every f32 and f64 operation is rounded on its own
// (-ffp-contract=off), in the order of the NumPy restatement of the tests
// (tests/sv_flow_oracle.py); every exp and the moment-matrix inverse are evaluated on the host
// and arrive as tables, so the results are bit-identical to that restatement.  R, M and the
// per-level flow are planes, so every load but the gather is coalesced.  Rows and columns
// outside the image are clamped (BORDER_REPLICATE), as OpenCV's loops do.
//
// The stencil kernels use the tile of sv_fuse.hip: 256 threads own 16 x 64 outputs, wave w,
// lane l computes (w + 4 j, l), j = 0..3.
#include "sv_fold.h"
#include "sv_stencil.h"

namespace sv {
namespace {

constexpr int kTH = 16, kTW = 64, kPix = 4;
constexpr int kPolyPitch = kTW + 2 * kFbMaxPolyN + 1;
constexpr int kBoxR = kFbMaxWin / 2;
constexpr int kBoxCols = kTW + 2 * kBoxR;

__global__ __launch_bounds__(256) void k_fb_u8_f32(const uint8_t* __restrict__ src, int H, int W, int pitch,
                                                   float* __restrict__ dst) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x < W) dst[(size_t)y * W + x] = (float)src[(size_t)y * pitch + x];
}

__global__ __launch_bounds__(256) void k_fb_scale(float* __restrict__ x, size_t n, float k) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) x[i] = x[i] * k;
}

// Vertical pass into LDS (three f32 channels: sum g p, sum xg (below - above), sum xxg p, rows
// clamped), then the horizontal pass over LDS with six f64 accumulators (columns clamped: the
// halo column of a clamped x is the border column's own vertical result).
__global__ __launch_bounds__(256) void k_fb_polyexp(FbPolyArgs a) {
    __shared__ float v[3][kTH][kPolyPitch];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int n = a.n, cols = kTW + 2 * n;
    for (int i = tid; i < kTH * cols; i += 256) {
        const int ly = i / cols, lx = i - ly * cols;
        const int gy = min(y0 + ly, a.H - 1);          // rows past a partial tile are never used
        const int gx = clampi(x0 - n + lx, 0, a.W - 1);
        const float* col = a.src + gx;
        float c0 = col[(size_t)gy * a.W] * a.g[0], c1 = 0.0f, c2 = 0.0f;
        for (int k = 1; k <= n; ++k) {
            const float above = col[(size_t)max(gy - k, 0) * a.W];
            const float below = col[(size_t)min(gy + k, a.H - 1) * a.W];
            const float p = above + below;
            c0 = c0 + a.g[k] * p;
            c1 = c1 + a.xg[k] * (below - above);
            c2 = c2 + a.xxg[k] * p;
        }
        v[0][ly][lx] = c0;
        v[1][ly][lx] = c1;
        v[2][ly][lx] = c2;
    }
    __syncthreads();
    const int tx = tid & 63, ty = tid >> 6;
    const int x = x0 + tx;
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const int ly = ty + 4 * j, y = y0 + ly;
        const float* r0 = &v[0][ly][tx + n];
        const float* r1 = &v[1][ly][tx + n];
        const float* r2 = &v[2][ly][tx + n];
        const float g0 = a.g[0];
        double b1 = (double)(r0[0] * g0), b2 = 0.0, b3 = (double)(r1[0] * g0);
        double b4 = 0.0, b5 = (double)(r2[0] * g0), b6 = 0.0;
        for (int k = 1; k <= n; ++k) {
            const float gk = a.g[k], xgk = a.xg[k];
            const double tg = (double)(r0[k] + r0[-k]);
            b1 = b1 + tg * (double)gk;
            b4 = b4 + tg * (double)a.xxg[k];
            b2 = b2 + (double)((r0[k] - r0[-k]) * xgk);
            b3 = b3 + (double)((r1[k] + r1[-k]) * gk);
            b6 = b6 + (double)((r1[k] - r1[-k]) * xgk);
            b5 = b5 + (double)((r2[k] + r2[-k]) * gk);
        }
        if (y < a.H && x < a.W) {
            float* o = a.R + (size_t)y * a.W + x;
            o[0] = (float)(b3 * a.ig11);
            o[a.plane] = (float)(b2 * a.ig11);
            o[2 * a.plane] = (float)(b1 * a.ig03 + b5 * a.ig33);
            o[3 * a.plane] = (float)(b1 * a.ig03 + b4 * a.ig33);
            o[4 * a.plane] = (float)(b6 * a.ig55);
        }
    }
}

__device__ __forceinline__ float fb_border(int i, int n) {
    // {0.14, 0.14, 0.4472, 0.4472, 0.4472} towards either edge
    const float lo = i < 5 ? (i < 2 ? 0.14f : 0.4472f) : 1.0f;
    const int k = n - i - 1;
    const float hi = i >= n - 5 ? (k < 2 ? 0.14f : 0.4472f) : 1.0f;
    return lo * hi;
}

// The gather's address is data-dependent: the in-image test is made on the floored floats, so a
// flow of any finite size neither indexes outside R1 nor converts an out-of-range float.
__global__ __launch_bounds__(256) void k_fb_update_matrices(FbUpdateArgs a) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t i = (size_t)y * a.W + x, P = a.plane;
    const float dx = a.flow[i], dy = a.flow[P + i];
    float fx = (float)x + dx, fy = (float)y + dy;
    const float x1 = floorf(fx), y1 = floorf(fy);
    const float* R0 = a.R0 + i;
    float r2, r3, r4, r5, r6;
    if (x1 >= 0.0f && x1 < (float)(a.W - 1) && y1 >= 0.0f && y1 < (float)(a.H - 1)) {
        const float* p = a.R1 + (size_t)(int)y1 * a.W + (int)x1;
        fx = fx - x1;
        fy = fy - y1;
        const float a00 = (1.0f - fx) * (1.0f - fy), a01 = fx * (1.0f - fy);
        const float a10 = (1.0f - fx) * fy, a11 = fx * fy;
        const int W = a.W;
        r2 = ((a00 * p[0] + a01 * p[1]) + a10 * p[W]) + a11 * p[W + 1];
        p += P;
        r3 = ((a00 * p[0] + a01 * p[1]) + a10 * p[W]) + a11 * p[W + 1];
        p += P;
        r4 = ((a00 * p[0] + a01 * p[1]) + a10 * p[W]) + a11 * p[W + 1];
        p += P;
        r5 = ((a00 * p[0] + a01 * p[1]) + a10 * p[W]) + a11 * p[W + 1];
        p += P;
        r6 = ((a00 * p[0] + a01 * p[1]) + a10 * p[W]) + a11 * p[W + 1];
        r4 = (R0[2 * P] + r4) * 0.5f;
        r5 = (R0[3 * P] + r5) * 0.5f;
        r6 = (R0[4 * P] + r6) * 0.25f;
    } else {
        r2 = r3 = 0.0f;
        r4 = R0[2 * P];
        r5 = R0[3 * P];
        r6 = R0[4 * P] * 0.5f;
    }
    r2 = (R0[0] - r2) * 0.5f;
    r3 = (R0[P] - r3) * 0.5f;
    r2 = r2 + (r4 * dy + r6 * dx);
    r3 = r3 + (r6 * dy + r5 * dx);
    if (x < 5 || x >= a.W - 5 || y < 5 || y >= a.H - 5) {
        // ((x low * x high) * y low) * y high
        const int k = a.H - y - 1;
        const float yl = y < 5 ? (y < 2 ? 0.14f : 0.4472f) : 1.0f;
        const float yh = y >= a.H - 5 ? (k < 2 ? 0.14f : 0.4472f) : 1.0f;
        const float s = (fb_border(x, a.W) * yl) * yh;
        r2 = r2 * s;
        r3 = r3 * s;
        r4 = r4 * s;
        r5 = r5 * s;
        r6 = r6 * s;
    }
    float* M = a.M + i;
    M[0] = r4 * r4 + r6 * r6;
    M[P] = (r4 + r5) * r6;
    M[2 * P] = r5 * r5 + r6 * r6;
    M[3 * P] = r4 * r2 + r6 * r3;
    M[4 * P] = r6 * r2 + r5 * r3;
}

// Plane by plane: the f32 tile and its halo of m in LDS, f64 column sums (rows of the window top
// to bottom) in LDS, then each pixel's row of 2m+1 column sums left to right.  Then the solve.
__global__ __launch_bounds__(256) void k_fb_blur_solve(FbSolveArgs a) {
    __shared__ float tile[kTH + 2 * kBoxR][kBoxCols + 1];
    __shared__ double colsum[kTH][kBoxCols];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
    const int m = a.m, rows = kTH + 2 * m, cols = kTW + 2 * m, taps = 2 * m + 1;
    const int tx = tid & 63, ty = tid >> 6;
    double sum[5][kPix];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const float* src = a.M + c * a.plane;
        for (int i = tid; i < rows * cols; i += 256) {
            const int ly = i / cols, lx = i - ly * cols;
            const int gy = clampi(y0 - m + ly, 0, a.H - 1);
            const int gx = clampi(x0 - m + lx, 0, a.W - 1);
            tile[ly][lx] = src[(size_t)gy * a.W + gx];
        }
        __syncthreads();
        for (int i = tid; i < kTH * cols; i += 256) {
            const int ly = i / cols, lx = i - ly * cols;
            double s = 0.0;
            for (int d = 0; d < taps; ++d) s = s + (double)tile[ly + d][lx];
            colsum[ly][lx] = s;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            const double* p = &colsum[ty + 4 * j][tx];
            double s = 0.0;
            for (int d = 0; d < taps; ++d) s = s + p[d];
            sum[c][j] = s;
        }
    }
    const int x = x0 + tx;
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const int y = y0 + ty + 4 * j;
        if (y >= a.H || x >= a.W) continue;
        const double g11 = sum[0][j] * a.scale, g12 = sum[1][j] * a.scale, g22 = sum[2][j] * a.scale;
        const double h1 = sum[3][j] * a.scale, h2 = sum[4][j] * a.scale;
        const double idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3);
        const float u = (float)((g11 * h2 - g12 * h1) * idet);
        const float w = (float)((g22 * h1 - g12 * h2) * idet);
        const size_t i = (size_t)y * a.W + x;
        if (a.interleaved) {
            a.flow[2 * i] = u;
            a.flow[2 * i + 1] = w;
        } else {
            a.flow[i] = u;
            a.flow[a.plane + i] = w;
        }
    }
}

// cv2.perspectiveTransform on the f32 pixel grid (f64 inside), the residual, its magnitude as
// f32(sqrt(f64 rx^2 + f64 ry^2)), depth = 1 / (m + 0.5), and stable = alpha stable + beta depth.
__global__ __launch_bounds__(256) void k_flow_depth(FlowDepthArgs a) {
    __shared__ uint32_t red[4][4];
    const size_t n = (size_t)a.H * a.W;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t kmin_inv = 0, kmax = 0;
    if (i < n) {
        const int y = (int)(i / a.W), x = (int)(i - (size_t)y * a.W);
        const float xf = (float)x, yf = (float)y;
        const double xd = (double)xf, yd = (double)yf;
        double w = (xd * a.m[6] + yd * a.m[7]) + a.m[8];
        w = fabs(w) > 2.220446049250313e-16 ? 1.0 / w : 0.0;
        const float X = (float)(((xd * a.m[0] + yd * a.m[1]) + a.m[2]) * w);
        const float Y = (float)(((xd * a.m[3] + yd * a.m[4]) + a.m[5]) * w);
        const float ex = X - xf, ey = Y - yf;
        const float rx = a.flow[2 * i] - ex, ry = a.flow[2 * i + 1] - ey;
        const double rxd = (double)rx, ryd = (double)ry;
        const float mag = (float)sqrt(rxd * rxd + ryd * ryd);
        const float depth = 1.0f / (mag + 0.5f);
        a.depth[i] = depth;
        if (a.stable) a.stable[i] = a.alpha * a.stable[i] + a.beta * depth;
        const uint32_t k = fkey(depth);
        kmin_inv = ~k;
        kmax = k;
    }
    fold_stats(kmin_inv, kmax, 0, 0, red, a.stats);
}

// The flow at the ego-motion grid (fused_depth_map.py:1447-1455): out[j * nx + i] = flow[y0 + j
// step][x0 + i step], y0 = x0 = step / 2.  One lane per point, one 8-byte load and store each.
__global__ __launch_bounds__(256) void k_flow_grid(const float2* __restrict__ flow, int W, int step, int nx, int np,
                                                   float2* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= np) return;
    const int j = p / nx, i = p - j * nx;
    const int y = step / 2 + j * step, x = step / 2 + i * step;
    out[p] = flow[(size_t)y * W + x];
}

dim3 tile_grid(int H, int W) { return dim3((W + kTW - 1) / kTW, (H + kTH - 1) / kTH); }

}  // namespace

int flow_grid_points(int n, int step) { return n > step / 2 ? (n - step / 2 + step - 1) / step : 0; }

int launch_flow_grid(const float* flow, int H, int W, int step, float* out, hipStream_t s) {
    if (H <= 0 || W <= 0 || step < 1) return (int)hipErrorInvalidValue;
    const int ny = flow_grid_points(H, step), nx = flow_grid_points(W, step);
    const long long np = (long long)ny * nx;
    if (np == 0) return 0;
    if (np > 0x7fffffffll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_flow_grid, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const float2*>(flow), W, step, nx, (int)np, reinterpret_cast<float2*>(out));
    return (int)hipGetLastError();
}

int launch_fb_u8_f32(const uint8_t* src, int H, int W, int pitch, float* dst, hipStream_t s) {
    if (H <= 0 || W <= 0 || pitch < W) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fb_u8_f32, dim3((W + 255) / 256, H), dim3(256), 0, s, src, H, W, pitch, dst);
    return (int)hipGetLastError();
}

int launch_fb_scale(float* x, size_t n, float k, hipStream_t s) {
    if (n == 0) return 0;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_fb_scale, dim3(blocks), dim3(256), 0, s, x, n, k);
    return (int)hipGetLastError();
}

int launch_fb_polyexp(const FbPolyArgs& a, hipStream_t s) {
    if (a.H <= 0 || a.W <= 0 || a.n < 1 || a.n > kFbMaxPolyN || a.plane < (size_t)a.H * a.W)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fb_polyexp, tile_grid(a.H, a.W), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_fb_update_matrices(const FbUpdateArgs& a, hipStream_t s) {
    if (a.H <= 0 || a.W <= 0 || a.plane < (size_t)a.H * a.W) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fb_update_matrices, dim3((a.W + 63) / 64, (a.H + 3) / 4), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_fb_blur_solve(const FbSolveArgs& a, hipStream_t s) {
    if (a.H <= 0 || a.W <= 0 || a.m < 1 || a.m > kBoxR || a.plane < (size_t)a.H * a.W)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fb_blur_solve, tile_grid(a.H, a.W), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_flow_depth(const FlowDepthArgs& a, hipStream_t s) {
    if (a.H <= 0 || a.W <= 0) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)a.H * a.W;
    hipLaunchKernelGGL(k_flow_depth, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace sv
