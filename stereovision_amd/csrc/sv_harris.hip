// sv_harris.hip — Harris response, cornerHarris(3, 3, 0.04) convention (north_star), in three
// bit-identical forms (gfx950):
//  * k_harris_lds   one LDS stencil pass per 64 x 16 tile (images under 8 px, SV_HARRIS=lds)
//  * k_harris_dpp   register/DPP bands, one column per lane (the default for W, H >= 8)
//  * k_harris_dpp4  register/DPP bands, four columns per lane (the default for W >= 1024)
// The DPP bands themselves live in sv_harris_wave.h: k_median_i16 runs them too.
#include <cstdlib>
#include <cstring>
#include "sv_harris_wave.h"

namespace sv {
namespace {

// ---------------------------------------------------------------------------------------
// Harris as one LDS stencil pass (north_star: Sobel + structure tensor fused): a block
// stages the (64+4) x (16+4) image bytes of its 64 x 16 output tile once, forms the
// gradient products of the (64+2) x (16+2) in-image positions around it from LDS, and box-
// sums them per output (4 rows per thread).  Reflect-101 borders index the staged rows/cols
// directly (every reflected index used lies inside the staged window), so the response is
// identical to cv2.cornerHarris's convention.  grid.z = frame of a batch.
constexpr int HX2 = 64, HY2 = 16;
__global__ __launch_bounds__(256) void k_harris_lds(const uint8_t* __restrict__ g, int H, int W, int pitch,
                                                    float* __restrict__ out, long long fs_in, long long fs_out) {
    __shared__ uint8_t img[HY2 + 4][HX2 + 4];
    __shared__ int pxx[HY2 + 2][HX2 + 2], pxy[HY2 + 2][HX2 + 2], pyy[HY2 + 2][HX2 + 2];
    g += blockIdx.z * fs_in;
    out += blockIdx.z * fs_out;
    const int x0 = blockIdx.x * HX2, y0 = blockIdx.y * HY2;
    for (int i = threadIdx.x; i < (HY2 + 4) * (HX2 + 4); i += 256) {
        const int r = i / (HX2 + 4), c = i - r * (HX2 + 4);
        img[r][c] = g[(size_t)clampi(y0 - 2 + r, 0, H - 1) * pitch + clampi(x0 - 2 + c, 0, W - 1)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (HY2 + 2) * (HX2 + 2); i += 256) {
        const int r = i / (HX2 + 2), c = i - r * (HX2 + 2);
        const int y = y0 - 1 + r, x = x0 - 1 + c;
        if (y < 0 || y >= H || x < 0 || x >= W) continue;   // never read (box sums reflect)
        const int ym = refl101(y - 1, H) - (y0 - 2), yp = refl101(y + 1, H) - (y0 - 2), yc = y - (y0 - 2);
        const int xm = refl101(x - 1, W) - (x0 - 2), xp = refl101(x + 1, W) - (x0 - 2), xc = x - (x0 - 2);
        int gx, gy;
        sobel_tile(img, ym, yc, yp, xm, xc, xp, gx, gy);
        pxx[r][c] = gx * gx;
        pxy[r][c] = gx * gy;
        pyy[r][c] = gy * gy;
    }
    __syncthreads();
    const int tx = threadIdx.x % HX2, tq = 4 * (threadIdx.x / HX2);
    const int x = x0 + tx;
    if (x >= W) return;
    const int cm = refl101(x - 1, W) - (x0 - 1), cc = x - (x0 - 1), cp = refl101(x + 1, W) - (x0 - 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int y = y0 + tq + q;
        if (y >= H) break;
        const int rows[3] = {refl101(y - 1, H) - (y0 - 1), y - (y0 - 1), refl101(y + 1, H) - (y0 - 1)};
        int sxx = 0, sxy = 0, syy = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int rr = rows[j];
            sxx += pxx[rr][cm] + pxx[rr][cc] + pxx[rr][cp];
            sxy += pxy[rr][cm] + pxy[rr][cc] + pxy[rr][cp];
            syy += pyy[rr][cm] + pyy[rr][cc] + pyy[rr][cp];
        }
        out[(size_t)y * W + x] = harris_response(sxx, sxy, syy);
    }
}

template <int HB, int PF>
__global__ __launch_bounds__(64) void k_harris_dpp(const uint8_t* __restrict__ g, int H, int W, int pitch,
                                                   float* __restrict__ out, long long fs_in, long long fs_out) {
    harris_wave<HB, PF>(g + blockIdx.z * fs_in, H, W, pitch, out + blockIdx.z * fs_out, blockIdx.x * 60,
                        blockIdx.y * HB, threadIdx.x);
}

template <int HB, int PF>
__global__ __launch_bounds__(64) void k_harris_dpp4(const uint8_t* __restrict__ g, int H, int W, int pitch,
                                                    float* __restrict__ out, long long fs_in, long long fs_out) {
    harris_wave4<HB, PF>(g + blockIdx.z * fs_in, H, W, pitch, out + blockIdx.z * fs_out, blockIdx.x * 248,
                         blockIdx.y * HB, threadIdx.x);
}

}  // namespace

int launch_harris(const uint8_t* g, int H, int W, int pitch, float* out, hipStream_t s, int nf,
                  long long fs_in, long long fs_out) {
    if (nf <= 0) return 0;
    // SV_HARRIS (A/B) = lds: the LDS-tile kernel everywhere (it also serves images under 8 px);
    // = dpp1: one column per lane everywhere
    static const int form = [] {
        const char* e = std::getenv("SV_HARRIS");
        return e && e[0] == 'l' ? 'l' : e && std::strcmp(e, "dpp1") == 0 ? '1' : 0;
    }();
    if (form != 'l' && W >= 8 && H >= 8) {
        // 8 output rows per wave: C2 16.8 us per 16 VGA frames (16 rows: 17.7, 32: 21.0; 1080p
        // 99 / 98 / 105 us; the SV_HARRIS_HB A/B switch was removed in round 4)
        // 4 columns per lane from 1024 columns (1080p: 91.6 vs 98.6 us per 16 frames); narrower
        // frames keep 1 per lane (VGA: 16.7 vs 21.6 us — a quarter of the waves hides less latency)
        if (form != '1' && W >= 1024) {
            hipLaunchKernelGGL((k_harris_dpp4<8, 4>), dim3((W + 247) / 248, (H + 7) / 8, nf), dim3(64), 0, s, g, H, W,
                               pitch, out, fs_in, fs_out);
            return (int)hipGetLastError();
        }
        hipLaunchKernelGGL((k_harris_dpp<8, 4>), dim3((W + 59) / 60, (H + 7) / 8, nf), dim3(64), 0, s, g, H, W, pitch,
                           out, fs_in, fs_out);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(k_harris_lds, dim3((W + HX2 - 1) / HX2, (H + HY2 - 1) / HY2, nf), dim3(256), 0, s, g,
                       H, W, pitch, out, fs_in, fs_out);
    return (int)hipGetLastError();
}

}  // namespace sv
