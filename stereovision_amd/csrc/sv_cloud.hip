// sv_cloud.hip — 3D reprojection of a disparity map and the ordered, coloured point cloud
// (DESIGN.md §5j): the dense H x W x 3 map of cv2.reprojectImageTo3D (k_reproject), the map's
// minimum for handleMissingValues (k_cloud_min) and the order-keeping compaction in three
// launches (k_cloud_count, k_cloud_scan, k_cloud_emit).  Semantics: tests/sv_cloud_oracle.py.
// gfx950 (wave64).  No block waits on another: the passes are ordered by the stream.
#include <cfloat>

#include "sv_internal.h"

namespace sv {
namespace {

constexpr int kRun = 4;                       // consecutive pixels per lane (k_reproject, k_cloud_min)
constexpr int kMapW = 64 * kRun, kMapH = 4;   // their block: one wave per row, 256 columns
constexpr int kSub = kCloudTile / 256;        // compaction: pixels per thread, 256 apart

// ---- one pixel ---------------------------------------------------------------------------
// The raw word of a pixel: the int16 value sign-extended, or the f32's bits.
template <int FMT>
__device__ __forceinline__ int load_raw(const void* disp, size_t i) {
    if (FMT == CLOUD_I16X16) return static_cast<const int16_t*>(disp)[i];
    return __float_as_int(static_cast<const float*>(disp)[i]);
}

// kRun pixels from element i on; n < kRun, or a run that is not aligned for one wide load, goes
// pixel by pixel (row ends and pitched rows).
template <int FMT>
__device__ __forceinline__ void load_run(const void* disp, size_t i, int n, int raw[kRun]) {
    if (FMT == CLOUD_I16X16) {
        const int16_t* p = static_cast<const int16_t*>(disp) + i;
        if (n == kRun && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
            const short4 v = *reinterpret_cast<const short4*>(p);
            raw[0] = v.x, raw[1] = v.y, raw[2] = v.z, raw[3] = v.w;
            return;
        }
    } else {
        const float* p = static_cast<const float*>(disp) + i;
        if (n == kRun && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const float4 v = *reinterpret_cast<const float4*>(p);
            raw[0] = __float_as_int(v.x), raw[1] = __float_as_int(v.y);
            raw[2] = __float_as_int(v.z), raw[3] = __float_as_int(v.w);
            return;
        }
    }
    for (int k = 0; k < kRun; ++k) raw[k] = k < n ? load_raw<FMT>(disp, i + k) : 0;
}

template <int FMT>
__device__ __forceinline__ double disp_of(int raw) {
    if (FMT == CLOUD_I16X16) return (double)((float)raw / 16.0f);
    return (double)__int_as_float(raw);
}

// A u32 key that orders like the value; NaNs take no part (kCloudNoMin, which no value maps to).
template <int FMT>
__device__ __forceinline__ uint32_t key_of(int raw) {
    if (FMT == CLOUD_I16X16) return (uint32_t)(raw + 32768);
    const uint32_t u = (uint32_t)raw;
    if ((u & 0x7fffffffu) > 0x7f800000u) return kCloudNoMin;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int FMT>
__device__ __forceinline__ double dmin_of(uint32_t key) {
    if (key == kCloudNoMin) return (double)INFINITY;
    if (FMT == CLOUD_I16X16) return disp_of<FMT>((int)key - 32768);
    return disp_of<FMT>((int)((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key));
}

// Row r of Q times (x, y, d, 1), summed from 0 in Matx's order.
__device__ __forceinline__ double q_row(const CloudQ& q, int r, double x, double y, double d) {
    return (((0.0 + q.m[4 * r] * x) + q.m[4 * r + 1] * y) + q.m[4 * r + 2] * d) + q.m[4 * r + 3] * 1.0;
}

// (X, Y, Z) of pixel (x, y) with disparity d: the homogeneous point narrowed to f32, then scaled
// by the f64 reciprocal of its fourth coordinate.
__device__ __forceinline__ void reproject_px(const CloudQ& q, int x, int y, double d, float o[3]) {
    const double fx = (double)x, fy = (double)y;
    const double ia = 1.0 / q_row(q, 3, fx, fy, d);
    for (int r = 0; r < 3; ++r) o[r] = (float)((double)(float)q_row(q, r, fx, fy, d) * ia);
}

__device__ __forceinline__ bool is_missing(double d, double dmin) {
    return fabs(d - dmin) <= (double)FLT_EPSILON;
}

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ---- the dense map -------------------------------------------------------------------------
template <int FMT>
__global__ __launch_bounds__(256) void k_reproject(CloudArgs a) {
    const CloudQ q = a.Q;
    const int nbx = (a.W + kMapW - 1) / kMapW;
    const int by = blockIdx.x / nbx, bx = blockIdx.x - by * nbx;
    const int x = bx * kMapW + (threadIdx.x & 63) * kRun, y = by * kMapH + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const int n = min(kRun, a.W - x);
    int raw[kRun];
    load_run<FMT>(a.disp, (size_t)y * a.pitch + x, n, raw);
    const bool missing = a.dmin != nullptr;
    const double dmin = missing ? dmin_of<FMT>(*a.dmin) : 0.0;
    float o[3 * kRun];
    for (int k = 0; k < kRun; ++k) {
        const double d = disp_of<FMT>(raw[k]);
        reproject_px(q, x + k, y, d, o + 3 * k);
        if (missing && is_missing(d, dmin)) o[3 * k + 2] = 10000.0f;
    }
    float* dst = a.xyz + ((size_t)y * a.W + x) * 3;
    if (n == kRun && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        float4* d4 = reinterpret_cast<float4*>(dst);
        d4[0] = make_float4(o[0], o[1], o[2], o[3]);
        d4[1] = make_float4(o[4], o[5], o[6], o[7]);
        d4[2] = make_float4(o[8], o[9], o[10], o[11]);
    } else {
        for (int k = 0; k < 3 * n; ++k) dst[k] = o[k];
    }
}

// ---- the map's minimum -----------------------------------------------------------------------
// Registers, then the wave, then at most one atomic per block into *out (kCloudNoMin on entry).
template <int FMT>
__global__ __launch_bounds__(256) void k_cloud_min(const void* __restrict__ disp, int H, int W, int pitch,
                                                   uint32_t* __restrict__ out) {
    __shared__ uint32_t wmin[4];
    const int nbx = (W + kMapW - 1) / kMapW;
    const int by = blockIdx.x / nbx, bx = blockIdx.x - by * nbx;
    const int x = bx * kMapW + (threadIdx.x & 63) * kRun, y = by * kMapH + (threadIdx.x >> 6);
    uint32_t key = kCloudNoMin;
    if (x < W && y < H) {
        const int n = min(kRun, W - x);
        int raw[kRun];
        load_run<FMT>(disp, (size_t)y * pitch + x, n, raw);
        for (int k = 0; k < kRun; ++k)
            if (k < n) key = min(key, key_of<FMT>(raw[k]));
    }
    for (int o = 32; o > 0; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o, 64));
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        key = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
        // the word only falls: a block whose minimum does not beat the value it reads (however
        // stale) has nothing to add, which spares the word most of its same-address atomics
        if (key < __atomic_load_n(out, __ATOMIC_RELAXED)) atomicMin(out, key);
    }
}

// ---- the cloud ---------------------------------------------------------------------------------
// Whether pixel p = y W + x is a point of the cloud, and its coordinates.
template <int FMT>
__device__ __forceinline__ bool cloud_point(const CloudArgs& a, const CloudQ& q, uint32_t p, bool missing,
                                            double dmin, float o[3], int* px, int* py) {
    const int y = (int)(p / (uint32_t)a.W), x = (int)(p - (uint32_t)y * (uint32_t)a.W);
    *px = x, *py = y;
    if (x < a.rx || x >= a.rx + a.rw || y < a.ry || y >= a.ry + a.rh) return false;
    const double d = disp_of<FMT>(load_raw<FMT>(a.disp, (size_t)y * a.pitch + x));
    if (!(d >= (double)a.min_valid)) return false;
    if (missing && is_missing(d, dmin)) return false;
    reproject_px(q, x, y, d, o);
    if (!finite_f32(o[0]) || !finite_f32(o[1]) || !finite_f32(o[2])) return false;
    return a.z_min <= o[2] && o[2] <= a.z_max;
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Tile b holds pixels [b kCloudTile, (b + 1) kCloudTile) in row-major order; sub-tile j, wave w,
// lane l looks at pixel b kCloudTile + 256 j + 64 w + l, so a ballot covers 64 consecutive pixels.
template <int FMT>
__global__ __launch_bounds__(256) void k_cloud_count(CloudArgs a) {
    __shared__ uint32_t wsum[4];
    const CloudQ q = a.Q;
    const uint32_t n = (uint32_t)a.H * (uint32_t)a.W, p0 = blockIdx.x * (uint32_t)kCloudTile + threadIdx.x;
    const bool missing = a.dmin != nullptr;
    const double dmin = missing ? dmin_of<FMT>(*a.dmin) : 0.0;
    uint32_t cnt = 0;
    for (int j = 0; j < kSub; ++j) {
        const uint32_t p = p0 + 256u * j;
        float o[3];
        int x, y;
        const bool ok = p < n && cloud_point<FMT>(a, q, p, missing, dmin, o, &x, &y);
        cnt += (uint32_t)__popcll(__ballot(ok));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) a.counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One block: the tile counts become their exclusive prefix sums, in place; the total goes to
// *total and, when given, to the caller's device word.
__global__ __launch_bounds__(256) void k_cloud_scan(uint32_t* __restrict__ counts, uint32_t nb,
                                                    uint32_t* __restrict__ total, uint32_t* __restrict__ d_count) {
    __shared__ uint32_t part[256];
    const uint32_t t = threadIdx.x, seg = (nb + 255u) / 256u;
    const uint32_t b = min(t * seg, nb), e = min(b + seg, nb);
    uint32_t s = 0;
    for (uint32_t i = b; i < e; ++i) s += counts[i];
    part[t] = s;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint32_t v = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (uint32_t i = b; i < e; ++i) {
        const uint32_t c = counts[i];
        counts[i] = run;
        run += c;
    }
    if (t == 0) {
        *total = part[255];
        if (d_count) *d_count = part[255];
    }
}

// The tile's points go to LDS at their rank inside the tile, then out as contiguous runs from
// the tile's offset; what lies at or past `cap` is not written.
template <int FMT>
__global__ __launch_bounds__(256) void k_cloud_emit(CloudArgs a) {
    __shared__ float sxyz[3 * kCloudTile];
    __shared__ uint32_t sidx[kCloudTile];
    __shared__ uint8_t sbgr[3 * kCloudTile];
    __shared__ uint32_t wcnt[kSub * 4];
    const CloudQ q = a.Q;
    const uint32_t n = (uint32_t)a.H * (uint32_t)a.W, p0 = blockIdx.x * (uint32_t)kCloudTile + threadIdx.x;
    const int w = threadIdx.x >> 6;
    const bool missing = a.dmin != nullptr;
    const double dmin = missing ? dmin_of<FMT>(*a.dmin) : 0.0;
    float o[kSub][3];
    int x[kSub], y[kSub];
    bool ok[kSub];
    uint32_t below[kSub];
    for (int j = 0; j < kSub; ++j) {
        const uint32_t p = p0 + 256u * j;
        ok[j] = p < n && cloud_point<FMT>(a, q, p, missing, dmin, o[j], &x[j], &y[j]);
        const unsigned long long m = __ballot(ok[j]);
        below[j] = lanes_below(m);
        if ((threadIdx.x & 63) == 0) wcnt[4 * j + w] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t total = 0, before[kSub] = {};
    for (int i = 0; i < kSub * 4; ++i) {
        for (int j = 0; j < kSub; ++j)
            if (i == 4 * j + w) before[j] = total;
        total += wcnt[i];
    }
    for (int j = 0; j < kSub; ++j) {
        if (!ok[j]) continue;
        const uint32_t r = before[j] + below[j];
        sxyz[3 * r] = o[j][0], sxyz[3 * r + 1] = o[j][1], sxyz[3 * r + 2] = o[j][2];
        sidx[r] = p0 + 256u * j;
        if (a.out_bgr) {
            const uint8_t* c = a.bgr + (size_t)y[j] * a.bgr_pitch + 3 * x[j];
            sbgr[3 * r] = c[0], sbgr[3 * r + 1] = c[1], sbgr[3 * r + 2] = c[2];
        }
    }
    __syncthreads();
    const long long base = a.counts[blockIdx.x];
    const long long room = a.cap - base;
    const uint32_t m = room <= 0 ? 0u : (uint32_t)min((long long)total, room);
    float* oxyz = a.xyz + 3 * base;
    for (uint32_t i = threadIdx.x; i < 3 * m; i += 256) oxyz[i] = sxyz[i];
    if (a.out_bgr) {
        uint8_t* ob = a.out_bgr + 3 * base;
        for (uint32_t i = threadIdx.x; i < 3 * m; i += 256) ob[i] = sbgr[i];
    }
    if (a.out_index)
        for (uint32_t i = threadIdx.x; i < m; i += 256) a.out_index[base + i] = sidx[i];
}

dim3 map_grid(int H, int W) {
    return dim3((unsigned)(((W + kMapW - 1) / kMapW) * ((H + kMapH - 1) / kMapH)));
}

}  // namespace

uint32_t cloud_tiles(int H, int W) { return (uint32_t)(((long long)H * W + kCloudTile - 1) / kCloudTile); }

int launch_reproject(const CloudArgs& a, hipStream_t s) {
    if (a.fmt == CLOUD_I16X16) hipLaunchKernelGGL((k_reproject<CLOUD_I16X16>), map_grid(a.H, a.W), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_reproject<CLOUD_F32>), map_grid(a.H, a.W), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_cloud_min(const void* disp, int fmt, int H, int W, int pitch, uint32_t* out, hipStream_t s) {
    if (fmt == CLOUD_I16X16)
        hipLaunchKernelGGL((k_cloud_min<CLOUD_I16X16>), map_grid(H, W), dim3(256), 0, s, disp, H, W, pitch, out);
    else hipLaunchKernelGGL((k_cloud_min<CLOUD_F32>), map_grid(H, W), dim3(256), 0, s, disp, H, W, pitch, out);
    return (int)hipGetLastError();
}

int launch_cloud_count(const CloudArgs& a, hipStream_t s) {
    const dim3 grid(cloud_tiles(a.H, a.W));
    if (a.fmt == CLOUD_I16X16) hipLaunchKernelGGL((k_cloud_count<CLOUD_I16X16>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_cloud_count<CLOUD_F32>), grid, dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_cloud_scan(uint32_t* counts, uint32_t nb, uint32_t* total, uint32_t* d_count, hipStream_t s) {
    hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(256), 0, s, counts, nb, total, d_count);
    return (int)hipGetLastError();
}

int launch_cloud_emit(const CloudArgs& a, hipStream_t s) {
    const dim3 grid(cloud_tiles(a.H, a.W));
    if (a.fmt == CLOUD_I16X16) hipLaunchKernelGGL((k_cloud_emit<CLOUD_I16X16>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_cloud_emit<CLOUD_F32>), grid, dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace sv
