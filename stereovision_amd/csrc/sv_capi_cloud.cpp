// sv_capi_cloud.cpp — the C ABI of the 3D reprojection and the ordered point cloud
// (include/stereovision_amd.h).  Kernels: sv_cloud.hip.
#include <cmath>

#include "sv_ctx.h"

namespace {

// the context's scratch words (DevBuf cloud): the minimum's key, the count, then the tile counts
constexpr size_t kMinWord = 0, kCountWord = 1, kTileWords = 4;

size_t elem_bytes(int fmt) { return fmt == SV_DISP_F32 ? sizeof(float) : sizeof(int16_t); }

// The argument rules both entry points share (nothing is enqueued before them).
int check_disp(const void* disp, int fmt, int H, int W, int pitch, const double* Q, const void* xyz) {
    if (!disp || !Q || !xyz) return fail(SV_EINVAL, "null disparity map, Q or xyz output");
    if (fmt != SV_DISP_I16X16 && fmt != SV_DISP_F32) return fail(SV_EINVAL, "unknown disparity format");
    if (H < 1 || W < 1) return fail(SV_EINVAL, "non-positive map size");
    if ((int64_t)H * W >= ((int64_t)1 << 31)) return fail(SV_EINVAL, "H * W must stay below 2^31");
    if (pitch < W) return fail(SV_EINVAL, "pitch smaller than width");
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(Q[i])) return fail(SV_EINVAL, "Q holds a non-finite entry");
    return 0;
}

int check_cloud(int H, int W, const uint8_t* bgr, int64_t bgr_pitch, const sv_cloud_params* p, int64_t cap,
                const uint8_t* out_bgr) {
    if (!p) return fail(SV_EINVAL, "null cloud parameters");
    if (cap < 0) return fail(SV_EINVAL, "negative capacity");
    if (out_bgr && !bgr) return fail(SV_EINVAL, "a colour output without a colour image");
    if (bgr && bgr_pitch < (int64_t)3 * W) return fail(SV_EINVAL, "bgr_pitch smaller than a row");
    if (std::isnan(p->min_valid) || std::isnan(p->z_min) || std::isnan(p->z_max))
        return fail(SV_EINVAL, "NaN in min_valid, z_min or z_max");
    if (p->z_min > p->z_max) return fail(SV_EINVAL, "z_min above z_max");
    if (p->roi_w != 0 && p->roi_h != 0 &&
        (p->roi_x < 0 || p->roi_y < 0 || p->roi_w < 0 || p->roi_h < 0 || (int64_t)p->roi_x + p->roi_w > W ||
         (int64_t)p->roi_y + p->roi_h > H))
        return fail(SV_EINVAL, "region of interest outside the map");
    return 0;
}

sv::CloudArgs map_args(const void* disp, int fmt, int H, int W, int pitch, const double* Q, float* xyz) {
    sv::CloudArgs a{};
    a.disp = disp;
    a.fmt = fmt;
    a.H = H;
    a.W = W;
    a.pitch = pitch;
    std::memcpy(a.Q.m, Q, sizeof a.Q.m);
    a.xyz = xyz;
    return a;
}

// The minimum of the map into the context's word; it stays on the device for the launches behind it.
int enqueue_min(sv_ctx* c, const sv::CloudArgs& a, hipStream_t s, const uint32_t** dmin) {
    SV_HIP(c->cloud.ensure((kTileWords + sv::cloud_tiles(a.H, a.W)) * sizeof(uint32_t)));
    uint32_t* w = c->cloud.as<uint32_t>() + kMinWord;
    SV_HIP(hipMemsetAsync(w, 0xff, sizeof(uint32_t), s));
    SV_LAUNCH(c, SV_K_CLOUD_MIN, s, sv::launch_cloud_min(a.disp, a.fmt, a.H, a.W, a.pitch, w, s));
    *dmin = w;
    return 0;
}

int enqueue_reproject(sv_ctx* c, sv::CloudArgs a, int handle_missing, hipStream_t s) {
    if (handle_missing)
        if (const int rc = enqueue_min(c, a, s, &a.dmin)) return rc;
    SV_LAUNCH(c, SV_K_REPROJECT, s, sv::launch_reproject(a, s));
    return 0;
}

// count, scan, emit; the count lands in the context's word and in d_count
int enqueue_cloud(sv_ctx* c, sv::CloudArgs a, const uint8_t* bgr, int bgr_pitch, const sv_cloud_params& p,
                  int64_t cap, uint8_t* out_bgr, uint32_t* index, uint32_t* d_count, hipStream_t s) {
    const uint32_t nb = sv::cloud_tiles(a.H, a.W);
    SV_HIP(c->cloud.ensure((kTileWords + nb) * sizeof(uint32_t)));
    if (p.handle_missing)
        if (const int rc = enqueue_min(c, a, s, &a.dmin)) return rc;
    const bool whole = p.roi_w == 0 || p.roi_h == 0;
    a.bgr = bgr;
    a.bgr_pitch = bgr_pitch;
    a.min_valid = p.min_valid;
    a.z_min = p.z_min;
    a.z_max = p.z_max;
    a.rx = whole ? 0 : p.roi_x;
    a.ry = whole ? 0 : p.roi_y;
    a.rw = whole ? a.W : p.roi_w;
    a.rh = whole ? a.H : p.roi_h;
    a.cap = cap;
    a.out_bgr = out_bgr;
    a.out_index = index;
    a.counts = c->cloud.as<uint32_t>() + kTileWords;
    SV_LAUNCH(c, SV_K_CLOUD_COUNT, s, sv::launch_cloud_count(a, s));
    SV_LAUNCH(c, SV_K_CLOUD_SCAN, s,
              sv::launch_cloud_scan(a.counts, nb, c->cloud.as<uint32_t>() + kCountWord, d_count, s));
    SV_LAUNCH(c, SV_K_CLOUD_EMIT, s, sv::launch_cloud_emit(a, s));
    return 0;
}

// the count word, read on stream s; the call waits for it
int read_count(sv_ctx* c, hipStream_t s, int64_t* n_points) {
    SV_HIP(c->hout.ensure(256));
    SV_HIP(c->copy(c->hout.p, c->cloud.as<uint32_t>() + kCountWord, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    SV_HIP(hipStreamSynchronize(s));
    *n_points = *c->hout.as<uint32_t>();
    return 0;
}

// One host map (and its colour image) into cl_in through the staging helper.
int stage_inputs(sv_ctx* c, const void* disp, int fmt, int H, int W, int stride, const uint8_t* bgr, int bgr_stride) {
    const size_t row = (size_t)W * elem_bytes(fmt), n = ((size_t)H * row + 255) & ~(size_t)255;
    SV_HIP(c->hin.ensure(n + (bgr ? (size_t)H * W * 3 : 0)));
    if (const int rc = stage_image(c, disp, H, row, (size_t)stride * elem_bytes(fmt), 0, c->cl_in[0])) return rc;
    if (bgr) return stage_image(c, bgr, H, (size_t)W * 3, (size_t)bgr_stride, n, c->cl_in[1]);
    return 0;
}

}  // namespace

extern "C" {

int sv_reproject_3d_dev(sv_ctx* c, const void* d_disp, int fmt, int H, int W, int pitch, const double Q[16],
                        int handle_missing, float* d_xyz, void* stream) {
    SV_ENTER(c);
    if (const int rc = check_disp(d_disp, fmt, H, W, pitch, Q, d_xyz)) return rc;
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    return enqueue_reproject(c, map_args(d_disp, fmt, H, W, pitch, Q, d_xyz), handle_missing, s);
}

int sv_point_cloud_dev(sv_ctx* c, const void* d_disp, int fmt, int H, int W, int pitch, const double Q[16],
                       const uint8_t* d_bgr, int bgr_pitch, const sv_cloud_params* params, int64_t cap,
                       float* d_xyz, uint8_t* d_out_bgr, uint32_t* d_index, uint32_t* d_count,
                       int64_t* n_points, void* stream) {
    SV_ENTER(c);
    int rc = check_disp(d_disp, fmt, H, W, pitch, Q, d_xyz);
    if (!rc) rc = check_cloud(H, W, d_bgr, bgr_pitch, params, cap, d_out_bgr);
    if (rc) return rc;
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    rc = enqueue_cloud(c, map_args(d_disp, fmt, H, W, pitch, Q, d_xyz), d_bgr, bgr_pitch, *params, cap, d_out_bgr,
                       d_index, d_count, s);
    if (rc || !n_points) return rc;
    return read_count(c, s, n_points);
}

int sv_reproject_3d(sv_ctx* c, const void* disp, int fmt, int H, int W, int stride, const double Q[16],
                    int handle_missing, float* xyz) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    int rc = check_disp(disp, fmt, H, W, stride, Q, xyz);
    if (rc) return rc;
    rc = stage_inputs(c, disp, fmt, H, W, stride, nullptr, 0);
    if (rc) return rc;
    const size_t bytes = (size_t)H * W * 3 * sizeof(float);
    SV_HIP(c->cl_out[0].ensure(bytes));
    rc = enqueue_reproject(c, map_args(c->cl_in[0].p, fmt, H, W, W, Q, c->cl_out[0].as<float>()), handle_missing,
                           c->stream);
    if (rc) return rc;
    Out o[] = {{xyz, c->cl_out[0].p, bytes}};
    return collect(c, o, 1);
}

int sv_point_cloud(sv_ctx* c, const void* disp, int fmt, int H, int W, int stride, const double Q[16],
                   const uint8_t* bgr, int bgr_stride, const sv_cloud_params* params, int64_t cap, float* xyz,
                   uint8_t* out_bgr, uint32_t* index, int64_t* n_points) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    int rc = check_disp(disp, fmt, H, W, stride, Q, xyz);
    if (!rc) rc = check_cloud(H, W, bgr, bgr_stride, params, cap, out_bgr);
    if (rc) return rc;
    rc = stage_inputs(c, disp, fmt, H, W, stride, out_bgr ? bgr : nullptr, bgr_stride);
    if (rc) return rc;
    const size_t room = (size_t)std::min<int64_t>(cap, (int64_t)H * W);   // no cloud holds more points
    SV_HIP(c->cl_out[0].ensure(std::max<size_t>(room, 1) * 3 * sizeof(float)));
    if (out_bgr) SV_HIP(c->cl_out[1].ensure(std::max<size_t>(room, 1) * 3));
    if (index) SV_HIP(c->cl_out[2].ensure(std::max<size_t>(room, 1) * sizeof(uint32_t)));
    rc = enqueue_cloud(c, map_args(c->cl_in[0].p, fmt, H, W, W, Q, c->cl_out[0].as<float>()),
                       out_bgr ? c->cl_in[1].as<uint8_t>() : nullptr, 3 * W, *params, (int64_t)room,
                       out_bgr ? c->cl_out[1].as<uint8_t>() : nullptr, index ? c->cl_out[2].as<uint32_t>() : nullptr,
                       nullptr, c->stream);
    if (rc) return rc;
    int64_t n = 0;
    rc = read_count(c, c->stream, &n);
    if (rc) return rc;
    if (n_points) *n_points = n;
    const size_t m = (size_t)std::min<int64_t>(n, (int64_t)room);
    if (m == 0) return 0;
    Out o[] = {{xyz, c->cl_out[0].p, m * 3 * sizeof(float)},
               {out_bgr, c->cl_out[1].p, m * 3},
               {index, c->cl_out[2].p, m * sizeof(uint32_t)}};
    return collect(c, o, 3);
}

}  // extern "C"
