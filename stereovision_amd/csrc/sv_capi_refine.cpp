// sv_capi_refine.cpp — the C ABI of the refinement stage (include/stereovision_amd.h,
// DESIGN.md §5i): the right-referenced match, the refinement of a winner-take-all map and
// the chain of both behind one call.  Kernels: sv_refine.hip.
#include "sv_ctx.h"

namespace {

// The argument rules every entry point of the stage shares (nothing is enqueued before them).
int check_stage(const void* d_left, const void* d_right, int H, int W, int pitch, int out_pitch, int min_disp,
                int num_disp, int win, int cost) {
    if (check_image(d_left, H, W) || check_image(d_right, H, W)) return SV_EINVAL;
    if (pitch < W || out_pitch < W) return fail(SV_EINVAL, "pitch smaller than width");
    if (H > 65535) return fail(SV_EINVAL, "refinement: more than 65535 rows");
    if (cost == SV_COST_SGBM) return fail(SV_EINVAL, "the refinement stage takes SAD, SSD, HOG and census maps, not SGBM");
    sv::MatchPlan plan;
    return check_match(H, W, min_disp, num_disp, win, cost, &plan);
}

int check_params(const sv_refine_params* p, int cost) {
    if (!p) return fail(SV_EINVAL, "null refinement parameters");
    if (p->min_curvature < 0) return fail(SV_EINVAL, "min_curvature must be >= 0");
    if (cost == SV_COST_HOG && (p->subpixel || p->min_curvature > 0))
        return fail(SV_EINVAL, "HOG maps take the left-right check and the speckle filter only");
    if (cost == SV_COST_CENSUS && (p->subpixel || p->min_curvature > 0))
        return fail(SV_EINVAL, "census maps take the left-right check and the speckle filter only");
    return 0;
}

// flipx(disparity16(flipx(R), flipx(L))): the mirrors go through the context's scratch
int enqueue_right(sv_ctx* c, const uint8_t* L, const uint8_t* R, int H, int W, int pitch, int min_disp, int num_disp,
                  int win, int cost, int16_t* out, int opitch, hipStream_t s) {
    const size_t n = (size_t)H * W;
    SV_HIP(c->rf_img[0].ensure(n));
    SV_HIP(c->rf_img[1].ensure(n));
    SV_HIP(c->rf_map.ensure(n * sizeof(int16_t)));
    uint8_t* ml = c->rf_img[0].as<uint8_t>();   // the mirrored right frame: the match's left
    uint8_t* mr = c->rf_img[1].as<uint8_t>();
    SV_LAUNCH(c, SV_K_FLIP, s, sv::launch_flip_u8(R, L, ml, mr, H, W, pitch, W, s));
    const int rc = enqueue_disparity(c, ml, mr, H, W, W, min_disp, num_disp, win, cost, 0, H,
                                     c->rf_map.as<int16_t>(), W, s);
    if (rc) return rc;
    c->scratch_written(out);
    SV_LAUNCH(c, SV_K_FLIP, s, sv::launch_flip_i16(c->rf_map.as<int16_t>(), out, H, W, W, opitch, s));
    return 0;
}

int enqueue_refine(sv_ctx* c, const uint8_t* L, const uint8_t* R, int H, int W, int pitch, const int16_t* dl,
                   const int16_t* dr, int min_disp, int num_disp, int win, int cost, const sv_refine_params& p,
                   int16_t* out, int opitch, hipStream_t s) {
    sv::RefineArgs a{};
    a.L = L;
    a.R = R;
    a.H = H;
    a.W = W;
    a.pitch = pitch;
    a.dl = dl;
    a.dr = p.lr_max_diff >= 0 ? dr : nullptr;
    a.out = out;
    a.mpitch = opitch;
    a.minD = min_disp;
    a.D = num_disp;
    a.r = win / 2;
    a.lr_max_diff = p.lr_max_diff;
    a.min_curv = p.min_curvature;
    a.subpixel = p.subpixel ? 1 : 0;
    c->scratch_written(out);
    SV_LAUNCH(c, SV_K_REFINE, s, sv::launch_refine(a, cost, s));
    return enqueue_speckles(c, out, H, W, opitch, (min_disp - 1) * 16, p.speckle_window, 16 * p.speckle_range, s);
}

int enqueue_refined(sv_ctx* c, const uint8_t* L, const uint8_t* R, int H, int W, int pitch, int min_disp,
                    int num_disp, int win, int cost, const sv_refine_params& p, int16_t* out, int opitch,
                    hipStream_t s) {
    int rc = enqueue_disparity(c, L, R, H, W, pitch, min_disp, num_disp, win, cost, 0, H, out, opitch, s);
    if (rc) return rc;
    const int16_t* dr = nullptr;
    if (p.lr_max_diff >= 0) {
        SV_HIP(c->rf_right.ensure((size_t)H * opitch * sizeof(int16_t)));
        rc = enqueue_right(c, L, R, H, W, pitch, min_disp, num_disp, win, cost, c->rf_right.as<int16_t>(), opitch, s);
        if (rc) return rc;
        dr = c->rf_right.as<int16_t>();
    }
    return enqueue_refine(c, L, R, H, W, pitch, out, dr, min_disp, num_disp, win, cost, p, out, opitch, s);
}

}  // namespace

extern "C" {

int sv_refine_plan(int num_disp, int win, int* lds_bytes, int* lds_form) {
    if (num_disp <= 0 || num_disp > 512) return fail(SV_EINVAL, "num_disp must be in [1, 512]");
    if (check_win(win)) return SV_EINVAL;
    if (lds_bytes) *lds_bytes = (int)sv::refine_lds_bytes(num_disp, win);
    if (lds_form) *lds_form = sv::refine_lds_form(num_disp, win) ? 1 : 0;
    return 0;
}

int sv_disparity_right_dev(sv_ctx* c, const uint8_t* d_left, const uint8_t* d_right, int H, int W, int pitch,
                           int min_disp, int num_disp, int win, int cost, int16_t* d_disp16_right, int out_pitch,
                           void* stream) {
    SV_ENTER(c);
    if (!d_disp16_right) return fail(SV_EINVAL, "null disparity output");
    const int rc = check_stage(d_left, d_right, H, W, pitch, out_pitch, min_disp, num_disp, win, cost);
    if (rc) return rc;
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    return enqueue_right(c, d_left, d_right, H, W, pitch, min_disp, num_disp, win, cost, d_disp16_right, out_pitch,
                         s);
}

int sv_refine_dev(sv_ctx* c, const uint8_t* d_left, const uint8_t* d_right, int H, int W, int pitch,
                  const int16_t* d_disp16, const int16_t* d_disp16_right, int min_disp, int num_disp, int win,
                  int cost, const sv_refine_params* params, int16_t* d_out16, int out_pitch, void* stream) {
    SV_ENTER(c);
    if (!d_disp16 || !d_out16) return fail(SV_EINVAL, "null disparity map");
    if (d_disp16_right && d_disp16_right == d_out16)
        return fail(SV_EINVAL, "the right-referenced map cannot be refined in place");
    int rc = check_stage(d_left, d_right, H, W, pitch, out_pitch, min_disp, num_disp, win, cost);
    if (!rc) rc = check_params(params, cost);
    if (rc) return rc;
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    return enqueue_refine(c, d_left, d_right, H, W, pitch, d_disp16, d_disp16_right, min_disp, num_disp, win, cost,
                          *params, d_out16, out_pitch, s);
}

int sv_disparity_refined_dev(sv_ctx* c, const uint8_t* d_left, const uint8_t* d_right, int H, int W, int pitch,
                             int min_disp, int num_disp, int win, int cost, const sv_refine_params* params,
                             int16_t* d_out16, int out_pitch, void* stream) {
    SV_ENTER(c);
    if (!d_out16) return fail(SV_EINVAL, "null disparity output");
    int rc = check_stage(d_left, d_right, H, W, pitch, out_pitch, min_disp, num_disp, win, cost);
    if (!rc) rc = check_params(params, cost);
    if (rc) return rc;
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    return enqueue_refined(c, d_left, d_right, H, W, pitch, min_disp, num_disp, win, cost, *params, d_out16,
                           out_pitch, s);
}

int sv_disparity_refined(sv_ctx* c, const uint8_t* left, const uint8_t* right, int H, int W, int channels,
                         int stride, int min_disp, int num_disp, int win, int cost, const sv_refine_params* params,
                         int16_t* disp16) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (!disp16) return fail(SV_EINVAL, "null disparity output");
    int rc = check_stage(left, right, H, W, W, W, min_disp, num_disp, win, cost);
    if (!rc) rc = check_params(params, cost);
    if (rc) return rc;
    rc = stage_pair(c, left, right, H, W, channels, stride);
    if (rc) return rc;
    SV_HIP(c->d16.ensure((size_t)H * W * sizeof(int16_t)));
    rc = enqueue_refined(c, c->gray[0].as<uint8_t>(), c->gray[1].as<uint8_t>(), H, W, W, min_disp, num_disp, win,
                         cost, *params, c->d16.as<int16_t>(), W, c->stream);
    if (rc) return rc;
    Out o[] = {{disp16, c->d16.p, (size_t)H * W * sizeof(int16_t)}};
    return collect(c, o, 1);
}

}  // extern "C"
