// sv_capi_dev.cpp — the stereo entry points of the C ABI on device memory (frames resident in HBM):
// gray, disparity, median, post, their batch forms, Harris, HOG, SGBM-3WAY and the speckle filter.
#include "sv_ctx.h"

extern "C" {

int sv_gray_dev(sv_ctx* c, const uint8_t* d_bgr, int H, int W, int pitch, uint8_t* d_gray, void* stream) {
    SV_ENTER(c);
    if (check_image(d_bgr, H, W) || !d_gray) return fail(SV_EINVAL, "bad gray arguments");
    hipStream_t s = pick(c, stream);
    SV_LAUNCH(c, SV_K_GRAY, s, sv::launch_gray(d_bgr, H, W, pitch, d_gray, s));
    return 0;
}

int sv_disparity_dev(sv_ctx* c, const uint8_t* d_left, const uint8_t* d_right, int H, int W, int pitch,
                     int min_disp, int num_disp, int win, int cost, int row0, int row1, int16_t* d_disp16,
                     int out_pitch, void* stream) {
    SV_ENTER(c);
    if (check_image(d_left, H, W) || check_image(d_right, H, W) || !d_disp16)
        return fail(SV_EINVAL, "bad disparity arguments");
    if (pitch < W || out_pitch < W) return fail(SV_EINVAL, "pitch smaller than width");
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    return enqueue_disparity(c, d_left, d_right, H, W, pitch, min_disp, num_disp, win, cost, row0, row1,
                             d_disp16, out_pitch, s);
}

int sv_median_rows_dev(sv_ctx* c, const int16_t* d_disp16, int H, int W, int row0, int row1, int min_disp,
                       int num_disp, int cost, const sv_map_out* out, void* stream) {
    SV_ENTER(c);
    if (check_image(d_disp16, H, W)) return fail(SV_EINVAL, "bad median arguments");
    if ((long long)H * W >= (1LL << 30)) return fail(SV_EINVAL, "frame too large for the median kernel");
    if (row0 < 0) row0 = 0;
    if (row1 > H) row1 = H;
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    sv::PostParams pp;
    float* disp = nullptr;
    int rc = map_out_post(c, out, min_disp, num_disp, cost, false, s, &pp, &disp);
    if (rc) return rc;
    SV_LAUNCH(c, SV_K_MEDIAN, s, sv::launch_median_i16(d_disp16, H, W, row0, row1, disp, pp, s));
    return 0;
}

int sv_post_m16_dev(sv_ctx* c, const int16_t* d_med16, int64_t n, int mode, float min_depth, float max_depth,
                    float depth_range, float min_disp_global, int min_disp, int num_disp, float* d_disparity,
                    float* d_out_a, uint8_t* d_out_u8, float* d_out_b, void* stream) {
    SV_ENTER(c);
    if (n < 0 || (n > 0 && !d_med16)) return fail(SV_EINVAL, "bad median map");
    if (mode != SV_POST_NONE && mode != SV_POST_DEPTH && mode != SV_POST_SCALED) return fail(SV_EINVAL, "bad mode");
    if (mode == SV_POST_NONE && !d_disparity) return fail(SV_EINVAL, "no outputs");
    if (mode == SV_POST_DEPTH && (!d_out_a || !d_out_u8)) return fail(SV_EINVAL, "depth post outputs missing");
    if (mode == SV_POST_SCALED && (!d_out_a || !d_out_u8 || !d_out_b || num_disp <= 0))
        return fail(SV_EINVAL, "scaled post outputs missing");
    if (n == 0) return 0;
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    sv::PostParams pp = make_post(mode, min_depth, max_depth, depth_range, min_disp_global, min_disp, num_disp,
                                  d_out_a, d_out_u8, d_out_b);
    int rc = attach_lut(c, pp, s);
    if (rc) return rc;
    SV_LAUNCH(c, SV_K_POST, s, sv::launch_post_m16(d_med16, (long long)n, d_disparity, pp, s));
    return 0;
}

int sv_disparity_batch_dev(sv_ctx* c, const uint8_t* d_left, const uint8_t* d_right, int n_frames, int H,
                           int W, int pitch, int64_t frame_stride, int min_disp, int num_disp, int win,
                           int cost, int16_t* d_disp16, int out_pitch, int64_t out_frame_stride,
                           void* stream) {
    SV_ENTER(c);
    if (check_image(d_left, H, W) || check_image(d_right, H, W) || !d_disp16 || n_frames < 0)
        return fail(SV_EINVAL, "bad disparity arguments");
    if (pitch < W || out_pitch < W) return fail(SV_EINVAL, "pitch smaller than width");
    if (check_frame_stride(n_frames, frame_stride, (int64_t)pitch * H) ||
        check_frame_stride(n_frames, out_frame_stride, (int64_t)out_pitch * H)) return SV_EINVAL;
    if (n_frames == 0) return 0;
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    return enqueue_disparity(c, d_left, d_right, H, W, pitch, min_disp, num_disp, win, cost, 0, H, d_disp16,
                             out_pitch, s, n_frames, frame_stride, out_frame_stride);
}

int sv_depth_map_batch_dev(sv_ctx* c, const uint8_t* d_left, const uint8_t* d_right, int n_frames, int H, int W,
                           int pitch, int64_t frame_stride, int min_disp, int num_disp, int win, int cost, int stages,
                           int16_t* d_disp16, const sv_map_out* out, void* stream) {
    SV_ENTER(c);
    if (stages != SV_STAGE_ALL && stages != SV_STAGE_MATCH && stages != SV_STAGE_MEDIAN)
        return fail(SV_EINVAL, "stages must be SV_STAGE_MATCH, SV_STAGE_MEDIAN or SV_STAGE_ALL");
    const bool match = stages & SV_STAGE_MATCH, median = stages & SV_STAGE_MEDIAN;
    if (n_frames < 0 || H <= 0 || W <= 0) return fail(SV_EINVAL, "bad depth-map arguments");
    if (match && (check_image(d_left, H, W) || check_image(d_right, H, W)))
        return fail(SV_EINVAL, "bad depth-map arguments");
    if (!d_disp16 && stages != SV_STAGE_ALL)
        return fail(SV_EINVAL, "the stages run apart exchange the int16 maps through d_disp16");
    if (median && !out) return fail(SV_EINVAL, "null outputs");
    if (median && out->harris && check_image(d_left, H, W)) return fail(SV_EINVAL, "Harris needs the left frames");
    if (pitch < W) return fail(SV_EINVAL, "pitch smaller than width");
    if (check_frame_stride(n_frames, frame_stride, (int64_t)pitch * H)) return SV_EINVAL;
    if ((long long)H * W >= (1LL << 30)) return fail(SV_EINVAL, "frame too large for the median kernel");
    if (n_frames == 0) return 0;
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    const long long fs = (long long)H * W;
    int16_t* d16 = d_disp16;
    if (!d16) {
        SV_HIP(c->d16.ensure((size_t)n_frames * fs * sizeof(int16_t)));
        d16 = c->d16.as<int16_t>();
    }
    if (match) {
        // (the scratch map's invalid margins are written once per geometry: d16_margins)
        const int rc = enqueue_disparity(c, d_left, d_right, H, W, pitch, min_disp, num_disp, win, cost, 0, H, d16, W,
                                         s, n_frames, frame_stride, fs, !d_disp16);
        if (rc) return rc;
    }
    if (!median) return 0;
    sv::PostParams pp;
    float* disp = nullptr;
    int rc = map_out_post(c, out, min_disp, num_disp, cost, true, s, &pp, &disp);
    if (rc) return rc;
    // the maps are this call's own integer-matcher output and the whole-disparity table covers
    // every value they can hold: the epilogue looks up unchecked.  Maps handed in (the median
    // stage alone) and SGBM's keep the checked form
    pp.lut_unchecked = match && cost != SV_COST_SGBM && pp.lut_shift == 4 && pp.lut_m0 == (min_disp - 1) * 16 &&
                       pp.lut_n == num_disp + 1;
    const long long fin = n_frames > 1 ? frame_stride : 0;
    if (out->harris && (W < 8 || H < 8)) {   // the DPP form needs 8 px a side: a launch of its own
        SV_LAUNCH(c, SV_K_MEDIAN, s, sv::launch_median_i16(d16, H, W, 0, H, disp, pp, s, n_frames, fs, fs));
        SV_LAUNCH(c, SV_K_HARRIS, s, sv::launch_harris(d_left, H, W, pitch, out->harris, s, n_frames, fin, fs));
        return 0;
    }
    // the Harris response rides in the median launch (extra blocks)
    sv::HarrisParams hp{d_left, pitch, fin, out->harris, fs, 0, 0};
    SV_LAUNCH(c, SV_K_MEDIAN, s,
              sv::launch_median_i16(d16, H, W, 0, H, disp, pp, s, n_frames, fs, fs, out->harris ? &hp : nullptr));
    return 0;
}

int sv_harris_dev(sv_ctx* c, const uint8_t* d_gray, int H, int W, int pitch, float* d_out, void* stream) {
    SV_ENTER(c);
    if (check_image(d_gray, H, W) || !d_out) return fail(SV_EINVAL, "bad harris arguments");
    hipStream_t s = pick(c, stream);
    SV_LAUNCH(c, SV_K_HARRIS, s, sv::launch_harris(d_gray, H, W, pitch, d_out, s));
    return 0;
}

int sv_harris_batch_dev(sv_ctx* c, const uint8_t* d_gray, int n_frames, int H, int W, int pitch,
                        int64_t frame_stride, float* d_out, void* stream) {
    SV_ENTER(c);
    if (check_image(d_gray, H, W) || !d_out || n_frames < 0) return fail(SV_EINVAL, "bad harris arguments");
    if (pitch < W) return fail(SV_EINVAL, "pitch smaller than width");
    if (check_frame_stride(n_frames, frame_stride, (int64_t)pitch * H)) return SV_EINVAL;
    if (n_frames == 0) return 0;
    hipStream_t s = pick(c, stream);
    SV_LAUNCH(c, SV_K_HARRIS, s,
              sv::launch_harris(d_gray, H, W, pitch, d_out, s, n_frames, (long long)frame_stride,
                                (long long)H * W));
    return 0;
}

int sv_hog_hist_dev(sv_ctx* c, const uint8_t* d_gray, int H, int W, int pitch, int win, int row0, int row1,
                    uint16_t* d_out, void* stream) {
    SV_ENTER(c);
    if (check_image(d_gray, H, W) || !d_out) return fail(SV_EINVAL, "bad hog arguments");
    if (check_win(win)) return SV_EINVAL;
    hipStream_t s = pick(c, stream);
    SV_LAUNCH(c, SV_K_HOG, s, sv::launch_hog_hist(d_gray, H, W, pitch, win, row0, row1, d_out, s));
    return 0;
}

// ---------------------------------------------------------------- SGBM-3WAY mode
int sv_sgbm_dev(sv_ctx* c, const uint8_t* d_left, const uint8_t* d_right, int H, int W, int pitch, int min_disp,
                int num_disp, int block_size, int P1, int P2, int disp12_max_diff, int pre_filter_cap,
                int uniqueness_ratio, int speckle_window_size, int speckle_range, int16_t* d_disp16, int out_pitch,
                void* stream) {
    SV_ENTER(c);
    sv::MatchPlan plan;
    int rc = check_match(H, W, min_disp, num_disp, block_size, SV_COST_SGBM, &plan);
    if (rc) return rc;
    if (check_image(d_left, H, W) || check_image(d_right, H, W) || !d_disp16 || pitch < W || out_pitch < W)
        return fail(SV_EINVAL, "bad SGBM arguments");
    SgbmParams p{P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio, speckle_window_size, speckle_range};
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    return enqueue_sgbm(c, d_left, d_right, H, W, pitch, min_disp, num_disp, block_size, p, d_disp16, out_pitch,
                        s);
}

// cv2.filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on an int16 map, in place.
int sv_filter_speckles_dev(sv_ctx* c, int16_t* d_img, int H, int W, int pitch, int new_val, int max_speckle_size,
                           int max_diff, void* stream) {
    SV_ENTER(c);
    if (!d_img || H <= 0 || W <= 0 || pitch < W) return fail(SV_EINVAL, "bad speckle-filter arguments");
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    return enqueue_speckles(c, d_img, H, W, pitch, new_val, max_speckle_size, max_diff, s);
}

}  // extern "C"
