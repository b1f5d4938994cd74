// sv_capi_census.cpp — the C ABI of the census / Hamming cost on device memory
// (include/stereovision_amd.h): the transform of one gray image and the fused
// matcher over two caller-supplied code planes.  Kernels: sv_census.hip.  cost = SV_COST_CENSUS
// of every other entry point runs both through enqueue_disparity (sv_capi.cpp).
#include "sv_ctx.h"

extern "C" {

int sv_census_dev(sv_ctx* c, const uint8_t* d_gray, int H, int W, int pitch, int row0, int row1, uint64_t* d_codes,
                  int code_pitch, void* stream) {
    SV_ENTER(c);
    if (check_image(d_gray, H, W)) return SV_EINVAL;
    if (!d_codes) return fail(SV_EINVAL, "null census output");
    if (pitch < W || code_pitch < W) return fail(SV_EINVAL, "pitch smaller than width");
    if (row0 < 0) row0 = 0;
    if (row1 > H) row1 = H;
    if (row1 <= row0) return 0;
    hipStream_t s = pick(c, stream);
    sv::CensusArgs a{};
    a.g0 = a.g1 = d_gray;
    a.H = H;
    a.W = W;
    a.pitch = pitch;
    a.y0 = row0;
    a.y1 = row1;
    a.c0 = a.c1 = d_codes;
    a.cpitch = code_pitch;
    a.nz = 1;
    SV_LAUNCH(c, SV_K_CENSUS, s, sv::launch_census(a, s));
    return 0;
}

int sv_census_match_dev(sv_ctx* c, const uint64_t* d_codes_left, const uint64_t* d_codes_right, int H, int W,
                        int code_pitch, int min_disp, int num_disp, int win, int row0, int row1, int16_t* d_disp16,
                        int out_pitch, void* stream) {
    SV_ENTER(c);
    if (check_image(d_codes_left, H, W) || check_image(d_codes_right, H, W)) return SV_EINVAL;
    if (!d_disp16) return fail(SV_EINVAL, "null disparity output");
    if (code_pitch < W || out_pitch < W) return fail(SV_EINVAL, "pitch smaller than width");
    sv::MatchPlan plan;
    const int rc = check_match(H, W, min_disp, num_disp, win, SV_COST_CENSUS, &plan);
    if (rc) return rc;
    if (row0 < 0) row0 = 0;
    if (row1 > H) row1 = H;
    if (row1 <= row0) return 0;
    hipStream_t s = pick(c, stream);
    return enqueue_census_match(c, d_codes_left, d_codes_right, H, W, code_pitch, min_disp, num_disp, win, row0, row1,
                                d_disp16, out_pitch, s);
}

}  // extern "C"
