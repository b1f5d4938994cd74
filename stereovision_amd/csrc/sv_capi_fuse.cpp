// sv_capi_fuse.cpp — fuse_depth_maps in the C ABI (Gaussian blur, bilateral filter, blend) and its flow
// input (Farneback flow, flow depth, flow grid), which shares gauss_coef and c->fuse's accumulators.
#include "sv_ctx.h"

extern "C" {

// c->fuse: the launch's accumulator copies, then the bilateral colour table
constexpr size_t kFuseLutOff = sv::kFuseStatsBytes;
constexpr size_t kFuseBytes = kFuseLutOff + sv::kBilateralLut * sizeof(float);

// ksize odd in [3, 31] and the map larger than the radius; fills c[0..r] centre first
static int gauss_coef(const float* coef, int ksize, int H, int W, float* c) {
    if (ksize < 3 || ksize > 31 || ksize % 2 == 0) return fail(SV_EINVAL, "Gaussian ksize must be odd in [3, 31]");
    if (!coef) return fail(SV_EINVAL, "null Gaussian coefficients");
    const int r = ksize / 2;
    if (H <= r || W <= r) return fail(SV_EINVAL, "map not larger than the Gaussian radius (H, W > ksize / 2)");
    for (int i = 0; i < 16; ++i) c[i] = i <= r ? coef[r + i] : 0.f;
    return 0;
}

// The accumulator slots of the launch just enqueued on s: copied back, waited for, folded into w.
static int read_fuse_stats(sv_ctx* c, const uint32_t* d_stats, hipStream_t s, uint32_t w[4]) {
    uint32_t slots[sv::kFuseSlots * sv::kFuseSlotStride];
    SV_HIP(c->copy(slots, d_stats, sizeof(slots), hipMemcpyDeviceToHost, s));
    SV_HIP(hipStreamSynchronize(s));
    sv::fuse_stats_fold(slots, w);
    return 0;
}

int sv_gauss_blur_f32_dev(sv_ctx* c, const float* d_src, int H, int W, const float* coef, int ksize, float* d_dst,
                          void* stream) {
    SV_ENTER(c);
    if (!d_src || !d_dst || d_src == d_dst || H <= 0 || W <= 0) return fail(SV_EINVAL, "bad Gaussian blur arguments");
    sv::GaussArgs a{};
    int rc = gauss_coef(coef, ksize, H, W, a.c);
    if (rc) return rc;
    a.src = d_src;
    a.dst = d_dst;
    a.H = H;
    a.W = W;
    a.r = ksize / 2;
    hipStream_t s = pick(c, stream);
    SV_LAUNCH(c, SV_K_FUSE, s, sv::launch_gauss_f32(a, s));
    return 0;
}

int sv_bilateral_f32_dev(sv_ctx* c, const float* d_src, int H, int W, int radius, const float* space_w,
                         const float* lut, float scale, float* d_dst_f32, uint8_t* d_dst_u8, uint8_t* d_dst_bgr,
                         const uint8_t* cmap_bgr, float* minmax_out, void* stream) {
    SV_ENTER(c);
    if (!d_src || H <= 0 || W <= 0) return fail(SV_EINVAL, "bad bilateral filter arguments");
    if (radius < 0 || radius > sv::kBilateralMaxR) return fail(SV_EINVAL, "bilateral radius must be in [0, 7]");
    if (radius > 0 && (!space_w || !lut)) return fail(SV_EINVAL, "null bilateral tables");
    if (radius > 0 && (H <= radius || W <= radius))
        return fail(SV_EINVAL, "map not larger than the bilateral radius (H, W > radius)");
    if (!d_dst_f32 && !d_dst_u8 && !d_dst_bgr && !minmax_out) return fail(SV_EINVAL, "no bilateral output");
    if (d_dst_f32 == d_src) return fail(SV_EINVAL, "bilateral filter in place");
    if (d_dst_bgr && !cmap_bgr) return fail(SV_EINVAL, "colormap output without a table");
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    SV_HIP(c->fuse.ensure(kFuseBytes));
    sv::BilateralArgs a{};
    a.src = d_src;
    a.H = H;
    a.W = W;
    a.r = radius;
    a.scale = scale;
    a.dst_f32 = d_dst_f32;
    a.dst_u8 = d_dst_u8;
    if (d_dst_bgr) {
        sv::PostParams pp{};
        int rc = attach_cmap(c, pp, cmap_bgr, d_dst_bgr, s);
        if (rc) return rc;
        a.dst_bgr = pp.out_bgr;
        a.cmap = pp.cmap;
    }
    if (d_dst_u8 || d_dst_bgr || minmax_out) {
        a.stats = c->fuse.as<uint32_t>();
        SV_HIP(hipMemsetAsync(a.stats, 0, sv::kFuseStatsBytes, s));
    }
    if (radius > 0) {
        float* d_lut = reinterpret_cast<float*>(c->fuse.as<char>() + kFuseLutOff);
        SV_HIP(c->copy(d_lut, lut, sv::kBilateralLut * sizeof(float), hipMemcpyHostToDevice, s));
        SV_HIP(hipStreamSynchronize(s));   // the caller's table may go once this call returns
        a.lut = d_lut;
    }
    SV_LAUNCH(c, SV_K_FUSE, s, sv::launch_bilateral_f32(a, space_w, s));
    if (minmax_out) {
        uint32_t w[4];
        if (const int rc = read_fuse_stats(c, a.stats, s, w)) return rc;
        minmax_out[0] = sv::fuse_stat_min(w);
        minmax_out[1] = sv::fuse_stat_max(w);
    }
    return 0;
}

int sv_fuse_blend_dev(sv_ctx* c, const sv_fuse_args* g, float* d_fused, sv_fuse_stats* stats, void* stream) {
    SV_ENTER(c);
    if (!g || !d_fused) return fail(SV_EINVAL, "null fuse arguments");
    if (g->H <= 0 || g->W <= 0) return fail(SV_EINVAL, "bad fuse map size");
    if (g->base < 0 || g->base > 2) return fail(SV_EINVAL, "fuse base must be 0 (stereo), 1 (midas) or 2 (flow)");
    const bool mfill = g->midas_fill != 0, ffill = g->flow_fill != 0;
    if (mfill && g->base != sv::FUSE_BASE_STEREO) return fail(SV_EINVAL, "midas fill needs the stereo base");
    if (ffill && g->base == sv::FUSE_BASE_FLOW) return fail(SV_EINVAL, "flow fill on the flow base");
    if ((g->base == sv::FUSE_BASE_STEREO && !g->d_stereo) || ((g->base == sv::FUSE_BASE_MIDAS || mfill) && !g->d_midas) ||
        ((g->base == sv::FUSE_BASE_FLOW || ffill) && !g->d_flow))
        return fail(SV_EINVAL, "null fuse input map");
    sv::FuseBlendArgs a{};
    if (mfill) {
        int rc = gauss_coef(g->coef, g->ksize, g->H, g->W, a.c);
        if (rc) return rc;
        a.r = g->ksize / 2;
    }
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    SV_HIP(c->fuse.ensure(kFuseBytes));
    a.stereo = g->d_stereo;
    a.conf = g->d_conf;
    a.midas = g->d_midas;
    a.flow = g->d_flow;
    a.fused = d_fused;
    a.stats = c->fuse.as<uint32_t>();
    a.H = g->H;
    a.W = g->W;
    a.base = g->base;
    a.midas_fill = mfill;
    a.flow_fill = ffill;
    a.sw = g->stereo_weight;
    a.mfw = g->midas_fill_weight;
    a.thr = g->conf_threshold;
    a.hthr = g->hole_threshold;
    a.k1 = g->flow_k1;
    a.k2 = g->flow_k2;
    SV_HIP(hipMemsetAsync(a.stats, 0, sv::kFuseStatsBytes, s));
    SV_LAUNCH(c, SV_K_FUSE, s, sv::launch_fuse_blend(a, s));
    if (stats) {
        uint32_t w[4];
        if (const int rc = read_fuse_stats(c, a.stats, s, w)) return rc;
        stats->min = sv::fuse_stat_min(w);
        stats->max = sv::fuse_stat_max(w);
        stats->n_midas = w[2];
        stats->n_hole = w[3];
    }
    return 0;
}

// ---------------------------------------------------------------- Farneback optical flow
static int fb_poly_tables(int poly_n, const float* g, const float* xg, const float* xxg, const double* ig,
                          sv::FbPolyArgs* a) {
    if (poly_n != 5 && poly_n != 7) return fail(SV_EINVAL, "poly_n must be 5 or 7");
    if (!g || !xg || !xxg || !ig) return fail(SV_EINVAL, "null polynomial expansion tables");
    a->n = poly_n;
    for (int i = 0; i <= poly_n; ++i) {
        a->g[i] = g[i];
        a->xg[i] = xg[i];
        a->xxg[i] = xxg[i];
    }
    a->ig11 = ig[0];
    a->ig03 = ig[1];
    a->ig33 = ig[2];
    a->ig55 = ig[3];
    return 0;
}

static int fb_winsize(int winsize) {
    if (winsize < 3 || winsize > sv::kFbMaxWin || winsize % 2 == 0)
        return fail(SV_EINVAL, "winsize must be odd in [3, 31]");
    return 0;
}

int sv_fb_polyexp_dev(sv_ctx* c, const float* d_img, int H, int W, int poly_n, const float* g, const float* xg,
                      const float* xxg, const double ig[4], float* d_R, void* stream) {
    SV_ENTER(c);
    if (!d_img || !d_R || H <= 0 || W <= 0) return fail(SV_EINVAL, "bad polynomial expansion arguments");
    sv::FbPolyArgs a{};
    int rc = fb_poly_tables(poly_n, g, xg, xxg, ig, &a);
    if (rc) return rc;
    a.src = d_img;
    a.R = d_R;
    a.plane = (size_t)H * W;
    a.H = H;
    a.W = W;
    hipStream_t s = pick(c, stream);
    SV_LAUNCH(c, SV_K_FLOW, s, sv::launch_fb_polyexp(a, s));
    return 0;
}

int sv_fb_update_matrices_dev(sv_ctx* c, const float* d_R0, const float* d_R1, const float* d_flow, int H, int W,
                              float* d_M, void* stream) {
    SV_ENTER(c);
    if (!d_R0 || !d_R1 || !d_flow || !d_M || H <= 0 || W <= 0)
        return fail(SV_EINVAL, "bad update-matrices arguments");
    sv::FbUpdateArgs a{d_R0, d_R1, d_flow, d_M, (size_t)H * W, H, W};
    hipStream_t s = pick(c, stream);
    SV_LAUNCH(c, SV_K_FLOW, s, sv::launch_fb_update_matrices(a, s));
    return 0;
}

int sv_fb_blur_solve_dev(sv_ctx* c, const float* d_M, int H, int W, int winsize, float* d_flow, int interleaved,
                         void* stream) {
    SV_ENTER(c);
    if (!d_M || !d_flow || H <= 0 || W <= 0) return fail(SV_EINVAL, "bad blur-solve arguments");
    int rc = fb_winsize(winsize);
    if (rc) return rc;
    sv::FbSolveArgs a{d_M, (size_t)H * W, d_flow, interleaved ? 1 : 0, H, W, winsize / 2,
                      1.0 / ((double)winsize * winsize)};
    hipStream_t s = pick(c, stream);
    SV_LAUNCH(c, SV_K_FLOW, s, sv::launch_fb_blur_solve(a, s));
    return 0;
}

int sv_farneback_flow_dev(sv_ctx* c, const uint8_t* d_prev, const uint8_t* d_next, int H, int W, int pitch,
                          const sv_farneback_params* p, float* d_flow, void* stream) {
    SV_ENTER(c);
    if (!d_prev || !d_next || !d_flow || !p) return fail(SV_EINVAL, "null optical-flow arguments");
    if (H < 16 || W < 16) return fail(SV_EINVAL, "optical flow needs H, W >= 16");
    if (pitch < W) return fail(SV_EINVAL, "pitch smaller than a row");
    if (p->n_scales < 1 || p->n_scales > SV_FB_MAX_SCALES) return fail(SV_EINVAL, "1..16 pyramid scales");
    if (!p->scale_h || !p->scale_w || !p->scale_ksize || !p->scale_coef)
        return fail(SV_EINVAL, "null pyramid tables");
    if (p->iterations < 1) return fail(SV_EINVAL, "iterations must be >= 1");
    int rc = fb_winsize(p->winsize);
    if (rc) return rc;
    sv::FbPolyArgs poly{};
    rc = fb_poly_tables(p->poly_n, p->poly_g, p->poly_xg, p->poly_xxg, p->ig, &poly);
    if (rc) return rc;
    if (p->scale_h[0] != H || p->scale_w[0] != W) return fail(SV_EINVAL, "pyramid scale 0 must be H x W");
    sv::GaussArgs blur[SV_FB_MAX_SCALES];
    for (int k = 0; k < p->n_scales; ++k) {
        const int h = p->scale_h[k], w = p->scale_w[k];
        if (h < 1 || w < 1 || (k > 0 && (h > p->scale_h[k - 1] || w > p->scale_w[k - 1])))
            return fail(SV_EINVAL, "pyramid scales must be positive and not grow");
        blur[k] = sv::GaussArgs{};
        rc = gauss_coef(p->scale_coef + 32 * k, p->scale_ksize[k], H, W, blur[k].c);
        if (rc) return rc;
        blur[k].H = H;
        blur[k].W = W;
        blur[k].r = p->scale_ksize[k] / 2;
    }
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    // floats: two converted frames, the blurred frame, the level image, R0, R1, M, two flows
    const size_t N = (size_t)H * W;
    SV_HIP(c->flow.ensure(23 * N * sizeof(float)));
    float* base = c->flow.as<float>();
    float* fimg[2] = {base, base + N};
    float* blurred = base + 2 * N;
    float* level = base + 3 * N;
    float* R[2] = {base + 4 * N, base + 9 * N};
    float* M = base + 14 * N;
    float* fl[2] = {base + 19 * N, base + 21 * N};
    const uint8_t* frames[2] = {d_prev, d_next};
    for (int i = 0; i < 2; ++i) SV_LAUNCH(c, SV_K_FLOW, s, sv::launch_fb_u8_f32(frames[i], H, W, pitch, fimg[i], s));
    int cur = 0;
    for (int k = p->n_scales - 1; k >= 0; --k, cur ^= 1) {
        const int h = p->scale_h[k], w = p->scale_w[k];
        const size_t n = (size_t)h * w;
        float* flow = fl[cur];
        if (k == p->n_scales - 1) {
            SV_HIP(hipMemsetAsync(flow, 0, 2 * n * sizeof(float), s));
        } else {
            const int ph = p->scale_h[k + 1], pw = p->scale_w[k + 1];
            const float* prev = fl[cur ^ 1];
            for (int comp = 0; comp < 2; ++comp)
                SV_LAUNCH(c, SV_K_FLOW, s,
                          sv::launch_resize_linear(prev + comp * (size_t)ph * pw, ph, pw, 1, pw * 4, 0, flow + comp * n,
                                                   h, w, w * 4, 0, 1, true, s));
            SV_LAUNCH(c, SV_K_FLOW, s, sv::launch_fb_scale(flow, 2 * n, p->flow_scale, s));
        }
        for (int i = 0; i < 2; ++i) {
            sv::GaussArgs g = blur[k];
            g.src = fimg[i];
            g.dst = blurred;
            SV_LAUNCH(c, SV_K_FLOW, s, sv::launch_gauss_f32(g, s));
            const float* img = blurred;
            if (h != H || w != W) {
                SV_LAUNCH(c, SV_K_FLOW, s,
                          sv::launch_resize_linear(blurred, H, W, 1, W * 4, 0, level, h, w, w * 4, 0, 1, true, s));
                img = level;
            }
            sv::FbPolyArgs a = poly;
            a.src = img;
            a.R = R[i];
            a.plane = n;
            a.H = h;
            a.W = w;
            SV_LAUNCH(c, SV_K_FLOW, s, sv::launch_fb_polyexp(a, s));
        }
        sv::FbUpdateArgs u{R[0], R[1], flow, M, n, h, w};
        SV_LAUNCH(c, SV_K_FLOW, s, sv::launch_fb_update_matrices(u, s));
        for (int it = 0; it < p->iterations; ++it) {
            const bool last = k == 0 && it == p->iterations - 1;
            sv::FbSolveArgs b{M, n, last ? d_flow : flow, last ? 1 : 0, h, w, p->winsize / 2,
                              1.0 / ((double)p->winsize * p->winsize)};
            SV_LAUNCH(c, SV_K_FLOW, s, sv::launch_fb_blur_solve(b, s));
            if (it < p->iterations - 1) SV_LAUNCH(c, SV_K_FLOW, s, sv::launch_fb_update_matrices(u, s));
        }
    }
    return 0;
}

int sv_flow_depth_dev(sv_ctx* c, const float* d_flow, int H, int W, const double Hm[9], float* d_depth,
                      float* d_stable, float alpha, float one_minus_alpha, float* minmax_out, void* stream) {
    SV_ENTER(c);
    if (!d_flow || !d_depth || !Hm || H <= 0 || W <= 0) return fail(SV_EINVAL, "bad flow-depth arguments");
    if (d_stable == d_depth) return fail(SV_EINVAL, "flow depth: stable map aliases the depth map");
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    SV_HIP(c->fuse.ensure(kFuseBytes));
    sv::FlowDepthArgs a{};
    a.flow = d_flow;
    a.depth = d_depth;
    a.stable = d_stable;
    a.stats = c->fuse.as<uint32_t>();
    a.H = H;
    a.W = W;
    for (int i = 0; i < 9; ++i) a.m[i] = Hm[i];
    a.alpha = alpha;
    a.beta = one_minus_alpha;
    SV_HIP(hipMemsetAsync(a.stats, 0, sv::kFuseStatsBytes, s));
    SV_LAUNCH(c, SV_K_FLOW, s, sv::launch_flow_depth(a, s));
    if (minmax_out) {
        uint32_t w[4];
        if (const int rc = read_fuse_stats(c, a.stats, s, w)) return rc;
        minmax_out[0] = sv::fuse_stat_min(w);
        minmax_out[1] = sv::fuse_stat_max(w);
    }
    return 0;
}

int sv_flow_grid_dev(sv_ctx* c, const float* d_flow, int H, int W, int step, float* d_out, void* stream) {
    SV_ENTER(c);
    if (!d_flow || !d_out || H <= 0 || W <= 0 || step < 1) return fail(SV_EINVAL, "bad flow-grid arguments");
    if ((((uintptr_t)d_flow) | ((uintptr_t)d_out)) & 7) return fail(SV_EINVAL, "flow grid: pointers must be 8-byte aligned");
    hipStream_t s = pick(c, stream);
    SV_LAUNCH(c, SV_K_FLOW, s, sv::launch_flow_grid(d_flow, H, W, step, d_out, s));
    return 0;
}

}  // extern "C"
