// sv_capi_host.cpp — the stereo entry points of the C ABI on host buffers (the drop-ins' path,
// NumPy frames in and out), host-range registration, the host profile and host_frame_path.
#include "sv_ctx.h"

namespace {

// Host ranges registered through sv_host_register (page-locked and device-visible): the
// host-buffer frame path DMAs its outputs straight into them instead of expanding the int16
// medians on the host.
std::mutex g_reg_mu;
std::map<uintptr_t, size_t> g_reg;   // start -> bytes

bool host_registered(const void* p, size_t bytes) {
    if (!p) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> lk(g_reg_mu);
    auto it = g_reg.upper_bound(a);
    if (it == g_reg.begin()) return false;
    --it;
    return a >= it->first && a + bytes <= it->first + it->second;
}

// Host memory -> pinned staging -> device, in chunks: the DMA of one chunk runs while the
// host threads copy the next (one call per frame, as the reference calls the path).
// Rows [y0, y1) of a host image -> the pinned staging buffer (host pool threads) -> the
// device image (one async H2D per sub-chunk on the compute stream, so a sub-chunk's DMA
// overlaps the next one's copy).
int stage_rows(sv_ctx* c, const uint8_t* src, int y0, int y1, size_t row, int stride, uint8_t* stage, uint8_t* dev,
               int nsub) {
    // contiguous rows go to the device straight from the caller's pageable memory (the HIP
    // runtime's own pinned staging, pipelined with its DMA): measured faster than copying
    // into our pinned buffer on the pool threads (1080p create_depth_map 1.03-1.11k vs
    // 0.79-0.89k frames/s per call, 1.49-1.57k vs 0.72-1.18k with 4 in flight,
    // gpurun_out/host3; round 4 the same rates either way, profiles/r04_misc/
    // host_stage_ab_r04h.txt); strided rows take the pinned copy.
    if ((size_t)stride == row) {
        SV_HIP(c->copy(dev + (size_t)y0 * row, src + (size_t)y0 * row, (size_t)(y1 - y0) * row,
                       hipMemcpyHostToDevice, c->stream));
        return 0;
    }
    sv::HostPool& pool = sv::HostPool::get();
    for (int k = 0; k < nsub; ++k) {
        const int a0 = y0 + (int)((long long)(y1 - y0) * k / nsub), a1 = y0 + (int)((long long)(y1 - y0) * (k + 1) / nsub);
        if (a1 <= a0) continue;
        const int parts = pool.threads();
        pool.parallel_for(parts, [&](int p) {
            const int a = a0 + (int)((long long)(a1 - a0) * p / parts), b = a0 + (int)((long long)(a1 - a0) * (p + 1) / parts);
            if (b <= a) return;
            for (int y = a; y < b; ++y) std::memcpy(stage + (size_t)y * row, src + (size_t)y * stride, row);
        });
        SV_HIP(c->copy(dev + (size_t)a0 * row, stage + (size_t)a0 * row, (size_t)(a1 - a0) * row,
                       hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}

// Host copy of the context's post-processing table (the one attach_lut attached).
int host_lut(sv_ctx* c, const sv::PostParams& pp) {
    if (c->hl_valid && c->hl_key == c->lut_key) return 0;
    const size_t n = (size_t)pp.lut_n;
    try {
        c->hl_a.resize(n);
        c->hl_b.resize(n);
        c->hl_u8.resize(n);
    } catch (...) {
        return fail(SV_ENOMEM, "host table allocation failed");
    }
    SV_HIP(c->copy(c->hl_a.data(), pp.lut_a, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SV_HIP(c->copy(c->hl_b.data(), pp.lut_b, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SV_HIP(c->copy(c->hl_u8.data(), pp.lut_u8, n, hipMemcpyDeviceToHost, c->stream));
    SV_HIP(hipStreamSynchronize(c->stream));
    c->hl_key = c->lut_key;
    c->hl_valid = true;
    return 0;
}

struct FrameOut {
    float* a;        // DEPTH: depth_final; SCALED: disparity_normalized
    float* disp;     // disparity (f32 = median / 16)
    uint8_t* u8;     // DEPTH: depth_normalized; SCALED: its u8 image (nullable)
    float* b;        // SCALED: confidence
    uint8_t* bgr;    // colormap of u8 through `table` (nullable)
};

// create_depth_map / create_depth_map_stereo_scaled on host buffers (depth_map.py:868-937,
// fused_depth_map.py:976-1024): the frames go up in chunks, gray + disparity + median run on
// the device, and only the int16 x16 median map comes back (2 B/px).  The host expands it
// with the table the device built (bit-identical to the median kernel's epilogue, which
// reads the same table): disparity = m / 16, the post-processing outputs = table[m - m0],
// the colormap = table_bgr[u8].  Chunks of rows come back behind events, so the expansion
// of one chunk runs while the next is in flight.
// Pixels [a, b) of the host expansion: disparity = m / 16 (a power of two: exact), the f32
// output and u8 / BGR from the packed table entry.  The BGR triple goes out as one 4-byte
// store whose 4th byte the next pixel overwrites (same thread); the last pixel of the range
// stores 3 bytes, so ranges of different threads never overlap.  Returns the number of
// medians outside the table (left unwritten).
template <bool U8, bool SCALED, bool BGR>
int expand_rows(const int16_t* med, size_t a, size_t b, int m0, int nl, const HostEnt* ent, const float* lb,
                const FrameOut& o) {
    for (size_t i = a; i < b; ++i) o.disp[i] = (float)med[i] * 0.0625f;
    int nbad = 0;
    for (size_t i = a; i < b; ++i) {
        const uint32_t li = (uint32_t)(med[i] - m0);
        if (__builtin_expect(li >= (uint32_t)nl, 0)) {
            ++nbad;
            continue;
        }
        const HostEnt e = ent[li];
        o.a[i] = e.a;
        if (U8) o.u8[i] = (uint8_t)e.ubgr;
        if (SCALED) o.b[i] = lb[li];
        if (BGR) {
            const uint32_t v = e.ubgr >> 8;
            uint8_t* d = o.bgr + 3 * i;
            if (i + 1 < b) std::memcpy(d, &v, 4);
            else std::memcpy(d, &v, 3);
        }
    }
    return nbad;
}

// Host-side stage timings of the host-buffer path (sv_host_profile_enable / _read; the
// device side — uploads, kernels, downloads — is the context's own event profile,
// SV_K_H2D / SV_K_GRAY / SV_K_MATCH / SV_K_MEDIAN / SV_K_D2H).  SV_HOST_PROFILE=1 also prints
// the averages on stderr every 200 calls.
struct HostProf {
    std::atomic<bool> on{std::getenv("SV_HOST_PROFILE") != nullptr};
    bool print = std::getenv("SV_HOST_PROFILE") != nullptr;
    std::mutex mu;
    double t[6] = {0, 0, 0, 0, 0, 0};     // since the last print (stderr)
    double acc[6] = {0, 0, 0, 0, 0, 0};   // since the last reset (sv_host_profile_read)
    long n = 0, nacc = 0;
    void add(const double* d) {
        std::lock_guard<std::mutex> lk(mu);
        for (int i = 0; i < 6; ++i) {
            t[i] += d[i];
            acc[i] += d[i];
        }
        ++nacc;
        if (print && ++n % 200 == 0) {
            std::fprintf(stderr, "[sv host] per call (ms): prepare %.3f  stage+issue %.3f  wait-first %.3f  expand %.3f  "
                         "wait-rest %.3f  total %.3f\n", t[0] / n, t[1] / n, t[2] / n, t[3] / n, t[4] / n, t[5] / n);
            for (double& v : t) v = 0;
            n = 0;
        }
    }
};
HostProf& host_prof() {
    static HostProf* p = new HostProf();
    return *p;
}
int env_int(const char* name, int dflt, int lo, int hi) {
    const char* e = std::getenv(name);
    if (!e) return dflt;
    const int v = std::atoi(e);
    return v < lo ? lo : v > hi ? hi : v;
}
double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int host_frame_path(sv_ctx* c, const uint8_t* left, const uint8_t* right, int H, int W, int channels, int stride,
                    int min_disp, int num_disp, int win, int cost, sv::PostParams pp, const uint8_t* table,
                    FrameOut o) {
    const bool prof = host_prof().on;
    double tm[6] = {0, 0, 0, 0, 0, 0}, t0 = prof ? now_ms() : 0, tp = t0;
    sv::MatchPlan plan;
    int rc = check_match(H, W, min_disp, num_disp, win, cost, &plan);
    if (rc) return rc;
    if ((long long)H * W >= (1LL << 30)) return fail(SV_EINVAL, "frame too large");
    if (check_image(left, H, W) || check_image(right, H, W)) return SV_EINVAL;
    if (check_channels(channels)) return SV_EINVAL;
    const size_t row = (size_t)W * channels;
    if (stride < (int)row) return fail(SV_EINVAL, "stride smaller than a row");
    const size_t n = (size_t)H * W;
    SV_HIP(c->hin.ensure(2 * row * H));
    SV_HIP(c->gray[0].ensure(n));
    SV_HIP(c->gray[1].ensure(n));
    if (channels == 3) {
        SV_HIP(c->img[0].ensure(row * H));
        SV_HIP(c->img[1].ensure(row * H));
    }
    SV_HIP(c->d16.ensure(n * sizeof(int16_t)));
    SV_HIP(c->m16.ensure(n * sizeof(int16_t)));
    SV_HIP(c->hout.ensure(n * sizeof(int16_t)));
    rc = attach_lut(c, pp, c->stream);
    if (rc) return rc;
    if (pp.lut_n <= 0) return fail(SV_EINVAL, "no post-processing table for these parameters");
    const bool scaled = pp.mode == SV_POST_SCALED;
    // registered outputs: the median kernel's epilogue writes every output on the device and
    // they come back by DMA; otherwise only the int16 medians come back and the host expands
    // them with the table the device built
    const bool reg = host_registered(o.a, n * 4) && host_registered(o.disp, n * 4) &&
                     (!o.u8 || host_registered(o.u8, n)) && (!scaled || host_registered(o.b, n * 4)) &&
                     (!o.bgr || host_registered(o.bgr, 3 * n));
    sv::PostParams mp = pp;
    int m0 = 0, nl = 0;
    const HostEnt* ent = nullptr;
    const float* lb = nullptr;
    if (reg) {
        SV_HIP(c->fa.ensure(n * 4));
        SV_HIP(c->fb.ensure(n * 4));
        SV_HIP(c->u8.ensure(n));
        if (scaled) SV_HIP(c->fc.ensure(n * 4));
        if (o.bgr) SV_HIP(c->bgr.ensure(3 * n));
        mp.out_a = c->fa.as<float>();
        mp.out_u8 = c->u8.as<uint8_t>();
        mp.out_b = scaled ? c->fc.as<float>() : nullptr;
        rc = attach_cmap(c, mp, table, o.bgr ? c->bgr.as<uint8_t>() : nullptr, c->stream);
        if (rc) return rc;
    } else {
        rc = host_lut(c, pp);
        if (rc) return rc;
        mp.mode = SV_POST_NONE;      // the median kernel writes only the int16 medians
        mp.out_m16 = c->m16.as<int16_t>();
        m0 = pp.lut_m0;
        nl = pp.lut_n;
        // one 8-byte entry per table index: the f32 output and (u8, B, G, R) packed, so a
        // pixel costs one L1 load instead of the dependent u8 -> colormap lookups
        try {
            c->hl_ent.resize((size_t)nl);
        } catch (...) {
            return fail(SV_ENOMEM, "host table allocation failed");
        }
        for (int i = 0; i < nl; ++i) {
            const uint8_t u = c->hl_u8[i];
            const uint32_t bgr = table ? (uint32_t)table[3 * u] | (uint32_t)table[3 * u + 1] << 8 |
                                         (uint32_t)table[3 * u + 2] << 16 : 0u;
            c->hl_ent[i] = HostEnt{c->hl_a[i], u | bgr << 8};
        }
        ent = c->hl_ent.data();
        lb = c->hl_b.data();
    }
    if (prof) { const double t = now_ms(); tm[0] = t - tp; tp = t; }

    // One pass over the whole frame (round 3 also built pipelined row bands, band k's outputs
    // returning on a download stream while band k+1 uploaded: bit-exact but no faster in
    // rounds 3 and 4, so it was removed): stage + upload, gray, disparity, median, then the
    // outputs return in 8 pieces on the compute stream, each behind its own event so the host
    // expansion of one piece runs while the next is in flight.
    // D2H pieces: every hipMemcpyAsync costs ~15-90 us of copy-engine setup on these boxes
    // (tools/microbench/pcie_rate: 4.1 MB pinned in 1 piece 0.08-0.33 ms, 8 pieces 0.2-1.0 ms),
    // so the DMA path (nothing to overlap on the host) downloads each output in one piece and
    // the expansion path in two, the second's transfer under the first's host expansion
    // (round 5 A/B, profiles/r05b/host_ab.txt: 2 pieces 1.47-1.51k frames/s per call, 4
    // pieces 1.41-1.45k, 8 pieces 1.23-1.35k).
    // SV_HOST_PIECES / SV_HOST_PIECES_DMA override (A/B measurements).
    static const int pieces_exp = env_int("SV_HOST_PIECES", 2, 1, 8);
    static const int pieces_dma = env_int("SV_HOST_PIECES_DMA", 1, 1, 8);
    constexpr int kmaxp = 8;
    const int npiece = reg ? pieces_dma : pieces_exp;
    hipStream_t ds = c->stream;
    int bands[kmaxp][2] = {};   // output rows of each D2H piece
    std::atomic<int> bad{0};
    sv::HostPool& pool = sv::HostPool::get();
    auto expand = [&](int k) -> int {   // host expansion of piece k's medians
        const int y0 = bands[k][0], y1 = bands[k][1];
        if (y1 <= y0) return 0;
        SV_HIP(hipEventSynchronize(c->dev_done[k]));
        if (prof) { const double t = now_ms(); tm[k ? 4 : 2] += t - tp; tp = t; }
        const size_t i0 = (size_t)y0 * W, i1 = (size_t)y1 * W;
        const int16_t* med = c->hout.as<int16_t>();
        const int parts = pool.threads();
        pool.parallel_for(parts, [&](int p) {
            const size_t a = i0 + (i1 - i0) * p / parts, b = i0 + (i1 - i0) * (p + 1) / parts;
            const int sel = (o.u8 ? 1 : 0) | (scaled ? 2 : 0) | (o.bgr ? 4 : 0);
            int nb = 0;
            switch (sel) {   // the output set picks the instantiation (no per-pixel branches)
                case 0: nb = expand_rows<false, false, false>(med, a, b, m0, nl, ent, lb, o); break;
                case 1: nb = expand_rows<true, false, false>(med, a, b, m0, nl, ent, lb, o); break;
                case 2: nb = expand_rows<false, true, false>(med, a, b, m0, nl, ent, lb, o); break;
                case 3: nb = expand_rows<true, true, false>(med, a, b, m0, nl, ent, lb, o); break;
                case 4: nb = expand_rows<false, false, true>(med, a, b, m0, nl, ent, lb, o); break;
                case 5: nb = expand_rows<true, false, true>(med, a, b, m0, nl, ent, lb, o); break;
                case 6: nb = expand_rows<false, true, true>(med, a, b, m0, nl, ent, lb, o); break;
                default: nb = expand_rows<true, true, true>(med, a, b, m0, nl, ent, lb, o); break;
            }
            if (nb) bad.fetch_add(nb);
        });
        if (prof) { const double t = now_ms(); tm[3] += t - tp; tp = t; }
        return 0;
    };
    const uint8_t* src[2] = {left, right};
    for (int i = 0; i < 2; ++i) {
        uint8_t* stage = c->hin.as<uint8_t>() + (size_t)i * row * H;
        uint8_t* dst = channels == 1 ? c->gray[i].as<uint8_t>() : c->img[i].as<uint8_t>();
        {   // (profile on: device events around each upload; closed on every exit path)
            ProfScope ph(c, SV_K_H2D, c->stream);
            rc = stage_rows(c, src[i], 0, H, row, stride, stage, dst, 6);
            if (rc) return rc;
            ph.done();
        }
        if (channels == 3)
            SV_LAUNCH(c, SV_K_GRAY, c->stream,
                      sv::launch_gray(c->img[i].as<uint8_t>(), H, W, (int)row, c->gray[i].as<uint8_t>(), c->stream));
    }
    rc = enqueue_disparity(c, c->gray[0].as<uint8_t>(), c->gray[1].as<uint8_t>(), H, W, W, min_disp, num_disp, win,
                           cost, 0, H, c->d16.as<int16_t>(), W, c->stream);
    if (rc) return rc;
    SV_LAUNCH(c, SV_K_MEDIAN, c->stream,
              sv::launch_median_i16(c->d16.as<int16_t>(), H, W, 0, H, reg ? c->fb.as<float>() : nullptr, mp,
                                    c->stream));
    {
        ProfScope pd(c, SV_K_D2H, ds);   // an SV_HIP failure below returns through prof_abort
        for (int q = 0; q < npiece; ++q) {
            const int p0 = (int)((long long)H * q / npiece), p1 = (int)((long long)H * (q + 1) / npiece);
            bands[q][0] = p0;
            bands[q][1] = p1;
            if (p1 <= p0) continue;
            const size_t i0 = (size_t)p0 * W, m = (size_t)(p1 - p0) * W;
            if (reg) {
                SV_HIP(c->copy(o.disp + i0, c->fb.as<float>() + i0, m * 4, hipMemcpyDeviceToHost, ds));
                SV_HIP(c->copy(o.a + i0, c->fa.as<float>() + i0, m * 4, hipMemcpyDeviceToHost, ds));
                if (o.u8) SV_HIP(c->copy(o.u8 + i0, c->u8.as<uint8_t>() + i0, m, hipMemcpyDeviceToHost, ds));
                if (scaled) SV_HIP(c->copy(o.b + i0, c->fc.as<float>() + i0, m * 4, hipMemcpyDeviceToHost, ds));
                if (o.bgr)
                    SV_HIP(c->copy(o.bgr + 3 * i0, c->bgr.as<uint8_t>() + 3 * i0, 3 * m, hipMemcpyDeviceToHost, ds));
            } else {
                SV_HIP(c->copy(c->hout.as<int16_t>() + i0, c->m16.as<int16_t>() + i0, m * 2, hipMemcpyDeviceToHost,
                               ds));
                if (!c->dev_done[q]) SV_HIP(hipEventCreateWithFlags(&c->dev_done[q], hipEventDisableTiming));
                SV_HIP(hipEventRecord(c->dev_done[q], ds));
            }
        }
        pd.done();
    }
    if (prof) { const double t = now_ms(); tm[1] = t - tp; tp = t; }
    if (!reg) {
        for (int q = 0; q < npiece; ++q) {
            rc = expand(q);
            if (rc) return rc;
        }
    }
    SV_HIP(hipStreamSynchronize(ds));
    if (prof) {
        const double t = now_ms();
        tm[4] += t - tp;
        tm[5] = t - t0;
        host_prof().add(tm);
    }
    if (bad.load()) return fail(SV_EHIP, "median value outside the post-processing table");
    return 0;
}

}  // namespace

extern "C" {

int sv_gray(sv_ctx* c, const uint8_t* bgr, int H, int W, int stride, uint8_t* gray) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (check_image(bgr, H, W) || !gray) return fail(SV_EINVAL, "bad gray arguments");
    const size_t row = (size_t)W * 3, n = row * H;
    if (stride < (int)row) return fail(SV_EINVAL, "stride smaller than a row");
    SV_HIP(c->hin.ensure(n));
    SV_HIP(c->gray[0].ensure((size_t)H * W));
    if (const int rc = stage_image(c, bgr, H, row, stride, 0, c->img[0])) return rc;
    SV_LAUNCH(c, SV_K_GRAY, c->stream,
              sv::launch_gray(c->img[0].as<uint8_t>(), H, W, (int)row, c->gray[0].as<uint8_t>(), c->stream));
    Out o[] = {{gray, c->gray[0].p, (size_t)H * W}};
    return collect(c, o, 1);
}

// Rows [row0, row1) (clamped) of the pair's map come back, and the left image's Harris response if wanted.
static int disparity_host(sv_ctx* c, const uint8_t* left, const uint8_t* right, int H, int W, int channels,
                          int stride, int min_disp, int num_disp, int win, int cost, int row0, int row1,
                          int16_t* disp16, float* harris) {
    sv::MatchPlan plan;
    if (const int rc = check_match(H, W, min_disp, num_disp, win, cost, &plan)) return rc;
    if (const int rc = stage_pair(c, left, right, H, W, channels, stride)) return rc;
    SV_HIP(c->d16.ensure((size_t)H * W * sizeof(int16_t)));
    const int rc = enqueue_disparity(c, c->gray[0].as<uint8_t>(), c->gray[1].as<uint8_t>(), H, W, W, min_disp,
                                     num_disp, win, cost, row0, row1, c->d16.as<int16_t>(), W, c->stream);
    if (rc) return rc;
    if (harris) {
        SV_HIP(c->harris.ensure((size_t)H * W * sizeof(float)));
        SV_LAUNCH(c, SV_K_HARRIS, c->stream,
                  sv::launch_harris(c->gray[0].as<uint8_t>(), H, W, W, c->harris.as<float>(), c->stream));
    }
    const size_t off = (size_t)row0 * W;
    Out o[] = {{disp16 + off, c->d16.as<int16_t>() + off, (size_t)(row1 - row0) * W * sizeof(int16_t)},
               {harris, c->harris.p, (size_t)H * W * sizeof(float)}};
    return collect(c, o, 2);
}

int sv_disparity(sv_ctx* c, const uint8_t* left, const uint8_t* right, int H, int W, int channels, int stride,
                 int min_disp, int num_disp, int win, int cost, int16_t* disp16, float* harris) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (!disp16) return fail(SV_EINVAL, "null disparity output");
    return disparity_host(c, left, right, H, W, channels, stride, min_disp, num_disp, win, cost, 0, H, disp16, harris);
}

int sv_disparity_rows(sv_ctx* c, const uint8_t* left, const uint8_t* right, int H, int W, int channels,
                      int stride, int min_disp, int num_disp, int win, int cost, int row0, int row1,
                      int16_t* disp16) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (!disp16) return fail(SV_EINVAL, "null disparity output");
    if (row0 < 0) row0 = 0;
    if (row1 > H) row1 = H;
    if (row1 <= row0) return 0;
    return disparity_host(c, left, right, H, W, channels, stride, min_disp, num_disp, win, cost, row0, row1, disp16,
                          nullptr);
}

int sv_median5_f32(sv_ctx* c, const float* in, int H, int W, float* out) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (check_image(in, H, W) || !out) return fail(SV_EINVAL, "bad median arguments");
    const size_t n = (size_t)H * W * sizeof(float);
    SV_HIP(c->hin.ensure(n));
    SV_HIP(c->fa.ensure(n));
    if (const int rc = stage_image(c, in, 1, n, n, 0, c->fin)) return rc;   // dense: one row of n bytes
    SV_LAUNCH(c, SV_K_MEDIAN, c->stream, sv::launch_median_f32(c->fin.as<float>(), H, W, c->fa.as<float>(), c->stream));
    Out o[] = {{out, c->fa.p, n}};
    return collect(c, o, 1);
}

static int post_common(sv_ctx* c, const float* disparity, int n, const sv::PostParams& tmpl, float* a,
                       uint8_t* u8, float* b) {
    if (!disparity || n <= 0) return fail(SV_EINVAL, "bad post arguments");
    const size_t nb = (size_t)n * sizeof(float);
    SV_HIP(c->hin.ensure(nb));
    SV_HIP(c->fa.ensure(nb));
    SV_HIP(c->fb.ensure(nb));
    SV_HIP(c->u8.ensure((size_t)n));
    if (const int rc = stage_image(c, disparity, 1, nb, nb, 0, c->fin)) return rc;   // dense: one row of nb bytes
    sv::PostParams pp = tmpl;
    pp.out_a = c->fa.as<float>();
    pp.out_u8 = c->u8.as<uint8_t>();
    pp.out_b = c->fb.as<float>();
    SV_LAUNCH(c, SV_K_POST, c->stream, sv::launch_post(c->fin.as<float>(), n, pp, c->stream));
    Out o[] = {{a, c->fa.p, nb}, {u8, c->u8.p, (size_t)n}, {b, c->fb.p, nb}};
    return collect(c, o, 3);
}

int sv_depth_post(sv_ctx* c, const float* disparity, int n, float min_depth, float max_depth, float depth_range,
                  float min_disp_global, float* depth_final, uint8_t* depth_normalized) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (!depth_final || !depth_normalized) return fail(SV_EINVAL, "null outputs");
    sv::PostParams pp = make_post(SV_POST_DEPTH, min_depth, max_depth, depth_range, min_disp_global, 0, 0,
                                  nullptr, nullptr, nullptr);
    return post_common(c, disparity, n, pp, depth_final, depth_normalized, nullptr);
}

int sv_scaled_post(sv_ctx* c, const float* disparity, int n, int min_disp, int num_disp,
                   float* disparity_normalized, uint8_t* normalized_u8, float* confidence) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (!disparity_normalized || !normalized_u8 || !confidence || num_disp <= 0)
        return fail(SV_EINVAL, "bad scaled post arguments");
    sv::PostParams pp = make_post(SV_POST_SCALED, 0.f, 0.f, 0.f, 0.f, min_disp, num_disp, nullptr, nullptr,
                                  nullptr);
    return post_common(c, disparity, n, pp, disparity_normalized, normalized_u8, confidence);
}

int sv_host_profile_enable(int enable) {
    host_prof().on = enable != 0;
    return 0;
}

int sv_host_profile_read(double* ms6, long long* calls, int reset) {
    HostProf& hp = host_prof();
    std::lock_guard<std::mutex> lk(hp.mu);
    if (ms6)
        for (int i = 0; i < 6; ++i) ms6[i] = hp.acc[i];
    if (calls) *calls = hp.nacc;
    if (reset) {
        for (double& v : hp.acc) v = 0;
        hp.nacc = 0;
    }
    return 0;
}

int sv_host_register(void* ptr, uint64_t bytes) {
    if (!ptr || bytes == 0) return fail(SV_EINVAL, "null or empty host range");
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        if (g_reg.count(reinterpret_cast<uintptr_t>(ptr))) return fail(SV_EINVAL, "host range already registered");
    }
    SV_HIP(hipHostRegister(ptr, (size_t)bytes, hipHostRegisterPortable));
    std::lock_guard<std::mutex> lk(g_reg_mu);
    g_reg[reinterpret_cast<uintptr_t>(ptr)] = (size_t)bytes;
    return 0;
}

int sv_host_unregister(void* ptr) {
    {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        auto it = g_reg.find(reinterpret_cast<uintptr_t>(ptr));
        if (it == g_reg.end()) return fail(SV_EINVAL, "host range not registered");
        g_reg.erase(it);
    }
    SV_HIP(hipHostUnregister(ptr));
    return 0;
}

int sv_depth_map(sv_ctx* c, const uint8_t* left, const uint8_t* right, int H, int W, int channels, int stride,
                 int min_disp, int num_disp, int win, int cost, float min_depth, float max_depth,
                 float depth_range, float min_disp_global, float* depth_final, float* disparity,
                 uint8_t* depth_normalized) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (!depth_final || !disparity || !depth_normalized) return fail(SV_EINVAL, "null outputs");
    sv::PostParams pp = make_post(SV_POST_DEPTH, min_depth, max_depth, depth_range, min_disp_global, min_disp,
                                  num_disp, nullptr, nullptr, nullptr);
    return host_frame_path(c, left, right, H, W, channels, stride, min_disp, num_disp, win, cost, pp, nullptr,
                           FrameOut{depth_final, disparity, depth_normalized, nullptr, nullptr});
}

int sv_stereo_scaled(sv_ctx* c, const uint8_t* left, const uint8_t* right, int H, int W, int channels,
                     int stride, int min_disp, int num_disp, int win, int cost, float* disparity_normalized,
                     float* disparity, uint8_t* normalized_u8, float* confidence) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (!disparity_normalized || !disparity || !normalized_u8 || !confidence)
        return fail(SV_EINVAL, "null outputs");
    sv::PostParams pp = make_post(SV_POST_SCALED, 0.f, 0.f, 0.f, 0.f, min_disp, num_disp, nullptr, nullptr, nullptr);
    return host_frame_path(c, left, right, H, W, channels, stride, min_disp, num_disp, win, cost, pp, nullptr,
                           FrameOut{disparity_normalized, disparity, normalized_u8, confidence, nullptr});
}

int sv_depth_map_color(sv_ctx* c, const uint8_t* left, const uint8_t* right, int H, int W, int channels,
                       int stride, int min_disp, int num_disp, int win, int cost, float min_depth, float max_depth,
                       float depth_range, float min_disp_global, const uint8_t* cmap_bgr, float* depth_final,
                       float* disparity, uint8_t* depth_normalized, uint8_t* depth_colormap) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (!depth_final || !disparity || !depth_colormap || !cmap_bgr) return fail(SV_EINVAL, "null outputs");
    sv::PostParams pp = make_post(SV_POST_DEPTH, min_depth, max_depth, depth_range, min_disp_global, min_disp,
                                  num_disp, nullptr, nullptr, nullptr);
    return host_frame_path(c, left, right, H, W, channels, stride, min_disp, num_disp, win, cost, pp, cmap_bgr,
                           FrameOut{depth_final, disparity, depth_normalized, nullptr, depth_colormap});
}

int sv_stereo_scaled_color(sv_ctx* c, const uint8_t* left, const uint8_t* right, int H, int W, int channels,
                           int stride, int min_disp, int num_disp, int win, int cost, const uint8_t* cmap_bgr,
                           float* disparity_normalized, float* disparity, uint8_t* normalized_u8,
                           float* confidence, uint8_t* depth_colormap) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (!disparity_normalized || !disparity || !confidence || !depth_colormap || !cmap_bgr)
        return fail(SV_EINVAL, "null outputs");
    sv::PostParams pp = make_post(SV_POST_SCALED, 0.f, 0.f, 0.f, 0.f, min_disp, num_disp, nullptr, nullptr, nullptr);
    return host_frame_path(c, left, right, H, W, channels, stride, min_disp, num_disp, win, cost, pp, cmap_bgr,
                           FrameOut{disparity_normalized, disparity, normalized_u8, confidence, depth_colormap});
}

int sv_harris(sv_ctx* c, const uint8_t* gray, int H, int W, int stride, float* out) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (check_image(gray, H, W) || !out || stride < W) return fail(SV_EINVAL, "bad harris arguments");
    const size_t n = (size_t)H * W;
    SV_HIP(c->hin.ensure(n));
    SV_HIP(c->harris.ensure(n * sizeof(float)));
    if (const int rc = stage_image(c, gray, H, W, stride, 0, c->gray[0])) return rc;
    SV_LAUNCH(c, SV_K_HARRIS, c->stream,
              sv::launch_harris(c->gray[0].as<uint8_t>(), H, W, W, c->harris.as<float>(), c->stream));
    Out o[] = {{out, c->harris.p, n * sizeof(float)}};
    return collect(c, o, 1);
}

int sv_hog_hist(sv_ctx* c, const uint8_t* gray, int H, int W, int stride, int win, uint16_t* out) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (check_image(gray, H, W) || !out || stride < W) return fail(SV_EINVAL, "bad hog arguments");
    if (check_win(win)) return SV_EINVAL;
    const size_t n = (size_t)H * W;
    SV_HIP(c->hin.ensure(n));
    SV_HIP(c->hog[0].ensure(n * 10 * sizeof(uint16_t)));
    if (const int rc = stage_image(c, gray, H, W, stride, 0, c->gray[0])) return rc;
    SV_LAUNCH(c, SV_K_HOG, c->stream,
              sv::launch_hog_hist(c->gray[0].as<uint8_t>(), H, W, W, win, 0, H, c->hog[0].as<uint16_t>(), c->stream));
    Out o[] = {{out, c->hog[0].p, n * 10 * sizeof(uint16_t)}};
    return collect(c, o, 1);
}

int sv_sgbm(sv_ctx* c, const uint8_t* left, const uint8_t* right, int H, int W, int channels, int stride,
            int min_disp, int num_disp, int block_size, int P1, int P2, int disp12_max_diff, int pre_filter_cap,
            int uniqueness_ratio, int speckle_window_size, int speckle_range, int16_t* disp16) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (!disp16) return fail(SV_EINVAL, "null disparity output");
    sv::MatchPlan plan;
    int rc = check_match(H, W, min_disp, num_disp, block_size, SV_COST_SGBM, &plan);
    if (rc) return rc;
    rc = stage_pair(c, left, right, H, W, channels, stride);
    if (rc) return rc;
    SV_HIP(c->d16.ensure((size_t)H * W * sizeof(int16_t)));
    SgbmParams p{P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio, speckle_window_size, speckle_range};
    rc = enqueue_sgbm(c, c->gray[0].as<uint8_t>(), c->gray[1].as<uint8_t>(), H, W, W, min_disp, num_disp,
                      block_size, p, c->d16.as<int16_t>(), W, c->stream);
    if (rc) return rc;
    Out o[] = {{disp16, c->d16.p, (size_t)H * W * sizeof(int16_t)}};
    return collect(c, o, 1);
}

int sv_filter_speckles(sv_ctx* c, int16_t* img, int H, int W, int new_val, int max_speckle_size, int max_diff) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (!img || H <= 0 || W <= 0) return fail(SV_EINVAL, "bad speckle-filter arguments");
    const size_t bytes = (size_t)H * W * sizeof(int16_t);
    SV_HIP(c->d16.ensure(bytes));
    SV_HIP(c->hin.ensure(bytes));
    c->scratch_written(c->d16.p);
    if (const int rc = stage_image(c, img, 1, bytes, bytes, 0, c->d16)) return rc;   // dense: one row of `bytes`
    const int rc = enqueue_speckles(c, c->d16.as<int16_t>(), H, W, W, new_val, max_speckle_size, max_diff, c->stream);
    if (rc) return rc;
    Out o[] = {{img, c->d16.p, bytes}};
    return collect(c, o, 1);
}

}  // extern "C"
