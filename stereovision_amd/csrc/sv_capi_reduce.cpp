// sv_capi_reduce.cpp — the reductions of the C ABI: frame statistics, radix select (order
// statistics) and the affine map.
#include "sv_ctx.h"

extern "C" {

static void stats_blocks(int H, int W, int* bh, int* bw) {
    *bh = H / 48 > 0 ? H / 48 : 1;
    *bw = W / 48 > 0 ? W / 48 : 1;
}

// The statistics launch over n_frames checked device images (or pairs: d_img1), outputs dense per image.
static int enqueue_frame_stats(sv_ctx* c, const uint8_t* d_img0, const uint8_t* d_img1, int n_frames,
                               int64_t frame_stride, int H, int W, int channels, int pitch, uint32_t* d_block_sum,
                               uint32_t* d_block_sq, uint32_t* d_hist, hipStream_t s) {
    const int per = d_img1 ? 2 : 1, nimg = n_frames * per;
    SV_HIP(c->hist_copies.ensure_zeroed((size_t)sv::kHistCopies * nimg * 256 * sizeof(uint32_t)));
    sv::FrameStatsArgs a{};
    a.hist_copies = c->hist_copies.as<uint32_t>();
    a.img0 = d_img0;
    a.img1 = d_img1;
    a.H = H;
    a.W = W;
    a.pitch = pitch;
    a.cn = channels;
    a.per = per;
    a.fs = n_frames > 1 ? frame_stride : 0;
    stats_blocks(H, W, &a.bh, &a.bw);
    a.block_sum = d_block_sum;
    a.block_sq = d_block_sq;
    a.hist = d_hist;
    SV_LAUNCH(c, SV_K_STATS, s, sv::launch_frame_stats(a, nimg, s));
    return 0;
}

int sv_frame_stats_batch_dev(sv_ctx* c, const uint8_t* d_img0, const uint8_t* d_img1, int n_frames,
                             int64_t frame_stride, int H, int W, int channels, int pitch, uint32_t* d_block_sum,
                             uint32_t* d_block_sq, uint32_t* d_hist, void* stream) {
    SV_ENTER(c);
    if (check_image(d_img0, H, W) || !d_block_sum || !d_block_sq || !d_hist || n_frames < 1)
        return fail(SV_EINVAL, "bad frame-stats arguments");
    if (check_channels(channels)) return SV_EINVAL;
    if (pitch < W * channels) return fail(SV_EINVAL, "pitch smaller than a row");
    if (check_frame_stride(n_frames, frame_stride, (int64_t)pitch * H)) return SV_EINVAL;
    if ((long long)n_frames * (d_img1 ? 2 : 1) > 65535) return fail(SV_EINVAL, "too many images in one batch");
    hipStream_t s = pick(c, stream);
    SV_SCRATCH(c, s);
    return enqueue_frame_stats(c, d_img0, d_img1, n_frames, frame_stride, H, W, channels, pitch, d_block_sum,
                               d_block_sq, d_hist, s);
}

int sv_frame_stats(sv_ctx* c, const uint8_t* img0, const uint8_t* img1, int H, int W, int channels, int stride,
                   uint32_t* block_sum, uint32_t* block_sq, uint32_t* hist) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (check_image(img0, H, W) || !block_sum || !block_sq || !hist) return fail(SV_EINVAL, "bad frame-stats arguments");
    if (check_channels(channels)) return SV_EINVAL;
    const size_t row = (size_t)W * channels, n = row * H;
    if (stride < (int)row) return fail(SV_EINVAL, "stride smaller than a row");
    const int nimg = img1 ? 2 : 1;
    int bh, bw;
    stats_blocks(H, W, &bh, &bw);
    const size_t nb = (size_t)bh * bw;
    SV_HIP(c->hin.ensure(nimg * n));
    const uint8_t* src[2] = {img0, img1};
    for (int k = 0; k < nimg; ++k)
        if (const int rc = stage_image(c, src[k], H, row, stride, k * n, c->img[k])) return rc;
    SV_HIP(c->stats.ensure(nimg * (2 * nb + 256) * sizeof(uint32_t)));
    uint32_t* d = c->stats.as<uint32_t>();
    const int rc = enqueue_frame_stats(c, c->img[0].as<uint8_t>(), nimg == 2 ? c->img[1].as<uint8_t>() : nullptr, 1, 0,
                                       H, W, channels, (int)row, d, d + nimg * nb, d + 2 * nimg * nb, c->stream);
    if (rc) return rc;
    Out o[] = {{block_sum, d, nimg * nb * 4}, {block_sq, d + nimg * nb, nimg * nb * 4},
               {hist, d + 2 * nimg * nb, (size_t)nimg * 256 * 4}};
    return collect(c, o, 3);
}

// One select pass over the context stream (a batch of a.narr arrays): hist [narr][kMaxRanks]
// [2048] (null: not wanted) and counts [narr][2] (null: not wanted) back on the host.
static int select_pass(sv_ctx* c, sv::SelectArgs& a, uint32_t* hist_host, unsigned long long* counts_host) {
    // device: [kSelBatch][copies][kMaxRanks][2048] accumulators | [kSelBatch] count slots |
    // counts [narr][2] | folded hist [narr][kMaxRanks][2048].  The accumulator regions are
    // laid out for the largest batch whatever narr is: the folds leave them zeroed, and a
    // smaller batch's outputs must never land where a larger batch accumulates
    const size_t na = (size_t)(a.narr > 0 ? a.narr : 1);
    const size_t hb = (size_t)sv::kMaxRanks * 2048 * sizeof(uint32_t);
    const size_t ab = (size_t)sv::kSelBatch * sv::kHistCopies * hb;
    const size_t cb = (size_t)sv::kSelBatch * sv::kCountSlots * 16 * sizeof(unsigned long long);
    const size_t ob = na * 16 + na * hb;
    SV_HIP(c->sel.ensure_zeroed(ab + cb + ob));
    uint8_t* base = c->sel.as<uint8_t>();
    a.ghist = reinterpret_cast<uint32_t*>(base);
    a.counts = reinterpret_cast<unsigned long long*>(base + ab);
    a.counts_out = reinterpret_cast<unsigned long long*>(base + ab + cb);
    a.hist_out = reinterpret_cast<uint32_t*>(base + ab + cb + na * 16);
    SV_LAUNCH(c, SV_K_SELECT, c->stream, sv::launch_select_hist(a, c->stream));
    // one copy, and only of what the host reads: the counts, then the histograms up to the last
    // bin of the last rank of the last array this pass fills (pass digits have `bits` bits; a
    // count-only call reads no histogram)
    const size_t nr = hist_host ? (size_t)(a.nranks > 0 ? a.nranks : 1) : 0;
    const size_t used = nr ? (na - 1) * hb + ((nr - 1) * 2048 + ((size_t)1 << a.bits)) * sizeof(uint32_t) : 0;
    SV_HIP(c->hout.ensure(ob));
    SV_HIP(c->copy(c->hout.p, a.counts_out, na * 16 + used, hipMemcpyDeviceToHost, c->stream));
    SV_HIP(hipStreamSynchronize(c->stream));
    if (counts_host) std::memcpy(counts_host, c->hout.p, na * 16);
    if (used) std::memcpy(hist_host, c->hout.as<uint8_t>() + na * 16, used);
    return 0;
}

// np.percentile's order statistics of a batch of narr arrays (array y at d_x + y * x_stride,
// its mask at d_mask + y * mask_stride): selected / nan counts (nullable) and, with nranks
// > 0, the values of ranks[y][r] (radix select in three passes of 11/11/10 bits, one launch
// + one fold per pass for the whole batch).
static int select_batch(sv_ctx* c, const float* d_x, int64_t n, int64_t x_stride, int narr, int mask_mode,
                        const float* d_mask, int64_t mask_stride, float thr, const int64_t* ranks, int nranks,
                        float* values, int64_t* selected, int64_t* nans) {
    if (!d_x || n < 0) return fail(SV_EINVAL, "bad select arguments");
    if (mask_mode < 0 || mask_mode > 2) return fail(SV_EINVAL, "mask_mode must be 0, 1 or 2");
    if (mask_mode == 2 && !d_mask) return fail(SV_EINVAL, "mask_mode 2 needs a mask array");
    if (narr < 1 || narr > sv::kSelBatch) return fail(SV_EINVAL, "1..16 arrays per batch");
    if (narr > 1 && (x_stride < n || (mask_mode == 2 && mask_stride < n))) return fail(SV_EINVAL, "array stride below n");
    if (nranks < 0 || nranks > sv::kMaxRanks || (nranks > 0 && (!ranks || !values))) return fail(SV_EINVAL, "0..4 ranks");
    sv::SelectArgs a{};
    a.x = d_x;
    a.mask = mask_mode == 2 ? d_mask : nullptr;
    a.thr = thr;
    a.mask_mode = mask_mode;
    a.n = (size_t)n;
    a.narr = narr;
    a.xstride = narr > 1 ? (size_t)x_stride : 0;
    a.mstride = narr > 1 ? (size_t)mask_stride : 0;
    std::vector<uint32_t> h((size_t)narr * sv::kMaxRanks * 2048);
    std::vector<unsigned long long> cnt((size_t)narr * 2, 0ull);
    const size_t hs = (size_t)sv::kMaxRanks * 2048;
    uint32_t prefix[sv::kSelBatch][sv::kMaxRanks] = {};
    int64_t rem[sv::kSelBatch][sv::kMaxRanks];
    for (int y = 0; y < narr; ++y)
        for (int r = 0; r < nranks; ++r) {
            if (ranks[(size_t)y * nranks + r] < 0) return fail(SV_EINVAL, "negative rank");
            rem[y][r] = ranks[(size_t)y * nranks + r];
        }
    const int shifts[3] = {21, 10, 0}, bits[3] = {11, 11, 10};
    const int passes = nranks > 0 ? 3 : 1;
    for (int p = 0; p < passes; ++p) {
        a.shift = shifts[p];
        a.bits = bits[p];
        a.nranks = p == 0 ? 1 : nranks;          // pass 0: one histogram serves every rank
        for (int y = 0; y < narr; ++y)
            for (int r = 0; r < sv::kMaxRanks; ++r) a.prefix[y][r] = p == 0 ? 0u : prefix[y][r];
        if (n > 0) {
            int rc = select_pass(c, a, nranks > 0 ? h.data() : nullptr, p == 0 ? cnt.data() : nullptr);
            if (rc) return rc;
        }
        if (p == 0) {
            for (int y = 0; y < narr; ++y) {
                if (selected) selected[y] = (int64_t)cnt[2 * y];
                if (nans) nans[y] = (int64_t)cnt[2 * y + 1];
                for (int r = 0; r < nranks; ++r)
                    if ((unsigned long long)rem[y][r] >= cnt[2 * y]) return fail(SV_ERANGE, "rank beyond the selection");
            }
        }
        for (int y = 0; y < narr; ++y)
            for (int r = 0; r < nranks; ++r) {
                const uint32_t* hr = h.data() + (size_t)y * hs + (p == 0 ? 0 : r) * 2048;
                int64_t acc = 0;
                int d = 0;
                for (; d < (1 << bits[p]); ++d) {
                    if (acc + (int64_t)hr[d] > rem[y][r]) break;
                    acc += hr[d];
                }
                if (d == (1 << bits[p])) return fail(SV_EHIP, "select: histogram inconsistent (data changed?)");
                rem[y][r] -= acc;
                prefix[y][r] = (prefix[y][r] << bits[p]) | (uint32_t)d;
            }
    }
    for (int y = 0; y < narr; ++y)
        for (int r = 0; r < nranks; ++r) {
            const uint32_t k = prefix[y][r];
            const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
            std::memcpy(&values[(size_t)y * nranks + r], &u, sizeof(float));
        }
    return 0;
}

int sv_select_count_batch(sv_ctx* c, const float* d_x, int64_t n, int64_t x_stride, int n_arrays, int mask_mode,
                          const float* d_mask, int64_t mask_stride, float thr, int64_t* selected, int64_t* nans) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    return select_batch(c, d_x, n, x_stride, n_arrays, mask_mode, d_mask, mask_stride, thr, nullptr, 0, nullptr,
                        selected, nans);
}

int sv_select_ranks_batch(sv_ctx* c, const float* d_x, int64_t n, int64_t x_stride, int n_arrays, int mask_mode,
                          const float* d_mask, int64_t mask_stride, float thr, const int64_t* ranks, int nranks,
                          float* values) {
    SV_ENTER(c);
    SV_SCRATCH(c, c->stream);
    if (!ranks || !values || nranks < 1 || nranks > sv::kMaxRanks) return fail(SV_EINVAL, "1..4 ranks");
    return select_batch(c, d_x, n, x_stride, n_arrays, mask_mode, d_mask, mask_stride, thr, ranks, nranks, values,
                        nullptr, nullptr);
}

int sv_affine_f32_dev(sv_ctx* c, const float* d_x, int64_t n, int mode, float fa, float fb, float fc, float fd,
                      double ds, double doff, float* d_out, void* stream) {
    SV_ENTER(c);
    if (!d_x || !d_out || n < 0 || mode < 0 || mode > sv::AFF_NORM_CLIP255) return fail(SV_EINVAL, "bad affine arguments");
    hipStream_t s = pick(c, stream);
    sv::AffineArgs a{};
    a.x = d_x;
    a.out = d_out;
    a.n = (size_t)n;
    a.mode = mode;
    a.fa = fa;
    a.fb = fb;
    a.fc = fc;
    a.fd = fd;
    a.ds = ds;
    a.doff = doff;
    SV_LAUNCH(c, SV_K_AFFINE, s, sv::launch_affine_f32(a, s));
    return 0;
}

}  // extern "C"
