// Internal declarations shared by the HIP kernel files and the C-ABI (sv_capi.cpp).
// gfx950 (CDNA4, wave64) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <string>

struct sv_comm;

namespace sv {

// v_sad_u32: a = |a - b| + c (unsigned) — a running window sum's update `sum - leaving +
// entering` in ONE VOP3 whenever sum >= leaving (the sum holds the leaving term as a summand);
// also exact on two u16 halves per word when each half's sum holds its own leaving term and
// stays below 2^16 (no borrow, no carry).  No clang builtin, and the umax - umin + c pattern
// is split into several ops inside large bodies, so inline asm (plain VOP3: no hazards).
__device__ __forceinline__ void sad_u32_acc(uint32_t& a, uint32_t b, uint32_t c) {
    asm("v_sad_u32 %0, %0, %1, %2" : "+v"(a) : "v"(b), "v"(c));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// cv2.cvtColor(BGR2GRAY), 14-bit fixed point (depth_map.py:871-880)
__device__ __forceinline__ int bgr_to_gray(int b, int g, int r) {
    return (b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14;
}

// ---- environment switches (A/B measurements): callers keep the value in a function-local
// static, so each is read once per process -----------------------------------------------
// default on: off with NAME=0; default off: on with NAME=1
inline bool env_flag(const char* name, bool default_on) {
    const char* e = std::getenv(name);
    return default_on ? !(e && e[0] == '0') : (e && e[0] == '1');
}
// the integer value of NAME when it lies in [lo, hi], else 0 (unset, unparsable, out of range)
inline int env_int(const char* name, int lo, int hi) {
    const char* e = std::getenv(name);
    const int v = e ? std::atoi(e) : 0;
    return v >= lo && v <= hi ? v : 0;
}

// Sets the calling thread's sv_last_error() message; returns `code`.
int set_error(int code, const std::string& msg);

// RCCL transfers of the multi-device entry points (sv_comm.cpp; librccl loaded on first use).
int comm_group_start();
int comm_group_end();
int comm_send(sv_comm* c, const void* buf, size_t bytes, int peer, hipStream_t s);
int comm_recv(sv_comm* c, void* buf, size_t bytes, int peer, hipStream_t s);
int comm_rank(const sv_comm* c);
int comm_size(const sv_comm* c);
int comm_device(const sv_comm* c);

enum Cost { COST_SAD = 0, COST_SSD = 1, COST_HOG = 2, COST_SGBM = 3, COST_CENSUS = 4 };

// Disparity lanes: each wave is split into groups of LPG lanes (16/32/64); every lane of a
// group owns DPL consecutive disparities of the same output pixel, so one group covers
// LPG*DPL candidates and the per-pixel argmin is an in-lane min3 chain plus a
// log2(LPG)-step DPP reduction.
struct MatchPlan {
    int dpl;     // disparities per lane: 4, 6 or 8
    int lpg;     // lanes per group: 16, 32 or 64
    int ndw;     // dwords per column pack: ceil(win/4) (SAD/SSD), 5 for HOG
    int dbits;   // argmin key index bits
    int mfma_only = 0;   // SSD whose keys only the matrix-core kind holds (its own key form)
};

struct MatchParams {
    const uint8_t* L;      // left gray (device), row pitch `pitch` bytes
    const uint8_t* R;      // right gray
    const uint16_t* HL;    // HOG window histograms [H][W][10] (cost == HOG)
    const uint16_t* HR;
    int H, W, pitch;
    int minD, D, r;        // r = win/2 (0 for HOG: the window lives in the histograms)
    int win;
    int X0, X1;            // matched column band [X0, X1)
    int row0, row1;        // output rows [row0, row1)
    int lpg, lpg_log2, dbits;
    int16_t* out;
    int opitch;            // elements
    // frame batch (grid.z): frame z reads L/R + z*fs_in bytes, HL/HR + z*fs_hist elements
    // and writes out + z*fs_out elements
    int nf;
    long long fs_in, fs_out, fs_hist;
    uint32_t pad_key;      // (max_cost + 1) << dbits: key offset of padding disparities
    // set by the launchers.  k_match: segment length per lane group in units of LPG columns;
    // k_match_ring: segment width per lane group in columns (sv_match_packs.h)
    int segm;
    // ring kind: XCD-aware tile order (launch_ring_rl).  16-byte aligned: the fields from here
    // on keep the argument-block offsets that the ring kernels' scalar loads were measured with
    alignas(16) int xcd_map;
    // split ring (SAD, 256 < D <= 512): two argmin-key planes laid out like `out` (opitch,
    // fs_out) as u32, `keys_stride` elements apart; the caller owns them (ring_split_elems)
    uint32_t* keys;
    long long keys_stride;
    // The columns outside [X0, X1) of rows [row0, row1) of every frame of `out` already hold
    // the invalid value (minD - 1) * 16 and nothing has written them since: the ring kind then
    // leaves them alone.  Only a caller that owns `out` and tracks every writer of it may set
    // this (enqueue_disparity, for the context's own scratch map); the other kinds ignore it.
    int margins_done;
};

// Host-side launchers (return hipError_t as int).
int plan_match(int num_disp, int win, int cost, MatchPlan* plan);
uint64_t max_cost(int win, int cost);   // largest window cost of a (win, cost) pair
size_t match_lds_bytes(const MatchPlan& p, int r, int cost);
int launch_match(const MatchParams& a, const MatchPlan& p, int cost, hipStream_t s);
// D > 256 SAD windows run the ring kind twice (d < 256, d >= 256) into key planes and merge:
// whether a launch takes that form, and the elements of one key plane it needs
bool ring_split(int cost, int win, int num_disp);
bool ring_ssd(int cost, int win, int num_disp);   // SSD windows 5..9, D <= 256: the ring kind
// SSD on the matrix cores (sv_ssd_mfma.hip): odd windows <= 15, D a multiple of 32 up to 256
// (the key range decides: D > 128 up to win 13)
bool ssd_mfma(int cost, int win, int num_disp);
bool ssd_mfma_fits(const MatchParams& a, int cost);   // + operand alignment, r == win / 2
int launch_ssd_mfma(const MatchParams& a, hipStream_t s);
// The shape launch_ssd_mfma runs `a` with (ssd_shape of its window, D and rows): x-tiles per
// wave, x'-tiles, key index bits, rows per block band, edge masking by accumulator offset
bool ssd_mfma_shape(const MatchParams& a, int* xt, int* nt, int* mb, int* hb, int* big);
// Whether launch_match hands `a` to the matrix-core kind (its own test; nothing is launched)
bool match_is_ssd_mfma(const MatchParams& a, int cost);
long long ring_split_elems(int nf, long long fs_out, int row1, int opitch);
int launch_fill_i16(int16_t* out, int opitch, int H, int W, int16_t v, hipStream_t s);

int launch_gray(const uint8_t* bgr, int H, int W, int pitch, uint8_t* gray, hipStream_t s);
// nf frames (grid.z): frame z reads g + z*fs_in bytes and writes out + z*fs_out floats.
int launch_harris(const uint8_t* g, int H, int W, int pitch, float* out, hipStream_t s, int nf = 1,
                  long long fs_in = 0, long long fs_out = 0);
int launch_hog_hist(const uint8_t* g, int H, int W, int pitch, int win, int row0, int row1,
                    uint16_t* hist, hipStream_t s);
// Both images of nf frame pairs in one launch (grid.z = 2 nf): frame z's left/right images at
// g0/g1 + z*fs_in bytes, their histograms at h0/h1 + z*fs_hist elements.
int launch_hog_hist_pairs(const uint8_t* g0, const uint8_t* g1, int H, int W, int pitch, int win, int row0,
                          int row1, uint16_t* h0, uint16_t* h1, int nf, long long fs_in, long long fs_hist,
                          hipStream_t s);

// Census / Hamming cost (sv_census.hip).  A code plane holds one little-endian
// uint64 per pixel, row pitch `cpitch` elements: bit k = 0..61 over dy = -3..3 (outer), dx =
// -4..4 (inner) without (0, 0) is Ip(x + dx, y + dy) < I(x, y) on the replicate-clamped image.
struct CensusArgs {
    const uint8_t* g0;         // gray images, row pitch `pitch` bytes
    const uint8_t* g1;         // the pair's second image (nz > 1)
    int H, W, pitch;
    int y0, y1;                // code rows written, inside [0, H); image rows read: [y0 - 3, y1 + 3) clamped to [0, H)
    uint64_t* c0;
    uint64_t* c1;
    int cpitch;
    // images per launch (grid.z): 1 (g0 -> c0), or 2 nf: z = 2 * frame + side, frame f's images
    // at g0 / g1 + f * fs_in bytes and its planes at c0 / c1 + f * fs_codes elements
    int nz;
    long long fs_in, fs_codes;
};
// cost(x, y, d) = sum over the win x win window of popcount(CLp(x+i, y+j) ^ CRp(x+i-d, y+j)), the
// planes' coordinates replicate-clamped, all 64 bits counted; first argmin over the sweep.  Fields
// as in MatchParams: every element of rows [row0, row1) of width W is written, (minD + idx) * 16
// inside [X0, X1) and (minD - 1) * 16 outside; code rows [row0 - r, row1 + r) of [0, H) are read.
struct CensusMatchArgs {
    const uint64_t* CL;
    const uint64_t* CR;
    int H, W, cpitch;
    int minD, D, r;
    int X0, X1, row0, row1;
    int16_t* out;
    int opitch;
    int nf;                    // grid.z: frame z's planes at + z * fs_codes, its map at + z * fs_out
    long long fs_codes, fs_out;
};
int launch_census(const CensusArgs& a, hipStream_t s);
int launch_census_match(const CensusMatchArgs& a, hipStream_t s);

// Rectification (sv_rectify.hip).  ir = inv(P[:, :3] * R) row-major; k = k1 k2 p1 p2 k3 k4
// k5 k6 s1 s2 s3 s4 (OpenCV distCoeffs order, zero-padded).
struct UndistortParams {
    double ir[9];
    double fx, fy, u0, v0;
    double k[12];
    int H, W;
};
int launch_undistort_map(const UndistortParams& p, short2* map1, uint16_t* map2, hipStream_t s);
int launch_remap(const uint8_t* src, int sH, int sW, int channels, int spitch, long long sfs,
                 const short2* map1, const uint16_t* map2, int H, int W, bool gray_out, uint8_t* dst,
                 int dpitch, long long dfs, int nf, hipStream_t s);

// u8 (f32 = false) or float32 images; pitches and frame strides in bytes.
int launch_resize_linear(const void* src, int sH, int sW, int cn, int spitch, long long sfs, void* dst,
                         int dH, int dW, int dpitch, long long dfs, int nf, bool f32, hipStream_t s);

// Reductions (sv_stats.hip).
struct FrameStatsArgs {
    const uint8_t* img0;
    const uint8_t* img1;      // grid.z = 2: the second image of the pair
    int H, W, pitch, cn;
    int bh, bw;               // blocks of compute_block_homogeneity: max(1, H/48) x max(1, W/48)
    uint32_t* block_sum;      // [nimg][bh][bw]
    uint32_t* block_sq;
    uint32_t* hist;           // [nimg][256], written whole by the fold kernel
    uint32_t* hist_copies;    // accumulators [kHistCopies][nimg][256], zero on entry and exit
    // frame batches: image z of the launch (grid.z) is image z % per (img0 / img1) of frame
    // z / per, at + (z / per) * fs bytes; outputs are dense per image z
    int per;                  // images per frame: 1 or 2
    long long fs;
};
// Global histograms are accumulated into kHistCopies copies (block b adds into copy
// b % kHistCopies: hundreds of same-address atomics serialise at L2) and folded after.
constexpr int kHistCopies = 8;
int launch_frame_stats(const FrameStatsArgs& a, int nimg, hipStream_t s);

enum SelectMask { SEL_ALL = 0, SEL_POSITIVE = 1, SEL_MASK_GT = 2 };
constexpr int kMaxRanks = 4;
constexpr int kSelBatch = 16;   // arrays per batched select launch
struct SelectArgs {
    const float* x;
    const float* mask;        // SEL_MASK_GT: element i selected iff mask[i] > thr
    float thr;
    int mask_mode;
    size_t n;
    int shift, bits;          // digit = (key >> shift) & ((1 << bits) - 1)
    int nranks;
    // batches (grid.y = array y of narr): x + y * xstride, mask + y * mstride; every
    // accumulator / output below is per array (array y's block at + y * its size)
    int narr;
    size_t xstride, mstride;
    uint32_t prefix[kSelBatch][kMaxRanks];   // key >> (shift + bits) of each rank's target
    uint32_t* ghist;          // accumulators [narr][kHistCopies][kMaxRanks][2048], zero on entry and exit
    unsigned long long* counts;   // accumulators [narr][kCountSlots][16] (slot = {selected, nan, pad})
    uint32_t* hist_out;       // [narr][kMaxRanks][2048], folded by the launcher's second kernel
    unsigned long long* counts_out;   // [narr][2]: selected, nan
};
constexpr int kCountSlots = 32;   // blocks add their counts into slot blockIdx % 32 (128 B apart)
int launch_select_hist(const SelectArgs& a, hipStream_t s);

enum AffineMode {
    AFF_F32 = 0,
    AFF_F64 = 1,
    AFF_FILL = 2,
    // the frame loop's normalisations (fused_depth_map.py:2749-2759, :2793-2811)
    AFF_F32_INV = 3,          // 255 - AFF_F32
    AFF_CLIP255_INV = 4,      // 255 - clip(x * 255, 0, 255)
    AFF_NORM_CLIP255 = 5      // clip(((x - fa) / fb) * 255, 0, 255)
};
struct AffineArgs {
    const float* x;
    float* out;
    size_t n;
    int mode;
    float fa, fb, fc, fd;     // AFF_F32: fc + ((x - fa) / fb) * fd;  AFF_FILL: fc
    double ds, doff;          // AFF_F64: float(double(x) * ds + doff)
};
int launch_affine_f32(const AffineArgs& a, hipStream_t s);

// fuse_depth_maps and its filters (sv_fuse.hip; fused_depth_map.py:1560-1718).
struct GaussArgs {
    const float* src;
    float* dst;               // != src
    int H, W, r;              // r = ksize / 2 in [1, 15]; H, W > r
    float c[16];              // c[0] the centre coefficient, c[i] the one at distance i
};
enum FuseBase { FUSE_BASE_STEREO = 0, FUSE_BASE_MIDAS = 1, FUSE_BASE_FLOW = 2 };
struct FuseBlendArgs {
    const float* stereo;
    const float* conf;        // nullable: ones
    const float* midas;
    const float* flow;
    float* fused;
    uint32_t* stats;          // kFuseStatsBytes of accumulators, zero on entry (fuse_stats_fold)
    int H, W, base;
    int midas_fill, flow_fill;
    int r;                    // Gaussian radius of the fill weight (midas_fill)
    float sw, mfw, thr, hthr, k1, k2;
    float c[16];
};
constexpr int kBilateralMaxR = 7;
constexpr int kBilateralMaxTaps = 148;    // lattice points of the radius-7 disc, less the centre
constexpr int kBilateralLut = 4096 + 2;   // colour-table entries
struct BilateralArgs {
    const float* src;
    const float* lut;         // device, kBilateralLut entries (r > 0)
    float* dst_f32;           // nullable: the filter's output
    uint8_t* dst_u8;          // nullable: clip(out, 0, 255) truncated (needs stats)
    uint8_t* dst_bgr;         // nullable: cmap[dst_u8] as B, G, R bytes (needs stats)
    const uint32_t* cmap;     // 256 entries B | G << 8 | R << 16
    uint32_t* stats;          // nullable: kFuseStatsBytes of accumulators of the clipped map's range, zero on entry
    int H, W, r, ntaps;       // r = 0: no filter, the outputs elementwise; ntaps, sw, off: set by the launcher
    float scale;
    float sw[kBilateralMaxTaps];
    short off[kBilateralMaxTaps];
};
// the taps of radius r in the filter's order (dy outer, dx inner, the disc without its centre)
int bilateral_taps(int r, int* dy, int* dx);
int launch_gauss_f32(const GaussArgs& a, hipStream_t s);
int launch_fuse_blend(const FuseBlendArgs& a, hipStream_t s);
// space_w: host, one weight per tap
int launch_bilateral_f32(BilateralArgs a, const float* space_w, hipStream_t s);
// The accumulators (`stats`) of a launch: kFuseSlots copies of 4 words, kFuseSlotStride words
// apart, zero on entry; block b adds into copy b % kFuseSlots.  fuse_stats_fold merges the
// copies of a finished launch; words [0] and [1] then decode to the map's minimum and maximum.
constexpr int kFuseSlots = 32, kFuseSlotStride = 32;
constexpr size_t kFuseStatsBytes = (size_t)kFuseSlots * kFuseSlotStride * sizeof(uint32_t);
inline void fuse_stats_fold(const uint32_t* slots, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    for (int s = 0; s < kFuseSlots; ++s) {
        const uint32_t* p = slots + s * kFuseSlotStride;
        w[0] = p[0] > w[0] ? p[0] : w[0];
        w[1] = p[1] > w[1] ? p[1] : w[1];
        w[2] += p[2];
        w[3] += p[3];
    }
}
inline float fuse_stat_decode(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    float f;
    __builtin_memcpy(&f, &u, sizeof f);
    return f;
}
inline float fuse_stat_min(const uint32_t* w) { return fuse_stat_decode(~w[0]); }
inline float fuse_stat_max(const uint32_t* w) { return fuse_stat_decode(w[1]); }

// Farneback optical flow and the flow depth estimator (sv_flow.hip; fused_depth_map.py:1263-1501,
// DESIGN.md §9).  R, M and the per-level flow are planes, `plane` elements apart (>= H * W).
constexpr int kFbMaxPolyN = 7;
constexpr int kFbMaxWin = 31;
struct FbPolyArgs {
    const float* src;         // H x W, dense
    float* R;                 // 5 planes
    size_t plane;
    int H, W, n;              // n = poly_n: 2 n + 1 taps per axis
    float g[kFbMaxPolyN + 1], xg[kFbMaxPolyN + 1], xxg[kFbMaxPolyN + 1];
    double ig11, ig03, ig33, ig55;
};
struct FbUpdateArgs {
    const float* R0;          // 5 planes each
    const float* R1;
    const float* flow;        // 2 planes: dx, dy
    float* M;                 // 5 planes
    size_t plane;
    int H, W;
};
struct FbSolveArgs {
    const float* M;           // 5 planes
    size_t plane;
    float* flow;              // 2 planes, or H x W x 2 interleaved
    int interleaved;
    int H, W, m;              // m = winsize / 2
    double scale;             // 1 / winsize^2
};
struct FlowDepthArgs {
    const float* flow;        // H x W x 2
    float* depth;
    float* stable;            // nullable: stable = alpha * stable + beta * depth
    uint32_t* stats;          // kFuseStatsBytes of accumulators of depth's range, zero on entry
    int H, W;
    double m[9];
    float alpha, beta;
};
int launch_fb_u8_f32(const uint8_t* src, int H, int W, int pitch, float* dst, hipStream_t s);
int launch_fb_scale(float* x, size_t n, float k, hipStream_t s);
int launch_fb_polyexp(const FbPolyArgs& a, hipStream_t s);
int launch_fb_update_matrices(const FbUpdateArgs& a, hipStream_t s);
int launch_fb_blur_solve(const FbSolveArgs& a, hipStream_t s);
int launch_flow_depth(const FlowDepthArgs& a, hipStream_t s);
// The points step / 2, step / 2 + step, ... below n; the gather of an H x W x 2 flow (8-byte
// aligned) at that grid into out [ny * nx][2].
int flow_grid_points(int n, int step);
int launch_flow_grid(const float* flow, int H, int W, int step, float* out, hipStream_t s);

// SGBM-3WAY mode (sv_sgbm.hip).
struct SgbmArgs {
    const uint8_t* L;
    const uint8_t* R;
    int H, W, pitch;
    int minD, D, r;            // r = blockSize / 2
    int Dp;                    // per-pixel stride of the volumes: sgbm_dp(D)
    int X0, Wb;                // band [X0, X0 + Wb)
    int cap, P1, P2, uniq, disp12;
    uint16_t* hsum;            // [H][Wb][D] window-column sums of the pixel cost
    uint16_t* C;               // [H][Wb][D] window sums
    void* Llr;                 // [H][Wb][D] path costs, int16 (l32 = 0) or int32
    void* Lrl;
    void* Ltb;                 // [H][Wb][Dp] top->bottom path costs (same type as Llr)
    int l32;
    int fused;                 // R->L path fused with the WTA (L_rl never stored; see sgbm_fused)
    uint4* recs;               // [2][H][W] per-pixel BT records of L, R (k_sgbm_cost path)
    void* band;                // [H][Wb] {int16 x16 disparity after uniqueness + sub-pixel,
                               //  int16 argmin index, int32 min cost (INT_MAX: not unique)}
    int16_t* out;              // [H][opitch] final int16 x16 map
    int opitch;
    void* dummy;               // >= 64 x 128 bytes: store target of the padding lanes
    // frame batch (grid.z = frame): frame z reads L/R + z*fs_in bytes, writes out + z*fs_out
    // elements, and owns volume z (H*Wb*Dp elements of each volume's type) and band z
    long long fs_in, fs_out;
    __device__ __forceinline__ void select_frame(int z) {
        const size_t vol = (size_t)H * Wb * Dp * z;
        L += z * fs_in;
        R += z * fs_in;
        out += z * fs_out;
        hsum += vol;
        C += vol;
        const size_t lb = vol * (l32 ? 4 : 2);
        Llr = static_cast<char*>(Llr) + lb;
        Lrl = static_cast<char*>(Lrl) + lb;
        Ltb = static_cast<char*>(Ltb) + lb;
        band = static_cast<char*>(band) + (size_t)H * Wb * 8 * z;
        if (recs) recs += (size_t)2 * H * W * z;
    }
};
int sgbm_dp(int D);   // per-pixel volume stride for D disparities, -1 if D > 512
// Whether launches of nf frames of D disparities fuse the R->L path with the WTA
// (k_sgbm_rl_wta, L_rl never stored): batches of >= 8 frames with D <= 128, where the extra
// work per step hides behind other waves' chains.  Otherwise both horizontal directions run
// in k_sgbm_hpath, and for D > 128 the vertical path is fused with the WTA instead
// (k_sgbm_vpath_wta, L_tb never stored; measured faster at every batch size there: D=320
// 412 -> 459 frames/s at batch 8, 449 -> 491 at 16).  SV_SGBM_FUSED=0 / 1 forces either form.
bool sgbm_fused(int nf, int D);
// r <= 4: pixel cost and both window sums in one pass (k_sgbm_cost, no hsum
// volume); SV_SGBM_COST=0 restores k_sgbm_hsum_tiled + k_sgbm_vsum8
bool sgbm_cost_fused(int D, int r);
// aux / fork / join: a second stream and two events for the concurrent vertical path (aux =
// nullptr: everything on s)
// nf frames per launch (grid.z), laid out as described at SgbmArgs::select_frame
int launch_sgbm(const SgbmArgs& a, int nf, hipStream_t s, hipStream_t aux, hipEvent_t fork, hipEvent_t join);
// nf maps, map z at img + z*fimg; parent/size hold H*W ints per map
int launch_speckles(int16_t* img, int H, int W, int pitch, int newv, int maxsize, int maxdiff, int* parent,
                    int* size, hipStream_t s, int nf = 1, long long fimg = 0);

// Refinement of a winner-take-all map (sv_refine.hip).
struct RefineArgs {
    const uint8_t* L;          // gray frames, row pitch `pitch` bytes
    const uint8_t* R;
    int H, W, pitch;
    const int16_t* dl;         // the map to refine (may be `out`)
    const int16_t* dr;         // right-referenced map, nullable
    int16_t* out;
    int mpitch;                // elements: row pitch of dl, dr and out
    int minD, D, r;
    int lr_max_diff;           // < 0: no left-right check
    int min_curv;              // 0: no curvature test
    int subpixel;
};
// k_refine stages the tile's L rows and the R strip it can reach in LDS when both fit
// kRefineLdsBudget; beyond it the taps read global memory (same arithmetic, same results)
constexpr int kRefineLdsBudget = 8 * 1024;
size_t refine_lds_bytes(int num_disp, int win);
inline bool refine_lds_form(int num_disp, int win) { return refine_lds_bytes(num_disp, win) <= (size_t)kRefineLdsBudget; }
// cost: COST_SAD or COST_SSD when a.min_curv > 0 or a.subpixel; any cost otherwise (no taps)
int launch_refine(const RefineArgs& a, int cost, hipStream_t s);
// Column mirrors: dst[y][x] = src[y][W - 1 - x]; the u8 form mirrors two images in one launch
int launch_flip_u8(const uint8_t* s0, const uint8_t* s1, uint8_t* d0, uint8_t* d1, int H, int W, int spitch,
                   int dpitch, hipStream_t s);
int launch_flip_i16(const int16_t* src, int16_t* dst, int H, int W, int spitch, int dpitch, hipStream_t s);

// 3D reprojection and the ordered point cloud (sv_cloud.hip).
enum CloudFmt { CLOUD_I16X16 = 0, CLOUD_F32 = 1 };
struct CloudQ {
    double m[16];              // Q, row-major
};
constexpr int kCloudTile = 1024;               // pixels per compaction tile (one 256-thread block)
constexpr uint32_t kCloudNoMin = 0xffffffffu;  // the minimum's word before any value has reached it
struct CloudArgs {
    const void* disp;          // int16 x16 or f32, row pitch `pitch` elements
    int fmt, H, W, pitch;
    CloudQ Q;
    const uint32_t* dmin;      // the key k_cloud_min left; nullptr: no handleMissingValues
    float* xyz;                // k_reproject: H x W x 3; the cloud: cap x 3
    // the cloud only
    const uint8_t* bgr;        // H x W x 3, row pitch bgr_pitch bytes (read when out_bgr is set)
    int bgr_pitch;
    float min_valid, z_min, z_max;
    int rx, ry, rw, rh;        // region of interest, inside the map
    long long cap;             // points the outputs hold
    uint8_t* out_bgr;          // nullable
    uint32_t* out_index;       // nullable
    uint32_t* counts;          // cloud_tiles words: the tiles' counts, then (k_cloud_scan) their offsets
};
uint32_t cloud_tiles(int H, int W);
int launch_reproject(const CloudArgs& a, hipStream_t s);
// min over the map into *out, which holds kCloudNoMin on entry
int launch_cloud_min(const void* disp, int fmt, int H, int W, int pitch, uint32_t* out, hipStream_t s);
int launch_cloud_count(const CloudArgs& a, hipStream_t s);
int launch_cloud_scan(uint32_t* counts, uint32_t nb, uint32_t* total, uint32_t* d_count, hipStream_t s);
int launch_cloud_emit(const CloudArgs& a, hipStream_t s);

// Post-processing modes for the median kernel.
enum PostMode { POST_NONE = 0, POST_DEPTH = 1, POST_SCALED = 2 };
struct PostParams {
    int mode;
    float minf, maxf, rangef, min_disp_global;   // POST_DEPTH (depth_map.py:915-937)
    int min_disp, num_disp;                       // POST_SCALED (fused_depth_map.py:1010-1029)
    float* out_a;      // DEPTH: depth_final        SCALED: disparity_normalized (f32)
    uint8_t* out_u8;   // DEPTH: depth_normalized   SCALED: disparity_normalized (u8)
    float* out_b;      // SCALED: confidence
    // Optional display colormap of out_u8 (cv2.applyColorMap: TURBO at depth_map.py:937, JET
    // at fused_depth_map.py:1013), fused into the median kernel's epilogue: out_bgr[3i..3i+2]
    // = the B, G, R bytes of cmap[out_u8[i]] (cmap: 256 entries B | G << 8 | R << 16).
    uint8_t* out_bgr;
    const uint32_t* cmap;
    // Optional int16 x16 median map (the host paths expand it with the table on the host:
    // 2 B/px over PCIe instead of 9-11); the f32 disparity output of the median kernel is
    // then optional (disp == nullptr).
    int16_t* out_m16;
    // Optional u8 disparity index map: m / 16 - d8_base, for integer-disparity costs (SAD / SSD /
    // HOG: every median is a multiple of 16) with D <= 255 — 1 B/px for a gather over xGMI.
    uint8_t* out_d8;
    int d8_base;
    // Optional lookup table of the post-processing as a function of the int16 x16 median
    // value m in [lut_m0, lut_m0 + lut_n), built by launch_post_lut with the same f32 ops
    // (bit-identical to evaluating post_one per pixel; replaces two IEEE divisions).
    const float* lut_a;
    const uint8_t* lut_u8;
    const float* lut_b;
    int lut_m0, lut_n;
    // 4: the table holds whole disparities only (entry i = value lut_m0 + 16 i), for maps whose
    // medians are all multiples of 16 (integer-disparity costs): (D + 1) entries instead of
    // 16 (D + 1), so the epilogue's lookups stay in L1 at large D
    int lut_shift;
    // Every value of the map is an entry of the whole-disparity table: the map is the output of
    // an integer matcher (SAD / SSD / HOG: (min_disp + idx) * 16 or the invalid value, and a
    // median is one of its inputs) enqueued by the same call with this (min_disp, num_disp), and
    // the table (lut_shift 4) covers [min_disp - 1, min_disp + num_disp).  k_median_i16 then
    // indexes the table without the range and multiple-of-16 checks or the exact fallback.
    // Only the call that produced the map sets it; maps from outside keep the checks.  Each of
    // the three tables must then be readable for kLutWholeSpan entries (attach_lut allocates
    // the whole-disparity table so): the unchecked index keeps 12 bits.
    int lut_unchecked;
    int lut_cap;   // entries each of the three tables may be read for (attach_lut; >= lut_n)
};
constexpr int kLutWholeSpan = 4096;   // every int16 x16 value's whole-disparity index, mod 2^12
// Harris response computed by extra blocks of the median launch (C2): the left gray frames
// at g (+ z*fs_in bytes, row pitch `pitch`), f32 responses at out (+ z*fs_out floats, row
// pitch W).  Needs W, H >= 8 (the DPP form).  mbx is set by the launcher.
struct HarrisParams {
    const uint8_t* g;
    int pitch;
    long long fs_in;
    float* out;
    long long fs_out;
    int mbx;
    int form;   // 0: 60-column waves, 1: 248-column waves (set by the launcher)
};
// nf frames (grid.z): frame z reads in + z*fs_in and writes disp/out_* + z*fs_out elements.
// harris (nullable): also the Harris response of rows [row0, row1) of each frame.
int launch_median_i16(const int16_t* in, int H, int W, int row0, int row1, float* disp,
                      const PostParams& pp, hipStream_t s, int nf = 1, long long fs_in = 0,
                      long long fs_out = 0, const HarrisParams* harris = nullptr);
int launch_median_f32(const float* in, int H, int W, float* out, hipStream_t s);
// The median kernel's post-processing epilogue over an int16 x16 median map of n pixels
// (disp = m / 16 and the pp outputs, element-wise; the table must be attached).
int launch_post_m16(const int16_t* in, long long n, float* disp, const PostParams& pp, hipStream_t s);
int launch_post(const float* disp, int n, const PostParams& pp, hipStream_t s);
// Evaluates the post-processing of pp.mode for m = m0 .. m0+n-1 (d = m/16) into the tables.
int launch_post_lut(const PostParams& pp, int m0, int n, int step, float* lut_a, uint8_t* lut_u8,
                    float* lut_b, hipStream_t s);

}  // namespace sv
