/*
 * stereovision_amd.h — C ABI of the MI355X (gfx950) stereo-disparity engine.
 *
 * Drop-in boundary for the reference's disparity hot path.  Every entry point names the
 * reference call it replaces (file:line under AlexGr5/StereoVision):
 *
 *   sv_gray / sv_gray_dev            cv2.cvtColor(img, cv2.COLOR_BGR2GRAY)
 *                                    depth_map.py:871-880, fused_depth_map.py:979-980
 *   sv_disparity / sv_disparity_dev  cv2.StereoSGBM_create(...).compute(gl, gr)
 *                                    depth_map.py:894-909, fused_depth_map.py:988-1004
 *                                    (replaced by the north_star SAD/SSD/HOG WTA engine;
 *                                    same int16 x16 output convention)
 *   sv_median5_f32, sv_median_rows_dev   cv2.medianBlur(disparity, 5)
 *                                    depth_map.py:912, fused_depth_map.py:1007
 *   sv_depth_post                    depth/clip/mask/normalise NumPy block, depth_map.py:915-937
 *   sv_scaled_post                   clip/normalise/confidence NumPy block,
 *                                    fused_depth_map.py:1010-1029
 *   sv_depth_map                     the whole numeric body of create_depth_map
 *                                    (depth_map.py:868-937) minus the colormap
 *   sv_depth_map_color               ... including the colormap (depth_map.py:937)
 *   sv_stereo_scaled                 the whole numeric body of create_depth_map_stereo_scaled
 *                                    (fused_depth_map.py:976-1029) minus colormap/putText
 *   sv_harris, sv_hog_hist           north_star stages with no reference counterpart
 *   sv_init_undistort_rectify_map    cv2.initUndistortRectifyMap(K, dist, R, P, size, CV_16SC2)
 *                                    depth_map.py:636-641, fused_depth_map.py:402-407
 *   sv_remap / sv_remap_dev          cv2.remap(img, map1, map2, cv2.INTER_LINEAR)
 *                                    depth_map.py:815-826, fused_depth_map.py:480-491
 *   sv_resize_linear                 cv2.resize(img, size) INTER_LINEAR (fused_depth_map.py:474-476)
 *   sv_frame_stats                   image statistics of detect_camera_occlusion
 *                                    (fused_depth_map.py:131-301)
 *   sv_select_count/ranks            order statistics of np.percentile in
 *                                    calibrate_midas_to_stereo / normalize_to_stereo_range
 *                                    (fused_depth_map.py:1169-1257, 1503-1554)
 *   sv_gauss_blur_f32_dev            cv2.GaussianBlur(x, (k, k), 0) on a float32 map
 *                                    (fused_depth_map.py:1638)
 *   sv_bilateral_f32_dev             cv2.bilateralFilter on a float32 map
 *                                    (fused_depth_map.py:1688, :2769, :1403-1411), optionally with
 *                                    the clip / uint8 / colormap / range block (:1696-1708)
 *   sv_fuse_blend_dev                the blend of fuse_depth_maps (fused_depth_map.py:1603-1684)
 *   sv_farneback_flow_dev            cv2.calcOpticalFlowFarneback(prev, gray, None, 0.5, 3, 15, 3, 5,
 *                                    1.2, 0) (fused_depth_map.py:1361-1370)
 *   sv_flow_depth_dev                cv2.perspectiveTransform, the residual flow, 1 / (m + 0.5) and
 *                                    the exponential average of OpticalFlowDepthEstimator
 *                                    (fused_depth_map.py:1384-1400, :1492-1498)
 *   sv_flow_grid_dev                 the flow at the ego-motion grid of _estimate_ego_motion
 *                                    (fused_depth_map.py:1447-1455)
 *   sv_affine_f32_dev modes 3-5      the frame loop's normalisations of the flow depth and of the
 *                                    MiDaS map without stereo (fused_depth_map.py:2749-2759,
 *                                    :2793-2811)
 *   sv_multi_gpu_batch               the per-frame create_depth_map loop, frame-sharded over
 *                                    several devices from one process
 *   sv_rectify_pair                  the two remap calls of apply_stereo_rectification
 *                                    (depth_map.py:779-834, fused_depth_map.py:444-500) with
 *                                    the maps resident on the device
 *
 * Conventions
 *   - plain pointers and sizes only; images are row-major uint8, `stride` in bytes;
 *   - host (`sv_x`) entry points take caller-owned host buffers and block until the result
 *     is in them; device (`sv_x_dev`) entry points take device pointers and a hipStream_t
 *     passed as void* (NULL = the context's own stream) and return after enqueueing;
 *   - return 0 on success, a negative errno-style code otherwise; no C++ exception crosses
 *     the ABI; sv_last_error() gives the calling thread's last message;
 *   - a context is bound to one device; calls on one context are serialised by an internal
 *     mutex and each call selects the context's device first (device selection is
 *     per-thread in HIP), so contexts may be used from any thread (the reference calls the
 *     disparity path from a ThreadPoolExecutor worker, fused_depth_map.py:2591-2598);
 *   - the context owns its device buffers and pinned staging, grown on demand and reused.
 */
#ifndef STEREOVISION_AMD_H
#define STEREOVISION_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SV_API_VERSION 1

typedef struct sv_ctx sv_ctx;

/* SAD / SSD / HOG: the north_star winner-take-all engine.  SGBM: OpenCV's SGBM-3WAY
 * algorithm restated (the reference's own matcher), with the reference's parameters
 * P1 = 24 win^2, P2 = 96 win^2, disp12MaxDiff 1, uniquenessRatio 10, speckle 100 / 32,
 * preFilterCap 63 (depth_map.py:894-906) when selected through the generic entry points;
 * sv_sgbm / sv_sgbm_dev take every parameter.  SGBM is frame-only (no row bands).
 * CENSUS: winner-take-all over the Hamming distance of 9 x 7 census codes (sv_census_dev
 * below): unchanged by any monotone brightness change of either frame.  win odd in [1, 15],
 * num_disp in [1, 512]; the map is the int16 x16 whole-pixel map of SAD / SSD / HOG. */
enum sv_cost { SV_COST_SAD = 0, SV_COST_SSD = 1, SV_COST_HOG = 2, SV_COST_SGBM = 3, SV_COST_CENSUS = 4 };

enum sv_status {
    SV_OK = 0,
    SV_EHIP = -5,     /* HIP runtime error (message in sv_last_error) */
    SV_ENOMEM = -12,
    SV_ENODEV = -19,
    SV_EINVAL = -22,
    SV_ERANGE = -34   /* parameters whose argmin key would overflow 32 bits: (cmax << dbits)
                         >= 2^32, or ((2 cmax + 2) << dbits) >= 2^32 when num_disp leaves
                         padding disparities in the lane plan (cmax = largest window cost) */
};

/* post-processing modes of sv_map_out.mode / sv_post_m16_dev */
enum sv_post { SV_POST_NONE = 0, SV_POST_DEPTH = 1, SV_POST_SCALED = 2 };

/* kernel ids for the profiling counters */
enum sv_kernel {
    SV_K_GRAY = 0, SV_K_HARRIS = 1, SV_K_HOG = 2, SV_K_MATCH = 3, SV_K_MEDIAN = 4, SV_K_POST = 5,
    SV_K_REMAP = 6, SV_K_UNDISTORT = 7, SV_K_RESIZE = 8, SV_K_STATS = 9, SV_K_SELECT = 10,
    SV_K_AFFINE = 11, SV_K_SGBM = 12, SV_K_SPECKLE = 13,
    SV_K_GATHER = 14,   /* multi-GPU gathers to the root (RCCL / peer copies), root stream */
    SV_K_SCATTER = 15,  /* multi-GPU input scatters (row bands + halos), per context stream */
    SV_K_H2D = 16,      /* host-buffer entry points: the frame pair's upload (per image) */
    SV_K_D2H = 17,      /* host-buffer entry points: the outputs' download */
    SV_K_FUSE = 18,     /* fuse_depth_maps: the blend, the Gaussian and the bilateral filter */
    SV_K_FLOW = 19,     /* Farneback optical flow and the flow depth (every launch of sv_flow.hip) */
    SV_K_FLIP = 20,     /* k_flip_rows: the column mirrors around the right-referenced match */
    SV_K_REFINE = 21,   /* k_refine: L-R check, curvature test and sub-pixel step of a WTA map */
    SV_K_REPROJECT = 22,    /* k_reproject: the dense H x W x 3 map of a disparity map */
    SV_K_CLOUD_MIN = 23,    /* k_cloud_min: the map's minimum (handle_missing) */
    SV_K_CLOUD_COUNT = 24,  /* k_cloud_count: the points of every compaction tile */
    SV_K_CLOUD_SCAN = 25,   /* k_cloud_scan: the tiles' offsets and the cloud's size */
    SV_K_CLOUD_EMIT = 26,   /* k_cloud_emit: xyz, colours and pixel indices in pixel order */
    SV_K_CENSUS = 27,       /* k_census: the census transform (k_census_match counts as SV_K_MATCH) */
    SV_NKERNELS = 28
};

int sv_version(void);
const char* sv_last_error(void);
int sv_device_count(int* n);
int sv_create(int device, sv_ctx** out);
void sv_destroy(sv_ctx* ctx);
int sv_synchronize(sv_ctx* ctx);
/* Waits for the context's work and frees its grow-only device scratch (disparity, HOG and
 * SGBM volumes, band buffers); the next call allocates what it needs again.  SGBM batches
 * size their volumes to SV_SGBM_BUDGET_GB, default a quarter of the device's free memory
 * (at most 48 GiB). */
int sv_release_scratch(sv_ctx* ctx);
/* Cross-stream ordering on the context's device (NULL stream = the context stream), with 16
 * event slots per context: sv_event_record marks the work enqueued on `stream` so far;
 * sv_stream_wait_event makes work enqueued on `stream` afterwards wait for that mark (e.g.
 * a gather on a communication stream overlapping the next frame batch's kernels). */
int sv_event_record(sv_ctx* ctx, int slot, void* stream);
int sv_stream_wait_event(sv_ctx* ctx, int slot, void* stream);
void* sv_stream(sv_ctx* ctx);

/* Engine plan for a configuration: disparities per lane, lanes per group, LDS bytes per
 * 256-thread block of the matching kernel. */
int sv_plan(int num_disp, int win, int cost, int* dpl, int* lpg, int* lds_bytes);

/* Which matcher kind sv_disparity_dev / sv_disparity_batch_dev would run for these arguments
 * (n_frames = 1, frame_stride = 0 for sv_disparity_dev; whole frames are row0 = 0, row1 = H).
 * Launches nothing and reads no device memory: only the addresses' alignment counts.
 * mfma: the SSD matrix-core kind takes the call, with xt x-tiles per wave, nt x'-tiles, mb key
 * index bits, hb rows per block band, and big = 1 when the edge cells are masked by an
 * accumulator offset (0: by a per-cell select).  mfma_only: no other kind holds this
 * (num_disp, win) pair's keys, so a call with mfma = 0 (and rows and a matched band to
 * compute) returns an error.  Returns what the call's own argument checks return (SV_EINVAL,
 * SV_ERANGE). */
typedef struct sv_ssd_mfma_info {
    int mfma, mfma_only;
    int xt, nt, mb, hb, big;
} sv_ssd_mfma_info;
int sv_ssd_mfma_query(const uint8_t* d_left, const uint8_t* d_right, int H, int W, int pitch,
                      int64_t frame_stride, int n_frames, int min_disp, int num_disp, int win, int cost,
                      int row0, int row1, int out_pitch, sv_ssd_mfma_info* info);

/* ---- host-memory entry points (drop-in path) ------------------------------------- */
int sv_gray(sv_ctx* ctx, const uint8_t* bgr, int H, int W, int stride, uint8_t* gray);

/* left/right: HxW (channels = 1) or HxWx3 BGR (channels = 3).  disp16: HxW int16 = d*16,
 * invalid = (min_disp-1)*16.  Every entry point that computes a disparity map, for every
 * cost, requires min_disp >= -2047 and min_disp + num_disp - 1 <= 2047, so that the invalid
 * value and the largest disparity both fit the int16 x16 map (SV_EINVAL otherwise).
 * harris (nullable): HxW f32 Harris response of the left gray image. */
int sv_disparity(sv_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W,
                 int channels, int stride, int min_disp, int num_disp, int win, int cost,
                 int16_t* disp16, float* harris);

int sv_median5_f32(sv_ctx* ctx, const float* in, int H, int W, float* out);

/* min_depth/max_depth: float32 of the caller's bounds; depth_range: float32 of
 * (max_depth - min_depth) computed in double (NumPy-2 semantics of depth_map.py:936);
 * min_disp_global: the module global MIN_DISP (depth_map.py:932). */
int sv_depth_post(sv_ctx* ctx, const float* disparity, int n, float min_depth, float max_depth,
                  float depth_range, float min_disp_global, float* depth_final,
                  uint8_t* depth_normalized);

int sv_scaled_post(sv_ctx* ctx, const float* disparity, int n, int min_disp, int num_disp,
                   float* disparity_normalized, uint8_t* normalized_u8, float* confidence);

int sv_depth_map(sv_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W,
                 int channels, int stride, int min_disp, int num_disp, int win, int cost,
                 float min_depth, float max_depth, float depth_range, float min_disp_global,
                 float* depth_final, float* disparity, uint8_t* depth_normalized);

int sv_stereo_scaled(sv_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W,
                     int channels, int stride, int min_disp, int num_disp, int win, int cost,
                     float* disparity_normalized, float* disparity, uint8_t* normalized_u8,
                     float* confidence);

/* The same two entry points with the display colormap of the drop-ins fused into the
 * median/post kernel (cv2.applyColorMap(depth_normalized, COLORMAP_TURBO) at depth_map.py:937;
 * COLORMAP_JET of the normalised disparity at fused_depth_map.py:1013): cmap_bgr is the
 * 256 x 3 BGR table (the drop-ins pass cv2's own table, read back from cv2.applyColorMap, when
 * cv2 is importable), depth_colormap the H x W x 3 BGR output.  depth_normalized /
 * normalized_u8 are nullable here. */
int sv_depth_map_color(sv_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W,
                       int channels, int stride, int min_disp, int num_disp, int win, int cost,
                       float min_depth, float max_depth, float depth_range, float min_disp_global,
                       const uint8_t* cmap_bgr, float* depth_final, float* disparity,
                       uint8_t* depth_normalized, uint8_t* depth_colormap);
int sv_stereo_scaled_color(sv_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W,
                           int channels, int stride, int min_disp, int num_disp, int win, int cost,
                           const uint8_t* cmap_bgr, float* disparity_normalized, float* disparity,
                           uint8_t* normalized_u8, float* confidence, uint8_t* depth_colormap);

int sv_harris(sv_ctx* ctx, const uint8_t* gray, int H, int W, int stride, float* out);

/* Row band [row0, row1) of the disparity map (halo rows read from the full frame, so the
 * bands of a row-tiled multi-GPU split reassemble bit-exactly); only those rows of
 * disp16 (HxW) are written. */
int sv_disparity_rows(sv_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W,
                      int channels, int stride, int min_disp, int num_disp, int win, int cost,
                      int row0, int row1, int16_t* disp16);

/* out: [H][W][10] uint16 (9 bins + 1 zero pad) window histograms */
int sv_hog_hist(sv_ctx* ctx, const uint8_t* gray, int H, int W, int stride, int win,
                uint16_t* out);

/* ---- device-memory entry points (zero-copy, row bands for multi-GPU sharding) ---- */
int sv_gray_dev(sv_ctx* ctx, const uint8_t* d_bgr, int H, int W, int pitch, uint8_t* d_gray,
                void* stream);

/* Computes output rows [row0, row1) of the disparity map of full-frame gray device images
 * (halo rows are read from the full frame, so bands tile the frame bit-exactly). */
int sv_disparity_dev(sv_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int H, int W,
                     int pitch, int min_disp, int num_disp, int win, int cost, int row0,
                     int row1, int16_t* d_disp16, int out_pitch, void* stream);

/* Outputs of the median + post-processing epilogue: cv2.medianBlur(disparity, 5) of an int16
 * x16 disparity map (depth_map.py:909-912, fused_depth_map.py:1004-1007) and the NumPy post
 * that follows it — SV_POST_DEPTH: depth/clip/mask/normalise (depth_map.py:915-937),
 * SV_POST_SCALED: clip/normalise/confidence (fused_depth_map.py:1010-1029).  Every pointer is
 * nullable (not written) and, except cmap_bgr, a device pointer; at least one output must be
 * set.  One descriptor serves every median launch (row bands, frame batches, the root of a
 * multi-device call) instead of one entry point per output combination. */
typedef struct sv_map_out {
    int mode;                  /* sv_post: what out_a / out_u8 / out_b hold */
    float min_depth;           /* SV_POST_DEPTH: float32 of the caller's bounds */
    float max_depth;
    float depth_range;         /* float32 of (max_depth - min_depth) computed in double
                                  (NumPy-2 semantics of depth_map.py:936) */
    float min_disp_global;     /* the module global MIN_DISP (depth_map.py:932) */
    float* disparity;          /* f32 median / 16 (create_depth_map's `disparity`) */
    float* out_a;              /* DEPTH: depth_final       SCALED: disparity_normalized */
    uint8_t* out_u8;           /* DEPTH: depth_normalized  SCALED: its u8 image */
    float* out_b;              /* SCALED: confidence */
    int16_t* med16;            /* int16 x16 median map (OpenCV's fixed point; disparity =
                                  med16 / 16 exactly): 2 B/px for a gather or a download */
    uint8_t* d8;               /* u8 disparity index median / 16 - (min_disp - 1), 0 =
                                  invalid: integer-disparity costs (SAD / SSD / HOG) with
                                  num_disp <= 255, else -EINVAL (1 B/px) */
    const uint8_t* cmap_bgr;   /* with bgr: the 256 x 3 BGR colormap table (host memory) */
    uint8_t* bgr;              /* cv2.applyColorMap(out_u8, cmap) (TURBO at depth_map.py:937,
                                  JET at fused_depth_map.py:1013), H x W x 3 */
    float* harris;             /* sv_depth_map_batch_dev only: the Harris response of every
                                  LEFT frame, computed by extra blocks of the median launch */
} sv_map_out;

/* Median (+ post) of output rows [row0, row1) of an H x W int16 x16 map (halo rows read from
 * the full map, so row bands of a multi-GPU split reassemble bit-exactly); outputs at their
 * full-frame offsets.  cost: the matcher that produced the map (integer-disparity maps use the
 * whole-disparity post table; SGBM's sub-pixel maps the full one). */
int sv_median_rows_dev(sv_ctx* ctx, const int16_t* d_disp16, int H, int W, int row0, int row1,
                       int min_disp, int num_disp, int cost, const sv_map_out* out, void* stream);
/* The post-processing of n median values d_med16 (int16 x16, e.g. maps gathered over xGMI):
 * d_disparity = m / 16 (nullable), and mode's outputs element-wise, exactly as the median
 * kernel's epilogue writes them (depth_map.py:915-936 / fused_depth_map.py:1010-1024). */
int sv_post_m16_dev(sv_ctx* ctx, const int16_t* d_med16, int64_t n, int mode, float min_depth,
                    float max_depth, float depth_range, float min_disp_global, int min_disp,
                    int num_disp, float* d_disparity, float* d_out_a, uint8_t* d_out_u8,
                    float* d_out_b, void* stream);

/* ---- frame batches (one launch per kernel over grid.z) ------------------------------
 * A batch of n_frames equally-shaped gray pairs, frame z at d_left/d_right + z*frame_stride
 * bytes.  Replaces the reference's per-frame loop over the same calls (depth_map.py:837-946
 * called once per captured frame, fused_depth_map.py:2591-2598) when frames are queued:
 * one launch per kernel fills the GPU even for small frames.  The context's internal scratch
 * is ordered across streams (a call on another stream waits for the previous user of the
 * scratch).  cost = SV_COST_SGBM runs every SGBM stage once per chunk of up to 32 frames
 * (volumes of ~1.5 GB per 1080p D=128 frame, within the scratch budget of
 * sv_release_scratch); chunks of >= 8 frames fuse the right-to-left path with the
 * winner-take-all.
 *
 * sv_disparity_batch_dev: the int16 x16 maps only, at an explicit out_pitch /
 * out_frame_stride (elements). */
int sv_disparity_batch_dev(sv_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                           int n_frames, int H, int W, int pitch, int64_t frame_stride,
                           int min_disp, int num_disp, int win, int cost, int16_t* d_disp16,
                           int out_pitch, int64_t out_frame_stride, void* stream);
/* sv_depth_map_batch_dev: the whole device path (disparity -> median -> post) over the batch,
 * every output of `out` dense per frame (frame z at + z*H*W elements).  stages:
 *   SV_STAGE_ALL     both launches; d_disp16 nullable (the context's scratch, else the raw
 *                    int16 x16 maps are kept there, dense per frame)
 *   SV_STAGE_MATCH   the disparity launch only, into d_disp16 (required); out unused
 *   SV_STAGE_MEDIAN  the median launch only, from d_disp16 (required; d_left read only for
 *                    out->harris) — with SV_STAGE_MATCH on another stream or context, the two
 *                    launches of consecutive batches overlap (the HBM-bound median beside the
 *                    VALU-bound match). */
#define SV_STAGE_MATCH 1
#define SV_STAGE_MEDIAN 2
#define SV_STAGE_ALL 3
int sv_depth_map_batch_dev(sv_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                           int n_frames, int H, int W, int pitch, int64_t frame_stride,
                           int min_disp, int num_disp, int win, int cost, int stages,
                           int16_t* d_disp16, const sv_map_out* out, void* stream);

/* Frame-sharded batch over several devices from ONE host process:
 * replaces the reference's per-frame loop over create_depth_map (depth_map.py:837-946,
 * called once per captured frame; fused_depth_map.py:2591-2598 submits frames to a worker
 * pool).  Host frames f of left/right at + f*H*W*channels (channels 1 = gray, 3 = BGR);
 * outputs dense per frame (+ f*H*W).  Frames are split into ndev contiguous shards; context
 * k (its own device and stream) stages, computes and returns shard k on its own host
 * thread, concurrently with the others.  Every context must be distinct; the post-
 * processing is create_depth_map's (depth_final, disparity, depth_normalized). */
int sv_multi_gpu_batch(sv_ctx* const* ctxs, int ndev, const uint8_t* left, const uint8_t* right, int n_frames,
                       int H, int W, int channels, int min_disp, int num_disp, int win, int cost, float min_depth,
                       float max_depth, float depth_range, float min_disp_global, float* depth_final,
                       float* disparity, uint8_t* depth_normalized);
/* ---- multi-GPU: RCCL communicators + device-side gathers --------
 * The reference has no distributed code; its unit of work is one frame pair per call
 * (fused_depth_map.py:2591-2598 submits frames to a worker pool, depth_map.py:1181-1183
 * calls create_depth_map once per frame).  The MI355X build shards frames (C4) or the row
 * bands of one frame (C5) over GPUs and gathers the finished maps to one device over xGMI.
 * RCCL (librccl.so.1) is loaded with dlopen on first use.
 *   sv_comm_init_rank   one process per GPU (ncclCommInitRank; the id comes from one rank's
 *                       sv_comm_unique_id, shared out of band)
 *   sv_comm_init_all    one process, ndev distinct devices (ncclCommInitAll); comms[k] has
 *                       rank k
 *   sv_comm_barrier / sv_comm_allreduce_max_f64   blocking, one communicator per process
 *   sv_comm_gatherv     rank k's send_bytes land at d_recv + recv_offsets[k] on `root`
 *                       (ncclSend/ncclRecv in one group; the root's own block is a device
 *                       copy unless it is already in place); enqueued on `stream` (NULL =
 *                       the communicator's own stream, which nothing orders against the
 *                       caller's compute streams: pass the stream the data was produced on) */
typedef struct sv_comm sv_comm;
#define SV_COMM_ID_BYTES 128
int sv_comm_available(void);
int sv_comm_unique_id(uint8_t* id);
/* sv_comm_init_rank: non-blocking ncclCommInitRankConfig polled until it completes or
 * timeout_s seconds pass (<= 0: no limit); on an error or the deadline the half-built
 * communicator is aborted (ncclCommAbort) and -EHIP returned, so a rank whose peers failed
 * during bootstrap comes back instead of blocking forever. */
int sv_comm_init_rank(int device, int nranks, int rank, const uint8_t* id, double timeout_s,
                      sv_comm** out);
int sv_comm_init_all(int ndev, const int* devices, sv_comm** comms);
void sv_comm_destroy(sv_comm* comm);
int sv_comm_rank(sv_comm* comm, int* rank, int* nranks, int* device);
int sv_comm_barrier(sv_comm* comm);
int sv_comm_allreduce_max_f64(sv_comm* comm, double* value);
int sv_comm_gatherv(sv_comm* comm, const void* d_send, uint64_t send_bytes, void* d_recv,
                    const uint64_t* recv_offsets, const uint64_t* recv_bytes, int root, void* stream);
/* The inverse of sv_comm_gatherv: the root's send_bytes[k] bytes at d_send + send_offsets[k]
 * land in rank k's d_recv (recv_bytes); the root's own block is a device copy unless it is
 * already in place.  Enqueued on `stream` (NULL = the communicator's stream: the caller then
 * orders it against its own streams). */
int sv_comm_scatterv(sv_comm* comm, const void* d_send, const uint64_t* send_offsets,
                     const uint64_t* send_bytes, void* d_recv, uint64_t recv_bytes, int root,
                     void* stream);
int sv_comm_synchronize(sv_comm* comm);

/* Gather-only map formats (north_star: "a trivial RCCL gather of the final disparity rows"):
 *   SV_MAP_M16  int16 x16 medians (OpenCV's fixed-point disparity after medianBlur,
 *               depth_map.py:909-912), 2 B/px over xGMI
 *   SV_MAP_D8   u8 disparity indices median / 16 - (min_disp - 1) (0 = invalid), 1 B/px:
 *               exact for the integer-disparity costs (SAD / SSD / HOG) with num_disp <= 255 */
#define SV_MAP_M16 1
#define SV_MAP_D8 2

/* One process driving ndev contexts; replaces the reference's per-frame loop
 * over create_depth_map (depth_map.py:837-946; fused_depth_map.py:2591-2598 submits frames to a
 * worker pool) and returns the disparity rows the reference returns (depth_map.py:909-912).
 *   shard SV_SHARD_FRAMES (C4): context k computes its n_frames[k] frames at left[k] / right[k]
 *         (+ z*frame_stride bytes, on its own device); outputs dense in context order (frame z
 *         of context k at index sum(n_frames[:k]) + z).
 *   shard SV_SHARD_ROWS (C5): ONE frame; context k computes output rows
 *         [H*k/ndev, H*(k+1)/ndev) (window and median halos read locally, so the bands
 *         reassemble bit-exactly); n_frames and frame_stride unused.  inputs:
 *           SV_INPUTS_RESIDENT  every context holds the full gray frame (left[k] on its device)
 *           SV_INPUTS_SCATTER   the frame is on the root only (left[0]); context k > 0 first
 *                               receives the input rows its band reads (sv_band_rows_in) over
 *                               RCCL / peer copies (profiled as SV_K_SCATTER on the root)
 *           SV_INPUTS_HOST      the frame is in HOST memory (left[0], pinned for overlap: see
 *                               sv_host_register); every context uploads its own band's input
 *                               rows over its own PCIe link (no xGMI scatter; SV_K_H2D)
 *         Frames mode takes SV_INPUTS_RESIDENT only.
 * out (on ctxs[0]'s device) selects what the root holds: create_depth_map's outputs
 * (mode SV_POST_DEPTH with disparity, out_a, out_u8: the peers' maps cross xGMI as int16 x16
 * and are expanded on the root, k_post_m16 profiled as SV_K_POST), or gather-only the map of
 * every frame / the full frame as med16 (SV_MAP_M16) or d8 (SV_MAP_D8), nothing expanded.
 * comms (nullable; else comms[k] is rank k of an ndev-rank communicator on ctxs[k]'s device):
 * gathers / scatters as RCCL send/recv over xGMI; NULL: hipMemcpyPeerAsync (a plain device copy
 * when two contexts share a device).  Returns after enqueueing: the outputs are complete once
 * ctxs[0]'s stream is (sv_synchronize(ctxs[0])). */
#define SV_SHARD_FRAMES 0
#define SV_SHARD_ROWS 1
#define SV_INPUTS_RESIDENT 0
#define SV_INPUTS_SCATTER 1
#define SV_INPUTS_HOST 2
int sv_multi_gpu_dev(sv_ctx* const* ctxs, sv_comm* const* comms, int ndev, int shard, int inputs,
                     const uint8_t* const* left, const uint8_t* const* right, const int* n_frames,
                     int H, int W, int pitch, int64_t frame_stride, int min_disp, int num_disp,
                     int win, int cost, const sv_map_out* out);

/* Row bands of a `world`-way row tiling for rank `rank`: out6 = {r0, r1 (output rows), h0, h1
 * (disparity rows incl. the median halo), in0, in1 (input rows the band reads)}.  Device
 * buffers holding only input rows [in0, in1) must keep SV_BAND_MARGIN spare rows above and
 * below them (read-ahead of the row pipelines; never used as data). */
#define SV_BAND_MARGIN 8
int sv_band_rows_in(int H, int rank, int world, int win, int cost, int* out6);

int sv_harris_dev(sv_ctx* ctx, const uint8_t* d_gray, int H, int W, int pitch, float* d_out,
                  void* stream);
/* Harris response of n_frames gray frames (frame z at d_gray + z*frame_stride bytes, output
 * dense at d_out + z*H*W floats), one launch for the batch (C2: Harris beside the disparity
 * of a frame stream). */
int sv_harris_batch_dev(sv_ctx* ctx, const uint8_t* d_gray, int n_frames, int H, int W, int pitch,
                        int64_t frame_stride, float* d_out, void* stream);
int sv_hog_hist_dev(sv_ctx* ctx, const uint8_t* d_gray, int H, int W, int pitch, int win,
                    int row0, int row1, uint16_t* d_out, void* stream);

/* ---- rectification ---------------------------------------
 * K: 3x3 camera matrix, row-major doubles.  dist: ndist in {0, 4, 5, 8, 12, 14} OpenCV
 * distCoeffs (k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4 [tx ty]]]]; a nonzero tilt is
 * SV_EINVAL).  R: 3x3 rectification rotation or NULL (identity).  P: new camera matrix,
 * 3 x p_cols row-major (p_cols 3 or 4; NULL = K).  Maps (CV_16SC2 + CV_16UC1 layout, dense
 * H x W): map1 = int16 (x, y) pairs of the source pixel, map2 = (y & 31) * 32 + (x & 31) of
 * the 1/32-pixel fraction.  Rounding of the f64 source position follows cvRound. */
int sv_init_undistort_rectify_map(sv_ctx* ctx, const double* K, const double* dist, int ndist,
                                  const double* R, const double* P, int p_cols, int H, int W,
                                  int16_t* map1, uint16_t* map2);
int sv_init_undistort_rectify_map_dev(sv_ctx* ctx, const double* K, const double* dist, int ndist,
                                      const double* R, const double* P, int p_cols, int H, int W,
                                      int16_t* d_map1, uint16_t* d_map2, void* stream);

/* remap INTER_LINEAR, BORDER_CONSTANT 0: src sH x sW x channels (1 or 3) u8 with row pitch
 * `stride` bytes; map1/map2 (map2 nullable = integer maps) and dst are H x W.  Host memory. */
int sv_remap(sv_ctx* ctx, const uint8_t* src, int sH, int sW, int channels, int stride,
             const int16_t* map1, const uint16_t* map2, int H, int W, uint8_t* dst);
/* Device version over a batch of n_frames sources (frame z at d_src + z*src_frame_stride,
 * output at d_dst + z*dst_frame_stride), one launch.  gray_out (channels == 3 only) writes
 * cvtColor(remap(src), BGR2GRAY) instead of the BGR result: the rectified gray image the
 * matcher reads, in one pass. */
int sv_remap_dev(sv_ctx* ctx, const uint8_t* d_src, int sH, int sW, int channels, int src_pitch,
                 int64_t src_frame_stride, const int16_t* d_map1, const uint16_t* d_map2, int H, int W,
                 int gray_out, uint8_t* d_dst, int dst_pitch, int64_t dst_frame_stride, int n_frames,
                 void* stream);
/* apply_stereo_rectification with device-resident maps: host left/right (sH x sW x channels,
 * row pitch `stride`) -> host rectified left/right (H x W x channels, dense). */
int sv_rectify_pair(sv_ctx* ctx, const int16_t* d_map1_left, const uint16_t* d_map2_left,
                    const int16_t* d_map1_right, const uint16_t* d_map2_right, int H, int W,
                    const uint8_t* left, const uint8_t* right, int sH, int sW, int channels, int stride,
                    uint8_t* out_left, uint8_t* out_right);

/* cv2.resize(src, (dW, dH)) INTER_LINEAR for u8 gray/BGR (fused_depth_map.py:474-476 and
 * :2498-2507, depth_map.py:757-776, ensure_same_size depth_map.py:39-71): OpenCV's
 * fixed-point two-pass bilinear; an exact 2x downscale is OpenCV's INTER_AREA fast path. */
int sv_resize_linear(sv_ctx* ctx, const uint8_t* src, int sH, int sW, int channels, int stride,
                     uint8_t* dst, int dH, int dW);
int sv_resize_linear_dev(sv_ctx* ctx, const uint8_t* d_src, int sH, int sW, int channels,
                         int src_pitch, int64_t src_frame_stride, uint8_t* d_dst, int dH, int dW,
                         int dst_pitch, int64_t dst_frame_stride, int n_frames, void* stream);

/* ---- SGBM-3WAY mode -----------------------------------------
 * cv2.StereoSGBM_create(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff,
 * preFilterCap, uniquenessRatio, speckleWindowSize, speckleRange, MODE_SGBM_3WAY)
 * .compute(left, right) (depth_map.py:894-909): int16 x16 map, invalid = (minD-1)*16.
 * Semantics in oracle/sv_sgbm_oracle.py (one stripe; int32 aggregation).  Limits:
 * num_disp <= 512, block_size odd <= 15, P2 < 349525, P1 < P2 (P2 = max(P2, P1+1)),
 * W <= 16384, min_disp >= -2047 and min_disp + num_disp - 1 <= 2047 (the int16 x16 map).
 * disp12MaxDiff < 0 disables the left-right check; speckleWindowSize <= 0 the filter. */
int sv_sgbm(sv_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W, int channels,
            int stride, int min_disp, int num_disp, int block_size, int P1, int P2,
            int disp12_max_diff, int pre_filter_cap, int uniqueness_ratio,
            int speckle_window_size, int speckle_range, int16_t* disp16);
int sv_sgbm_dev(sv_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int H, int W, int pitch,
                int min_disp, int num_disp, int block_size, int P1, int P2, int disp12_max_diff,
                int pre_filter_cap, int uniqueness_ratio, int speckle_window_size,
                int speckle_range, int16_t* d_disp16, int out_pitch, void* stream);

/* cv2.filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) on an int16 map, in place: the
 * speckle stage of StereoSGBM (OpenCV calib3d, called from stereo.compute at
 * depth_map.py:909).  4-connected regions whose neighbours differ by <= max_diff and that
 * hold <= max_speckle_size pixels are set to new_val; max_speckle_size <= 0 is a no-op. */
int sv_filter_speckles(sv_ctx* ctx, int16_t* img, int H, int W, int new_val, int max_speckle_size, int max_diff);
int sv_filter_speckles_dev(sv_ctx* ctx, int16_t* d_img, int H, int W, int pitch, int new_val,
                           int max_speckle_size, int max_diff, void* stream);

/* ---- refinement of the winner-take-all maps ---------------------------
 * What cv2.StereoBM adds to its argmin, for the SAD / SSD / HOG maps: a left-right check, a
 * curvature (texture) test, the parabolic sub-pixel step in the int16 x16 convention and the
 * speckle filter.  Semantics: tests/sv_refine_oracle.py.  Whole frames only (no row bands, no
 * batches).  INV = (min_disp - 1) * 16.
 *
 * sv_disparity_right_dev: the right-referenced map, defined for every cost as the matcher run
 * on the column-mirrored pair (right as left) and mirrored back; valid columns
 * [max(-min_disp, 0), W - max(min_disp + num_disp, 0)), INV elsewhere.
 *
 * sv_refine_dev: per pixel of d_disp16 (any int16 map; d_out16 == d_disp16 allowed; the three
 * maps share out_pitch, in elements): values that are not 16 d with d in the sweep -> INV; with
 * lr_max_diff >= 0 and a right map, a pixel whose counterpart x - d lies in the image, is valid
 * there and differs by more than lr_max_diff -> INV; min_curvature > 0: cm + cp - 2 c0 <
 * min_curvature -> INV (the window costs at d - 1, d + 1 and d, mirrored at the ends of the
 * sweep); subpixel: d * 16 plus the parabola's vertex offset in [-8, 8]; speckle_window > 0:
 * sv_filter_speckles_dev(out, INV, speckle_window, 16 * speckle_range).  HOG takes the L-R
 * check and the speckle filter only.  SV_EINVAL before any launch: null pointers (the right
 * map may be NULL), pitch or out_pitch < W, d_disp16_right == d_out16, the int16 range rule,
 * an even win, cost = SV_COST_SGBM, min_curvature < 0, and subpixel or min_curvature > 0 with
 * SV_COST_HOG.
 *
 * sv_disparity_refined[_dev]: left match, right match (only when lr_max_diff >= 0), refine,
 * speckle.  sv_refine_plan: LDS bytes of k_refine's staged form for (num_disp, win) and whether
 * a launch with the costs takes it (*lds_form = 1) or the global-tap form (0). */
typedef struct sv_refine_params {
    int lr_max_diff;      /* < 0: no left-right check */
    int min_curvature;    /* 0: no curvature test */
    int subpixel;         /* != 0: parabolic sub-pixel step */
    int speckle_window;   /* <= 0: no speckle filter */
    int speckle_range;    /* in whole disparities */
} sv_refine_params;
int sv_refine_plan(int num_disp, int win, int* lds_bytes, int* lds_form);
int sv_disparity_right_dev(sv_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int H, int W,
                           int pitch, int min_disp, int num_disp, int win, int cost,
                           int16_t* d_disp16_right, int out_pitch, void* stream);
int sv_refine_dev(sv_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int H, int W, int pitch,
                  const int16_t* d_disp16, const int16_t* d_disp16_right, int min_disp, int num_disp,
                  int win, int cost, const sv_refine_params* params, int16_t* d_out16, int out_pitch,
                  void* stream);
int sv_disparity_refined_dev(sv_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int H, int W,
                             int pitch, int min_disp, int num_disp, int win, int cost,
                             const sv_refine_params* params, int16_t* d_out16, int out_pitch,
                             void* stream);
int sv_disparity_refined(sv_ctx* ctx, const uint8_t* left, const uint8_t* right, int H, int W,
                         int channels, int stride, int min_disp, int num_disp, int win, int cost,
                         const sv_refine_params* params, int16_t* disp16);

/* ---- census / Hamming cost ----------------------------------------------
 * Semantics: tests/sv_census_oracle.py.  Every entry point that takes a `cost` accepts
 * SV_COST_CENSUS and runs the two steps below on the context's scratch; in the refinement stage
 * census maps take the left-right check and the speckle filter only (subpixel or
 * min_curvature > 0: SV_EINVAL).
 *
 * sv_census_dev: the census code C(x, y) of rows [row0, row1) (clamped to [0, H)) of a gray
 * image, one little-endian uint64 per pixel, row pitch code_pitch in elements; other rows and
 * the pitch padding are left untouched.  The 9-wide x 7-tall neighbourhood is enumerated
 * row-major, dy = -3..3 outer, dx = -4..4 inner, skipping (0, 0): k = 0..61.  Bit k is 1 iff
 * Ip(x + dx, y + dy) < I(x, y) (strict), Ip the replicate-clamped image; bits 62 and 63 are 0.
 * Image rows [row0 - 3, row1 + 3) of [0, H) are read.
 *
 * sv_census_match_dev: winner-take-all over two code planes (the transform's, or any caller's
 * 64-bit binary descriptors): cost(x, y, d) = sum over |i|, |j| <= win / 2 of
 * popcount(CLp(x + i, y + j) xor CRp(x + i - d, y + j)), CLp / CRp the planes with
 * replicate-clamped coordinates, all 64 bits counted; d* = the first argmin over d in [min_disp,
 * min_disp + num_disp).  Every element of rows [row0, row1) of d_disp16 (width W, pitch
 * out_pitch elements) is written: d* x 16 inside the matched column band [max(min_disp +
 * num_disp, 0), W + min(min_disp, 0)), (min_disp - 1) x 16 outside it.  Code rows [row0 - win / 2,
 * row1 + win / 2) of [0, H) are read.  A cost is at most 64 * 15^2 = 14400, so no SV_ERANGE
 * case exists.  SV_EINVAL before any launch: null pointers, a pitch < W, an even win or one
 * outside [1, 15], num_disp outside [1, 512], the int16 range rule. */
int sv_census_dev(sv_ctx* ctx, const uint8_t* d_gray, int H, int W, int pitch, int row0, int row1,
                  uint64_t* d_codes, int code_pitch, void* stream);
int sv_census_match_dev(sv_ctx* ctx, const uint64_t* d_codes_left, const uint64_t* d_codes_right,
                        int H, int W, int code_pitch, int min_disp, int num_disp, int win,
                        int row0, int row1, int16_t* d_disp16, int out_pitch, void* stream);

/* ---- 3D reprojection and the ordered point cloud -----------------------
 * cv2.reprojectImageTo3D(disparity, Q, handleMissingValues, CV_32F) of a device map, and the
 * compaction of its valid pixels into a list that keeps the pixels' row-major order.
 * Semantics: tests/sv_cloud_oracle.py.  The map is int16 x16 (SV_DISP_I16X16: d = f32(m) / 16,
 * the disparity create_depth_map returns) or f32 (SV_DISP_F32), row pitch `pitch` in elements;
 * Q is any finite 4 x 4, row-major f64.
 *
 * sv_reproject_3d_dev: per pixel h = Q (x, y, d, 1) in f64, summed from 0 in that order;
 * (X, Y, Z) = f32(f64(f32(h_r)) * (1 / h_3)) into d_xyz (H x W x 3, dense).  handle_missing:
 * where |d - min(d)| <= FLT_EPSILON (the minimum ignores NaNs and the pitch padding), Z = 10000.
 *
 * sv_point_cloud_dev: the pixels, in row-major order, with d >= min_valid (a NaN fails), X, Y,
 * Z finite, z_min <= Z <= z_max, inside the region of interest and, with handle_missing, not
 * at the map's minimum.  Point k: d_xyz[3k..], d_out_bgr[3k..] = the pixel of d_bgr (H x W x 3,
 * row pitch bgr_pitch bytes), d_index[k] = y W + x.  The outputs hold `cap` points: the first
 * cap are written, nothing past them, and the count N is the whole cloud's.  n_points != NULL:
 * the call waits and returns N there; NULL: nothing waits, N is in d_count once the stream has
 * reached it.  The order is fixed by three launches (count, scan, emit), never by scheduling.
 *
 * SV_EINVAL before any launch: a null required pointer (the map, Q, d_xyz, the parameters),
 * an unknown fmt, pitch < W, bgr_pitch < 3 W, H or W < 1, H W >= 2^31, cap < 0, a region that
 * is not inside the map, a NaN in min_valid, z_min or z_max, z_min > z_max, a non-finite entry
 * of Q, d_out_bgr without d_bgr.
 *
 * sv_reproject_3d / sv_point_cloud: the same on host arrays (`stride` in elements, bgr_stride
 * in bytes); the cloud's outputs hold cap points and min(N, cap) of them are written. */
enum { SV_DISP_I16X16 = 0, SV_DISP_F32 = 1 };
typedef struct sv_cloud_params {
    float min_valid, z_min, z_max;
    int roi_x, roi_y, roi_w, roi_h;   /* roi_w or roi_h == 0: the whole map */
    int handle_missing;
} sv_cloud_params;
int sv_reproject_3d_dev(sv_ctx* ctx, const void* d_disp, int fmt, int H, int W, int pitch, const double Q[16],
                        int handle_missing, float* d_xyz, void* stream);
int sv_point_cloud_dev(sv_ctx* ctx, const void* d_disp, int fmt, int H, int W, int pitch, const double Q[16],
                       const uint8_t* d_bgr, int bgr_pitch, const sv_cloud_params* params, int64_t cap,
                       float* d_xyz, uint8_t* d_out_bgr, uint32_t* d_index, uint32_t* d_count,
                       int64_t* n_points, void* stream);
int sv_reproject_3d(sv_ctx* ctx, const void* disp, int fmt, int H, int W, int stride, const double Q[16],
                    int handle_missing, float* xyz);
int sv_point_cloud(sv_ctx* ctx, const void* disp, int fmt, int H, int W, int stride, const double Q[16],
                   const uint8_t* bgr, int bgr_stride, const sv_cloud_params* params, int64_t cap, float* xyz,
                   uint8_t* out_bgr, uint32_t* index, int64_t* n_points);

/* ---- reductions around the path ----------------------------
 * Image statistics of detect_camera_occlusion (fused_depth_map.py:131-301) for one image
 * or a pair (img1 nullable): per 48x48 block of compute_block_homogeneity
 * (bh = max(1, H/48) x bw = max(1, W/48) blocks, partial edge tiles excluded as in the
 * reference) the exact sum and sum of squares of the gray values, and the 256-bin
 * histogram of the whole image (cv2.calcHist).  channels 3 = BGR, converted with the
 * cvtColor BGR2GRAY fixed point first.  Outputs per image: block_sum/block_sq [bh*bw],
 * hist [256]; the pair's second image follows the first. */
int sv_frame_stats(sv_ctx* ctx, const uint8_t* img0, const uint8_t* img1, int H, int W, int channels,
                   int stride, uint32_t* block_sum, uint32_t* block_sq, uint32_t* hist);
/* The device version, over a batch of n_frames images or pairs in one launch (image z of the
 * batch: img0 / img1 of frame z / per at + (z / per) * frame_stride bytes, per = 2 with
 * d_img1, else 1); outputs dense per image z: block moments [n_img][bh*bw], hist [n_img][256].
 * detect_camera_occlusion runs once per checked frame (fused_depth_map.py:2515-2522); a
 * stream of queued frames is one launch plus one fold. */
int sv_frame_stats_batch_dev(sv_ctx* ctx, const uint8_t* d_img0, const uint8_t* d_img1, int n_frames,
                             int64_t frame_stride, int H, int W, int channels, int pitch,
                             uint32_t* d_block_sum, uint32_t* d_block_sq, uint32_t* d_hist,
                             void* stream);

/* Order statistics of a float32 device array for np.percentile (calibrate_midas_to_stereo
 * fused_depth_map.py:1169-1257, normalize_to_stereo_range :1503-1554) with the reference's
 * masks as predicates: mask_mode 0 = all elements, 1 = elements > 0 (stereo_disparity > 0),
 * 2 = elements whose d_mask value > thr (stereo_confidence > 0.7).  sv_select_count_batch gives
 * the number of selected elements and of NaNs among them (np.percentile returns nan if
 * any); sv_select_ranks_batch gives the values of the given 0-based ranks of the ascending
 * sorted selection (nranks <= 4; radix select in three passes of 11/11/10 bits).  Both
 * block until the result is on the host and take a batch of n_arrays <= 16 arrays of n
 * elements (array y at d_x + y * x_stride elements, its mask at d_mask + y * mask_stride; one
 * array: n_arrays = 1): one launch + one fold per radix pass for the whole batch (e.g. the
 * disparity maps of queued frames).  selected / nans: [n_arrays]; ranks / values:
 * [n_arrays][nranks]. */
int sv_select_count_batch(sv_ctx* ctx, const float* d_x, int64_t n, int64_t x_stride, int n_arrays,
                          int mask_mode, const float* d_mask, int64_t mask_stride, float thr,
                          int64_t* selected, int64_t* nans);
int sv_select_ranks_batch(sv_ctx* ctx, const float* d_x, int64_t n, int64_t x_stride, int n_arrays,
                          int mask_mode, const float* d_mask, int64_t mask_stride, float thr,
                          const int64_t* ranks, int nranks, float* values);
/* Elementwise epilogues: mode 0: out = fc + ((x - fa) / fb) * fd in float32, op by op;
 * mode 1: out = float32(float64(x) * ds + doff); mode 2: out = fc.  The frame loop's
 * normalisations (fused_depth_map.py:2749-2759, :2793-2811), float32 op by op, np.clip keeping a
 * NaN: mode 3: out = 255 - (mode 0); mode 4: out = 255 - clip(x * 255, 0, 255); mode 5: out =
 * clip(((x - fa) / fb) * 255, 0, 255). */
int sv_affine_f32_dev(sv_ctx* ctx, const float* d_x, int64_t n, int mode, float fa, float fb,
                      float fc, float fd, double ds, double doff, float* d_out, void* stream);

/* ---- fuse_depth_maps (fused_depth_map.py:1560-1718) and its two float32 filters ----------
 * Maps are float32 HxW, dense, finite; borders BORDER_REFLECT_101.  Every exp of the filters is
 * evaluated by the caller in float64 and passed as float32 tables (fusion.py: gaussian_kernel,
 * bilateral_tables), so the kernels' results are bit-identical to a NumPy restatement of the
 * same arithmetic (parity with a particular OpenCV build is unpinned).  All three
 * return SV_EINVAL before anything is enqueued for a null pointer, an unsupported ksize or
 * radius, or H or W <= the filter radius. */

/* cv2.GaussianBlur(x, (ksize, ksize), 0) (:1638): ksize odd in [3, 31], coef = the ksize
 * normalised coefficients (host), rows first with a float32 intermediate, each pass
 * s = c0 x0; s = s + c_i (x_-i + x_+i), i = 1..ksize/2.  d_dst != d_src. */
int sv_gauss_blur_f32_dev(sv_ctx* ctx, const float* d_src, int H, int W, const float* coef, int ksize,
                          float* d_dst, void* stream);

/* cv2.bilateralFilter(x, d, sigma_color, sigma_space) on one float32 channel (:1688, :2769,
 * :1403-1411) with the tables built by the caller: radius in [1, 7]; space_w (host) = one weight
 * per tap of the radius-r disc without its centre, dy outer and dx inner; lut (host) = the 4098
 * entries of the colour table over 4096 bins; scale = bins per unit of |difference|.  radius 0:
 * no filter (the copy path of a constant map, or the max <= 10 branch of :1687), the outputs
 * are formed from d_src elementwise.  Outputs, each optional: d_dst_f32 = the filter's output;
 * d_dst_u8 = np.clip(out, 0, 255).astype(uint8) (:1696-1697); d_dst_bgr = cmap_bgr[d_dst_u8]
 * (HxWx3; cmap_bgr: host, 256 x 3 BGR bytes; :1700); minmax_out (host) = min and max of the
 * clipped map (:1708) — the call then waits for the result.  With radius > 0 the call waits
 * once for the upload of the colour table (the caller's tables may go when it returns); the
 * filter itself is only enqueued. */
int sv_bilateral_f32_dev(sv_ctx* ctx, const float* d_src, int H, int W, int radius, const float* space_w,
                         const float* lut, float scale, float* d_dst_f32, uint8_t* d_dst_u8,
                         uint8_t* d_dst_bgr, const uint8_t* cmap_bgr, float* minmax_out, void* stream);

/* The blend of fuse_depth_maps (:1603-1684) in one launch.  base 0: stereo * stereo_weight
 * with conf (NULL: ones), 1: midas, 2: flow.  midas_fill (base 0): fw = clip(GaussianBlur((1 -
 * conf) * midas_fill_weight, ksize), 0, 1); where conf < conf_threshold and fw > 0.1:
 * fused = fused * (1 - fw) + midas * fw.  flow_fill (base 0 or 1): where fused <
 * hole_threshold or fused == 0: fused = fused * flow_k1 + flow * flow_k2 (k1 = float32(1 -
 * weight), k2 = float32(weight)).  coef / ksize as for sv_gauss_blur_f32_dev (midas_fill). */
typedef struct sv_fuse_args {
    const float* d_stereo;
    const float* d_conf;
    const float* d_midas;
    const float* d_flow;
    int H, W;
    int base;
    int midas_fill, flow_fill;
    float stereo_weight, midas_fill_weight, conf_threshold, hole_threshold, flow_k1, flow_k2;
    const float* coef;   /* host */
    int ksize;
} sv_fuse_args;
/* range of the blended map and the pixels each fill changed (the np.any guards of :1645, :1656) */
typedef struct sv_fuse_stats {
    float min, max;
    int64_t n_midas, n_hole;
} sv_fuse_stats;
/* stats (host, nullable): the call then waits for the result. */
int sv_fuse_blend_dev(sv_ctx* ctx, const sv_fuse_args* args, float* d_fused, sv_fuse_stats* stats,
                      void* stream);

/* ---- Farneback optical flow and the flow depth estimator (fused_depth_map.py:1263-1501) ----
 * cv2.calcOpticalFlowFarneback with flags = 0 and no initial flow, restated (DESIGN.md §9,
 * "Optical flow"): bit-identical to the NumPy restatement of the tests; parity with a particular
 * OpenCV build is unpinned.  Every exp and the inverse of the moment matrix are evaluated by the
 * caller (flow.py: farneback_levels, gaussian_coef, polyexp_tables) and passed as host tables.
 * Polynomial coefficients (R), the matrices (M) and a level's flow are dense float32 planes, H * W
 * elements apart: R = (y, x, y^2, x^2, xy), M = (G11, G12, G22, h1, h2), flow = (dx, dy).
 * All return SV_EINVAL before anything is enqueued for a null pointer or an argument outside the
 * stated limits. */
#define SV_FB_MAX_SCALES 16
typedef struct sv_farneback_params {
    int n_scales;              /* pyramid scales, 1..SV_FB_MAX_SCALES, finest first */
    const int* scale_h;        /* host, n_scales entries each: the size of every scale (scale 0 = */
    const int* scale_w;        /* H x W, no scale larger than the one before) and the ksize of its */
    const int* scale_ksize;    /* Gaussian blur, odd in [3, 31] */
    const float* scale_coef;   /* host, 32 floats per scale: the first ksize are the coefficients */
    float flow_scale;          /* float32(1 / pyr_scale): factor on the upsampled flow */
    int winsize;               /* odd in [3, 31] */
    int iterations;            /* >= 1 */
    int poly_n;                /* 5 or 7: 2 poly_n + 1 taps per axis */
    const float* poly_g;       /* host, poly_n + 1 entries each: g[x], x g[x], x^2 g[x], x = 0.. */
    const float* poly_xg;
    const float* poly_xxg;
    double ig[4];              /* ig11, ig03, ig33, ig55 of the inverse moment matrix */
} sv_farneback_params;
/* d_prev, d_next: gray uint8 H x W (H, W >= 16), rows `pitch` bytes apart; d_flow: float32
 * H x W x 2.  Scratch comes from the context; nothing waits for the device. */
int sv_farneback_flow_dev(sv_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_next, int H, int W,
                          int pitch, const sv_farneback_params* params, float* d_flow, void* stream);
/* The stages alone.  polyexp: d_img float32 H x W -> d_R (5 planes).  update_matrices: d_flow
 * = 2 planes -> d_M (5 planes).  blur_solve: d_M -> d_flow, 2 planes or (interleaved != 0)
 * H x W x 2. */
int sv_fb_polyexp_dev(sv_ctx* ctx, const float* d_img, int H, int W, int poly_n, const float* g,
                      const float* xg, const float* xxg, const double ig[4], float* d_R, void* stream);
int sv_fb_update_matrices_dev(sv_ctx* ctx, const float* d_R0, const float* d_R1, const float* d_flow,
                              int H, int W, float* d_M, void* stream);
int sv_fb_blur_solve_dev(sv_ctx* ctx, const float* d_M, int H, int W, int winsize, float* d_flow,
                         int interleaved, void* stream);
/* d_flow: H x W x 2.  e = perspectiveTransform((x, y), Hm) - (x, y) on float32 points (float64
 * inside, w = 0 where |w| <= DBL_EPSILON); r = flow - e; m = float32(sqrt(rx^2 + ry^2)) with the
 * squares and the root in float64; d_depth = 1 / (m + 0.5).  d_stable (nullable): stable = alpha
 * * stable + one_minus_alpha * depth in float32.  minmax_out (host, nullable): min and max of
 * d_depth; the call then waits for the result. */
int sv_flow_depth_dev(sv_ctx* ctx, const float* d_flow, int H, int W, const double Hm[9], float* d_depth,
                      float* d_stable, float alpha, float one_minus_alpha, float* minmax_out, void* stream);
/* The flow at the grid of _estimate_ego_motion (fused_depth_map.py:1447-1455): d_out[j * nx + i]
 * = d_flow[step / 2 + j * step][step / 2 + i * step] (both components), ny = the number of grid
 * rows below H, nx of grid columns below W; d_out holds ny * nx * 2 floats.  Both pointers
 * 8-byte aligned.  A host then downloads the grid instead of the H x W x 2 flow. */
int sv_flow_grid_dev(sv_ctx* ctx, const float* d_flow, int H, int W, int step, float* d_out, void* stream);

/* cv2.resize(x, (dW, dH), INTER_LINEAR) of a float32 HxW map (calibrate_midas_to_stereo,
 * fused_depth_map.py:1216-1217): OpenCV's float path, S0*b0 + S1*b1 without contraction.
 * Pitches in bytes. */
int sv_resize_linear_f32_dev(sv_ctx* ctx, const float* d_src, int sH, int sW, int src_pitch,
                             float* d_dst, int dH, int dW, int dst_pitch, void* stream);

/* ---- device memory helpers ----------------------------------------------------------
 * sv_copy_to_device / sv_copy_to_host: stream NULL = synchronous on the context stream (the
 * download first waits for the context's enqueued work); a stream = enqueued on it and
 * returned at once (the host buffer must stay valid until the stream reaches the copy, and be
 * page-locked — sv_host_register — for the copy to overlap device work). */
int sv_dev_alloc(sv_ctx* ctx, uint64_t bytes, void** out);
int sv_dev_free(sv_ctx* ctx, void* p);
int sv_copy_to_device(sv_ctx* ctx, void* dst, const void* src, uint64_t bytes, void* stream);
int sv_copy_to_host(sv_ctx* ctx, void* dst, const void* src, uint64_t bytes, void* stream);
/* Host <-> device traffic of this context since its creation (or the last reset): out[0], out[1]
 * = bytes and calls of the host-to-device copies, out[2], out[3] = of the device-to-host copies.
 * Every copy the library issues for the context counts, the scalar read-backs inside the `_dev`
 * entry points (blend statistics, min/max, select counts) included.  reset != 0: zero them after
 * reading.  Plain host counters: no device work. */
int sv_copy_counters(sv_ctx* ctx, uint64_t out[4], int reset);

/* Page-lock a host range and make it device-visible (hipHostRegister, portable).  Output
 * arrays of the host-buffer entry points (sv_depth_map, sv_depth_map_color,
 * sv_stereo_scaled, sv_stereo_scaled_color) that lie inside registered ranges are filled by
 * DMA from the device epilogue instead of by the host expansion of the int16 medians; the
 * results are identical.  A range stays registered until sv_host_unregister(ptr), which
 * takes the same start pointer.  No reference counterpart: an engine-side optimisation of
 * the numpy outputs depth_map.py:937-939 returns. */
int sv_host_register(void* ptr, uint64_t bytes);
int sv_host_unregister(void* ptr);

/* Host-side stage timings of the host-buffer entry points (process-wide, off by default):
 * ms6 = accumulated {prepare, stage + issue (the pageable uploads are synchronous), wait for
 * the first output piece, host expansion, wait for the rest, total} milliseconds over `calls`
 * calls since the last reset.  The device side of the same calls is the context's event
 * profile (sv_profile_enable): SV_K_H2D (one event pair per image upload), SV_K_GRAY,
 * SV_K_MATCH, SV_K_MEDIAN and SV_K_D2H. */
int sv_host_profile_enable(int enable);
int sv_host_profile_read(double* ms6, long long* calls, int reset);

/* ---- profiling: HIP events around every kernel this context launches -------------- */
int sv_profile_enable(sv_ctx* ctx, int on);
/* Waits for the recorded events and returns the accumulated device time and launch count
 * of kernel `kernel` (sv_kernel) since the last reset. */
int sv_profile_read(sv_ctx* ctx, int kernel, double* total_ms, long long* count);
int sv_profile_reset(sv_ctx* ctx);
/* Device time between two points of a stream (HIP events): sv_timer_begin records the
 * first, sv_timer_end the second, waits for it and returns the elapsed milliseconds.  For
 * timing a run of back-to-back launches (one event pair, so small kernels are not
 * dominated by per-launch event overhead). */
int sv_timer_begin(sv_ctx* ctx, void* stream);
int sv_timer_end(sv_ctx* ctx, void* stream, double* ms);
/* Caller-delimited profiling region on `stream` (NULL = the context's stream), counted under
 * `kernel` like a launch when profiling is enabled (a no-op otherwise): e.g. the RCCL gather a
 * process enqueues itself through sv_comm_gatherv (SV_K_GATHER).  Regions do not nest. */
int sv_profile_region_begin(sv_ctx* ctx, int kernel, void* stream);
int sv_profile_region_end(sv_ctx* ctx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STEREOVISION_AMD_H */
