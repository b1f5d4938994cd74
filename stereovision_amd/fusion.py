"""Reductions on either side of the disparity path, on the GPU.

Drop-ins for fused_depth_map.py's
  detect_camera_occlusion(left, right, occlusion_threshold=0.45)          :131-301
  calibrate_midas_to_stereo(midas_depth, stereo_disparity, stereo_conf)   :1169-1257
  normalize_to_stereo_range(depth_map, stereo_disparity)                  :1503-1554
with the reference's arguments, return values and decisions, and the numeric body of
  fuse_depth_maps(stereo, conf, midas, midas_conf, flow, camera_moving, ...)   :1560-1718
(``fuse_maps`` / ``fuse_maps_dev``; the drop-in itself is fused_depth_map.fuse_depth_maps)
with the two filters it is built on, ``gaussian_blur`` and ``bilateral_filter``.

* The occlusion statistics come from one ``k_frame_stats`` launch per pair: exact integer
  moments of every 48x48 block and the 256-bin histogram of each image.  np.mean and the
  entropy are then exact (the histogram is what cv2.calcHist returns and the entropy is
  the reference's NumPy expression over it); np.std is evaluated from the exact moments
  (sqrt((n*Q - S^2) / n^2)), i.e. the correctly rounded value, where NumPy's two-pass sum
  may differ in the last bits (tests: rtol 1e-12); the "std < 12" block test is done
  exactly on the integers.
* np.percentile is split the way NumPy computes it: the GPU finds the order statistics
  (``k_select_hist``, radix select with the reference's masks as predicates — the masked
  array is never built), and the interpolation runs here with NumPy's own dtype rules for
  the 'linear' method (scalar q on float32 -> float32 arithmetic, a list of q -> float64),
  so results are bit-identical to np.percentile.
* The elementwise epilogues run in ``k_affine_f32`` with the reference's precision.
* fuse_depth_maps runs in two launches (``k_fuse_blend``, ``k_bilateral_f32``) around one host
  step: the blended map's range comes back, ``bilateral_tables`` builds the colour table with
  NumPy in float64 and uploads it.  The kernels call no exp of their own, which is what makes
  the maps bit-identical to a NumPy restatement (OpenCV parity is unpinned).

Inputs are host NumPy arrays (as in the reference); ``*_dev`` variants take device
pointers for pipelines that keep the maps in HBM.
"""
from __future__ import annotations

import math

import numpy as np

from .engine import get_engine

SEL_ALL, SEL_POSITIVE, SEL_MASK_GT = 0, 1, 2
AFF_F32, AFF_F64, AFF_FILL = 0, 1, 2
# the frame loop's normalisations (fused_depth_map.py:2749-2759, :2793-2811)
AFF_F32_INV, AFF_CLIP255_INV, AFF_NORM_CLIP255 = 3, 4, 5


# ----------------------------------------------------------------------------------------
# np.percentile from GPU order statistics
# ----------------------------------------------------------------------------------------
def _quantile_ranks(cnt: int, q, dtype):
    """numpy/lib/_function_base_impl.py: percentile -> _quantile (method 'linear') up to the
    indices: (virtual index, previous, next, previous rank, next rank)."""
    qa = np.asanyarray(np.true_divide(q, dtype(100)))
    if np.any(qa < 0) or np.any(qa > 1):
        raise ValueError("Percentiles must be in the range [0, 100]")
    vi = np.asanyarray((cnt - 1) * qa)
    prev = np.asanyarray(np.floor(vi))
    nxt = np.asanyarray(prev + 1)
    above = vi >= cnt - 1
    if above.any():
        prev[above] = -1
        nxt[above] = -1
    below = vi < 0
    if below.any():
        prev[below] = 0
        nxt[below] = 0
    prev = prev.astype(np.intp)
    nxt = nxt.astype(np.intp)
    pr = np.where(prev < 0, cnt - 1, prev).ravel()
    nr = np.where(nxt < 0, cnt - 1, nxt).ravel()
    return vi, prev, nxt, pr, nr


def percentiles_dev(eng, d_x: int, n: int, qs, mask_mode: int = SEL_ALL, d_mask: int = 0,
                    thr: float = 0.0, dtype=np.float32) -> list:
    """[np.percentile(x[mask], q) for q in qs] (method 'linear') of a float32 device array: one
    count and the order statistics of every q fetched together (four ranks per select), each q
    then interpolated on its own with NumPy's dtype rules for that q."""
    sel, nans = eng.select_count(d_x, n, mask_mode, d_mask, thr)
    if sel + nans == 0:
        raise IndexError("index -1 is out of bounds for axis 0 with size 0")   # NumPy's error
    cnt = sel + nans
    plans = [_quantile_ranks(cnt, q, dtype) for q in qs]
    if nans:
        outs = [np.full(vi.shape, np.nan, dtype) for vi, *_ in plans]
        return [o[()] if o.ndim == 0 else o for o in outs]
    ranks = np.unique(np.concatenate([np.concatenate([pr, nr]) for *_, pr, nr in plans]))
    vals = {}
    for i in range(0, ranks.size, 4):
        chunk = ranks[i:i + 4]
        for r, v in zip(chunk, eng.select_ranks(d_x, n, chunk, mask_mode, d_mask, thr)):
            vals[int(r)] = v
    out = []
    for vi, prev, nxt, pr, nr in plans:
        previous = np.array([vals[int(r)] for r in pr], dtype).reshape(vi.shape)
        nextv = np.array([vals[int(r)] for r in nr], dtype).reshape(vi.shape)
        gamma = np.asanyarray(vi - prev)
        gamma = np.asanyarray(gamma, dtype=vi.dtype)
        # _lerp
        diff_b_a = np.subtract(nextv, previous)
        res = np.asanyarray(np.add(previous, diff_b_a * gamma))
        np.subtract(nextv, diff_b_a * (1 - gamma), out=res, where=gamma >= 0.5, casting="unsafe",
                    dtype=type(res.dtype))
        if res.ndim == 0:
            res = res[()]
        out.append(res)
    return out


def percentile_dev(eng, d_x: int, n: int, q, mask_mode: int = SEL_ALL, d_mask: int = 0,
                   thr: float = 0.0, dtype=np.float32):
    """np.percentile(x[mask], q) (method 'linear') of a float32 device array."""
    return percentiles_dev(eng, d_x, n, [q], mask_mode, d_mask, thr, dtype)[0]


def percentile(x: np.ndarray, q, positive: bool = False):
    """np.percentile(x[x > 0] if positive else x, q) of a float32 host array, on the GPU."""
    x = np.ascontiguousarray(x)
    if x.dtype != np.float32:
        raise TypeError(f"percentile: float32 maps only, got {x.dtype}")
    eng = get_engine()
    d_x = eng.upload("pct_x", x)
    return percentile_dev(eng, d_x, x.size, q, SEL_POSITIVE if positive else SEL_ALL)


# ----------------------------------------------------------------------------------------
# detect_camera_occlusion   fused_depth_map.py:131-301
# ----------------------------------------------------------------------------------------
def _std_from_moments(n: int, s: int, q: int) -> float:
    return math.sqrt((n * q - s * s) / (n * n))


def occlusion_metrics(block_sum, block_sq, hist, H: int, W: int) -> dict:
    """The five per-camera metrics of detect_camera_occlusion from exact moments."""
    bh, bw = block_sum.shape
    bsize = 48
    hs = [min((i + 1) * bsize, H) - i * bsize for i in range(bh)]
    ws = [min((j + 1) * bsize, W) - j * bsize for j in range(bw)]
    stds, low = [], 0
    for i in range(bh):
        for j in range(bw):
            n = hs[i] * ws[j]
            s, q = int(block_sum[i, j]), int(block_sq[i, j])
            stds.append(_std_from_moments(n, s, q))
            low += (n * q - s * s) < 144 * n * n          # np.std(block) < 12, exactly
    avg_std = np.mean(stds) if stds else 0
    low_var_ratio = low / max(len(stds), 1)
    h = hist.astype(np.int64)
    N = int(h.sum())
    levels = np.arange(256, dtype=np.int64)
    S = int((h * levels).sum())
    Q = int((h * levels * levels).sum())
    contrast = np.float64(_std_from_moments(N, S, Q))
    # compute_entropy (fused_depth_map.py:230-241) on cv2.calcHist's float32 counts
    hf = hist.astype(np.float32).flatten() + 1e-10
    hf = hf / hf.sum()
    entropy = -np.sum(hf * np.log2(hf + 1e-10))
    brightness = np.float64(S) / N                        # np.mean(gray): exact integer sum
    return {"std": avg_std, "low_var": low_var_ratio, "contrast": contrast, "entropy": entropy,
            "brightness": brightness}


def occlusion_decision(L: dict, R: dict, occlusion_threshold: float = 0.45):
    """The scoring and decision block of fused_depth_map.py:243-301, verbatim."""
    STD_THRESHOLD = 28.0
    LOW_VAR_THRESHOLD = 0.55
    CONTRAST_RATIO = 2.2
    ENTROPY_RATIO = 1.6
    BRIGHTNESS_DIFF = 45.0
    ls = rs = 0.0
    if L["std"] < STD_THRESHOLD * 0.8:
        ls += 0.35
    if L["low_var"] > LOW_VAR_THRESHOLD:
        ls += 0.35
    if L["contrast"] < R["contrast"] / CONTRAST_RATIO and R["contrast"] > 15:
        ls += 0.25
    if L["entropy"] < R["entropy"] / ENTROPY_RATIO and R["entropy"] > 5.0:
        ls += 0.25
    if abs(L["brightness"] - R["brightness"]) > BRIGHTNESS_DIFF and L["brightness"] < 80:
        ls += 0.2
    if R["std"] < STD_THRESHOLD * 0.8:
        rs += 0.35
    if R["low_var"] > LOW_VAR_THRESHOLD:
        rs += 0.35
    if R["contrast"] < L["contrast"] / CONTRAST_RATIO and L["contrast"] > 15:
        rs += 0.25
    if R["entropy"] < L["entropy"] / ENTROPY_RATIO and L["entropy"] > 5.0:
        rs += 0.25
    if abs(R["brightness"] - L["brightness"]) > BRIGHTNESS_DIFF and R["brightness"] < 80:
        rs += 0.2
    if ls > occlusion_threshold and rs < occlusion_threshold * 0.6:
        result = "left"
    elif rs > occlusion_threshold and ls < occlusion_threshold * 0.6:
        result = "right"
    elif ls > occlusion_threshold and rs > occlusion_threshold:
        result = "both"
    else:
        result = "none"
    return result, ls, rs


def detect_camera_occlusion(left_img, right_img, occlusion_threshold=0.45):
    """fused_depth_map.py:131-301 -> (result, left_score, right_score)."""
    left_img = np.asarray(left_img)
    right_img = np.asarray(right_img)
    if left_img.dtype != np.uint8 or right_img.dtype != np.uint8:
        raise TypeError("detect_camera_occlusion: uint8 frames only")
    eng = get_engine()
    if left_img.shape == right_img.shape:
        bs, bq, hist = eng.frame_stats(left_img, right_img)
    else:
        a = eng.frame_stats(left_img)
        b = eng.frame_stats(right_img)
        bs, bq, hist = [a[0][0], b[0][0]], [a[1][0], b[1][0]], [a[2][0], b[2][0]]
    mets = [occlusion_metrics(bs[k], bq[k], hist[k], *(im.shape[:2]))
            for k, im in enumerate((left_img, right_img))]
    return occlusion_decision(mets[0], mets[1], occlusion_threshold)


# ----------------------------------------------------------------------------------------
# calibrate_midas_to_stereo / normalize_to_stereo_range   :1169-1257, :1503-1554
# ----------------------------------------------------------------------------------------
def _f32_map(a, name):
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        raise TypeError(f"{name}: float32 maps only, got {a.dtype}")
    return a


def _affine(eng, d_x: int, shape, mode: int, **kw) -> np.ndarray:
    n = int(np.prod(shape))
    d_out = eng.scratch("aff_out", 4 * n)
    eng.affine_f32_dev(d_x, n, mode, d_out, **kw)
    return eng.to_host(d_out, shape, np.float32)


def _calibrate_plan(eng, d_md: int, d_sd: int, d_cf: int, n: int):
    """The scalars of calibrate_midas_to_stereo (:1222-1254) from the device maps: (affine mode,
    its parameters)."""
    sel, nans = eng.select_count(d_sd, n, SEL_MASK_GT, d_cf, 0.7)
    if sel + nans < 100:                       # np.sum(reliable_mask) < 100
        midas_min, midas_max = percentiles_dev(eng, d_md, n, [5, 95])
        stereo_min, stereo_max = percentiles_dev(eng, d_sd, n, [5, 95])
        if (midas_max - midas_min) < 1e-6:
            c = np.full((1,), (stereo_min + stereo_max) / 2.0, np.float32)[0]
            return AFF_FILL, dict(fc=c)
        den = midas_max - midas_min + 1e-8
        rng = stereo_max - stereo_min
        return AFF_F32, dict(fa=midas_min, fb=den, fc=stereo_min, fd=rng)
    stereo_min, stereo_max = percentile_dev(eng, d_sd, n, [10, 90], SEL_MASK_GT, d_cf, 0.7)
    midas_min, midas_max = percentile_dev(eng, d_md, n, [10, 90], SEL_MASK_GT, d_cf, 0.7)
    if (midas_max - midas_min) < 1e-6:
        scale = 1.0
    else:
        scale = (stereo_max - stereo_min) / (midas_max - midas_min + 1e-8)
    offset = stereo_min - midas_min * scale
    return AFF_F64, dict(ds=float(scale), doff=float(offset))


def calibrate_midas_to_stereo_dev(eng, d_midas: int, mH: int, mW: int, d_stereo: int, d_conf: int, H: int,
                                  W: int, d_out: int, d_resized: int = 0) -> None:
    """calibrate_midas_to_stereo on device maps: d_midas (mH x mW) is resized into d_resized
    (H x W floats) when its size differs (:1215-1217); the calibrated map goes to d_out (which
    may be d_resized).  The percentiles' order statistics come back to the host, no map does."""
    if (mH, mW) != (H, W):
        if not d_resized:
            raise ValueError("calibrate_midas_to_stereo_dev: a buffer for the resized map is needed")
        eng.resize_f32_dev(d_midas, mH, mW, d_resized, H, W)
        d_midas = d_resized
    mode, kw = _calibrate_plan(eng, d_midas, d_stereo, d_conf, H * W)
    eng.affine_f32_dev(d_midas, H * W, mode, d_out, **kw)


def calibrate_midas_to_stereo(midas_depth, stereo_disparity, stereo_confidence):
    """fused_depth_map.py:1169-1257 (percentile calibration of a relative depth map to the
    stereo disparity range) with the reductions and the epilogue on the GPU."""
    if midas_depth is None or stereo_disparity is None:
        return None
    eng = get_engine()
    sd = _f32_map(stereo_disparity, "stereo_disparity")
    md = _f32_map(midas_depth, "midas_depth")
    H, W = sd.shape[:2]
    d_md = eng.upload("cal_midas", md)
    if md.shape != sd.shape:   # cv2.resize(..., INTER_LINEAR) (:1215-1217)
        d_rs = eng.scratch("cal_midas_rs", 4 * H * W)
        eng.resize_f32_dev(d_md, md.shape[0], md.shape[1], d_rs, H, W)
        d_md = d_rs
    n = H * W
    d_sd = eng.upload("cal_disp", sd)
    d_cf = eng.upload("cal_conf", _f32_map(stereo_confidence, "stereo_confidence"))
    mode, kw = _calibrate_plan(eng, d_md, d_sd, d_cf, n)
    return _affine(eng, d_md, (H, W), mode, **kw)


def minmax_normalize_dev(eng, d_x: int, n: int, d_out: int):
    """The MiDaS normalisation without stereo (fused_depth_map.py:2749-2759) of a float32 device
    map: clip(((x - min) / (max - min + 1e-8)) * 255.0, 0, 255), zeros when max <= min + 1e-6,
    float32 throughout.  min and max are order statistics 0 and n - 1 of the radix select (a
    NaN in the map makes both NaN, as np.min / np.max do).  Returns (min, max)."""
    sel, nans = eng.select_count(d_x, n)
    if sel + nans == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    if nans:
        min_val = max_val = np.float32(np.nan)
    else:
        min_val, max_val = (np.float32(v) for v in eng.select_ranks(d_x, n, [0, n - 1]))
    if max_val > min_val + 1e-6:
        eng.affine_f32_dev(d_x, n, AFF_NORM_CLIP255, d_out, fa=min_val, fb=max_val - min_val + 1e-8)
    else:
        eng.affine_f32_dev(d_x, n, AFF_FILL, d_out, fc=0.0)
    return min_val, max_val


# ----------------------------------------------------------------------------------------
# fuse_depth_maps and its filters   :1560-1718
# ----------------------------------------------------------------------------------------
BILATERAL_BINS = 4096          # colour-table bins; the table holds BILATERAL_BINS + 2 entries
BILATERAL_MAX_RADIUS = 7
FLT_EPSILON = float(np.finfo(np.float32).eps)
BASE_STEREO, BASE_MIDAS, BASE_FLOW = 0, 1, 2


def gaussian_kernel(ksize: int) -> np.ndarray:
    """The ksize float32 coefficients of cv2.GaussianBlur(x, (ksize, ksize), 0): sigma =
    0.3 ((ksize - 1) / 2 - 1) + 0.8, exp in float64, normalised by the float64 sum of the
    float32 values."""
    ksize = int(ksize)
    if ksize < 3 or ksize > 31 or ksize % 2 == 0:
        raise ValueError(f"gaussian_kernel: ksize must be odd in [3, 31], got {ksize}")
    sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    scale2x = -0.5 / (sigma * sigma)
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    g = np.exp(scale2x * (x * x)).astype(np.float32)
    total = 0.0
    for v in g:                       # in index order: the sum is part of the definition
        total += float(v)
    return (g.astype(np.float64) * (1.0 / total)).astype(np.float32)


def bilateral_radius(d: int, sigma_space: float) -> int:
    if sigma_space <= 0:
        sigma_space = 1
    r = int(d) // 2 if d > 0 else int(round(1.5 * sigma_space))
    return max(r, 1)


def bilateral_tables(mn, mx, d: int, sigma_color: float, sigma_space: float):
    """Host tables of cv2.bilateralFilter on a float32 map whose values span [mn, mx]:
    (radius, space weights float32 [taps], colour table float32 [4098], scale float32).
    Taps: dy outer, dx inner over [-r, r], without the centre and the corners outside the
    disc.  Table entry i = exp((i / scale)^2 * (-0.5 / sigma_color^2)) until the first entry
    that rounds to zero, zeros after it."""
    if sigma_color <= 0:
        sigma_color = 1
    if sigma_space <= 0:
        sigma_space = 1
    r = bilateral_radius(d, sigma_space)
    if r > BILATERAL_MAX_RADIUS:
        raise ValueError(f"bilateral_tables: radius {r} > {BILATERAL_MAX_RADIUS} is not supported")
    gs = -0.5 / (float(sigma_space) * float(sigma_space))
    gc = -0.5 / (float(sigma_color) * float(sigma_color))
    r2 = np.array([dy * dy + dx * dx for dy in range(-r, r + 1) for dx in range(-r, r + 1)
                   if (dy or dx) and math.sqrt(dy * dy + dx * dx) <= r], np.float64)
    sw = np.exp(r2 * gs).astype(np.float32)
    length = np.float32(float(mx) - float(mn))
    scale = np.float32(BILATERAL_BINS) / length
    v = np.arange(BILATERAL_BINS + 2, dtype=np.float64) / float(scale)
    lut = np.exp(v * v * gc).astype(np.float32)
    zero = np.flatnonzero(lut == 0)
    if zero.size:                     # (monotone, so already so: stated for the contract)
        lut[zero[0]:] = 0
    return r, sw, lut, scale


def _check_maps(name, maps):
    """float32 (TypeError) maps of one 2-D shape (ValueError); None entries are skipped."""
    out, shape = [], None
    for label, m in maps:
        if m is None:
            out.append(None)
            continue
        m = _f32_map(m, f"{name}: {label}")
        if m.ndim != 2:
            raise ValueError(f"{name}: {label} must be HxW, got shape {m.shape}")
        if shape is None:
            shape = m.shape
        elif m.shape != shape:
            raise ValueError(f"{name}: {label} has shape {m.shape}, expected {shape}")
        out.append(m)
    return out, shape


def gaussian_blur(src, ksize: int, engine=None) -> np.ndarray:
    """cv2.GaussianBlur(src, (ksize, ksize), 0) of a float32 HxW host map, on the GPU."""
    (src,), (H, W) = _check_maps("gaussian_blur", [("src", src)])
    coef = gaussian_kernel(ksize)
    if H <= ksize // 2 or W <= ksize // 2:
        raise ValueError(f"gaussian_blur: map {H}x{W} not larger than the radius {ksize // 2}")
    eng = engine or get_engine()
    d_src = eng.upload("gb_src", src)
    d_dst = eng.scratch("gb_dst", src.nbytes)
    eng.gauss_blur_f32_dev(d_src, H, W, coef, d_dst)
    return eng.to_host(d_dst, (H, W), np.float32)


def bilateral_filter_dev(eng, d_src: int, H: int, W: int, mn, mx, d: int, sigma_color: float,
                         sigma_space: float, d_dst: int, stream: int = 0) -> None:
    """cv2.bilateralFilter of a float32 device map whose minimum and maximum are mn, mx
    (they size the colour table), into d_dst (!= d_src)."""
    if abs(float(mx) - float(mn)) < FLT_EPSILON:          # a constant map: a copy
        eng.bilateral_f32_dev(d_src, H, W, 0, None, None, 0.0, d_dst_f32=d_dst, stream=stream)
        return
    r, sw, lut, scale = bilateral_tables(mn, mx, d, sigma_color, sigma_space)
    if H <= r or W <= r:
        raise ValueError(f"bilateral_filter: map {H}x{W} not larger than the radius {r}")
    eng.bilateral_f32_dev(d_src, H, W, r, sw, lut, scale, d_dst_f32=d_dst, stream=stream)


def bilateral_filter(src, d: int, sigma_color: float, sigma_space: float, engine=None) -> np.ndarray:
    """cv2.bilateralFilter(src, d, sigma_color, sigma_space) of a float32 HxW host map, on the
    GPU (the range of src, an exact reduction, is taken here)."""
    (src,), (H, W) = _check_maps("bilateral_filter", [("src", src)])
    eng = engine or get_engine()
    d_src = eng.upload("bf_src", src)
    d_dst = eng.scratch("bf_dst", src.nbytes)
    bilateral_filter_dev(eng, d_src, H, W, src.min(), src.max(), d, sigma_color, sigma_space, d_dst)
    return eng.to_host(d_dst, (H, W), np.float32)


FUSE_DEFAULTS = dict(stereo_weight=0.8, midas_fill_weight=0.9, flow_fill_weight=0.5,
                     stereo_conf_threshold=0.5, flow_hole_threshold=15, use_midas_fill=True,
                     use_flow_fill=True, midas_blend_radius=15, bilateral_d=9, bilateral_sigma=75)


def fuse_maps_dev(eng, H: int, W: int, d_stereo: int, d_conf: int, d_midas: int, d_flow: int,
                  d_fused: int, d_u8: int, d_bgr: int = 0, cmap=None, stream: int = 0, **params) -> dict:
    """The numeric body of fuse_depth_maps (:1603-1700) on float32 device maps (0 = the map is
    absent or not valid): blend -> d_fused (float32 scratch), then the bilateral filter when
    max(fused) > 10, clip, uint8 -> d_u8 and the colormap -> d_bgr (optional).  One host
    round trip in between (the blended map's range sizes the colour table).  Returns info:
    base, n_midas, n_hole, blend_range, smoothed, range; None when no map is given."""
    p = dict(FUSE_DEFAULTS)
    unknown = set(params) - set(p)
    if unknown:
        raise TypeError(f"fuse_maps: unknown parameters {sorted(unknown)}")
    p.update(params)
    if d_stereo:
        base = BASE_STEREO
    elif d_midas:
        base = BASE_MIDAS
    elif d_flow:
        base = BASE_FLOW
    else:
        return None
    midas_fill = base == BASE_STEREO and bool(d_midas) and bool(p["use_midas_fill"])
    flow_fill = base != BASE_FLOW and bool(d_flow) and bool(p["use_flow_fill"])
    coef = gaussian_kernel(p["midas_blend_radius"]) if midas_fill else None
    if midas_fill and (H <= coef.size // 2 or W <= coef.size // 2):
        raise ValueError(f"fuse_maps: map {H}x{W} not larger than the blend radius {coef.size // 2}")
    fw = float(p["flow_fill_weight"])
    st = eng.fuse_blend_dev(
        d_fused, H, W, base, d_stereo=d_stereo, d_conf=d_conf if base == BASE_STEREO else 0,
        d_midas=d_midas if (base == BASE_MIDAS or midas_fill) else 0, d_flow=d_flow if (base == BASE_FLOW or flow_fill) else 0,
        midas_fill=midas_fill, flow_fill=flow_fill, stereo_weight=p["stereo_weight"],
        midas_fill_weight=p["midas_fill_weight"], conf_threshold=p["stereo_conf_threshold"],
        hole_threshold=p["flow_hole_threshold"], flow_k1=1.0 - fw, flow_k2=fw, coef=coef, stream=stream)
    mn, mx = st["min"], st["max"]
    smoothed = bool(mx > 10.0)                                       # :1687
    radius, sw, lut, scale = 0, None, None, 0.0
    if smoothed and not abs(float(mx) - float(mn)) < FLT_EPSILON:
        radius, sw, lut, scale = bilateral_tables(mn, mx, p["bilateral_d"], p["bilateral_sigma"],
                                                  p["bilateral_sigma"])
        if H <= radius or W <= radius:
            raise ValueError(f"fuse_maps: map {H}x{W} not larger than the bilateral radius {radius}")
    rng = eng.bilateral_f32_dev(d_fused, H, W, radius, sw, lut, scale, d_dst_u8=d_u8, d_dst_bgr=d_bgr,
                                cmap=cmap if d_bgr else None, minmax=True, stream=stream)
    return {"base": base, "midas_fill": midas_fill, "flow_fill": flow_fill, "n_midas": st["n_midas"],
            "n_hole": st["n_hole"], "blend_range": (mn, mx), "smoothed": smoothed, "range": rng,
            "params": p}


def fuse_maps(stereo, conf, midas, flow, *, cmap=None, engine=None, **params):
    """fuse_depth_maps' numeric body on host maps (None = absent): (fused_uint8, colormap,
    info), colormap = cmap[fused_uint8] (None without a table); None when every map is None.
    params: FUSE_DEFAULTS keys."""
    (stereo, conf, midas, flow), shape = _check_maps(
        "fuse_maps", [("stereo", stereo), ("conf", conf), ("midas", midas), ("flow", flow)])
    if stereo is None and midas is None and flow is None:
        return None
    H, W = shape
    eng = engine or get_engine()
    n = H * W
    up = lambda name, a: eng.upload(name, a) if a is not None else 0   # noqa: E731
    d_fused = eng.scratch("fuse_f32", 4 * n)
    d_u8 = eng.scratch("fuse_u8", n)
    d_bgr = eng.scratch("fuse_bgr", 3 * n) if cmap is not None else 0
    info = fuse_maps_dev(eng, H, W, up("fuse_stereo", stereo), up("fuse_conf", conf), up("fuse_midas", midas),
                         up("fuse_flow", flow), d_fused, d_u8, d_bgr, cmap, **params)
    u8 = eng.to_host(d_u8, (H, W), np.uint8)
    bgr = eng.to_host(d_bgr, (H, W, 3), np.uint8) if d_bgr else None
    return u8, bgr, info


def _normalize_plan(eng, d_dm: int, n_dm: int, d_sd: int, n_sd: int):
    """The scalars of normalize_to_stereo_range (:1523-1552) from the device maps: (affine mode,
    its parameters)."""
    sel, _ = eng.select_count(d_sd, n_sd, SEL_POSITIVE)
    if sel > 0:                                # np.any(stereo_valid)
        stereo_min, stereo_max = percentiles_dev(eng, d_sd, n_sd, [5, 95], SEL_POSITIVE)
    else:
        stereo_min, stereo_max = 0, 255
    d_min, d_max = percentiles_dev(eng, d_dm, n_dm, [5, 95])
    if (d_max - d_min) < 1e-6:
        c = np.full((1,), (stereo_min + stereo_max) / 2.0, np.float32)[0]
        return AFF_FILL, dict(fc=c)
    den = d_max - d_min + 1e-8
    rng = np.float32(stereo_max - stereo_min)
    return AFF_F32, dict(fa=d_min, fb=den, fc=np.float32(stereo_min), fd=rng)


def normalize_to_stereo_range(depth_map, stereo_disparity):
    """fused_depth_map.py:1503-1554 with the reductions and the epilogue on the GPU."""
    if depth_map is None or stereo_disparity is None:
        return None
    eng = get_engine()
    sd = _f32_map(stereo_disparity, "stereo_disparity")
    dm = _f32_map(depth_map, "depth_map")
    d_sd = eng.upload("nrm_disp", sd)
    d_dm = eng.upload("nrm_depth", dm)
    mode, kw = _normalize_plan(eng, d_dm, dm.size, d_sd, sd.size)
    return _affine(eng, d_dm, dm.shape, mode, **kw)


def flow_normalize_dev(eng, d_depth: int, n: int, d_stereo_disparity: int, d_out: int) -> None:
    """The flow normalisation of the frame loop (fused_depth_map.py:2793-2811) on device maps, in
    one elementwise pass: 255.0 - normalize_to_stereo_range(depth, disparity) with a stereo
    disparity, 255.0 - clip(depth * 255.0, 0, 255) without one (d_stereo_disparity = 0)."""
    if not d_stereo_disparity:
        eng.affine_f32_dev(d_depth, n, AFF_CLIP255_INV, d_out)
        return
    mode, kw = _normalize_plan(eng, d_depth, n, d_stereo_disparity, n)
    if mode == AFF_FILL:                        # 255.0 - np.full_like(x, c), in float32
        eng.affine_f32_dev(d_depth, n, AFF_FILL, d_out, fc=np.float32(255.0) - np.float32(kw["fc"]))
    else:
        eng.affine_f32_dev(d_depth, n, AFF_F32_INV, d_out, **kw)
