"""Farneback optical flow and the reference's flow depth estimator on the MI355X engine.

``farneback_flow(prev, next, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)``
keeps the positional order of ``cv2.calcOpticalFlowFarneback`` after its ``flow=None`` slot and
returns the float32 H x W x 2 flow; ``OpticalFlowDepthEstimator`` keeps the attributes, state
machine and never-raise behaviour of fused_depth_map.py:1263-1501, with the previous gray frame
and ``stable_depth`` resident on the device.

The kernels (csrc/sv_flow.hip) evaluate no exp and invert no matrix: the pyramid's Gaussian
coefficients, the polynomial expansion's tables and the four entries of its inverse moment
matrix are built here in float64 ("Optical flow").  The ego-motion homography is
a host step in float64 on the step-16 grid of the flow (about 880 points at 633 x 356); only
the grid's flow vectors come back from the device (``k_flow_grid``), never the whole flow.
"""
from __future__ import annotations

import functools
import math
import time

import numpy as np

from . import fusion as _fusion
from .engine import get_engine

MIN_SIZE = 32                 # optflowgf.cpp: no pyramid scale below 32 px
FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)
GRID_STEP = 16                # fused_depth_map.py:1447


# ----------------------------------------------------------------------------------------
# host tables
# ----------------------------------------------------------------------------------------
def _check_params(H, W, pyr_scale, levels, winsize, iterations, poly_n, flags=0):
    if int(H) < 16 or int(W) < 16:
        raise ValueError(f"farneback_flow: H, W >= 16 expected, got {H}x{W}")
    if not 0.0 < float(pyr_scale) < 1.0:
        raise ValueError(f"farneback_flow: 0 < pyr_scale < 1 expected, got {pyr_scale}")
    if int(levels) != levels or levels < 0:
        raise ValueError(f"farneback_flow: levels >= 0 expected, got {levels}")
    if int(winsize) != winsize or winsize < 3 or winsize > 31 or winsize % 2 == 0:
        raise ValueError(f"farneback_flow: winsize must be odd in [3, 31], got {winsize}")
    if int(iterations) != iterations or iterations < 1:
        raise ValueError(f"farneback_flow: iterations >= 1 expected, got {iterations}")
    if poly_n not in (5, 7):
        raise ValueError(f"farneback_flow: poly_n must be 5 or 7, got {poly_n}")
    if flags != 0:
        raise ValueError("farneback_flow: only flags=0 is supported (no initial flow, no Gaussian window)")


def farneback_levels(H: int, W: int, pyr_scale: float, levels: int) -> list:
    """The pyramid of calcOpticalFlowFarneback: [(h, w, ksize, sigma)], finest first.  The scale
    of level k is pyr_scale multiplied k times; levels stop before a side falls below 32 px;
    sizes round half to even (cvRound); the blur has sigma = (1 / scale - 1) / 2 and ksize =
    max(round(5 sigma) | 1, 3)."""
    if not 0.0 < float(pyr_scale) < 1.0:
        raise ValueError(f"farneback_levels: 0 < pyr_scale < 1 expected, got {pyr_scale}")
    if levels < 0:
        raise ValueError(f"farneback_levels: levels >= 0 expected, got {levels}")
    k, scale = 0, 1.0
    while k < levels:
        scale *= pyr_scale
        if W * scale < MIN_SIZE or H * scale < MIN_SIZE:
            break
        k += 1
    out = []
    for lv in range(k + 1):
        scale = 1.0
        for _ in range(lv):
            scale *= pyr_scale
        sigma = (1.0 / scale - 1) * 0.5
        ksize = max(int(np.rint(sigma * 5)) | 1, 3)
        if ksize > 31:
            raise ValueError(f"farneback_levels: level {lv} needs a Gaussian ksize of {ksize} > 31")
        out.append((int(np.rint(H * scale)), int(np.rint(W * scale)), ksize, sigma))
    return out


def gaussian_coef(ksize: int, sigma: float) -> np.ndarray:
    """cv2.getGaussianKernel(ksize, sigma, CV_32F): the rule of fusion.gaussian_kernel with an
    explicit sigma; sigma <= 0 with ksize 3 is OpenCV's fixed (0.25, 0.5, 0.25)."""
    ksize = int(ksize)
    if ksize < 3 or ksize > 31 or ksize % 2 == 0:
        raise ValueError(f"gaussian_coef: ksize must be odd in [3, 31], got {ksize}")
    if sigma <= 0:
        if ksize != 3:
            raise ValueError("gaussian_coef: sigma <= 0 is defined for ksize 3 only")
        return np.array([0.25, 0.5, 0.25], np.float32)
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    g = np.exp((-0.5 / (sigma * sigma)) * (x * x)).astype(np.float32)
    total = 0.0
    for v in g:                       # in index order: the sum is part of the definition
        total += float(v)
    return (g.astype(np.float64) * (1.0 / total)).astype(np.float32)


def polyexp_tables(poly_n: int, poly_sigma: float):
    """FarnebackPrepareGaussian: (g, xg, xxg, (ig11, ig03, ig33, ig55)); the tables hold x =
    0..poly_n (g is even in x, xg odd).  g = float32(exp(-x^2 / (2 sigma^2))) normalised by the
    float64 sum over x = -n..n; the moment sums take float32 products into float64 sums, y outer
    and x inner; the needed entries of the inverse are closed forms of the block structure."""
    n = int(poly_n)
    if n not in (5, 7):
        raise ValueError(f"polyexp_tables: poly_n must be 5 or 7, got {poly_n}")
    return _polyexp_tables(n, float(poly_sigma))


@functools.lru_cache(maxsize=16)
def _polyexp_tables(n, sigma):          # (read-only arrays: one set per (n, sigma) serves every frame)
    if sigma < FLT_EPSILON:
        sigma = n * 0.3
    xs = np.arange(-n, n + 1)
    g = np.exp(-(xs * xs).astype(np.float64) / (2 * sigma * sigma)).astype(np.float32)
    total = 0.0
    for v in g:
        total += float(v)
    g = (g.astype(np.float64) * (1.0 / total)).astype(np.float32)
    xf = xs.astype(np.float32)
    xg = xf * g
    xxg = (xf * xf) * g
    g00 = g11 = g33 = g55 = 0.0
    for iy in range(2 * n + 1):
        for ix in range(2 * n + 1):
            p = g[iy] * g[ix]
            x, y = xf[ix], xf[iy]
            g00 += float(p)
            g11 += float(p * x * x)
            g33 += float(p * x * x * x * x)
            g55 += float(p * x * x * y * y)
    # rows (1, x^2, y^2) of G: [[g00, g11, g11], [g11, g33, g55], [g11, g55, g33]]
    den = g00 * (g33 + g55) - (2.0 * g11) * g11
    ig = (1.0 / g11, -g11 / den, (g00 * g33 - g11 * g11) / ((g33 - g55) * den), 1.0 / g55)
    out = (g[n:].copy(), xg[n:].copy(), xxg[n:].copy())
    for t in out:
        t.setflags(write=False)
    return out + (ig,)


# ----------------------------------------------------------------------------------------
# the flow
# ----------------------------------------------------------------------------------------
def farneback_flow_dev(eng, d_prev: int, d_next: int, H: int, W: int, pyr_scale=0.5, levels=3, winsize=15,
                       iterations=3, poly_n=5, poly_sigma=1.2, flags=0, d_flow: int = 0, pitch: int = None,
                       stream: int = 0) -> None:
    """calcOpticalFlowFarneback of two gray uint8 device frames into d_flow (float32 H x W x 2).
    Every launch is enqueued on `stream`; nothing waits for the device."""
    _check_params(H, W, pyr_scale, levels, winsize, iterations, poly_n, flags)
    if not d_prev or not d_next or not d_flow:
        raise ValueError("farneback_flow_dev: null device pointer")
    lv = farneback_levels(H, W, pyr_scale, levels)
    scales = [(h, w, k, gaussian_coef(k, s)) for h, w, k, s in lv]
    eng.farneback_flow_dev(d_prev, d_next, H, W, W if pitch is None else pitch, scales,
                           np.float32(1.0 / float(pyr_scale)), winsize, iterations, poly_n,
                           polyexp_tables(poly_n, poly_sigma), d_flow, stream)


def _gray_u8(a, name):
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError(f"{name}: uint8 expected, got {a.dtype}")
    if a.ndim != 2:
        raise ValueError(f"{name}: a gray H x W frame expected, got shape {a.shape}")
    return np.ascontiguousarray(a)


def farneback_flow(prev, next, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2,
                   flags=0, engine=None) -> np.ndarray:
    """cv2.calcOpticalFlowFarneback(prev, next, None, ...) on the GPU: float32 H x W x 2."""
    prev, next = _gray_u8(prev, "prev"), _gray_u8(next, "next")
    if prev.shape != next.shape:
        raise ValueError(f"farneback_flow: frames differ in shape: {prev.shape} and {next.shape}")
    H, W = prev.shape
    _check_params(H, W, pyr_scale, levels, winsize, iterations, poly_n, flags)
    farneback_levels(H, W, pyr_scale, levels)          # a ksize above 31 raises before any upload
    eng = engine or get_engine()
    d_prev = eng.upload("fb_prev", prev)
    d_next = eng.upload("fb_next", next)
    d_flow = eng.scratch("fb_flow", 8 * H * W)
    farneback_flow_dev(eng, d_prev, d_next, H, W, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma,
                       flags, d_flow)
    return eng.to_host(d_flow, (H, W, 2), np.float32)


# ----------------------------------------------------------------------------------------
# ego motion: a RANSAC homography on the host (build-defined, deterministic)
# ----------------------------------------------------------------------------------------
def _normalization(p):
    c = p.mean(axis=0)
    d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    if not d > 0:
        return None
    s = math.sqrt(2.0) / d
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]], np.float64)


def _dlt(src, dst):
    """Normalised DLT (least squares for more than 4 pairs), scaled to h33 = 1; None when the
    configuration is degenerate."""
    T1, T2 = _normalization(src), _normalization(dst)
    if T1 is None or T2 is None:
        return None
    a = src * T1[0, 0] + T1[:2, 2]
    b = dst * T2[0, 0] + T2[:2, 2]
    n = len(a)
    A = np.zeros((2 * n, 9), np.float64)
    A[0::2, 0:2], A[0::2, 2] = a, 1
    A[0::2, 6:8], A[0::2, 8] = -b[:, 0:1] * a, -b[:, 0]
    A[1::2, 3:5], A[1::2, 5] = a, 1
    A[1::2, 6:8], A[1::2, 8] = -b[:, 1:2] * a, -b[:, 1]
    try:
        # the 9th right singular vector exists only in the full form when A has 8 rows
        _, s, vt = np.linalg.svd(A, full_matrices=2 * n < 9)
    except np.linalg.LinAlgError:
        return None
    if s.size < 8 or not s[7] > 1e-9 * s[0]:            # a null space of more than one dimension
        return None
    Hn = vt[8].reshape(3, 3)
    Hm = np.linalg.solve(T2, Hn @ T1)
    if not np.all(np.isfinite(Hm)) or abs(Hm[2, 2]) < 1e-12 * np.abs(Hm).max():
        return None
    return Hm / Hm[2, 2]


def _reproj_err2(Hm, src, dst):
    w = src[:, 0] * Hm[2, 0] + src[:, 1] * Hm[2, 1] + Hm[2, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (src[:, 0] * Hm[0, 0] + src[:, 1] * Hm[0, 1] + Hm[0, 2]) / w
        y = (src[:, 0] * Hm[1, 0] + src[:, 1] * Hm[1, 1] + Hm[1, 2]) / w
    e = (x - dst[:, 0]) ** 2 + (y - dst[:, 1]) ** 2
    return np.where(np.isfinite(e), e, np.inf)


def find_homography_ransac(src_points, dst_points, reproj_threshold=3.0, max_iters=2000, confidence=0.995,
                           seed=0):
    """cv2.findHomography(src, dst, RANSAC, 3.0, maxIters=2000, confidence=0.995), build-defined:
    normalised DLT on 4-point samples drawn by a generator seeded per call, the usual adaptive
    iteration count, and a normalised-DLT least-squares refit on the inliers of the best sample.
    Returns (H float64 3x3 with h33 = 1, mask uint8 N x 1) or (None, None)."""
    src = np.asarray(src_points, np.float64).reshape(-1, 2)
    dst = np.asarray(dst_points, np.float64).reshape(-1, 2)
    n = len(src)
    if n < 4 or len(dst) != n or not (np.all(np.isfinite(src)) and np.all(np.isfinite(dst))):
        return None, None
    rng = np.random.default_rng(seed)
    thr2 = float(reproj_threshold) ** 2
    best, best_mask = 0, None
    niters, i = int(max_iters), 0
    log_fail = math.log(1.0 - confidence)
    while i < niters:
        i += 1
        idx = rng.choice(n, 4, replace=False)
        Hm = _dlt(src[idx], dst[idx])
        if Hm is None:
            continue
        mask = _reproj_err2(Hm, src, dst) <= thr2
        count = int(mask.sum())
        if count > max(best, 3):
            best, best_mask = count, mask
            p4 = (count / n) ** 4
            if p4 >= 1.0:
                break
            niters = min(niters, max(int(math.ceil(log_fail / math.log(1.0 - p4))), 1))
    if best_mask is None:
        return None, None
    Hm = _dlt(src[best_mask], dst[best_mask])
    if Hm is None:
        return None, None
    return Hm, best_mask.astype(np.uint8).reshape(-1, 1)


# ----------------------------------------------------------------------------------------
# residual depth
# ----------------------------------------------------------------------------------------
def expected_flow(Hm, H: int, W: int) -> np.ndarray:
    """cv2.perspectiveTransform(grid, Hm) - grid on float32 points (fused_depth_map.py:1492-1498),
    on the host: float64 inside, w = 0 where |w| <= DBL_EPSILON."""
    m = np.asarray(Hm, np.float64).reshape(9)
    xf = np.arange(W, dtype=np.float32)[None, :]
    yf = np.arange(H, dtype=np.float32)[:, None]
    x, y = xf.astype(np.float64), yf.astype(np.float64)
    w = (x * m[6] + y * m[7]) + m[8]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(np.abs(w) > DBL_EPSILON, 1.0 / w, 0.0)
    out = np.empty((H, W, 2), np.float32)
    out[..., 0] = (((x * m[0] + y * m[1]) + m[2]) * w).astype(np.float32) - xf
    out[..., 1] = (((x * m[3] + y * m[4]) + m[5]) * w).astype(np.float32) - yf
    return out


def flow_depth_dev(eng, d_flow: int, H: int, W: int, Hm, d_depth: int, d_stable: int = 0, alpha=0.9,
                   minmax: bool = True, stream: int = 0):
    """depth = 1 / (|flow - expected_flow(Hm)| + 0.5) on the device, optionally with the
    exponential average stable = alpha stable + (1 - alpha) depth; (min, max) of depth."""
    Hm = np.asarray(Hm, np.float64)
    if Hm.size != 9 or not np.all(np.isfinite(Hm)):
        raise ValueError("flow_depth: a finite 3x3 homography expected")
    return eng.flow_depth_dev(d_flow, H, W, Hm, d_depth, d_stable, alpha, minmax, stream)


def flow_depth(flow, Hm, stable=None, alpha=0.9, engine=None):
    """Host arrays in and out: (depth, new stable or None, (min, max))."""
    flow = np.ascontiguousarray(flow)
    if flow.dtype != np.float32:
        raise TypeError(f"flow_depth: float32 flow expected, got {flow.dtype}")
    if flow.ndim != 3 or flow.shape[2] != 2:
        raise ValueError(f"flow_depth: H x W x 2 flow expected, got shape {flow.shape}")
    H, W = flow.shape[:2]
    eng = engine or get_engine()
    d_flow = eng.upload("fd_flow", flow)
    d_depth = eng.scratch("fd_depth", 4 * H * W)
    d_stable = 0
    if stable is not None:
        stable = np.ascontiguousarray(stable, np.float32)
        if stable.shape != (H, W):
            raise ValueError(f"flow_depth: stable map {stable.shape}, expected {(H, W)}")
        d_stable = eng.upload("fd_stable", stable)
    mm = flow_depth_dev(eng, d_flow, H, W, Hm, d_depth, d_stable, alpha)
    depth = eng.to_host(d_depth, (H, W), np.float32)
    return depth, (eng.to_host(d_stable, (H, W), np.float32) if d_stable else None), mm


# ----------------------------------------------------------------------------------------
# the estimator   fused_depth_map.py:1263-1501
# ----------------------------------------------------------------------------------------
class OpticalFlowDepthEstimator:
    """fused_depth_map.py:1263-1501 on the MI355X engine: Farneback flow between consecutive
    frames, a RANSAC homography for the camera's own motion, the residual flow turned into
    1 / (m + 0.5), an exponential average and a bilateral filter.  Returns a float32 map, or
    None on the first frame, on a size change, on a static scene and on any error.
    ``step_dev`` is the same call on a gray frame that is already on the device."""

    FLOW_ARGS = (0.5, 3, 15, 3, 5, 1.2, 0)             # :1361-1370

    def __init__(self, min_inliers=15, motion_timeout=1.5, engine=None):
        self.min_inliers = min_inliers
        self.motion_timeout = motion_timeout
        self.last_move_time = time.time()
        self.camera_moving = False
        self.last_homography = None
        self._eng = engine
        self._shape = None          # (H, W) of the previous gray frame on the device
        self._bufs = {}
        self._buf_shape = None
        self._prev = 0              # device pointer of the previous gray frame (own buffer or the caller's)
        self._have_stable = False
        print("[INFO] optical-flow depth estimator initialised")
        print(f"       inlier threshold: {min_inliers}, motion timeout: {motion_timeout} s")

    # -- device state ---------------------------------------------------------------------
    @property
    def prev_gray(self):
        if self._shape is None:
            return None
        return self._eng.to_host(self._prev, self._shape, np.uint8)

    @prev_gray.setter
    def prev_gray(self, value):
        if value is not None:
            raise ValueError("prev_gray lives on the device; only None (reset) can be assigned")
        self._shape = None

    @property
    def stable_depth(self):
        if not self._have_stable or self._shape is None:
            return None
        return self._eng.to_host(self._bufs["stable"], self._shape, np.float32)

    @stable_depth.setter
    def stable_depth(self, value):
        if value is not None:
            raise ValueError("stable_depth lives on the device; only None (reset) can be assigned")
        self._have_stable = False

    def _free(self):
        eng, bufs = self._eng, self._bufs
        self._bufs, self._buf_shape = {}, None
        for v in bufs.values():
            for p in (v if isinstance(v, list) else [v]):
                try:
                    eng.dev_free(p)
                except Exception:
                    pass

    def __del__(self):  # pragma: no cover - best effort
        try:
            if getattr(self._eng, "handle", None):
                self._free()
        except Exception:
            pass

    def _alloc(self, H, W):
        self._free()
        n, a = H * W, self._eng.dev_alloc
        points = len(range(GRID_STEP // 2, H, GRID_STEP)) * len(range(GRID_STEP // 2, W, GRID_STEP))
        self._bufs = {"gray": [a(n), a(n)], "flow": a(8 * n), "depth": a(4 * n), "stable": a(4 * n),
                      "out": a(4 * n), "grid": a(max(8 * points, 8))}
        self._buf_shape = (H, W)

    def _load_gray(self, frame, d_gray):
        """The device pointer of the new gray frame: the caller's (step_dev), or the own buffer
        that does not hold the previous frame, filled from the host frame."""
        if d_gray:
            return d_gray
        eng, g = self._eng, self._bufs["gray"]
        dst = g[1] if self._prev == g[0] else g[0]
        H, W = frame.shape[:2]
        if frame.ndim == 3:
            d_bgr = eng.upload("ofd_bgr", frame)
            eng.gray_dev(d_bgr, H, W, W * 3, dst)
        else:
            eng.to_device(dst, frame)
        return dst

    # -- the call ---------------------------------------------------------------------------
    def __call__(self, frame):
        try:
            return self._step(frame)
        except Exception:
            return None

    def step_dev(self, d_gray: int, H: int, W: int):
        """__call__ on a dense gray uint8 H x W frame in device memory: the same state machine
        and results, with no upload of the frame and no download of the map.  Returns the
        device pointer of the float32 H x W map (the estimator's buffer, valid until its next
        call), or None where __call__ returns None.  The frame at d_gray becomes the previous
        frame: the caller leaves it unchanged until the estimator's next call has returned."""
        try:
            if not d_gray or int(H) <= 0 or int(W) <= 0:
                return None
            return self._advance((int(H), int(W)), None, int(d_gray))
        except Exception:
            return None

    def _step(self, frame):
        if frame is None or frame.size == 0:
            return None
        frame = np.ascontiguousarray(frame)
        if frame.dtype != np.uint8 or not (frame.ndim == 2 or (frame.ndim == 3 and frame.shape[2] == 3)):
            return None
        shape = frame.shape[:2]
        d_out = self._advance(shape, frame, 0)
        return None if d_out is None else self._eng.to_host(d_out, shape, np.float32)

    def _advance(self, shape, frame, d_gray):
        if self._eng is None:
            self._eng = get_engine()
        if self._shape is None or shape != self._shape:      # the first frame, or a size change
            if self._shape is not None:
                self._have_stable = False
            self._shape = None
            if self._buf_shape != shape:
                self._have_stable = False
                self._alloc(*shape)
            self._prev = self._load_gray(frame, d_gray)
            self._shape = shape
            return None
        H, W = shape
        eng, b = self._eng, self._bufs
        nxt = self._load_gray(frame, d_gray)
        current_time = time.time()
        self.camera_moving = (current_time - self.last_move_time) < self.motion_timeout
        try:
            ego_valid, Hm = False, None
            if H >= 16 and W >= 16:
                farneback_flow_dev(eng, self._prev, nxt, H, W, *self.FLOW_ARGS, d_flow=b["flow"])
                ego_valid, Hm = self._estimate_ego_motion(H, W)
        finally:
            self._prev = nxt                             # the new frame is the previous one from now on
        if ego_valid:
            self.last_move_time = current_time
            self.camera_moving = True
            self.last_homography = Hm
            if self._have_stable:
                mn, mx = flow_depth_dev(eng, b["flow"], H, W, Hm, b["depth"], b["stable"], alpha=0.9)
            else:
                mn, mx = flow_depth_dev(eng, b["flow"], H, W, Hm, b["depth"])
                eng.bilateral_f32_dev(b["depth"], H, W, 0, None, None, 0.0, d_dst_f32=b["stable"])   # a copy
                self._have_stable = True
            _fusion.bilateral_filter_dev(eng, b["depth"], H, W, mn, mx, 9, 75, 75, b["out"])
            return b["out"]
        if self.camera_moving and self._have_stable:
            # the stable map lies in (0, 2], so the clipped range of the radius-0 pass is its range
            mn, mx = eng.bilateral_f32_dev(b["stable"], H, W, 0, None, None, 0.0, minmax=True)
            _fusion.bilateral_filter_dev(eng, b["stable"], H, W, mn, mx, 9, 75, 75, b["out"])
            return b["out"]
        return None

    def _estimate_ego_motion(self, H, W):
        """fused_depth_map.py:1419-1501 up to the homography: (valid, H)."""
        if H < 50 or W < 50:
            return False, None
        y_coords, x_coords = np.mgrid[GRID_STEP // 2:H:GRID_STEP, GRID_STEP // 2:W:GRID_STEP]
        points = np.vstack((x_coords.ravel(), y_coords.ravel())).T.astype(np.float32)
        if len(points) == 0 or len(points) < self.min_inliers * 2:
            return False, None
        # the flow at the grid alone crosses to the host (k_flow_grid), in the order of `points`
        self._eng.flow_grid_dev(self._bufs["flow"], H, W, GRID_STEP, self._bufs["grid"])
        flow_vectors = self._eng.to_host(self._bufs["grid"], (len(points), 2), np.float32)
        next_points = points + flow_vectors
        Hm, mask = find_homography_ransac(points, next_points, 3.0, 2000, 0.995)
        if Hm is None or mask is None or np.sum(mask) < self.min_inliers:
            return False, None
        return True, Hm
