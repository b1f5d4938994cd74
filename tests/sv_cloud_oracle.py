"""NumPy restatement of the 3D reprojection and the ordered point cloud: the
contract of sv_cloud.hip.  It follows cv2.reprojectImageTo3D(disparity, Q, handleMissingValues,
ddepth=CV_32F) as far as OpenCV's source is known: the homogeneous point is a Matx product in
f64 whose sums start from 0, it is narrowed to f32, and the division is a multiplication by the
f64 reciprocal (Vec /= double).  cv2 itself is not available to the tests, so parity with a
particular OpenCV build is unpinned.
"""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
MISSING_Z = np.float32(10000.0)


def disparity_f64(disp: np.ndarray) -> np.ndarray:
    """d of every pixel: f64(f32(m) / 16) of an int16 x16 map, f64(v) of an f32 map."""
    if disp.dtype == np.int16:
        return (disp.astype(np.float32) / np.float32(16)).astype(np.float64)
    if disp.dtype == np.float32:
        return disp.astype(np.float64)
    raise TypeError(f"int16 or float32 expected, got {disp.dtype}")


def map_minimum(d: np.ndarray) -> float:
    """The minimum of d, NaNs ignored; +inf when nothing is left."""
    v = d[~np.isnan(d)]
    return float(v.min()) if v.size else float("inf")


def missing_mask(d: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.abs(d - map_minimum(d)) <= FLT_EPSILON


def homogeneous(d: np.ndarray, Q: np.ndarray):
    """The four rows h_r = (((0 + q_r0 x) + q_r1 y) + q_r2 d) + q_r3 in f64."""
    H, W = d.shape
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        return [(((0.0 + Q[r, 0] * x) + Q[r, 1] * y) + Q[r, 2] * d) + Q[r, 3] * 1.0 for r in range(4)]


def reproject_image_to_3d(disp: np.ndarray, Q, handle_missing: bool = False) -> np.ndarray:
    """The dense H x W x 3 float32 map."""
    d = disparity_f64(disp)
    h = homogeneous(d, Q)
    with np.errstate(all="ignore"):
        ia = 1.0 / h[3]
        out = np.stack([(h[r].astype(np.float32).astype(np.float64) * ia).astype(np.float32) for r in range(3)],
                       axis=-1)
    if handle_missing:
        out[..., 2][missing_mask(d)] = MISSING_Z
    return out


def point_cloud(disp: np.ndarray, Q, colors=None, min_valid=0.0, z_min=-np.inf, z_max=np.inf, roi=None,
                handle_missing: bool = False, cap=None):
    """(xyz, bgr or None, index, N): the valid pixels in row-major order, the first `cap` of them."""
    H, W = disp.shape
    d = disparity_f64(disp)
    xyz = reproject_image_to_3d(disp, Q, False)
    with np.errstate(invalid="ignore"):
        ok = d >= np.float64(np.float32(min_valid))
        ok &= np.isfinite(xyz).all(axis=-1)
        ok &= (np.float32(z_min) <= xyz[..., 2]) & (xyz[..., 2] <= np.float32(z_max))
    if roi is not None:
        rx, ry, rw, rh = roi
        inside = np.zeros((H, W), bool)
        inside[ry:ry + rh, rx:rx + rw] = True
        ok &= inside
    if handle_missing:
        ok &= ~missing_mask(d)
    idx = np.flatnonzero(ok.ravel()).astype(np.uint32)
    n = int(idx.size)
    if cap is not None:
        idx = idx[:cap]
    pts = xyz.reshape(-1, 3)[idx]
    bgr = None if colors is None else np.ascontiguousarray(colors.reshape(-1, 3)[idx])
    return np.ascontiguousarray(pts), bgr, idx, n
