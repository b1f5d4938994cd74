"""NumPy restatement of fuse_depth_maps' arithmetic, the oracle of
test_fuse_cpu.py and test_fuse_gpu.py.  Independent of stereovision_amd: nothing is imported
from the package.  Vectorised over pixels, loops over taps; every float32 operation is one
NumPy operation on float32 arrays, so it rounds once, in the stated order.

  gauss_kernel / gauss_blur        cv2.GaussianBlur(x, (k, k), 0), BORDER_REFLECT_101
  bilateral_tables / bilateral     cv2.bilateralFilter on one float32 channel
  fuse                             the blend, smoothing and quantisation of fuse_depth_maps
"""
import numpy as np

F32 = np.float32
BINS = 4096
EPS = float(np.finfo(np.float32).eps)


def _pad(x, r):
    return np.pad(x, r, mode="reflect")          # reflect-101: the border pixel is not repeated


def gauss_kernel(k):
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    xs = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    g = np.exp((-0.5 / (sigma * sigma)) * (xs * xs)).astype(F32)
    s = 0.0
    for v in g:
        s += float(v)
    return (g.astype(np.float64) * (1.0 / s)).astype(F32)


def _pass(x, c, r, axis):
    n = x.shape[axis] - 2 * r

    def at(o):
        sl = [slice(None), slice(None)]
        sl[axis] = slice(r + o, r + o + n)
        return x[tuple(sl)]

    s = c[r] * at(0)
    for i in range(1, r + 1):
        s = s + c[r + i] * (at(-i) + at(i))
    return s


def gauss_blur(x, k):
    x = np.asarray(x, F32)
    r = k // 2
    assert x.shape[0] > r and x.shape[1] > r
    c = gauss_kernel(k)
    rows = _pass(_pad(x, r), c, r, 1)             # rows first: (H + 2r) x W, float32
    out = _pass(rows, c, r, 0)
    assert out.dtype == F32 and out.shape == x.shape
    return out


def bilateral_radius(d, sigma_space):
    if sigma_space <= 0:
        sigma_space = 1
    r = d // 2 if d > 0 else int(round(1.5 * sigma_space))
    return max(r, 1)


def taps(r):
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)
            if not (dy == 0 and dx == 0) and not np.sqrt(float(dy * dy + dx * dx)) > r]


def bilateral_tables(mn, mx, d, sigma_color, sigma_space):
    if sigma_color <= 0:
        sigma_color = 1
    if sigma_space <= 0:
        sigma_space = 1
    r = bilateral_radius(d, sigma_space)
    t = taps(r)
    d2 = np.array([dy * dy + dx * dx for dy, dx in t], np.float64)
    sw = np.exp(d2 * (-0.5 / (float(sigma_space) * float(sigma_space)))).astype(F32)
    length = F32(np.float64(mx) - np.float64(mn))
    scale = F32(BINS) / length
    assert scale.dtype == F32
    i = np.arange(BINS + 2, dtype=np.float64) / np.float64(scale)
    lut = np.exp(i * i * (-0.5 / (float(sigma_color) * float(sigma_color)))).astype(F32)
    first0 = np.flatnonzero(lut == 0)
    if first0.size:
        lut[first0[0]:] = 0
    return r, sw, lut, scale


def bilateral(src, d, sigma_color, sigma_space, check=None):
    src = np.asarray(src, F32)
    H, W = src.shape
    mn, mx = src.min(), src.max()
    if abs(float(mx) - float(mn)) < EPS:
        return src.copy()
    r, sw, lut, scale = bilateral_tables(mn, mx, d, sigma_color, sigma_space)
    assert H > r and W > r
    p = _pad(src, r)
    c = src
    total = np.zeros((H, W), F32)
    wsum = np.zeros((H, W), F32)
    top = 0
    for (dy, dx), w_s in zip(taps(r), sw):
        v = p[r + dy:r + dy + H, r + dx:r + dx + W]
        a = np.abs(v - c) * scale
        idx = a.astype(np.int32)
        top = max(top, int(idx.max()))
        a = a - idx.astype(F32)
        w = w_s * (lut[idx] + a * (lut[idx + 1] - lut[idx]))
        total = total + v * w
        wsum = wsum + w
    if check is not None:
        check["max_idx"] = top
    out = (total + c) / (wsum + F32(1))
    assert out.dtype == F32
    return out


def fuse(stereo, conf, midas, flow, *, stereo_weight=0.8, midas_fill_weight=0.9, flow_fill_weight=0.5,
         stereo_conf_threshold=0.5, flow_hole_threshold=15, use_midas_fill=True, use_flow_fill=True,
         midas_blend_radius=15, bilateral_d=9, bilateral_sigma=75):
    """Maps that are not valid are passed as None (flow: also when the camera is static).
    Returns None, or a dict: u8, f32 (the clipped map), n_midas, n_hole, range, base, smoothed."""
    if stereo is None and midas is None and flow is None:
        return None
    n_midas = n_hole = 0
    if stereo is not None:
        base = "stereo"
        fused = np.asarray(stereo, F32) * F32(stereo_weight)
        cf = np.asarray(conf, F32) if conf is not None else np.ones(fused.shape, F32)
        if midas is not None and use_midas_fill:
            fw = (F32(1) - cf) * F32(midas_fill_weight)
            fw = gauss_blur(fw, midas_blend_radius)
            fw = np.clip(fw, F32(0), F32(1))
            mask = (cf < F32(stereo_conf_threshold)) & (fw > F32(0.1))
            n_midas = int(mask.sum())
            t0 = fused * (F32(1) - fw)
            t1 = np.asarray(midas, F32) * fw
            fused = np.where(mask, t0 + t1, fused)
    elif midas is not None:
        base = "midas"
        fused = np.asarray(midas, F32).copy()
    else:
        base = "flow"
        fused = np.asarray(flow, F32).copy()
    if base != "flow" and flow is not None and use_flow_fill:
        hole = (fused < F32(flow_hole_threshold)) | (fused == 0)
        n_hole = int(hole.sum())
        k1 = F32(1.0 - float(flow_fill_weight))
        k2 = F32(flow_fill_weight)
        fused = np.where(hole, fused * k1 + np.asarray(flow, F32) * k2, fused)
    assert fused.dtype == F32
    smoothed = bool(fused.max() > 10.0)
    if smoothed:
        fused = bilateral(fused, bilateral_d, bilateral_sigma, bilateral_sigma)
    fused = np.clip(fused, F32(0), F32(255))
    u8 = fused.astype(np.uint8)
    return {"u8": u8, "f32": fused, "n_midas": n_midas, "n_hole": n_hole,
            "range": (fused.min(), fused.max()), "base": base, "smoothed": smoothed}
