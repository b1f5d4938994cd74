"""Frame pairs for test_flow_cpu.py and test_flow_gpu.py: deterministic for a seed, built with
NumPy only (no kernel of the package takes part)."""
import numpy as np

import sv_fuse_oracle as FO
from stereovision_amd import synthetic


def smooth_texture(H, W, seed, pad=16):
    """(H + 2 pad) x (W + 2 pad) float64 in [0, 255]: synthetic._texture blurred twice (k = 9)
    and stretched to the full range, so it is smooth at the scale of the flow's windows."""
    rng = np.random.default_rng(seed)
    t = synthetic._texture(rng, H + 2 * pad, W + 2 * pad).astype(np.float32)
    t = FO.gauss_blur(FO.gauss_blur(t, 9), 9).astype(np.float64)
    return (t - t.min()) * (255.0 / (t.max() - t.min()))


def _sample(t, ys, xs):
    y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
    fy, fx = ys - y0, xs - x0
    return ((1 - fy) * ((1 - fx) * t[y0, x0] + fx * t[y0, x0 + 1]) +
            fy * ((1 - fx) * t[y0 + 1, x0] + fx * t[y0 + 1, x0 + 1]))


def _u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def translated_pair(H, W, dx, dy, seed=0, pad=16):
    """(prev, next) uint8 with next(x, y) = prev(x - dx, y - dy): the flow is (dx, dy)."""
    t = smooth_texture(H, W, seed, pad)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    return _u8(_sample(t, ys + pad, xs + pad)), _u8(_sample(t, ys + pad - dy, xs + pad - dx))


def warped_pair(H, W, Hm, seed=0, pad=16):
    """(prev, next) uint8 where a point p of prev appears at Hm p in next (Hm near the
    identity: the displaced samples must stay inside the padded texture)."""
    t = smooth_texture(H, W, seed, pad)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    inv = np.linalg.inv(np.asarray(Hm, np.float64))
    w = inv[2, 0] * xs + inv[2, 1] * ys + inv[2, 2]
    sx = (inv[0, 0] * xs + inv[0, 1] * ys + inv[0, 2]) / w
    sy = (inv[1, 0] * xs + inv[1, 1] * ys + inv[1, 2]) / w
    assert sx.min() > -pad and sy.min() > -pad and sx.max() < W + pad - 1 and sy.max() < H + pad - 1
    return _u8(_sample(t, ys + pad, xs + pad)), _u8(_sample(t, sy + pad, sx + pad))


def noise_pair(H, W, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8))


def to_bgr(gray):
    return np.ascontiguousarray(np.repeat(gray[:, :, None], 3, axis=2))
