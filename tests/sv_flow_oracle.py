"""NumPy restatement of the Farneback optical flow and the flow depth estimator's arithmetic
("Optical flow"), the oracle of test_flow_cpu.py and test_flow_gpu.py.
Independent of stereovision_amd: nothing is imported from the package.  Vectorised over
pixels, loops over taps; every float32 / float64 operation is one NumPy operation on arrays of
that type, so it rounds once, in the stated order.

  levels                     the pyramid: (h, w, ksize, sigma) per scale, finest first
  gauss_coef / pyramid_image u8 -> f32, Gaussian blur with an explicit sigma, INTER_LINEAR resize
  polyexp_tables / polyexp   FarnebackPolyExp: five coefficient planes
  update_matrices            FarnebackUpdateMatrices: five planes of M
  blur_solve                 FarnebackUpdateFlow_Blur: box sums and the 2x2 solve
  farneback                  the whole of cv2.calcOpticalFlowFarneback(prev, next, None, ...)
  expected_flow / flow_depth the homography's flow, residual, 1/(m + 0.5), exponential average

R, M and the per-level flow are planes (5 x H x W, 5 x H x W, 2 x H x W); the result of
farneback is H x W x 2 as OpenCV returns it.
"""
import numpy as np

import sv_fuse_oracle as FO

F32 = np.float32
F64 = np.float64
MIN_SIZE = 32
BORDER = np.array([0.14, 0.14, 0.4472, 0.4472, 0.4472], F32)
DBL_EPSILON = float(np.finfo(np.float64).eps)
FLT_EPSILON = float(np.finfo(np.float32).eps)


# ---------------------------------------------------------------------------- pyramid
def levels(H, W, pyr_scale, nlevels):
    k, scale = 0, 1.0
    while k < nlevels:
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
        out.append((int(np.rint(H * scale)), int(np.rint(W * scale)), ksize, sigma))
    return out


def gauss_coef(ksize, sigma):
    if sigma <= 0:
        assert ksize == 3
        return np.array([0.25, 0.5, 0.25], F32)
    xs = np.arange(ksize, dtype=F64) - (ksize - 1) * 0.5
    g = np.exp((-0.5 / (sigma * sigma)) * (xs * xs)).astype(F32)
    s = 0.0
    for v in g:
        s += float(v)
    return (g.astype(F64) * (1.0 / s)).astype(F32)


def gauss_blur(x, coef):
    x = np.asarray(x, F32)
    r = coef.size // 2
    assert x.shape[0] > r and x.shape[1] > r
    rows = FO._pass(FO._pad(x, r), coef, r, 1)
    out = FO._pass(rows, coef, r, 0)
    assert out.dtype == F32
    return out


def _resize_axis(dn, sn, scale, zero_frac):
    f = ((np.arange(dn, dtype=F64) + 0.5) * scale - 0.5).astype(F32)
    i = np.floor(f).astype(np.int64)
    f = f - i.astype(F32)
    if zero_frac:                                   # columns: clamped with a zero fraction
        f[(i < 0) | (i >= sn - 1)] = 0
        i = np.clip(i, 0, sn - 1)
    return np.clip(i, 0, sn - 1), np.clip(i + 1, 0, sn - 1), f


def resize_f32(src, h, w):
    """cv2.resize(float32 map, (w, h), INTER_LINEAR) as sv_resize_linear_f32_dev defines it."""
    src = np.asarray(src, F32)
    sH, sW = src.shape
    if (sH, sW) == (h, w):
        return src.copy()
    sx, sy = 1.0 / (w / sW), 1.0 / (h / sH)
    if sx == 2.0 and sy == 2.0:                     # the exact 2x downscale: 2x2 mean
        s = src
        return ((((s[0::2, 0::2] + s[0::2, 1::2]) + s[1::2, 0::2]) + s[1::2, 1::2]) * F32(0.25))[:h, :w]
    x0, x1, fx = _resize_axis(w, sW, sx, True)
    y0, y1, fy = _resize_axis(h, sH, sy, False)
    ax0, by0 = F32(1) - fx, (F32(1) - fy)[:, None]
    h0 = src[y0][:, x0] * ax0 + src[y0][:, x1] * fx
    h1 = src[y1][:, x0] * ax0 + src[y1][:, x1] * fx
    out = h0 * by0 + h1 * fy[:, None]
    assert out.dtype == F32
    return out


def pyramid_image(img_u8, level):
    h, w, ksize, sigma = level
    f = gauss_blur(np.asarray(img_u8, np.uint8).astype(F32), gauss_coef(ksize, sigma))
    return resize_f32(f, h, w)


# ---------------------------------------------------------------------------- polynomial expansion
def polyexp_tables(n, sigma):
    """g, xg, xxg for x = 0..n (g is even, xg odd) and (ig11, ig03, ig33, ig55) in float64."""
    if sigma < FLT_EPSILON:
        sigma = n * 0.3
    xs = np.arange(-n, n + 1)
    g = np.exp(-(xs * xs).astype(F64) / (2 * sigma * sigma)).astype(F32)
    s = 0.0
    for v in g:
        s += float(v)
    g = (g.astype(F64) * (1.0 / s)).astype(F32)
    xf = xs.astype(F32)
    xg = xf * g
    xxg = (xf * xf) * g
    a = b = c = d = 0.0                              # G00, G11, G33, G55: f32 products, f64 sums
    for iy in range(2 * n + 1):
        for ix in range(2 * n + 1):
            p = g[iy] * g[ix]
            x, y = xf[ix], xf[iy]
            a += float(p)
            b += float(p * x * x)
            c += float(p * x * x * x * x)
            d += float(p * x * x * y * y)
    # G = [[a, b, b], [b, c, d], [b, d, c]] on (1, x^2, y^2); b on x and y; d on xy
    den = a * (c + d) - (2.0 * b) * b
    ig11 = 1.0 / b
    ig03 = -b / den
    ig33 = (a * c - b * b) / ((c - d) * den)
    ig55 = 1.0 / d
    return g[n:].copy(), xg[n:].copy(), xxg[n:].copy(), (ig11, ig03, ig33, ig55)


def polyexp(img, n, sigma):
    img = np.asarray(img, F32)
    H, W = img.shape
    g, xg, xxg, (ig11, ig03, ig33, ig55) = polyexp_tables(n, sigma)
    rows = np.arange(H)
    c0 = img * g[0]
    c1 = np.zeros((H, W), F32)
    c2 = np.zeros((H, W), F32)
    for k in range(1, n + 1):
        above = img[np.maximum(rows - k, 0)]
        below = img[np.minimum(rows + k, H - 1)]
        p = above + below
        c0 = c0 + g[k] * p
        c1 = c1 + xg[k] * (below - above)
        c2 = c2 + xxg[k] * p
    assert c0.dtype == c1.dtype == c2.dtype == F32
    cols = np.arange(W)
    b1 = (c0 * g[0]).astype(F64)
    b3 = (c1 * g[0]).astype(F64)
    b5 = (c2 * g[0]).astype(F64)
    b2 = np.zeros((H, W), F64)
    b4 = np.zeros((H, W), F64)
    b6 = np.zeros((H, W), F64)
    for k in range(1, n + 1):
        xp, xm = np.minimum(cols + k, W - 1), np.maximum(cols - k, 0)
        tg = (c0[:, xp] + c0[:, xm]).astype(F64)
        b1 = b1 + tg * F64(g[k])
        b4 = b4 + tg * F64(xxg[k])
        b2 = b2 + ((c0[:, xp] - c0[:, xm]) * xg[k]).astype(F64)
        b3 = b3 + ((c1[:, xp] + c1[:, xm]) * g[k]).astype(F64)
        b6 = b6 + ((c1[:, xp] - c1[:, xm]) * xg[k]).astype(F64)
        b5 = b5 + ((c2[:, xp] + c2[:, xm]) * g[k]).astype(F64)
    R = np.empty((5, H, W), F32)
    R[0] = (b3 * ig11).astype(F32)
    R[1] = (b2 * ig11).astype(F32)
    R[2] = (b1 * ig03 + b5 * ig33).astype(F32)
    R[3] = (b1 * ig03 + b4 * ig33).astype(F32)
    R[4] = (b6 * ig55).astype(F32)
    return R


# ---------------------------------------------------------------------------- update matrices
def border_scale(H, W):
    def axis(n):
        i = np.arange(n)
        lo = np.where(i < 5, BORDER[np.minimum(i, 4)], F32(1)).astype(F32)
        hi = np.where(i >= n - 5, BORDER[np.clip(n - i - 1, 0, 4)], F32(1)).astype(F32)
        return lo, hi
    xl, xh = axis(W)
    yl, yh = axis(H)
    s = ((xl * xh)[None, :] * yl[:, None]) * yh[:, None]
    assert s.dtype == F32
    return s


def update_matrices(R0, R1, flow, counters=None):
    R0, R1, flow = np.asarray(R0, F32), np.asarray(R1, F32), np.asarray(flow, F32)
    _, H, W = R0.shape
    dx, dy = flow[0], flow[1]
    xs = np.arange(W, dtype=F32)[None, :]
    ys = np.arange(H, dtype=F32)[:, None]
    fx, fy = xs + dx, ys + dy
    x1, y1 = np.floor(fx), np.floor(fy)
    inside = (x1 >= 0) & (x1 < W - 1) & (y1 >= 0) & (y1 < H - 1)   # on the floats, before any int
    xi = np.where(inside, x1, 0).astype(np.int64)
    yi = np.where(inside, y1, 0).astype(np.int64)
    if W < 2 or H < 2:
        xi[:] = 0
        yi[:] = 0
    xj, yj = np.minimum(xi + 1, W - 1), np.minimum(yi + 1, H - 1)
    fx, fy = fx - x1, fy - y1
    a00, a01 = (F32(1) - fx) * (F32(1) - fy), fx * (F32(1) - fy)
    a10, a11 = (F32(1) - fx) * fy, fx * fy

    def sample(p):
        return ((a00 * p[yi, xi] + a01 * p[yi, xj]) + a10 * p[yj, xi]) + a11 * p[yj, xj]

    with np.errstate(invalid="ignore", over="ignore"):
        r2 = np.where(inside, sample(R1[0]), F32(0))
        r3 = np.where(inside, sample(R1[1]), F32(0))
        r4 = np.where(inside, (R0[2] + sample(R1[2])) * F32(0.5), R0[2])
        r5 = np.where(inside, (R0[3] + sample(R1[3])) * F32(0.5), R0[3])
        r6 = np.where(inside, (R0[4] + sample(R1[4])) * F32(0.25), R0[4] * F32(0.5))
    r2 = (R0[0] - r2) * F32(0.5)
    r3 = (R0[1] - r3) * F32(0.5)
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)
    xa, ya = np.arange(W)[None, :], np.arange(H)[:, None]
    edge = (xa < 5) | (xa >= W - 5) | (ya < 5) | (ya >= H - 5)
    s = border_scale(H, W)
    r2, r3, r4, r5, r6 = (np.where(edge, r * s, r) for r in (r2, r3, r4, r5, r6))
    M = np.empty((5, H, W), F32)
    M[0] = r4 * r4 + r6 * r6
    M[1] = (r4 + r5) * r6
    M[2] = r5 * r5 + r6 * r6
    M[3] = r4 * r2 + r6 * r3
    M[4] = r6 * r2 + r5 * r3
    if counters is not None:
        counters["inside"] = counters.get("inside", 0) + int(inside.sum())
        counters["outside"] = counters.get("outside", 0) + int((~inside).sum())
    return M


# ---------------------------------------------------------------------------- blur and solve
def box_sums(M, winsize):
    """float64 window sums: rows top to bottom into a column sum, then columns left to right."""
    M = np.asarray(M, F32)
    _, H, W = M.shape
    m = winsize // 2
    rows, cols = np.arange(H), np.arange(W)
    M64 = M.astype(F64)
    col = np.zeros(M.shape, F64)
    for d in range(-m, m + 1):
        col = col + M64[:, np.clip(rows + d, 0, H - 1), :]
    out = np.zeros(M.shape, F64)
    for d in range(-m, m + 1):
        out = out + col[:, :, np.clip(cols + d, 0, W - 1)]
    return out


def blur_solve(M, winsize):
    s = box_sums(M, winsize)
    scale = 1.0 / (winsize * winsize)
    g11, g12, g22, h1, h2 = (s[i] * scale for i in range(5))
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    flow = np.empty((2,) + s.shape[1:], F32)
    flow[0] = ((g11 * h2 - g12 * h1) * idet).astype(F32)
    flow[1] = ((g22 * h1 - g12 * h2) * idet).astype(F32)
    return flow


# ---------------------------------------------------------------------------- the whole flow
def farneback(prev, nxt, pyr_scale=0.5, nlevels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2,
              counters=None):
    prev, nxt = np.asarray(prev, np.uint8), np.asarray(nxt, np.uint8)
    H, W = prev.shape
    assert nxt.shape == (H, W)
    lv = levels(H, W, pyr_scale, nlevels)
    up = F32(1.0 / pyr_scale)
    flow = None
    for level in reversed(lv):
        h, w = level[:2]
        if flow is None:
            flow = np.zeros((2, h, w), F32)
        else:
            flow = np.stack([resize_f32(flow[0], h, w) * up, resize_f32(flow[1], h, w) * up])
        R0 = polyexp(pyramid_image(prev, level), poly_n, poly_sigma)
        R1 = polyexp(pyramid_image(nxt, level), poly_n, poly_sigma)
        M = update_matrices(R0, R1, flow, counters)
        for i in range(iterations):
            flow = blur_solve(M, winsize)
            if i < iterations - 1:
                M = update_matrices(R0, R1, flow, counters)
    return np.ascontiguousarray(flow.transpose(1, 2, 0))


# ---------------------------------------------------------------------------- residual depth
def expected_flow(Hm, H, W, counters=None):
    m = np.asarray(Hm, F64).reshape(9)
    x = np.arange(W, dtype=F32)[None, :].astype(F64)
    y = np.arange(H, dtype=F32)[:, None].astype(F64)
    w = (x * m[6] + y * m[7]) + m[8]
    ok = np.abs(w) > DBL_EPSILON
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(ok, 1.0 / w, 0.0)
    X = (((x * m[0] + y * m[1]) + m[2]) * w).astype(F32)
    Y = (((x * m[3] + y * m[4]) + m[5]) * w).astype(F32)
    e = np.empty((H, W, 2), F32)
    e[..., 0] = X - np.arange(W, dtype=F32)[None, :]
    e[..., 1] = Y - np.arange(H, dtype=F32)[:, None]
    if counters is not None:
        counters["w_zero"] = int((~np.broadcast_to(ok, (H, W))).sum())
    return e


def flow_depth(flow, Hm, stable=None, alpha=0.9, counters=None):
    """(depth, new stable or None, min(depth), max(depth))."""
    flow = np.asarray(flow, F32)
    H, W, _ = flow.shape
    r = flow - expected_flow(Hm, H, W, counters)
    rx, ry = r[..., 0].astype(F64), r[..., 1].astype(F64)
    mag = np.sqrt(rx * rx + ry * ry).astype(F32)
    depth = F32(1) / (mag + F32(0.5))
    assert depth.dtype == F32
    if stable is not None:
        stable = F32(alpha) * np.asarray(stable, F32) + F32(1.0 - float(alpha)) * depth
    return depth, stable, depth.min(), depth.max()


def bilateral(x, d=9, sigma_color=75, sigma_space=75):
    return FO.bilateral(x, d, sigma_color, sigma_space)
