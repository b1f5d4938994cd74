"""The host-buffer entry points give the same outputs whatever the caller's row stride.

engine._image() makes every array contiguous, so the Python API only ever passes
stride = W * channels; a padded stride reaches the library from C callers alone.  Here every
host entry point is called through engine.lib twice: with the image contiguous and with the
same pixels in rows of stride = row + 5 whose pad bytes are random.  Every output must be
identical.  The contiguous results are pinned to the oracles elsewhere (test_gpu_parity.py,
test_rectify.py, test_fusion.py, test_sgbm.py); this file adds only "stride does not matter".

The packed rows are what crosses the bus, so the context's copy counters must agree between
the two calls as well, except for the whole-frame path (sv_depth_map, sv_stereo_scaled_color),
which uploads strided rows in sub-chunks on purpose.
"""
import numpy as np
import pytest

from stereovision_amd.engine import COSTS, _check

pytestmark = pytest.mark.gpu

H, W, PAD = 24, 81, 5        # W odd and W % 4 != 0
D, WIN = 16, 5
SAD = COSTS["sad"]


def _rows(img):
    """An HxW or HxWx3 image as its (H, row bytes) matrix."""
    return np.ascontiguousarray(img).reshape(img.shape[0], -1)


def _embed(rows, rng):
    """The same rows inside a (H, row + PAD) buffer whose pad bytes are random."""
    buf = rng.integers(0, 256, (rows.shape[0], rows.shape[1] + PAD), dtype=np.uint8)
    buf[:, :rows.shape[1]] = rows
    return buf


def _check_stride(engine, images, call, counters=True):
    """call(buffers, stride) -> tuple of output arrays, contiguous then padded."""
    rng = np.random.default_rng(7)
    rows = [_rows(im) for im in images]
    row = rows[0].shape[1]
    engine.copy_counters(reset=True)
    ref = call(rows, row)
    c_ref = engine.copy_counters(reset=True)
    got = call([_embed(r, rng) for r in rows], row + PAD)
    c_got = engine.copy_counters(reset=True)
    assert len(ref) == len(got) and len(ref) > 0
    for a, b in zip(ref, got):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(a, b)
    if counters:
        assert c_ref["h2d_calls"] > 0 and c_ref["d2h_calls"] > 0
        assert c_got == c_ref
    return ref


def _image(h, w, channels, seed):
    """Smooth texture plus noise (matchable, every byte value in play)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 120 + 70 * np.sin(x * 0.45 + seed) * np.cos(y * 0.3) + rng.integers(-40, 41, (h, w))
    g = np.clip(base, 0, 255).astype(np.uint8)
    if channels == 1:
        return g
    return np.stack([g, np.roll(g, 1, 0), 255 - g], axis=2)


def _pair(channels):
    wide = _image(H, W + 4, channels, 3)
    return np.ascontiguousarray(wide[:, :W]), np.ascontiguousarray(wide[:, 4:])   # disparity 4


@pytest.fixture(scope="module")
def maps(engine):
    """CV_16SC2 maps of a 24 x 81 output over a 20 x 33 source, mildly distorted."""
    K = np.array([[30.0, 0, 16.0], [0, 30.0, 10.0], [0, 0, 1]])
    P = np.array([[75.0, 0, 40.0], [0, 36.0, 12.0], [0, 0, 1]])
    m1, m2 = engine.init_undistort_rectify_map(K, [-0.05, 0.01, 0.001, 0.001, 0.0], None, P, W, H)
    assert m2.any()
    return m1, m2


def test_gray(engine):
    def call(b, stride):
        out = np.zeros((H, W), np.uint8)
        _check("sv_gray", engine.lib.sv_gray(engine.handle, b[0], H, W, stride, out))
        return (out,)
    _check_stride(engine, [_image(H, W, 3, 1)], call)


@pytest.mark.parametrize("harris", [False, True])
@pytest.mark.parametrize("channels", [1, 3])
def test_disparity(engine, channels, harris):
    def call(b, stride):
        d16 = np.zeros((H, W), np.int16)
        hr = np.zeros((H, W), np.float32) if harris else None
        _check("sv_disparity", engine.lib.sv_disparity(engine.handle, b[0], b[1], H, W, channels, stride, 0, D, WIN,
                                                       SAD, d16, hr))
        return (d16, hr) if harris else (d16,)
    ref = _check_stride(engine, _pair(channels), call)
    assert (ref[0][:, D + 2:] == 4 * 16).mean() > 0.5       # the map is a real one


@pytest.mark.parametrize("channels", [1, 3])
def test_disparity_rows(engine, channels):
    def call(b, stride):
        d16 = np.full((H, W), -7, np.int16)
        _check("sv_disparity_rows", engine.lib.sv_disparity_rows(engine.handle, b[0], b[1], H, W, channels, stride,
                                                                 0, D, WIN, SAD, 5, 17, d16))
        return (d16,)
    ref = _check_stride(engine, _pair(channels), call)
    assert (ref[0][:5] == -7).all() and (ref[0][17:] == -7).all() and (ref[0][5:17] != -7).all()


def test_harris(engine):
    def call(b, stride):
        out = np.zeros((H, W), np.float32)
        _check("sv_harris", engine.lib.sv_harris(engine.handle, b[0], H, W, stride, out))
        return (out,)
    _check_stride(engine, [_image(H, W, 1, 2)], call)


def test_hog_hist(engine):
    def call(b, stride):
        out = np.zeros((H, W, 10), np.uint16)
        _check("sv_hog_hist", engine.lib.sv_hog_hist(engine.handle, b[0], H, W, stride, WIN, out))
        return (out[:, :, :9].copy(),)
    _check_stride(engine, [_image(H, W, 1, 4)], call)


@pytest.mark.parametrize("channels", [1, 3])
def test_remap(engine, maps, channels):
    m1, m2 = maps

    def call(b, stride):
        out = np.zeros((H, W * channels), np.uint8)
        _check("sv_remap", engine.lib.sv_remap(engine.handle, b[0], 20, 33, channels, stride, m1, m2, H, W, out))
        return (out,)
    ref = _check_stride(engine, [_image(20, 33, channels, 5)], call)
    assert ref[0].any()


@pytest.mark.parametrize("channels", [1, 3])
def test_rectify_pair(engine, maps, channels):
    m1, m2 = maps
    d = [engine.upload("stride_m1l", m1), engine.upload("stride_m2l", m2),
         engine.upload("stride_m1r", m1[:, ::-1].copy()), engine.upload("stride_m2r", m2[:, ::-1].copy())]

    def call(b, stride):
        ol = np.zeros((H, W * channels), np.uint8)
        orr = np.zeros((H, W * channels), np.uint8)
        _check("sv_rectify_pair", engine.lib.sv_rectify_pair(engine.handle, d[0], d[1], d[2], d[3], H, W, b[0], b[1],
                                                             20, 33, channels, stride, ol, orr))
        return ol, orr
    ref = _check_stride(engine, [_image(20, 33, channels, 6), _image(20, 33, channels, 7)], call)
    assert ref[0].any() and ref[1].any()


@pytest.mark.parametrize("channels", [1, 3])
def test_resize_linear(engine, channels):
    def call(b, stride):
        out = np.zeros((H, W * channels), np.uint8)
        _check("sv_resize_linear", engine.lib.sv_resize_linear(engine.handle, b[0], 20, 33, channels, stride, out,
                                                               H, W))
        return (out,)
    _check_stride(engine, [_image(20, 33, channels, 8)], call)


@pytest.mark.parametrize("nimg", [1, 2])
@pytest.mark.parametrize("channels", [1, 3])
def test_frame_stats(engine, channels, nimg):
    h, w = 50, 97                 # one block row, two block columns
    bh, bw = 1, 2

    def call(b, stride):
        bs = np.zeros((nimg, bh, bw), np.uint32)
        bq = np.zeros((nimg, bh, bw), np.uint32)
        hist = np.zeros((nimg, 256), np.uint32)
        _check("sv_frame_stats", engine.lib.sv_frame_stats(engine.handle, b[0], b[1].ctypes.data if nimg == 2 else None,
                                                           h, w, channels, stride, bs, bq, hist))
        return bs, bq, hist
    ref = _check_stride(engine, [_image(h, w, channels, 9 + k) for k in range(nimg)], call)
    assert ref[0].all() and ref[2].any(axis=1).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_sgbm(engine, channels):
    def call(b, stride):
        d16 = np.zeros((H, W), np.int16)
        _check("sv_sgbm", engine.lib.sv_sgbm(engine.handle, b[0], b[1], H, W, channels, stride, 0, D, WIN,
                                             8 * 3 * WIN * WIN, 32 * 3 * WIN * WIN, 1, 63, 10, 0, 32, d16))
        return (d16,)
    _check_stride(engine, _pair(channels), call)


@pytest.mark.parametrize("channels", [1, 3])
def test_depth_map(engine, channels):
    def call(b, stride):
        depth = np.zeros((H, W), np.float32)
        disp = np.zeros((H, W), np.float32)
        norm = np.zeros((H, W), np.uint8)
        _check("sv_depth_map", engine.lib.sv_depth_map(engine.handle, b[0], b[1], H, W, channels, stride, 0, D, WIN,
                                                       SAD, np.float32(0.5), np.float32(10.0), np.float32(9.5),
                                                       np.float32(0.0), depth, disp, norm))
        return depth, disp, norm
    ref = _check_stride(engine, _pair(channels), call, counters=False)
    assert (ref[1][:, D + 2:] == 4.0).mean() > 0.5


@pytest.mark.parametrize("channels", [1, 3])
def test_stereo_scaled_color(engine, channels):
    lut = np.random.default_rng(11).integers(0, 256, (256, 3), dtype=np.uint8)

    def call(b, stride):
        dn = np.zeros((H, W), np.float32)
        disp = np.zeros((H, W), np.float32)
        du = np.zeros((H, W), np.uint8)
        cf = np.zeros((H, W), np.float32)
        cmap = np.zeros((H, W, 3), np.uint8)
        _check("sv_stereo_scaled_color", engine.lib.sv_stereo_scaled_color(
            engine.handle, b[0], b[1], H, W, channels, stride, 0, D, WIN, SAD, lut, dn, disp, du, cf, cmap))
        return dn, disp, du, cf, cmap
    ref = _check_stride(engine, _pair(channels), call, counters=False)
    assert ref[4].any()
