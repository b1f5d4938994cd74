"""GPU checks of sv_cloud.hip: the dense reprojection and the ordered point cloud,
bit-exact against tests/sv_cloud_oracle.py at the seams of the kernels (row ends, pitched rows,
tile, wave and block boundaries, the capacity), the argument rules, and the frame pipeline."""
import ctypes
import functools
import os
import pickle
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_chain as C  # noqa: E402
import sv_cloud_oracle as CO  # noqa: E402
from stereovision_amd import cloud  # noqa: E402
from stereovision_amd import engine as E  # noqa: E402
from stereovision_amd import flow as F  # noqa: E402
from stereovision_amd import fused_depth_map as FDM  # noqa: E402
from stereovision_amd import synthetic  # noqa: E402
from stereovision_amd.frame import OUTPUT_NAMES, FusionFramePipeline  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 1024                       # kCloudTile: pixels per compaction block
GUARD = 64                        # sentinel elements behind every output
# (1, 1); odd; W % 4 = 3 over several tiles; exactly one tile; a tile and one pixel; the app size
SHAPES = [(1, 1), (5, 3), (37, 131), (32, 32), (25, 41), (356, 633)]
FORMATS = [np.int16, np.float32]
# every entry non-zero and non-dyadic; h_3 changes sign inside the disparity range
Q_GENERAL = np.array([[1.013, 0.0171, -0.0093, -301.7], [-0.0127, 0.9871, 0.0113, -177.3],
                      [0.0031, -0.0047, 0.0197, 533.9], [0.00011, -0.00007, 12.37, -191.3]])
# a rectified pair's Q: f = 443.1, Tx = -0.08
Q_STEREO = np.array([[1, 0, 0, -316.9], [0, 1, 0, -178.2], [0, 0, 0, 443.1], [0, 0, 12.5, 0.0]])


def _same_bits(got, exp):
    """array_equal with NaNs equal, and the signs of the zeros as well."""
    assert got.dtype == exp.dtype and got.shape == exp.shape
    assert np.array_equal(got, exp, equal_nan=True)
    ok = ~np.isnan(exp)
    assert np.array_equal(np.signbit(got[ok]), np.signbit(exp[ok]))


def _random_map(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(-2047 * 16, 2047 * 16 + 1, shape).astype(np.int16)
    if dtype == np.int16:
        return m
    return (m.astype(np.float32) / np.float32(16)) + rng.random(shape, dtype=np.float32) * np.float32(0.01)


def _pitched(a, pitch, fill):
    """`a` in rows of `pitch` elements, the padding (and a tail) holding `fill`."""
    H, W = a.shape[:2]
    flat = a.reshape(H, -1)
    out = np.full((H + 1, pitch), fill, a.dtype)
    out[:H, :flat.shape[1]] = flat
    return out


class Out:
    """A device output of n elements with GUARD sentinels behind it."""

    def __init__(self, eng, name, n, dtype, fill):
        self.eng, self.n, self.dtype = eng, n, np.dtype(dtype)
        self.fill = np.full(n + GUARD, fill, dtype)
        self.ptr = eng.upload("tcg_" + name, self.fill)

    def read(self):
        return self.eng.to_host(self.ptr, (self.n + GUARD,), self.dtype)

    def untouched_from(self, k):
        return np.array_equal(self.read()[k:].view(np.uint8), self.fill[k:].view(np.uint8))


def _dense_dev(eng, disp, Q, handle_missing, pitch=None):
    H, W = disp.shape
    pitch = W if pitch is None else pitch
    fill = np.int16(-32768) if disp.dtype == np.int16 else np.float32(-np.inf)    # a sentinel below every value
    d = eng.upload("tcg_disp", _pitched(disp, pitch, fill))
    out = Out(eng, "dense", H * W * 3, np.float32, np.float32(-7.25))
    eng.reproject_3d_dev(d, "i16x16" if disp.dtype == np.int16 else "f32", H, W, pitch, Q, handle_missing, out.ptr)
    eng.synchronize()
    assert out.untouched_from(H * W * 3)
    return out.read()[:H * W * 3].reshape(H, W, 3)


def _cloud_dev(eng, disp, Q, colors=None, *, cap=None, pitch=None, bgr_pitch=None, want_bgr=True, want_index=True,
               wait=True, **kw):
    """sv_point_cloud_dev with guarded outputs -> (xyz, bgr, index, N), each cut to min(N, cap)."""
    H, W = disp.shape
    pitch = W if pitch is None else pitch
    cap = H * W if cap is None else cap
    fill = np.int16(32767) if disp.dtype == np.int16 else np.float32(np.inf)      # would be valid if it were read
    d = eng.upload("tcg_disp", _pitched(disp, pitch, fill))
    d_col, bp = 0, 0
    if colors is not None:
        bp = 3 * W if bgr_pitch is None else bgr_pitch
        d_col = eng.upload("tcg_col", _pitched(colors, bp, np.uint8(0xEE)))
    o_xyz = Out(eng, "xyz", 3 * cap, np.float32, np.float32(-7.25))
    o_bgr = Out(eng, "bgr", 3 * cap, np.uint8, 0xA5) if (want_bgr and colors is not None) else None
    o_idx = Out(eng, "idx", cap, np.uint32, 0xDEADBEEF) if want_index else None
    o_cnt = Out(eng, "cnt", 1, np.uint32, 0xDEADBEEF)
    p = E.cloud_params(kw.get("min_valid", 0.0), (kw.get("z_min", -np.inf), kw.get("z_max", np.inf)), kw.get("roi"),
                       kw.get("handle_missing", False))
    n = eng.point_cloud_dev(d, "i16x16" if disp.dtype == np.int16 else "f32", H, W, pitch, Q, p, cap, o_xyz.ptr,
                            d_col, bp, o_bgr.ptr if o_bgr else 0, o_idx.ptr if o_idx else 0, o_cnt.ptr, wait=wait)
    eng.synchronize()
    cnt = o_cnt.read()
    assert cnt[1:].tolist() == [0xDEADBEEF] * GUARD
    if wait:
        assert n == cnt[0]
    else:
        assert n is None
        n = int(cnt[0])
    k = min(n, cap)
    assert o_xyz.untouched_from(3 * k)                                            # the sentinel at cap, and all behind it
    assert o_bgr is None or o_bgr.untouched_from(3 * k)
    assert o_idx is None or o_idx.untouched_from(k)
    return (o_xyz.read()[:3 * k].reshape(k, 3), o_bgr.read()[:3 * k].reshape(k, 3) if o_bgr else None,
            o_idx.read()[:k] if o_idx else None, n)


def _check_cloud(got, exp, with_bgr=True, with_index=True):
    assert got[3] == exp[3]
    assert np.array_equal(got[0], exp[0])
    assert (got[1] is None) == (not with_bgr) and (got[2] is None) == (not with_index)
    if with_bgr:
        assert np.array_equal(got[1], exp[1])
    if with_index:
        assert np.array_equal(got[2], exp[2])


# ------------------------------------------------------------------------------ the dense map
@pytest.mark.parametrize("handle_missing", [False, True], ids=["plain", "missing"])
@pytest.mark.parametrize("dtype", FORMATS, ids=["i16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dense_general_q(engine, shape, dtype, handle_missing):
    disp = _random_map(shape, dtype, seed=shape[0] + shape[1])
    if handle_missing and disp.size > 4:          # the minimum at several pixels
        flat = disp.reshape(-1)
        flat[[0, disp.size // 2, disp.size - 1]] = disp.min()
    _same_bits(_dense_dev(engine, disp, Q_GENERAL, handle_missing), CO.reproject_image_to_3d(disp, Q_GENERAL, handle_missing))


@pytest.mark.parametrize("dtype", FORMATS, ids=["i16", "f32"])
@pytest.mark.parametrize("pitch", [132, 137, 200])
def test_dense_pitched_rows(engine, dtype, pitch):
    """pitch > W, aligned for the wide loads (132) and not (137, 200 with W % 4 = 3); the padding holds a
    value below the map's minimum, which handle_missing must not see."""
    disp = _random_map((37, 131), dtype, seed=pitch)
    for hm in (False, True):
        _same_bits(_dense_dev(engine, disp, Q_GENERAL, hm, pitch=pitch), CO.reproject_image_to_3d(disp, Q_GENERAL, hm))


def test_dense_special_values_and_signed_zeros(engine):
    d = np.full((9, 70), 2.0, np.float32)
    d[0, 0], d[1, 1], d[2, 2], d[3, 3], d[4, :] = np.nan, np.inf, -np.inf, 1.0, 0.0
    Qd = np.array([[1, 0, 0, -64], [0, 1, 0, -32], [0, 0, 0, 512], [0, 0, 0.125, 0]], np.float64)
    for hm in (False, True):
        _same_bits(_dense_dev(engine, d, Qd, hm), CO.reproject_image_to_3d(d, Qd, hm))
    d[2, 2] = 2.0                                                                 # the minimum is now 0.0, a row of it
    _same_bits(_dense_dev(engine, d, Qd, True), CO.reproject_image_to_3d(d, Qd, True))
    nan = np.full((3, 5), np.nan, np.float32)                                     # nothing left for the minimum
    _same_bits(_dense_dev(engine, nan, Qd, True), CO.reproject_image_to_3d(nan, Qd, True))
    Qz = np.zeros((4, 4))                                                         # every term of row 0 is -0.0 at (0, 0)
    Qz[0] = -1.0, -1.0, -1.0, -0.0
    Qz[1, 3], Qz[2, 3], Qz[3, 3] = 1.0, 1.0, 1.0
    z = np.zeros((2, 6), np.float32)
    _same_bits(_dense_dev(engine, z, Qz, False), CO.reproject_image_to_3d(z, Qz, False))
    # the order of the sum and the narrowing of h, as tests/test_cloud_cpu.py states them
    Qo = np.zeros((4, 4))
    Qo[0, :3] = 2.0 ** 60, -2.0 ** 60, 1.0
    Qo[1, :3] = 0.1, 0.2, 0.3
    Qo[2, 3], Qo[3, 3] = 1.0 + 2.0 ** -24 - 2.0 ** -30, 0.8
    o = np.ones((4, 7), np.float32)
    _same_bits(_dense_dev(engine, o, Qo, False), CO.reproject_image_to_3d(o, Qo, False))


def test_host_forms(engine):
    disp = _random_map((37, 131), np.int16, seed=5)
    col = np.random.default_rng(5).integers(0, 256, (37, 131, 3), dtype=np.uint8)
    _same_bits(cloud.reproject_image_to_3d(disp, Q_GENERAL, True, engine=engine),
               CO.reproject_image_to_3d(disp, Q_GENERAL, True))
    f = np.abs(disp).astype(np.float32) / np.float32(16)
    exp = CO.point_cloud(f, Q_STEREO, col, min_valid=20.0, z_min=0.1, z_max=3.0, roi=(3, 2, 120, 30))
    xyz, bgr, idx = cloud.point_cloud(f, Q_STEREO, col, min_disp=20, z_range=(0.1, 3.0), roi=(3, 2, 120, 30),
                                      with_index=True, engine=engine)
    _check_cloud((xyz, bgr, idx, len(xyz)), exp)
    assert 100 < exp[3] < f.size
    xyz, none = cloud.point_cloud(f, Q_STEREO, min_disp=20, capacity=7, engine=engine)
    assert none is None and np.array_equal(xyz, CO.point_cloud(f, Q_STEREO, min_valid=20.0)[0][:7])
    xyz, bgr = cloud.point_cloud(f, Q_STEREO, col, min_disp=5000, engine=engine)  # N = 0
    assert xyz.shape == (0, 3) and bgr.shape == (0, 3)
    xyz, bgr = cloud.point_cloud(f, Q_STEREO, col, min_disp=20, capacity=0, engine=engine)
    assert xyz.shape == (0, 3) and bgr.shape == (0, 3)


# ------------------------------------------------------------------------------ the cloud
def _valid_pattern(name, n, rng):
    v = np.zeros(n, bool)
    if name == "all":
        v[:] = True
    elif name == "last":
        v[-1] = True
    elif name == "first":
        v[0] = True
    elif name == "alternating":
        v[::2] = True
    elif name == "runs":          # across a wave boundary, a sub-tile boundary and a block boundary
        for a in (60, 250, TILE - 4, 2 * TILE - 1, 3 * TILE - 70):
            v[a:a + 10] = True
    elif name == "random":
        v[:] = rng.random(n) < 0.5
    return v                      # "none": nothing


PATTERNS = ["all", "none", "last", "first", "alternating", "runs", "random"]


def _patterned(shape, dtype, pattern, seed=11):
    """Disparities in [1, 120] where the pattern is set, the (min_disp - 1) marker elsewhere."""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    m = rng.integers(16, 120 * 16, n).astype(np.int16)
    v = _valid_pattern(pattern, n, rng)
    m[~v] = -16
    m = m.reshape(shape)
    col = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    return (m if dtype == np.int16 else m.astype(np.float32) / np.float32(16)), col, int(v.sum())


@pytest.mark.parametrize("dtype", FORMATS, ids=["i16", "f32"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_cloud_validity_patterns(engine, pattern, dtype):
    disp, col, nvalid = _patterned((37, 131), dtype, pattern)
    exp = CO.point_cloud(disp, Q_STEREO, col)
    assert exp[3] == nvalid
    _check_cloud(_cloud_dev(engine, disp, Q_STEREO, col), exp)


@pytest.mark.parametrize("handle_missing", [False, True], ids=["plain", "missing"])
@pytest.mark.parametrize("dtype", FORMATS, ids=["i16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cloud_shapes(engine, shape, dtype, handle_missing):
    disp, col, _ = _patterned(shape, dtype, "random", seed=shape[1])
    kw = dict(min_valid=-1.0 if handle_missing else 0.0, handle_missing=handle_missing)
    exp = CO.point_cloud(disp, Q_STEREO, col, **kw)
    _check_cloud(_cloud_dev(engine, disp, Q_STEREO, col, **kw), exp)
    # a general Q on a full-range map: the finite test and the z range do the cutting
    disp = _random_map(shape, dtype, seed=shape[0])
    kw = dict(min_valid=-1500.0, z_min=-0.04, z_max=0.05, handle_missing=handle_missing)
    exp = CO.point_cloud(disp, Q_GENERAL, col, **kw)
    _check_cloud(_cloud_dev(engine, disp, Q_GENERAL, col, **kw), exp)


@pytest.mark.parametrize("dtype", FORMATS, ids=["i16", "f32"])
def test_cloud_pitched_inputs(engine, dtype):
    """pitch > W for the map and the colours; the map's padding holds values that would be valid."""
    disp, col, _ = _patterned((37, 131), dtype, "random")
    for hm in (False, True):
        kw = dict(min_valid=-1.0, handle_missing=hm)
        exp = CO.point_cloud(disp, Q_STEREO, col, **kw)
        _check_cloud(_cloud_dev(engine, disp, Q_STEREO, col, pitch=150, bgr_pitch=3 * 131 + 17, **kw), exp)


def test_cloud_clauses(engine):
    disp, col, _ = _patterned((37, 131), np.float32, "random")
    disp[5, :] = 0.0                                                              # h_3 = 0: inf and NaN
    disp[6, 7] = np.nan
    Z = CO.reproject_image_to_3d(disp, Q_STEREO)[..., 2]
    some = np.sort(Z[np.isfinite(Z) & (Z > 0)])
    z_lo, z_hi = float(some[len(some) // 4]), float(some[3 * len(some) // 4])     # both ends are values of the map
    cases = [dict(min_valid=-5.0), dict(min_valid=30.0), dict(min_valid=-5.0, z_min=z_lo, z_max=z_hi),
             dict(min_valid=-5.0, roi=(17, 9, 50, 11)), dict(min_valid=-5.0, roi=(130, 36, 1, 1)),
             dict(min_valid=-5.0, roi=(0, 0, 131, 37)), dict(min_valid=-5.0, handle_missing=True),
             dict(min_valid=10.0, z_min=z_lo, z_max=z_hi, roi=(17, 9, 100, 25), handle_missing=True)]
    for kw in cases:
        exp = CO.point_cloud(disp, Q_STEREO, col, **kw)
        _check_cloud(_cloud_dev(engine, disp, Q_STEREO, col, **kw), exp)
    exp = CO.point_cloud(disp, Q_STEREO, col, min_valid=-5.0, z_min=z_lo, z_max=z_hi)
    assert exp[0][:, 2].min() == np.float32(z_lo) and exp[0][:, 2].max() == np.float32(z_hi)   # the ends are kept


@pytest.mark.parametrize("dtype", FORMATS, ids=["i16", "f32"])
def test_cloud_capacity(engine, dtype):
    disp, col, n = _patterned((37, 131), dtype, "random")
    full = CO.point_cloud(disp, Q_STEREO, col)
    # below N inside the first tile, at a tile's offset, one short of N, N, beyond N, nothing
    first = CO.point_cloud(disp.reshape(-1)[:TILE].reshape(1, TILE), Q_STEREO)[3]
    for cap in (0, 1, 100, first, first + 1, n - 1, n, n + 50):
        exp = tuple(a[:cap] for a in full[:3]) + (n,)
        _check_cloud(_cloud_dev(engine, disp, Q_STEREO, col, cap=cap), exp)


@pytest.mark.parametrize("want_bgr,want_index", [(True, True), (True, False), (False, True), (False, False)])
def test_cloud_optional_outputs(engine, want_bgr, want_index):
    disp, col, _ = _patterned((25, 41), np.int16, "random")
    exp = CO.point_cloud(disp, Q_STEREO, col)
    _check_cloud(_cloud_dev(engine, disp, Q_STEREO, col, want_bgr=want_bgr, want_index=want_index), exp,
                 want_bgr, want_index)
    if not want_bgr:      # no colour image at all
        _check_cloud(_cloud_dev(engine, disp, Q_STEREO, None, want_index=want_index), exp, False, want_index)


def test_cloud_count_without_waiting(engine):
    disp, col, n = _patterned((37, 131), np.int16, "random")
    got = _cloud_dev(engine, disp, Q_STEREO, col, wait=False)                     # N from d_count after a synchronise
    _check_cloud(got, CO.point_cloud(disp, Q_STEREO, col))
    assert got[3] == n
    before = engine.copy_counters(reset=True)
    assert before is not None
    _cloud_dev(engine, disp, Q_STEREO, col, wait=True)
    # (the helper's own uploads and read-backs are counted too; the call's share is one 4-byte read)
    with_wait = engine.copy_counters(reset=True)
    _cloud_dev(engine, disp, Q_STEREO, col, wait=False)
    without = engine.copy_counters(reset=True)
    assert with_wait["d2h_calls"] - without["d2h_calls"] == 1 and with_wait["d2h_bytes"] - without["d2h_bytes"] == 4
    assert with_wait["h2d_bytes"] == without["h2d_bytes"]


# ------------------------------------------------------------------------------ SV_EINVAL
def test_einval_leaves_the_outputs_untouched(engine):
    H, W = 12, 20
    disp = np.full((H, W), 64, np.int16)
    d = engine.upload("tcg_disp", disp)
    d_col = engine.upload("tcg_col", np.zeros((H, W, 3), np.uint8))
    outs = [Out(engine, "xyz", 3 * H * W, np.float32, np.float32(-7.25)), Out(engine, "bgr", 3 * H * W, np.uint8, 0xA5),
            Out(engine, "idx", H * W, np.uint32, 0xDEADBEEF), Out(engine, "cnt", 1, np.uint32, 0xDEADBEEF)]
    o_xyz, o_bgr, o_idx, o_cnt = outs
    good = dict(d=d, fmt=0, H=H, W=W, pitch=W, Q=Q_STEREO, bgr=d_col, bp=3 * W, p=E.cloud_params(), cap=H * W,
                xyz=o_xyz.ptr, obgr=o_bgr.ptr)
    P = E._CloudParams
    inf = np.inf

    def cloud_call(**kw):
        a = dict(good, **kw)
        engine.point_cloud_dev(a["d"], a["fmt"], a["H"], a["W"], a["pitch"], a["Q"], a["p"], a["cap"], a["xyz"],
                               a["bgr"], a["bp"], a["obgr"], o_idx.ptr, o_cnt.ptr)

    def dense_call(**kw):
        a = dict(good, **kw)
        engine.reproject_3d_dev(a["d"], a["fmt"], a["H"], a["W"], a["pitch"], a["Q"], True, a["xyz"])

    nanq, infq = Q_STEREO.copy(), Q_STEREO.copy()
    nanq[1, 2], infq[3, 3] = np.nan, -np.inf
    shared = [dict(d=0), dict(xyz=0), dict(fmt=2), dict(fmt=-1), dict(pitch=W - 1), dict(H=0), dict(W=0), dict(H=-3),
              dict(H=1 << 16, W=1 << 15, pitch=1 << 15), dict(Q=nanq), dict(Q=infq)]
    only_cloud = [dict(bp=3 * W - 1), dict(cap=-1), dict(bgr=0), dict(p=P(np.nan, -inf, inf, 0, 0, 0, 0, 0)),
                  dict(p=P(0, np.nan, inf, 0, 0, 0, 0, 0)), dict(p=P(0, -inf, np.nan, 0, 0, 0, 0, 0)),
                  dict(p=P(0, 2.0, 1.0, 0, 0, 0, 0, 0)), dict(p=P(0, -inf, inf, -1, 0, 5, 5, 0)),
                  dict(p=P(0, -inf, inf, 0, -1, 5, 5, 0)), dict(p=P(0, -inf, inf, 16, 0, 5, 5, 0)),
                  dict(p=P(0, -inf, inf, 0, 8, 5, 5, 0)), dict(p=P(0, -inf, inf, 0, 0, -2, 5, 0)),
                  dict(p=P(0, -inf, inf, 0, 0, 5, -2, 0)), dict(p=P(0, -inf, inf, 20, 12, 1, 1, 0))]
    for call, cases in ((cloud_call, shared + only_cloud), (dense_call, shared)):
        for kw in cases:
            with pytest.raises(E.SVError) as ei:
                call(**kw)
            assert ei.value.code == -22, kw
    # null Q and null parameters: through a binding without argument types
    raw = ctypes.CDLL(E.LIB_PATH)
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    q = np.ascontiguousarray(Q_STEREO)
    p = E.cloud_params()

    def raw_cloud(qp, pp):
        return raw.sv_point_cloud_dev(vp(engine.handle.value), vp(d), ci(0), ci(H), ci(W), ci(W), qp, vp(d_col), ci(3 * W),
                                      pp, i64(H * W), vp(o_xyz.ptr), vp(o_bgr.ptr), vp(o_idx.ptr), vp(o_cnt.ptr), vp(None),
                                      vp(None))

    assert raw_cloud(vp(None), ctypes.byref(p)) == -22
    assert raw_cloud(vp(q.ctypes.data), vp(None)) == -22
    assert raw.sv_reproject_3d_dev(vp(engine.handle.value), vp(d), ci(0), ci(H), ci(W), ci(W), vp(None), ci(0),
                                   vp(o_xyz.ptr), vp(None)) == -22
    engine.synchronize()
    assert all(o.untouched_from(0) for o in outs)
    cloud_call()                                                                  # and the arguments they vary are good
    assert raw_cloud(vp(q.ctypes.data), ctypes.byref(p)) == 0
    engine.synchronize()
    assert o_cnt.read()[0] == H * W


# ------------------------------------------------------------------------------ the frame pipeline
PH, PW = 88, 120
CH, CW = 176, 240
STEREO = dict(min_disp=0, num_disp=32, window_size=5)


@pytest.fixture
def clock(monkeypatch):
    now = [1000.0]
    monkeypatch.setattr(F.time, "time", lambda: now[0])
    return now


@functools.lru_cache(maxsize=None)
def _calibration(width, height, scale, seed=0):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "stereo_calibration_data.pkl")
        with open(p, "wb") as f:
            pickle.dump(synthetic.synthetic_calibration(width, height, seed), f)
        c = FDM.load_stereo_calibration_with_scaling(scale, p)
    assert c is not None and c["Q"].shape == (4, 4)
    return c


def _cloud_of(res, calib, engine, **kw):
    return cloud.point_cloud(res.stereo_disparity, calib["Q"], colors=res.processed_left,
                             min_disp=STEREO["min_disp"], engine=engine, **kw)


@pytest.mark.parametrize("refine", [None, E.RefineParams(1, 1, True)], ids=["plain", "refined"])
def test_pipeline_cloud_equals_the_host_call(engine, clock, refine):
    calib = _calibration(CW, CH, 0.5)
    frames = C.moving_stereo_sequence(CH, CW, 3, disparity=8)
    params = cloud.CloudParams(z_range=(0.05, 40.0), with_index=True)
    pipe = FusionFramePipeline(calib, engine=engine, outputs=("stereo_disparity", "processed_left", "fused_u8"),
                               cloud=params, refine=refine, **STEREO)
    sizes = []
    for fl, fr in frames:
        clock[0] += 0.1
        res = pipe.step(fl, fr)
        assert res.use_stereo and res.cloud is not None and len(res.cloud) == 3
        exp = _cloud_of(res, calib, engine, z_range=(0.05, 40.0), with_index=True)
        for g, e in zip(res.cloud, exp):
            assert g.dtype == e.dtype and np.array_equal(g, e)
        oracle = CO.point_cloud(res.stereo_disparity, calib["Q"], res.processed_left, min_valid=0.0, z_min=0.05, z_max=40.0)
        assert np.array_equal(res.cloud[0], oracle[0]) and np.array_equal(res.cloud[2], oracle[2])
        sizes.append(len(res.cloud[0]))
        if refine is not None:    # the pixels the refinement marked are not in the cloud
            marked = np.flatnonzero(res.stereo_disparity.ravel() < 0)
            assert marked.size > 0 and not np.isin(marked, res.cloud[2]).any()
    assert min(sizes) > 100
    pipe.close()


def test_pipeline_cloud_is_none_without_stereo_or_q(engine, clock):
    calib = _calibration(CW, CH, 0.5)
    frames = C.moving_stereo_sequence(CH, CW, 12, disparity=8)
    flat = np.full((CH, CW, 3), 117, np.uint8)
    pipe = FusionFramePipeline(calib, engine=engine, outputs=("stereo_disparity", "processed_left"),
                               cloud=cloud.CloudParams(), **STEREO)
    pipe.use_flow = False
    got = []
    for _, fr in frames:                                  # the left camera covered: stereo off from frame 8
        clock[0] += 0.1
        got.append(pipe.step(flat, fr))
    assert [r.use_stereo for r in got] == [True] * 8 + [False] * 4
    assert all((r.cloud is not None) == r.use_stereo for r in got)
    pipe.close()
    no_q = {k: v for k, v in calib.items() if k != "Q"}
    pipe = FusionFramePipeline(no_q, engine=engine, outputs=("stereo_disparity",), cloud=cloud.CloudParams(), **STEREO)
    clock[0] += 0.1
    r = pipe.step(*frames[0])
    assert r.use_stereo and r.stereo_disparity is not None and r.cloud is None
    pipe.close()


def test_pipeline_without_cloud_is_unchanged(engine, clock):
    """cloud=None: the outputs equal the host chain's as before, and the step moves what it moved:
    the same step with a cloud adds exactly the 4-byte count and the cloud's arrays."""
    calib = _calibration(CW, CH, 0.5)
    frames = C.moving_stereo_sequence(CH, CW, 3, disparity=8)
    pipes = [FusionFramePipeline(calib, engine=engine, outputs=OUTPUT_NAMES, cloud=c, **STEREO)
             for c in (None, cloud.CloudParams())]
    chain = C.HostChain(calib, **STEREO)
    for k, (fl, fr) in enumerate(frames):
        clock[0] += 0.1
        ctr, res = [], []
        for pipe in pipes:
            engine.copy_counters(reset=True)
            res.append(pipe.step(fl, fr))
            ctr.append(engine.copy_counters(reset=True))
        exp = chain.step(fl, fr)
        for r in res:
            for name in OUTPUT_NAMES:
                assert (getattr(r, name) is None) == (exp[name] is None), name
                if exp[name] is not None:
                    np.testing.assert_array_equal(getattr(r, name), exp[name], err_msg=name)
        assert res[0].cloud is None and res[1].cloud is not None
        n = len(res[1].cloud[0])
        if k == 0:        # the first step of the first pipeline also uploads what both share (maps, tables)
            continue
        assert ctr[1]["h2d_bytes"] == ctr[0]["h2d_bytes"] and ctr[1]["h2d_calls"] == ctr[0]["h2d_calls"]
        assert ctr[1]["d2h_bytes"] - ctr[0]["d2h_bytes"] == 4 + 15 * n
        assert ctr[1]["d2h_calls"] - ctr[0]["d2h_calls"] == 3
    for pipe in pipes:
        pipe.close()
