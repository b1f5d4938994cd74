"""CPU checks of the 3D reprojection and the point cloud: the NumPy contract
(tests/sv_cloud_oracle.py) against closed forms, the project's own calibration and a per-pixel
loop; write_ply; the Python argument checks, which need no engine."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sv_cloud_oracle as CO  # noqa: E402
from stereovision_amd import calib, cloud, synthetic  # noqa: E402
from stereovision_amd.frame import OUTPUT_NAMES, FrameResult, FusionFramePipeline  # noqa: E402

F32 = np.float32
# f = 512, cx = 64, cy = 32, q32 = 1/8, q33 = 0: every entry a power of two
Q_DYADIC = np.array([[1, 0, 0, -64], [0, 1, 0, -32], [0, 0, 0, 512], [0, 0, 0.125, 0]], np.float64)


def _q_only_constants(h0, h3):
    """A Q whose rows 0 and 3 are the constants h0 and h3 at every pixel."""
    Q = np.zeros((4, 4))
    Q[0, 3], Q[1, 3], Q[2, 3], Q[3, 3] = h0, 1.0, 1.0, h3
    return Q


# ------------------------------------------------------------------------------ the dense map
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_closed_form_with_dyadic_q(dtype):
    H, W = 48, 96
    rng = np.random.default_rng(0)
    d = 2.0 ** rng.integers(-4 if dtype == np.int16 else -8, 8, (H, W))          # powers of two
    disp = (d * 16).astype(np.int16) if dtype == np.int16 else d.astype(np.float32)
    out = CO.reproject_image_to_3d(disp, Q_DYADIC)
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    exp = np.stack([(x - 64) * 8 / d, (y - 32) * 8 / d, 512 * 8 / d], -1)
    assert out.dtype == np.float32 and out.shape == (H, W, 3)
    assert np.array_equal(out.astype(np.float64), exp)                            # exact: nothing rounds


def test_int16_map_equals_the_float_disparity_it_stands_for():
    rng = np.random.default_rng(1)
    m = rng.integers(-2047 * 16, 2047 * 16 + 1, (20, 30)).astype(np.int16)
    f = (m.astype(np.float32) / np.float32(16.0))                                 # create_depth_map's disparity
    assert np.array_equal(CO.reproject_image_to_3d(m, Q_DYADIC), CO.reproject_image_to_3d(f, Q_DYADIC),
                          equal_nan=True)


def test_planted_points_of_the_projects_calibration():
    """Points planted from P1 / P2 alone (Z = -P2[0,3] / d) project to whole pixels and 1/16
    disparities, and the reprojection with Q returns them.  Tolerance: h_r is narrowed to f32
    (relative error <= 2^-24), multiplied by an f64 reciprocal and narrowed again (2^-24 more):
    (1 + 2^-24)^2 - 1 < 2^-23 + 2^-40 of the coordinate; 1e-12 covers the f64 differences
    between the Q path and the P path."""
    c = synthetic.synthetic_calibration(640, 480, seed=3)
    R1, R2, P1, P2, Q, _, _ = calib.stereo_rectify(c["mtx_left"], c["dist_left"], c["mtx_right"], c["dist_right"],
                                                  (640, 480), c["R"], c["T"], alpha=0)
    rng = np.random.default_rng(2)
    n = 200
    xs, ys = rng.integers(0, 640, n), rng.integers(0, 480, n)
    m = rng.integers(16, 120 * 16, n).astype(np.int16)
    d = m / 16.0
    f, cx, cy = P1[0, 0], P1[0, 2], P1[1, 2]
    Z = -P2[0, 3] / d
    pts = np.stack([(xs - cx) * Z / f, (ys - cy) * Z / P1[1, 1], Z], 1)
    hom = np.vstack([pts.T, np.ones(n)])
    p1, p2 = P1 @ hom, P2 @ hom
    np.testing.assert_allclose(p1[0] / p1[2], xs, atol=1e-9)
    np.testing.assert_allclose(p1[1] / p1[2], ys, atol=1e-9)
    np.testing.assert_allclose(p1[0] / p1[2] - p2[0] / p2[2], d, atol=1e-9)
    disp = np.full((480, 640), 16, np.int16)
    disp[ys, xs] = m
    got = CO.reproject_image_to_3d(disp, Q)[ys, xs].astype(np.float64)
    tol = np.abs(pts) * (2.0 ** -23 + 2.0 ** -40) + 1e-12
    assert (np.abs(got - pts) <= tol).all(), np.abs(got - pts).max()
    assert (Z > 0).all() and np.abs(got - pts).max() > 0                          # f32 outputs: not vacuous


def test_accumulation_order_is_observable():
    # the last bit of the f64 sum: (0.1 + 0.2) + 0.3 against 0.1 + (0.2 + 0.3)
    Q = np.zeros((4, 4))
    Q[0, :3] = 0.1, 0.2, 0.3
    Q[3, 3] = 1.0
    d = np.ones((2, 2), np.float32)
    h0 = CO.homogeneous(d.astype(np.float64), Q)[0][1, 1]
    assert h0 == (0.1 + 0.2) + 0.3 and h0 != 0.1 + (0.2 + 0.3)
    # and a case that survives the narrowing: 2^60 - 2^60 + 1 is 1 in order, 0 when y and d pair up first
    Q[0, :3] = 2.0 ** 60, -2.0 ** 60, 1.0
    out = CO.reproject_image_to_3d(d, Q)
    assert out[1, 1, 0] == F32(1.0) and (2.0 ** 60) + (-2.0 ** 60 + 1.0) == 0.0


def test_sum_starts_from_zero():
    """Every term of row 0 is -0.0 at pixel (0, 0) with d = 0; Matx's sum from +0.0 makes h_0 = +0.0."""
    Q = np.zeros((4, 4))
    Q[0] = -1.0, -1.0, -1.0, -0.0
    Q[3, 3] = 1.0
    out = CO.reproject_image_to_3d(np.zeros((1, 1), np.float32), Q)
    assert out[0, 0, 0] == 0 and not np.signbit(out[0, 0, 0])
    assert np.signbit(((-1.0 * 0.0 + -1.0 * 0.0) + -1.0 * 0.0) + -0.0)            # without the leading 0


def test_homogeneous_point_is_narrowed_before_the_scale():
    h0, h3 = 1.0 + 2.0 ** -24 - 2.0 ** -30, 0.8
    ia = 1.0 / h3
    narrowed, direct = F32(np.float64(F32(h0)) * ia), F32(h0 * ia)
    assert narrowed != direct
    out = CO.reproject_image_to_3d(np.zeros((1, 1), np.float32), _q_only_constants(h0, h3))
    assert out[0, 0, 0] == narrowed
    # Vec /= double multiplies by the reciprocal: a division would give another value here
    h0 = 5.0
    h3 = 3.0 * 0.1
    assert F32(np.float64(F32(h0)) * (1.0 / h3)) == CO.reproject_image_to_3d(
        np.zeros((1, 1), np.float32), _q_only_constants(h0, h3))[0, 0, 0]


def test_zero_w_gives_inf_and_nan_and_leaves_the_cloud():
    disp = np.full((40, 70), 4.0, np.float32)
    disp[:, 60:] = 0.0                                                            # h_3 = d / 8 = 0
    out = CO.reproject_image_to_3d(disp, Q_DYADIC)
    assert np.isposinf(out[5, 66, 0]) and np.isneginf(out[5, 61, 0]) and np.isnan(out[5, 64, 0])
    assert np.isposinf(out[:, 60:, 2]).all() and np.isnan(out[32, 60:, 1]).all()
    xyz, _, idx, n = CO.point_cloud(disp, Q_DYADIC, min_valid=-1.0)
    assert n == 40 * 60 and (idx % 70 < 60).all() and np.isfinite(xyz).all()


def test_handle_missing_marks_every_minimum():
    m = np.full((6, 9), 160, np.int16)
    m[1, 2] = m[4, 8] = m[0, 0] = -16                                             # the minimum, three times
    m[3, 3] = -15                                                                 # 1/16 above it: not missing
    out = CO.reproject_image_to_3d(m, Q_DYADIC, True)
    plain = CO.reproject_image_to_3d(m, Q_DYADIC, False)
    miss = m == m.min()
    assert (out[..., 2][miss] == F32(10000.0)).all() and miss.sum() == 3
    assert np.array_equal(out[..., :2], plain[..., :2]) and np.array_equal(out[..., 2][~miss], plain[..., 2][~miss])
    _, _, idx, n = CO.point_cloud(m, Q_DYADIC, min_valid=-100.0, handle_missing=True)
    assert n == m.size - 3 and not np.isin(np.flatnonzero(miss.ravel()), idx).any()


def test_float_maps_with_nan_and_inf():
    d = np.full((5, 8), 2.0, np.float32)
    d[0, 0], d[1, 1], d[2, 2], d[3, 3] = np.nan, np.inf, -np.inf, 1.0
    out = CO.reproject_image_to_3d(d, Q_DYADIC, True)
    assert np.isnan(out[0, 0]).all()
    assert np.isnan(out[1, 1]).all() and np.isnan(out[2, 2]).all()                # q_r2 d = 0 * inf in rows 0..2
    # the minimum is -inf (NaN ignored); |-inf - -inf| is NaN, so nothing is within FLT_EPSILON of it
    assert CO.map_minimum(d.astype(np.float64)) == -np.inf and not (out[..., 2] == F32(10000.0)).any()
    d[2, 2] = 2.0
    out = CO.reproject_image_to_3d(d, Q_DYADIC, True)
    assert out[3, 3, 2] == F32(10000.0) and (out[..., 2] == F32(10000.0)).sum() == 1
    assert CO.map_minimum(np.full((2, 2), np.nan)) == np.inf
    assert not (CO.reproject_image_to_3d(np.full((2, 2), np.nan, np.float32), Q_DYADIC, True) == 10000).any()
    # the cloud: a NaN fails d >= min_valid; +inf passes it and falls to the finite test
    xyz, _, idx, n = CO.point_cloud(d, Q_DYADIC, min_valid=1.5)
    assert n == d.size - 3 and 0 not in idx and 3 * 8 + 3 not in idx and 1 * 8 + 1 not in idx


# ------------------------------------------------------------------------------ the cloud
def _loop_cloud(disp, Q, colors, min_valid, z_min, z_max, roi, handle_missing, cap):
    """The list, pixel by pixel, from the dense map."""
    H, W = disp.shape
    dense = CO.reproject_image_to_3d(disp, Q, False)
    d = CO.disparity_f64(disp)
    dmin = CO.map_minimum(d)
    rx, ry, rw, rh = roi if roi is not None else (0, 0, W, H)
    pts, cols, idx = [], [], []
    for y in range(H):
        for x in range(W):
            X = dense[y, x]
            if not d[y, x] >= float(F32(min_valid)) or not all(math.isfinite(v) for v in X):
                continue
            if not (F32(z_min) <= X[2] <= F32(z_max)) or not (rx <= x < rx + rw and ry <= y < ry + rh):
                continue
            if handle_missing and abs(d[y, x] - dmin) <= CO.FLT_EPSILON:
                continue
            pts.append(X)
            cols.append(colors[y, x])
            idx.append(y * W + x)
    n = len(idx)
    k = n if cap is None else min(cap, n)
    return (np.array(pts[:k], np.float32).reshape(k, 3), np.array(cols[:k], np.uint8).reshape(k, 3),
            np.array(idx[:k], np.uint32), n)


def _scene(seed=3, H=23, W=37):
    rng = np.random.default_rng(seed)
    m = (2 ** rng.integers(2, 9, (H, W))).astype(np.int16)        # d = 1/4 .. 16: Z = 4096 / d in 256 .. 16384
    m[rng.random((H, W)) < 0.3] = -16                             # the (min_disp - 1) marker, min_disp = 0
    m[rng.random((H, W)) < 0.1] = 0                               # d = 0: h_3 = 0
    colors = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return m, colors


CLAUSES = {
    "min_valid": dict(min_valid=0.5),
    "finite_only": dict(min_valid=-1.0),
    "z_range": dict(min_valid=-1e9, z_min=512.0, z_max=4096.0),
    "roi": dict(min_valid=-1e9, roi=(5, 4, 11, 7)),
    "missing": dict(min_valid=-1e9, handle_missing=True),
    "all": dict(min_valid=0.25, z_min=512.0, z_max=4096.0, roi=(5, 4, 20, 15), handle_missing=True),
    "roi_one_pixel": dict(min_valid=-1e9, roi=(36, 22, 1, 1)),
}


@pytest.mark.parametrize("name", sorted(CLAUSES))
def test_compaction_clauses(name):
    m, colors = _scene()
    if name == "roi_one_pixel":
        m[22, 36] = 64
    kw = dict(min_valid=0.0, z_min=-np.inf, z_max=np.inf, roi=None, handle_missing=False)
    kw.update(CLAUSES[name])
    xyz, bgr, idx, n = CO.point_cloud(m, Q_DYADIC, colors, **kw)
    e_xyz, e_bgr, e_idx, e_n = _loop_cloud(m, Q_DYADIC, colors, cap=None, **kw)
    assert n == e_n and 0 < n < m.size
    assert np.array_equal(xyz, e_xyz) and np.array_equal(bgr, e_bgr) and np.array_equal(idx, e_idx)
    assert (np.diff(idx.astype(np.int64)) > 0).all() if n > 1 else n == 1         # row-major order
    if name == "z_range":   # Z exactly at both ends is kept: d = 8 -> 512, d = 1 -> 4096
        Z = set(xyz[:, 2].tolist())
        assert 512.0 in Z and 4096.0 in Z and min(Z) == 512.0 and max(Z) == 4096.0
    if name == "roi_one_pixel":
        assert n == 1 and idx[0] == 22 * 37 + 36


def test_capacity_and_the_empty_and_full_clouds():
    m, colors = _scene()
    full = CO.point_cloud(m, Q_DYADIC, colors)
    n = full[3]
    for cap in (n + 5, n, n - 1, 1, 0):
        xyz, bgr, idx, got = CO.point_cloud(m, Q_DYADIC, colors, cap=cap)
        k = min(cap, n)
        assert got == n and len(xyz) == len(bgr) == len(idx) == k
        assert np.array_equal(xyz, full[0][:k]) and np.array_equal(bgr, full[1][:k]) and np.array_equal(idx, full[2][:k])
    xyz, bgr, idx, got = CO.point_cloud(m, Q_DYADIC, colors, min_valid=1000.0)     # N = 0
    assert got == 0 and xyz.shape == (0, 3) and bgr.shape == (0, 3) and idx.shape == (0,)
    ones = np.full((7, 9), 16, np.int16)                                          # N = H W
    xyz, _, idx, got = CO.point_cloud(ones, Q_DYADIC)
    assert got == 63 and np.array_equal(idx, np.arange(63, dtype=np.uint32))
    assert np.array_equal(xyz, CO.reproject_image_to_3d(ones, Q_DYADIC).reshape(-1, 3))


# ------------------------------------------------------------------------------ write_ply
def _read_ply(path):
    with open(path, "rb") as f:
        assert f.readline() == b"ply\n" and f.readline() == b"format binary_little_endian 1.0\n"
        n = int(f.readline().split()[2])
        props = []
        while True:
            line = f.readline().decode().split()
            if line == ["end_header"]:
                break
            assert line[0] == "property"
            props.append((line[2], {"float": "<f4", "uchar": "u1"}[line[1]]))
        body = f.read()
    rec = np.frombuffer(body, np.dtype(props))
    assert len(rec) == n
    return rec


@pytest.mark.parametrize("with_color", [True, False])
def test_write_ply_round_trip(tmp_path, with_color):
    rng = np.random.default_rng(4)
    xyz = rng.normal(size=(17, 3)).astype(np.float32)
    bgr = rng.integers(0, 256, (17, 3), dtype=np.uint8)
    p = tmp_path / "cloud.ply"
    cloud.write_ply(p, xyz, bgr if with_color else None)
    rec = _read_ply(p)
    assert rec.dtype.names == (("x", "y", "z", "red", "green", "blue") if with_color else ("x", "y", "z"))
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), xyz)
    if with_color:
        assert np.array_equal(np.stack([rec["blue"], rec["green"], rec["red"]], 1), bgr)
    cloud.write_ply(p, np.empty((0, 3), np.float32))
    assert len(_read_ply(p)) == 0
    with pytest.raises(ValueError):
        cloud.write_ply(p, xyz[:, :2])
    with pytest.raises(ValueError):
        cloud.write_ply(p, xyz, bgr[:5])


# ------------------------------------------------------------------------------ arguments
def test_python_argument_errors_need_no_engine():
    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError("the engine was reached")

    eng = NoEngine()
    d = np.ones((6, 8), np.float32)
    col = np.zeros((6, 8, 3), np.uint8)
    for fn in (lambda *a, **k: cloud.reproject_image_to_3d(*a, engine=eng, **k),
               lambda *a, **k: cloud.point_cloud(*a, engine=eng, **k)):
        with pytest.raises(TypeError, match="NumPy array"):
            fn([[1.0]], Q_DYADIC)
        with pytest.raises(TypeError, match="int16"):
            fn(d.astype(np.float64), Q_DYADIC)
        with pytest.raises(ValueError, match="H x W"):
            fn(d[None], Q_DYADIC)
        with pytest.raises(ValueError, match="H x W"):
            fn(d[:0], Q_DYADIC)
        with pytest.raises(ValueError, match="4 x 4"):
            fn(d, Q_DYADIC[:3])
        with pytest.raises(ValueError, match="non-finite"):
            fn(d, np.where(Q_DYADIC == 512, np.inf, Q_DYADIC))
        with pytest.raises(TypeError, match="real matrix"):
            fn(d, Q_DYADIC.astype(complex))
    pc = lambda **k: cloud.point_cloud(d, Q_DYADIC, engine=eng, **k)  # noqa: E731
    with pytest.raises(TypeError, match="uint8"):
        pc(colors=col.astype(np.float32))
    with pytest.raises(ValueError, match="match the map"):
        pc(colors=col[:, :7])
    with pytest.raises(ValueError, match="match the map"):
        pc(colors=col[..., 0])
    for bad in ((3.0, 1.0), (np.nan, 1.0), (1.0,)):
        with pytest.raises(ValueError, match="z_range"):
            pc(z_range=bad)
    for bad in ((0, 0, 9, 6), (0, 0, 8, 7), (-1, 0, 2, 2), (0, 0, 0, 3), (1, 2, 3)):
        with pytest.raises(ValueError, match="roi"):
            pc(roi=bad)
    with pytest.raises(ValueError, match="capacity"):
        pc(capacity=-1)
    with pytest.raises(ValueError, match="min_disp"):
        pc(min_disp=np.nan)
    p = cloud.CloudParams(min_disp=2, z_range=(0.5, 30.0), roi=(1, 2, 3, 4), handle_missing_values=True)
    s = p.check(6, 8).c_struct()
    assert (s.min_valid, s.z_min, s.z_max, s.roi_x, s.roi_y, s.roi_w, s.roi_h, s.handle_missing) == \
        (2.0, 0.5, 30.0, 1, 2, 3, 4, 1)
    s = cloud.CloudParams().c_struct()
    assert (s.min_valid, s.z_min, s.z_max, s.roi_w, s.roi_h, s.handle_missing) == (0.0, -np.inf, np.inf, 0, 0, 0)


def test_pipeline_takes_cloud_params_and_keeps_its_outputs():
    pipe = FusionFramePipeline(cloud=cloud.CloudParams(z_range=(0.1, 50.0)))
    assert pipe.cloud.z_range == (0.1, 50.0) and FusionFramePipeline().cloud is None
    with pytest.raises(TypeError, match="CloudParams"):
        FusionFramePipeline(cloud={"min_disp": 0})
    with pytest.raises(ValueError, match="z_range"):
        FusionFramePipeline(cloud=cloud.CloudParams(z_range=(2.0, 1.0)))
    assert "cloud" not in OUTPUT_NAMES and len(OUTPUT_NAMES) == 11
    with pytest.raises(ValueError, match="unknown outputs"):
        FusionFramePipeline(outputs=("fused_u8", "fused_depth"), cloud=cloud.CloudParams())
    with pytest.raises(ValueError, match="unknown outputs"):
        FusionFramePipeline(outputs=("cloud",))
    r = FrameResult()
    assert r.cloud is None
    with pytest.raises(ValueError):
        r.device("cloud")
