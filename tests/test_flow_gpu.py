"""Farneback optical flow and the flow depth estimator on the GPU, bit-exact against the NumPy
restatement (tests/sv_flow_oracle.py).  Shapes, the smallest at which each mechanism can go
wrong: 16x16 (an interior of 6x6 outside the border table, the 15-wide box clamped on both
sides at once), 37x70 (odd, partial tiles on both axes, one scale), 64x80 (the coarse level
exactly at the minimum size), 67x133 (half-to-even level sizes), 130x150 (three scales) and the
fusion app's processing size 356x633 once (four scales, ksize 19)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flow_scenes as S  # noqa: E402
import sv_flow_oracle as O  # noqa: E402
import sv_fuse_oracle as FO  # noqa: E402
import sv_fusion_oracle as NO  # noqa: E402
from stereovision_amd import colormap, fusion  # noqa: E402
from stereovision_amd import flow as F  # noqa: E402
from stereovision_amd import fused_depth_map as FDM  # noqa: E402
from stereovision_amd.engine import SVError  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16), (37, 70), (64, 80), (67, 133), (130, 150)]
STAGE_SHAPES = [(16, 16), (37, 70), (130, 150)]
APP = (356, 633)


def _launches(engine):
    return engine.profile_read("flow")[1]


@functools.lru_cache(maxsize=None)
def _textured(shape, seed=1):
    """A smooth textured pair with planted motion (+1.5, -0.75) and the restatement's flow."""
    prev, nxt = S.translated_pair(shape[0], shape[1], 1.5, -0.75, seed=seed)
    exp = O.farneback(prev, nxt)
    exp.setflags(write=False)
    return prev, nxt, exp


# ---------------------------------------------------------------------------- per stage
def _polyexp_gpu(engine, img, n, sigma):
    H, W = img.shape
    d_img = engine.upload("fl_t_img", img)
    d_R = engine.scratch("fl_t_R", 20 * H * W)
    engine.fb_polyexp_dev(d_img, H, W, n, F.polyexp_tables(n, sigma), d_R)
    return engine.to_host(d_R, (5, H, W), np.float32)


@pytest.mark.parametrize("n,sigma", [(5, 1.2), (7, 1.5)])
@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_polyexp_bit_exact(engine, shape, n, sigma):
    rng = np.random.default_rng(21)
    img = (rng.random(shape) * 255).astype(np.float32)
    np.testing.assert_array_equal(_polyexp_gpu(engine, img, n, sigma), O.polyexp(img, n, sigma))
    steps = np.where(rng.random(shape) < 0.5, 0.0, 255.0).astype(np.float32)
    steps[:, shape[1] // 2:] = np.where(np.arange(shape[0])[:, None] % 6 < 3, 0.0, 255.0)
    np.testing.assert_array_equal(_polyexp_gpu(engine, steps, n, sigma), O.polyexp(steps, n, sigma))


def _mixed_flow(shape, seed):
    """Sub-pixel, whole-pixel, exactly-on-the-last-column / -row and far-outside vectors."""
    H, W = shape
    rng = np.random.default_rng(seed)
    flow = ((rng.random((2, H, W)) - 0.5) * 6).astype(np.float32)
    whole = rng.random((H, W)) < 0.25
    flow[:, whole] = np.rint(flow[:, whole])
    ys, xs = np.mgrid[0:H, 0:W]
    last = rng.random((H, W)) < 0.05
    flow[0][last] = (W - 1 - xs)[last]                       # x + dx = W - 1 exactly
    last = rng.random((H, W)) < 0.05
    flow[1][last] = (H - 1 - ys)[last]
    far = rng.random((H, W)) < 0.05
    flow[0][far] = rng.choice(np.array([-1e30, -3e9, -70000.5, -1.25, 3e9, 1e30], np.float32), int(far.sum()))
    far = rng.random((H, W)) < 0.05
    flow[1][far] = rng.choice(np.array([-1e30, -3e9, -70000.5, 3e9, 1e30], np.float32), int(far.sum()))
    flow[:, 0, 0] = (-0.5, -0.5)                             # floor -1: outside by one
    flow[:, H - 1, W - 1] = (-1.0, -1.0)                     # the last cell that is inside
    return flow


@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_update_matrices_bit_exact(engine, shape):
    H, W = shape
    rng = np.random.default_rng(22)
    R0 = rng.standard_normal((5, H, W)).astype(np.float32)
    R1 = rng.standard_normal((5, H, W)).astype(np.float32)
    flow = _mixed_flow(shape, 23)
    c = {}
    with np.errstate(over="ignore", invalid="ignore"):
        exp = O.update_matrices(R0, R1, flow, c)
    assert c["inside"] > H * W // 4 and c["outside"] > H * W // 20
    d_M = engine.scratch("fl_t_M", 20 * H * W)
    engine.fb_update_matrices_dev(engine.upload("fl_t_R0", R0), engine.upload("fl_t_R1", R1),
                                  engine.upload("fl_t_flow", flow), H, W, d_M)
    got = engine.to_host(d_M, (5, H, W), np.float32)
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("winsize", [3, 15, 31])
@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_blur_solve_bit_exact(engine, shape, winsize):
    H, W = shape
    rng = np.random.default_rng(24)
    M = (rng.standard_normal((5, H, W)) * rng.choice([1e-3, 1.0, 50.0], (5, H, W))).astype(np.float32)
    exp = O.blur_solve(M, winsize)
    d_M = engine.upload("fl_t_M2", M)
    d_flow = engine.scratch("fl_t_flow2", 8 * H * W)
    engine.fb_blur_solve_dev(d_M, H, W, winsize, d_flow)
    np.testing.assert_array_equal(engine.to_host(d_flow, (2, H, W), np.float32), exp)
    engine.fb_blur_solve_dev(d_M, H, W, winsize, d_flow, interleaved=True)
    np.testing.assert_array_equal(engine.to_host(d_flow, (H, W, 2), np.float32), exp.transpose(1, 2, 0))


# ---------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("shape", SHAPES + [APP])
def test_flow_textured_pair_bit_exact(engine, shape):
    prev, nxt, exp = _textured(shape)
    got = F.farneback_flow(prev, nxt, 0.5, 3, 15, 3, 5, 1.2, 0)
    assert got.dtype == np.float32 and got.shape == shape + (2,)
    np.testing.assert_array_equal(got, exp)
    if min(shape) >= 64:                                     # and it is the planted motion
        epe = np.hypot(got[..., 0] - 1.5, got[..., 1] + 0.75)[16:-16, 16:-16]
        assert float(np.median(epe)) < 0.5 * float(np.hypot(1.5, 0.75))


def test_flow_noise_constant_and_identical_pairs(engine):
    prev, nxt = S.noise_pair(67, 133, seed=0)
    c = {}
    exp = O.farneback(prev, nxt, counters=c)
    assert c["outside"] > 3 * sum(h + w - 1 for h, w, _, _ in O.levels(67, 133, 0.5, 3))
    np.testing.assert_array_equal(F.farneback_flow(prev, nxt), exp)
    a, b = np.full((37, 70), 9, np.uint8), np.full((37, 70), 200, np.uint8)
    got = F.farneback_flow(a, b)
    assert not got.any()
    np.testing.assert_array_equal(got, O.farneback(a, b))
    same = _textured((64, 80))[0]
    np.testing.assert_array_equal(F.farneback_flow(same, same), O.farneback(same, same))


@pytest.mark.parametrize("kw", [dict(levels=0), dict(iterations=1), dict(pyr_scale=0.8),
                                dict(winsize=21, poly_n=7, poly_sigma=1.5)])
def test_flow_non_default_arguments(engine, kw):
    prev, nxt, _ = _textured((130, 150))
    okw = {("nlevels" if k == "levels" else k): v for k, v in kw.items()}
    np.testing.assert_array_equal(F.farneback_flow(prev, nxt, **kw), O.farneback(prev, nxt, **okw))


def test_rejected_arguments_launch_nothing(engine):
    g = _textured((37, 70))[0]
    if FDM.warmup_done is not None:                           # its flow step must not land in the count
        FDM.warmup_done.wait()
    engine.profile(True)
    try:
        engine.synchronize()
        before = _launches(engine)
        for kw in (dict(pyr_scale=1.0), dict(pyr_scale=0.0), dict(levels=-1), dict(winsize=4), dict(winsize=1),
                   dict(winsize=33), dict(iterations=0), dict(poly_n=6), dict(flags=256), dict(flags=4)):
            with pytest.raises(ValueError):
                F.farneback_flow(g, g, **kw)
        with pytest.raises(ValueError):
            F.farneback_flow(g[:15], g[:15])
        with pytest.raises(ValueError):
            F.farneback_flow(np.zeros((2048, 2048), np.uint8), np.zeros((2048, 2048), np.uint8), 0.5, 4)   # ksize 39
        d_g = engine.upload("fl_t_g", g)
        d_f = engine.scratch("fl_t_f", 8 * g.size)
        with pytest.raises(ValueError):
            F.farneback_flow_dev(engine, d_g, d_g, 37, 70, winsize=16, d_flow=d_f)
        with pytest.raises(ValueError):
            F.farneback_flow_dev(engine, d_g, 0, 37, 70, d_flow=d_f)
        # the C ABI's own checks
        tables = F.polyexp_tables(7, 1.5)                     # long enough for any poly_n tried
        scales = [(37, 70, 3, F.gaussian_coef(3, 0.0))]
        for args in ((scales, 2.0, 16, 3, 5), (scales, 2.0, 15, 0, 5), (scales, 2.0, 15, 3, 6),
                     ([(36, 70, 3, F.gaussian_coef(3, 0.0))], 2.0, 15, 3, 5), ([], 2.0, 15, 3, 5),
                     (scales + [(40, 35, 3, F.gaussian_coef(3, 0.5))], 2.0, 15, 3, 5)):
            with pytest.raises(SVError) as ei:
                engine.farneback_flow_dev(d_g, d_g, 37, 70, 70, args[0], args[1], args[2], args[3], args[4],
                                          tables, d_f)
            assert ei.value.code == -22
        with pytest.raises(SVError):
            engine.farneback_flow_dev(d_g, d_g, 15, 70, 70, [(15, 70, 3, F.gaussian_coef(3, 0.0))], 2.0, 15, 3, 5,
                                      tables, d_f)
        with pytest.raises(SVError):
            engine.fb_blur_solve_dev(d_f, 37, 70, 33, d_f)
        with pytest.raises(SVError):
            engine.fb_polyexp_dev(d_f, 37, 70, 6, tables, d_f)
        with pytest.raises(ValueError):
            F.flow_depth_dev(engine, d_f, 37, 70, np.full((3, 3), np.nan), d_f)
        engine.synchronize()
        assert _launches(engine) == before
        F.farneback_flow(g, g)                                # a good call is counted
        assert _launches(engine) > before
    finally:
        engine.profile(False)


# ---------------------------------------------------------------------------- flow depth
PROJECTIVE = np.array([[1.01, 0.02, 1.5], [-0.015, 0.99, -0.75], [2e-4, -3e-4, 1.0]])


@pytest.mark.parametrize("shape", [(16, 16), (37, 70), (130, 150)])
def test_flow_depth_bit_exact(engine, shape):
    rng = np.random.default_rng(31)
    flow = ((rng.random(shape + (2,)) - 0.5) * 8).astype(np.float32)
    flow[1, 2] = (1e4, -1e4)
    depth, stable, (mn, mx) = F.flow_depth(flow, PROJECTIVE)
    e_depth, _, e_mn, e_mx = O.flow_depth(flow, PROJECTIVE)
    np.testing.assert_array_equal(depth, e_depth)
    assert stable is None
    assert mn == e_mn == depth.min() and mx == e_mx == depth.max()
    s0 = (rng.random(shape) * 2).astype(np.float32)
    for alpha in (0.9, 0.99):
        depth, stable, _ = F.flow_depth(flow, PROJECTIVE, stable=s0, alpha=alpha)
        e_depth, e_stable, _, _ = O.flow_depth(flow, PROJECTIVE, stable=s0, alpha=alpha)
        np.testing.assert_array_equal(depth, e_depth)
        np.testing.assert_array_equal(stable, e_stable)


def test_flow_depth_zero_denominator(engine):
    Hm = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0], [0.25, 0.5, -5.0]])      # w = 0 at x = 4, y = 8
    rng = np.random.default_rng(32)
    flow = ((rng.random((37, 70, 2)) - 0.5) * 8).astype(np.float32)
    c = {}
    e_depth, _, e_mn, e_mx = O.flow_depth(flow, Hm, counters=c)
    assert c["w_zero"] == 11                                                   # x + 2 y = 20, x even
    depth, _, (mn, mx) = F.flow_depth(flow, Hm)
    np.testing.assert_array_equal(depth, e_depth)
    assert (mn, mx) == (e_mn, e_mx)


# ---------------------------------------------------------------------------- the estimator
EGO = [np.array([[1.004, 0.006, 1.2], [-0.005, 0.997, -0.8], [1e-5, -2e-5, 1.0]]),
       np.array([[0.998, -0.004, -0.9], [0.004, 1.002, 1.1], [-1e-5, 1e-5, 1.0]])]
EST = (96, 128)


def _grid_homography(flow, min_inliers=15):
    H, W = flow.shape[:2]
    ys, xs = np.mgrid[8:H:16, 8:W:16]
    pts = np.vstack((xs.ravel(), ys.ravel())).T.astype(np.float32)
    Hm, mask = F.find_homography_ransac(pts, pts + flow[ys.ravel(), xs.ravel()], 3.0, 2000, 0.995)
    assert Hm is not None and mask.sum() >= min_inliers
    return Hm


@functools.lru_cache(maxsize=None)
def _sequence():
    """Three frames (the second and third warped by known homographies) and the restatement's
    maps: [(depth, returned map)] for the two pairs."""
    f0, f1 = S.warped_pair(EST[0], EST[1], EGO[0], seed=4)
    _, f2 = S.warped_pair(EST[0], EST[1], EGO[1] @ EGO[0], seed=4)
    out = []
    for a, b in ((f0, f1), (f1, f2)):
        flow = O.farneback(a, b)
        depth = O.flow_depth(flow, _grid_homography(flow))[0]
        out.append((depth, O.bilateral(depth)))
    return (f0, f1, f2), out


def test_estimator_sequence(engine):
    (f0, f1, f2), exp = _sequence()
    est = F.OpticalFlowDepthEstimator()
    assert est.min_inliers == 15 and est.motion_timeout == 1.5
    assert est.prev_gray is None and est.stable_depth is None and est.camera_moving is False
    assert est(S.to_bgr(f0)) is None                                          # the first frame
    np.testing.assert_array_equal(est.prev_gray, f0)
    got = est(S.to_bgr(f1))
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, exp[0][1])
    assert est.camera_moving is True
    np.testing.assert_array_equal(est.stable_depth, exp[0][0])
    np.testing.assert_array_equal(est.prev_gray, f1)
    got = est(S.to_bgr(f2))
    np.testing.assert_array_equal(got, exp[1][1])
    stable = np.float32(0.9) * exp[0][0] + np.float32(1.0 - 0.9) * exp[1][0]
    np.testing.assert_array_equal(est.stable_depth, stable)
    # an invalid homography while the camera was moving a moment ago: the smoothed stable map
    est.min_inliers = 10 ** 6
    est.motion_timeout = 3600.0
    got = est(S.to_bgr(f0))
    np.testing.assert_array_equal(got, O.bilateral(stable))
    np.testing.assert_array_equal(est.prev_gray, f0)
    est.motion_timeout = 0.0                                                   # a static scene
    assert est(S.to_bgr(f1)) is None
    assert est.camera_moving is False
    # a size change: None, and the state starts again
    small = S.translated_pair(64, 80, 1.0, 0.5, seed=5)
    assert est(S.to_bgr(small[0])) is None
    assert est.stable_depth is None
    np.testing.assert_array_equal(est.prev_gray, small[0])


def test_estimator_small_frames_and_garbage(engine):
    est = F.OpticalFlowDepthEstimator(min_inliers=4, motion_timeout=3600.0)
    a, b = S.translated_pair(40, 48, 1.0, 0.5, seed=6)                         # below 50 px: no homography
    assert est(S.to_bgr(a)) is None
    assert est(S.to_bgr(b)) is None
    assert est.stable_depth is None
    for junk in (None, "frame", np.zeros((0, 0, 3), np.uint8), np.zeros((40, 48, 4), np.uint8),
                 np.zeros((40, 48, 3), np.float32), np.zeros((8, 8, 3), np.uint8), object()):
        assert est(junk) is None


def test_estimator_chain_to_fuse(engine):
    (f0, f1, _), exp = _sequence()
    rng = np.random.default_rng(41)
    disparity = (rng.random(EST) * 96).astype(np.float32)
    disparity[rng.random(EST) < 0.2] = 0
    est = F.OpticalFlowDepthEstimator()
    est(S.to_bgr(f0))
    depth = est(S.to_bgr(f1))
    normalized = FDM.normalize_to_stereo_range(depth, disparity)
    e_norm = NO.normalize_to_stereo_range(exp[0][1], disparity)
    np.testing.assert_array_equal(normalized, e_norm)
    u8, bgr = FDM.fuse_depth_maps(None, None, None, None, normalized, est.camera_moving)
    e = FO.fuse(None, None, None, e_norm)
    np.testing.assert_array_equal(u8, e["u8"])
    np.testing.assert_array_equal(bgr, colormap.table("jet")[u8])
    assert FDM.last_fuse_info["mode_parts"] == ["Flow_base"]
    assert fusion.BASE_FLOW == FDM.last_fuse_info["base"]
