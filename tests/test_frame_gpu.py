"""FusionFramePipeline on the GPU: every output and scalar of every frame array_equal / == to the
chain of the host-array drop-ins (tests/frame_chain.py), the branch cases, the new kernels alone
against NumPy, and the transfer cap at the app size."""
import functools
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("SV_WARMUP_AT_IMPORT", "0")
import frame_chain as C  # noqa: E402
from stereovision_amd import flow as F  # noqa: E402
from stereovision_amd import fused_depth_map as FDM  # noqa: E402
from stereovision_amd import fusion, synthetic  # noqa: E402
from stereovision_amd.frame import OUTPUT_NAMES, FusionFramePipeline  # noqa: E402

pytestmark = pytest.mark.gpu

PH, PW = 88, 120            # the processing size: every branch can run (35 grid points, 3 pyramid levels)
CH, CW = 176, 240           # the camera frames: the resize in front of the remap runs
STEREO = dict(min_disp=0, num_disp=32, window_size=5)


@pytest.fixture
def clock(monkeypatch):
    """stereovision_amd.flow.time.time under the test's control: the pipeline's estimator and the
    chain's see the same instants, so the motion timeout decides the same way in both."""
    now = [1000.0]
    monkeypatch.setattr(F.time, "time", lambda: now[0])
    return now


@functools.lru_cache(maxsize=None)
def _calibration(width, height, scale, seed=0):
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "stereo_calibration_data.pkl")
        with open(p, "wb") as f:
            pickle.dump(synthetic.synthetic_calibration(width, height, seed), f)
        c = FDM.load_stereo_calibration_with_scaling(scale, p)
    assert c is not None
    return c


@functools.lru_cache(maxsize=None)
def _frames(H=CH, W=CW, n=6, disparity=8):
    return C.moving_stereo_sequence(H, W, n, disparity=disparity)


def _midas(shape, k):
    """A relative depth map that changes per frame, with values on both sides of [0, 255]."""
    h, w = shape
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    rng = np.random.default_rng(100 + k)
    return (np.float32(3.0) * xs + np.float32(2.0) * ys - np.float32(40.0) +
            rng.random((h, w), dtype=np.float32) * np.float32(30.0)).astype(np.float32)


def _same(res, exp, names, where):
    for s in C.SCALARS:
        assert getattr(res, s) == exp[s], (where, s, getattr(res, s), exp[s])
    for name in names:
        got, e = getattr(res, name), exp[name]
        assert (got is None) == (e is None), (where, name)
        if e is not None:
            assert got.dtype == e.dtype and got.shape == e.shape, (where, name, got.dtype, e.dtype, got.shape, e.shape)
            np.testing.assert_array_equal(got, e, err_msg=f"{where}: {name}")


def _run(pipe, chain, frames, clock, midas_for=lambda k: None, names=OUTPUT_NAMES, tag="", before=None):
    """Both through the sequence, frame by frame; returns the pipeline's results."""
    out = []
    for k, (fl, fr) in enumerate(frames):
        clock[0] += 0.1
        if before is not None:
            before(k, pipe, chain)
        m = midas_for(k)
        res = pipe.step(fl, fr, m)
        exp = chain.step(fl, fr, m)
        _same(res, exp, names, f"{tag} frame {k}")
        assert pipe.frame_counter == chain.loop.frame_counter == len(out) + 1
        out.append(res)
    return out


# ------------------------------------------------------------------------------------------
# 1. whole-step equality, small
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("midas_shape", [None, (PH, PW), (40, 50)], ids=["no_midas", "midas", "midas_40x50"])
def test_step_equals_the_chain(engine, clock, midas_shape):
    calib = _calibration(CW, CH, 0.5)
    assert calib["img_size_proc"] == (PW, PH)
    pipe = FusionFramePipeline(calib, engine=engine, outputs=OUTPUT_NAMES, **STEREO)
    chain = C.HostChain(calib, **STEREO)
    midas_for = (lambda k: None) if midas_shape is None else \
        (lambda k: (_midas(midas_shape, k), np.ones(midas_shape, np.float32)) if k % 2 else _midas(midas_shape, k))
    res = _run(pipe, chain, _frames(), clock, midas_for, tag=str(midas_shape))
    # no dead branch: the flow returns nothing on the first frame and a map on two frames at least,
    # stereo runs, the fuse runs, the MiDaS map exists exactly when one was given
    assert res[0].flow_depth_raw is None and res[0].flow_depth_normalized is None
    assert sum(r.flow_depth_raw is not None for r in res) >= 2
    assert all(r.use_stereo and r.source == "left" and r.occlusion_state == "none" for r in res)
    assert all(r.fused_u8 is not None and r.fused_u8.shape == (PH, PW) and r.fused_colormap.shape == (PH, PW, 3)
               for r in res)
    assert all(r.stereo_disparity.max() > 0 and r.processed_left.shape == (PH, PW, 3) for r in res)
    assert all((r.midas_calibrated is not None) == (midas_shape is not None) for r in res)
    assert any("Flow_fill" in r.mode_text or r.camera_moving for r in res[1:])
    # the device maps of the last step: pointer, shape, dtype
    ptr, shape, dt = res[-1].device("fused_u8")
    assert shape == (PH, PW) and dt == np.uint8
    np.testing.assert_array_equal(engine.to_host(ptr, shape, dt), res[-1].fused_u8)
    ptr, shape, dt = res[-1].device("stereo_conf")
    np.testing.assert_array_equal(engine.to_host(ptr, shape, dt), res[-1].stereo_conf)
    pipe.close()


# ------------------------------------------------------------------------------------------
# 2. branch cases at the same size
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_calib", [True, False], ids=["calibration", "default_640x480"])
def test_without_rectification(engine, clock, with_calib):
    calib = _calibration(CW, CH, 0.5) if with_calib else None
    pipe = FusionFramePipeline(calib, use_rectify=False, engine=engine, outputs=OUTPUT_NAMES, **STEREO)
    chain = C.HostChain(calib, use_rectify=False, **STEREO)
    res = _run(pipe, chain, _frames()[:3], clock, tag="no rectify")
    assert res[0].processed_left.shape == ((PH, PW, 3) if with_calib else (480, 640, 3))
    assert res[0].fused_u8 is not None
    pipe.close()


def test_covered_left_camera(engine, clock):
    calib = _calibration(CW, CH, 0.5)
    frames = C.moving_stereo_sequence(CH, CW, 22, disparity=8)
    flat = np.full((CH, CW, 3), 117, np.uint8)
    seq = [(flat, fr) for _, fr in frames[:12]] + frames[12:]
    pipe = FusionFramePipeline(calib, engine=engine, outputs=OUTPUT_NAMES, **STEREO)
    chain = C.HostChain(calib, **STEREO)
    res = _run(pipe, chain, seq, clock, lambda k: _midas((PH, PW), k), tag="covered")
    # checks fall on frames 0, 2, 4, 6, 8: the fifth 'left' in a row confirms the change
    assert [r.occlusion_state for r in res[:12]] == ["none"] * 8 + ["left"] * 4
    assert [r.use_stereo for r in res[:12]] == [True] * 8 + [False] * 4
    assert [r.source for r in res[:12]] == ["left"] * 8 + ["right"] * 4
    assert res[8].left_score > 0.45 > res[8].right_score
    # the flow restarts on nothing: the right camera has the same size, so the estimator goes on
    covered = [r for r in res[8:12]]
    assert all(r.stereo_disparity is not None and not r.stereo_disparity.any() and not r.stereo_conf.any()
               for r in covered)                                             # the reference's zero maps
    assert any(r.flow_depth_raw is not None for r in covered)
    for k, r in enumerate(covered, 8):
        # the no-stereo normalisations (:2749-2759, :2809-2811) are the ones used
        if r.flow_depth_raw is not None:
            np.testing.assert_array_equal(
                r.flow_depth_normalized, 255.0 - np.clip(r.flow_depth_raw * 255.0, 0, 255).astype(np.float32))
        m = _midas((PH, PW), k)
        nrm = np.clip(((m - m.min()) / (m.max() - m.min() + 1e-8)) * 255.0, 0, 255).astype(np.float32)
        np.testing.assert_array_equal(r.midas_calibrated, fusion.bilateral_filter(nrm, 5, 50, 50))
        assert r.mode_text.startswith("MiDaS_base")
    # uncovered from frame 12: checks on 12, 14, 16, 18, 20 -> back on frame 20
    assert [r.occlusion_state for r in res[12:]] == ["left"] * 8 + ["none"] * 2
    assert [r.use_stereo for r in res[12:]] == [False] * 8 + [True] * 2
    assert [r.source for r in res[12:]] == ["right"] * 8 + ["left"] * 2
    assert res[20].stereo_disparity.max() > 0 and res[20].mode_text.startswith("Stereo")
    pipe.close()


@pytest.mark.parametrize("case", ["use_flow_off", "show_fused_off", "all_off", "manual_stereo_off"])
def test_switches(engine, clock, case):
    calib = _calibration(CW, CH, 0.5)
    pipe = FusionFramePipeline(calib, engine=engine, outputs=OUTPUT_NAMES, **STEREO)
    chain = C.HostChain(calib, **STEREO)
    if case in ("use_flow_off", "all_off"):
        pipe.use_flow = chain.USE_OPTICAL_FLOW = False
    if case == "show_fused_off":
        pipe.show_fused = chain.show_fused_depth = False
    if case in ("all_off", "manual_stereo_off"):
        pipe.use_stereo = chain.loop.USE_STEREO = False
    if case == "all_off":
        pipe.use_midas = chain.USE_MIDAS = False
    res = _run(pipe, chain, _frames()[:4], clock, lambda k: _midas((PH, PW), k), tag=case)
    if case == "use_flow_off":
        assert all(r.flow_depth_raw is None and r.camera_moving is False and r.fused_u8 is not None for r in res)
    if case == "show_fused_off":
        assert all(r.fused_u8 is None and r.fused_colormap is None and r.mode_text is None and r.range is None
                   for r in res)
        assert any(r.flow_depth_normalized is not None for r in res)
    if case == "all_off":
        assert all(r.fused_u8 is None and r.fused_colormap is None and r.midas_calibrated is None for r in res)
        assert all(r.device("fused_u8") is None for r in res)
    if case == "manual_stereo_off":
        assert all(not r.use_stereo and r.mode_text.startswith("MiDaS_base") for r in res)
        assert any(r.flow_depth_normalized is not None for r in res)
    pipe.close()


def test_frame_size_change_resets_the_estimator(engine, clock):
    big, small = _calibration(CW, CH, 0.5), _calibration(CW, CH, 0.45, seed=1)
    assert small["img_size_proc"] == (108, 79)            # 5 x 7 grid points, as at 88 x 120
    pipe = FusionFramePipeline(big, engine=engine, outputs=OUTPUT_NAMES, **STEREO)
    chain = C.HostChain(big, **STEREO)

    def swap(k, pipe, chain):
        if k == 3:
            pipe.stereo_calib = chain.stereo_calib = small
        if k == 5:
            pipe.stereo_calib = chain.stereo_calib = big

    res = _run(pipe, chain, _frames(), clock, tag="size change", before=swap)
    assert [r.processed_left.shape[:2] for r in res] == [(PH, PW)] * 3 + [(79, 108)] * 2 + [(PH, PW)]
    assert res[2].flow_depth_raw is not None
    assert res[3].flow_depth_raw is None and res[5].flow_depth_raw is None        # the estimator starts again
    assert res[4].flow_depth_raw is not None and res[4].flow_depth_raw.shape == (79, 108)
    pipe.close()


# ------------------------------------------------------------------------------------------
# 3. the new kernels alone
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(50, 50), (88, 120), (57, 131), (8, 8)])
def test_flow_grid(engine, shape):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    flow = rng.standard_normal((H, W, 2)).astype(np.float32)
    ys, xs = np.mgrid[8:H:16, 8:W:16]
    exp = flow[ys.ravel(), xs.ravel()]
    # (8 x 8 has no point on the step-16 grid, whose first point is (8, 8): nothing is launched)
    assert len(exp) == {(50, 50): 9, (88, 120): 35, (57, 131): 32, (8, 8): 0}[shape]
    d_flow = engine.upload("t_fg_flow", flow)
    d_out = engine.scratch("t_fg_out", 8 * max(len(exp), 1) + 64)
    guard = np.full(2 * len(exp) + 16, np.float32(-7.0))
    engine.to_device(d_out, guard)
    ny, nx = engine.flow_grid_dev(d_flow, H, W, 16, d_out)
    assert (ny, nx) == ys.shape
    got = engine.to_host(d_out, (2 * len(exp) + 16,), np.float32)
    np.testing.assert_array_equal(got[:2 * len(exp)].reshape(-1, 2), exp)
    assert (got[2 * len(exp):] == np.float32(-7.0)).all()                        # nothing past the grid


def test_flow_grid_one_point_and_edges(engine):
    # 8 x 8 with step 16 has no point at (8, 8); step 8 has exactly one, at (4, 4)
    flow = np.arange(8 * 8 * 2, dtype=np.float32).reshape(8, 8, 2)
    d_flow = engine.upload("t_fg_flow", flow)
    d_out = engine.scratch("t_fg_out", 256)
    assert engine.flow_grid_dev(d_flow, 8, 8, 8, d_out) == (1, 1)
    np.testing.assert_array_equal(engine.to_host(d_out, (1, 2), np.float32), flow[4:5, 4])
    # 57 x 131: the last grid row (56) and column (120) lie at the edge and before it
    ys, xs = np.mgrid[8:57:16, 8:131:16]
    assert ys.max() == 56 and xs.max() == 120


@pytest.mark.parametrize("n", [1, 63, 64, 65, PH * PW])
def test_affine_modes(engine, n):
    rng = np.random.default_rng(n)
    x = (rng.random(n, dtype=np.float32) * np.float32(3.0) - np.float32(1.0)).astype(np.float32)   # [-1, 2)
    if n > 2:
        x[1], x[2] = np.float32(-2.0), np.float32(5.0)                      # both clip ends
    d_x = engine.upload("t_aff_x", x)
    d_out = engine.scratch("t_aff_out", 4 * n + 16)

    def run(mode, **kw):
        engine.affine_f32_dev(d_x, n, mode, d_out, **kw)
        return engine.to_host(d_out, (n,), np.float32)

    fa, fb, fc, fd = np.float32(0.25), np.float32(1.7), np.float32(3.5), np.float32(91.0)
    np.testing.assert_array_equal(run(fusion.AFF_F32_INV, fa=fa, fb=fb, fc=fc, fd=fd),
                                  np.float32(255.0) - (fc + ((x - fa) / fb) * fd))
    np.testing.assert_array_equal(run(fusion.AFF_F32_INV, fa=fa, fb=fb, fc=fc, fd=fd),
                                  np.float32(255.0) - run(fusion.AFF_F32, fa=fa, fb=fb, fc=fc, fd=fd))
    np.testing.assert_array_equal(run(fusion.AFF_CLIP255_INV),
                                  255.0 - np.clip(x * 255.0, 0, 255).astype(np.float32))
    mn, mx = x.min(), x.max()
    den = np.float32(mx - mn + 1e-8)
    np.testing.assert_array_equal(run(fusion.AFF_NORM_CLIP255, fa=mn, fb=den),
                                  np.clip(((x - mn) / den) * 255.0, 0, 255).astype(np.float32))
    # a normalisation whose range does not cover the data clips at both ends
    got = run(fusion.AFF_NORM_CLIP255, fa=np.float32(0.0), fb=np.float32(1.0))
    np.testing.assert_array_equal(got, np.clip((x / np.float32(1.0)) * 255.0, 0, 255).astype(np.float32))
    if n > 2:
        assert got[1] == 0.0 and got[2] == 255.0
    # the existing modes are untouched
    np.testing.assert_array_equal(run(fusion.AFF_F64, ds=1.5, doff=-2.0),
                                  (x.astype(np.float64) * 1.5 - 2.0).astype(np.float32))
    np.testing.assert_array_equal(run(fusion.AFF_FILL, fc=fc), np.full(n, fc))
    with pytest.raises(Exception):
        run(6)


def test_minmax_normalize_degenerate_range(engine):
    # max - min < 1e-6: the reference's zeros (:2755-2756); and the regular case at one size
    for n in (1, 65, PH * PW):
        x = np.full(n, np.float32(3.25))
        if n > 1:
            x[n // 2] += np.float32(2e-7)
        d_x = engine.upload("t_mm_x", x)
        d_out = engine.scratch("t_mm_out", 4 * n)
        mn, mx = fusion.minmax_normalize_dev(engine, d_x, n, d_out)
        assert (mn, mx) == (x.min(), x.max()) and not mx > mn + 1e-6
        np.testing.assert_array_equal(engine.to_host(d_out, (n,), np.float32), np.zeros(n, np.float32))
    x = _midas((PH, PW), 3).ravel()
    x[5] = np.float32(np.nan)                                               # NaN: np.min / np.max are NaN -> zeros
    d_x = engine.upload("t_mm_x", x)
    mn, mx = fusion.minmax_normalize_dev(engine, d_x, x.size, d_out)
    assert np.isnan(mn) and np.isnan(mx)
    np.testing.assert_array_equal(engine.to_host(d_out, (x.size,), np.float32), np.zeros(x.size, np.float32))


def test_copy_counters(engine):
    engine.copy_counters(reset=True)
    a = np.arange(1000, dtype=np.float32)
    d = engine.upload("t_cc", a)
    engine.to_host(d, (1000,), np.float32)
    engine.to_host(d, (10,), np.float32)
    c = engine.copy_counters()
    assert c == {"h2d_bytes": 4000, "h2d_calls": 1, "d2h_bytes": 4040, "d2h_calls": 2}
    sel, _ = engine.select_count(d, 1000)                                    # a scalar read-back counts
    c2 = engine.copy_counters(reset=True)
    assert sel == 1000 and c2["d2h_calls"] == 3 and 0 < c2["d2h_bytes"] - 4040 <= 64
    assert engine.copy_counters() == {"h2d_bytes": 0, "h2d_calls": 0, "d2h_bytes": 0, "d2h_calls": 0}


# ------------------------------------------------------------------------------------------
# 4. the app size
# ------------------------------------------------------------------------------------------
def test_app_size_and_transfer_cap(engine, clock):
    H, W = 356, 633
    calib = _calibration(W, H, 1.0, seed=2)
    assert calib["img_size_proc"] == (W, H)
    frames = C.moving_stereo_sequence(H, W, 5, disparity=20, step=(2.0, 1.0))
    stereo = dict(min_disp=0, num_disp=96, window_size=5)
    pipe = FusionFramePipeline(calib, engine=engine, outputs=OUTPUT_NAMES, **stereo)
    chain = C.HostChain(calib, **stereo)
    res = _run(pipe, chain, frames[:4], clock, tag="app size")              # frames 2 and 3: steady state
    assert res[2].flow_depth_raw is not None and res[3].flow_depth_raw is not None
    assert res[3].fused_u8.shape == (H, W)
    # one steady-state step (a frame with the occlusion check), only fused_u8 asked for
    pipe.outputs = ("fused_u8",)
    clock[0] += 0.1
    fl, fr = frames[4]
    engine.copy_counters(reset=True)
    r = pipe.step(fl, fr)
    got = engine.copy_counters(reset=True)
    exp = chain.step(fl, fr)
    ref = engine.copy_counters(reset=True)
    _same(r, exp, ("fused_u8",), "app size frame 4")
    assert r.device("flow_depth_normalized") is not None and r.stereo_depth is None
    allowance = H * W                                                        # one u8 map, 225 KB
    print(f"pipeline per frame: {got}; chain per frame: {ref}")
    assert got["h2d_bytes"] - (fl.nbytes + fr.nbytes) < allowance, got
    assert got["d2h_bytes"] - r.fused_u8.nbytes < allowance, got
    # the cap discriminates: the chain moves more than ten allowances each way beyond the same payload
    assert ref["h2d_bytes"] - (fl.nbytes + fr.nbytes) > 10 * allowance, ref
    assert ref["d2h_bytes"] - r.fused_u8.nbytes > 10 * allowance, ref
    pipe.close()
