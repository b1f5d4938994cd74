"""The refinement stage of the SAD / SSD / HOG maps on the GPU (sv_refine.hip):
every map array_equal to the NumPy restatement tests/sv_refine_oracle.py — the right-referenced
map, k_refine in both its forms, adversarial inputs, the composition up to the drop-ins and the
frame pipeline, and the argument checks."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("SV_WARMUP_AT_IMPORT", "0")
import sv_oracle as O  # noqa: E402
import sv_refine_oracle as RO  # noqa: E402
from stereovision_amd import colormap  # noqa: E402
from stereovision_amd import depth_map as DM  # noqa: E402
from stereovision_amd import engine as E  # noqa: E402
from stereovision_amd import fused_depth_map as FDM  # noqa: E402
from stereovision_amd.engine import RefineParams, SVError  # noqa: E402

pytestmark = pytest.mark.gpu

COSTS = {"sad": O.COST_SAD, "ssd": O.COST_SSD, "hog": O.COST_HOG}
# (H, W, numD, win, minD): odd widths (pitches that are no multiple of 4), a window of every size
# class, negative / zero / positive minD, and the split ring kind of the matcher (D > 256)
SHAPES = [(20, 33, 16, 3, 0), (40, 97, 16, 9, -3), (41, 130, 32, 15, 5), (24, 352, 272, 5, 0)]
SMALL = (5, 70, 16, 9, 0)            # H < win, the second tile a partial one
SENTINEL = 12345                     # what the padding columns of a pitched map hold


@functools.lru_cache(maxsize=None)
def pair(H, W, numD, minD, seed=0):
    """A textured pair at disparity minD + numD // 3 with noise on the right frame.  Inside the
    matched band, the last third is nearly flat (costs tie, curvatures are small) and the right
    frame shows something else where the second quarter should be (the L-R check has work)."""
    rng = np.random.default_rng(seed + 7 * H + W)
    d = minD + numD // 3
    pad = abs(d) + 2
    x0, x1 = O.valid_columns(W, minD, numD)
    bw = x1 - x0
    bg = rng.integers(0, 256, (H, W + 2 * pad)).astype(np.int64)
    flat0 = pad + x1 - bw // 3
    bg[:, flat0:] = 120 + rng.integers(0, 3, (H, W + 2 * pad - flat0))
    L = bg[:, pad:pad + W]
    R = bg[:, pad + d:pad + d + W] + rng.integers(-6, 7, (H, W))
    c0, c1 = np.clip([x0 + bw // 4 - d, x0 + bw // 2 - d], 0, W)
    R[H // 3:H // 3 * 2, c0:c1] = rng.integers(0, 256, (H // 3 * 2 - H // 3, c1 - c0))
    return np.clip(L, 0, 255).astype(np.uint8), np.clip(R, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def ref_maps(shape, cost):
    H, W, numD, win, minD = shape
    L, R = pair(H, W, numD, minD)
    return (O.disparity16(L, R, minD, numD, win, COSTS[cost]),
            RO.disparity16_right(L, R, minD, numD, win, COSTS[cost]))


def curvature_threshold(win, cost):
    """Between the curvature of the nearly flat third (pixel noise of amplitude 2) and of the
    texture: 3 per window pixel for SAD, 12 for SSD."""
    return win * win * (3 if cost == "sad" else 12)


def param_sets(win, cost):
    k = curvature_threshold(win, cost)
    return {"lr": RefineParams(1, 0, False), "curvature": RefineParams(-1, k, False),
            "subpixel": RefineParams(-1, 0, True), "all": RefineParams(1, k, True)}


def oracle_refine(L, R, dl, dr, shape, cost, p):
    _, _, numD, win, minD = shape
    return RO.refine(L, R, dl, minD, numD, win, COSTS[cost], dr, p.lr_max_diff, p.min_curvature, p.subpixel,
                     p.speckle_window, p.speckle_range)


def pitched(a, pitch, fill=SENTINEL):
    out = np.full((a.shape[0], pitch), fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


def gpu_refine(eng, L, R, dl, dr, shape, cost, p, inplace=True, opitch=None, ipitch=None):
    """sv_refine_dev on device buffers -> the H x W result; the padding of a pitched output must
    come back untouched."""
    H, W, numD, win, minD = shape
    opitch, ipitch = opitch or W, ipitch or W
    d_l, d_r = eng.upload("t_l", pitched(L, ipitch, 0)), eng.upload("t_r", pitched(R, ipitch, 0))
    d_in = eng.upload("t_in", pitched(dl, opitch))
    d_dr = eng.upload("t_dr", pitched(dr, opitch)) if dr is not None else 0
    d_out = d_in if inplace else eng.upload("t_out", np.full((H, opitch), SENTINEL, np.int16))
    eng.refine_dev(d_l, d_r, H, W, ipitch, d_in, d_dr, minD, numD, win, cost, p, d_out, opitch)
    out = eng.to_host(d_out, (H, opitch), np.int16)
    assert (out[:, W:] == SENTINEL).all()
    if not inplace:   # the input map is read only
        np.testing.assert_array_equal(eng.to_host(d_in, (H, opitch), np.int16)[:, :W], dl)
    return np.ascontiguousarray(out[:, :W])


# ------------------------------------------------------------------------------------------
# 1. the right-referenced map
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,cost", [(s, c) for s in SHAPES for c in ("sad", "ssd")] + [(SHAPES[1], "hog")],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_right_map(engine, shape, cost):
    H, W, numD, win, minD = shape
    L, R = pair(H, W, numD, minD)
    exp = ref_maps(shape, cost)[1]
    np.testing.assert_array_equal(engine.disparity_right(L, R, minD, numD, win, cost), exp)
    x0, x1 = RO.right_valid_columns(W, minD, numD)
    inv = (minD - 1) * 16
    assert (exp[:, :x0] == inv).all() and (exp[:, x1:] == inv).all() and (exp[:, x0:x1] != inv).all()
    # pitched in and out (an odd input pitch), and the frames are left as they were
    ip, op = W + 3, W + 5
    d_l, d_r = engine.upload("t_l", pitched(L, ip, 0)), engine.upload("t_r", pitched(R, ip, 0))
    d_out = engine.upload("t_out", np.full((H, op), SENTINEL, np.int16))
    engine.disparity_right_dev(d_l, d_r, H, W, ip, minD, numD, win, cost, d_out, op)
    out = engine.to_host(d_out, (H, op), np.int16)
    np.testing.assert_array_equal(out[:, :W], exp)
    assert (out[:, W:] == SENTINEL).all()
    np.testing.assert_array_equal(engine.to_host(d_l, (H, ip), np.uint8)[:, :W], L)


# ------------------------------------------------------------------------------------------
# 2. k_refine on the matcher's maps
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("shape", SHAPES + [SMALL], ids=lambda s: "x".join(map(str, s)))
def test_refine_matched_maps(engine, shape, cost):
    H, W, numD, win, minD = shape
    L, R = pair(H, W, numD, minD)
    dl, dr = ref_maps(shape, cost)
    inv = (minD - 1) * 16
    assert E.refine_plan(numD, win)["form"] == "lds"
    for name, p in param_sets(win, cost).items():
        for right in (dr, None):
            exp = oracle_refine(L, R, dl, right, shape, cost, p)
            got = gpu_refine(engine, L, R, dl, right, shape, cost, p, inplace=True)
            np.testing.assert_array_equal(got, exp, err_msg=f"{name} right={right is not None} in place")
            got = gpu_refine(engine, L, R, dl, right, shape, cost, p, inplace=False, opitch=W + 3, ipitch=W + 1)
            np.testing.assert_array_equal(got, exp, err_msg=f"{name} right={right is not None} pitched")
        # no dead case: with its right map every set but the sub-pixel one rejects pixels and keeps pixels
        exp = oracle_refine(L, R, dl, dr, shape, cost, p)
        band = exp[:, slice(*O.valid_columns(W, minD, numD))]
        if band.size:
            assert (band != inv).any(), name
            if name != "subpixel":
                assert (band == inv).any(), name
            else:
                assert (band % 16 != 0).any(), name


def test_refine_hog_takes_the_check_and_the_speckles(engine):
    shape = SHAPES[1]
    H, W, numD, win, minD = shape
    L, R = pair(H, W, numD, minD)
    dl, dr = ref_maps(shape, "hog")
    p = RefineParams(1, 0, False, speckle_window=12, speckle_range=1)
    exp = oracle_refine(L, R, dl, dr, shape, "hog", p)
    np.testing.assert_array_equal(gpu_refine(engine, L, R, dl, dr, shape, "hog", p), exp)
    np.testing.assert_array_equal(engine.disparity_refined(L, R, minD, numD, win, "hog", p), exp)
    assert (exp == (minD - 1) * 16).any() and (exp != (minD - 1) * 16).any()


# ------------------------------------------------------------------------------------------
# 3. adversarial inputs
# ------------------------------------------------------------------------------------------
def handed_in_maps(H, W, minD, numD, seed=1):
    rng = np.random.default_rng(seed)
    inv, dmax = (minD - 1) * 16, minD + numD - 1
    rnd = (rng.integers(minD, dmax + 1, (H, W)) * 16).astype(np.int16)
    return {"random": rnd, "low end": np.full((H, W), minD * 16, np.int16),
            "high end": np.full((H, W), dmax * 16, np.int16),
            "holes": np.where(rng.random((H, W)) < 0.3, inv, rnd).astype(np.int16),
            "fractions": (rnd + rng.integers(0, 16, (H, W))).astype(np.int16),
            "junk": rng.integers(-32768, 32768, (H, W)).astype(np.int16)}


@pytest.mark.parametrize("cost", ["sad", "ssd"])
@pytest.mark.parametrize("shape", [(23, 97, 16, 9, -3), (9, 70, 1, 5, 2)], ids=lambda s: "x".join(map(str, s)))
def test_handed_in_maps(engine, shape, cost):
    H, W, numD, win, minD = shape
    L, R = pair(H, W, numD, minD)
    dr = RO.disparity16_right(L, R, minD, numD, win, COSTS[cost])
    p_all = RefineParams(1, curvature_threshold(win, cost), True)
    p_sub = RefineParams(-1, 0, True)
    for name, m in handed_in_maps(H, W, minD, numD).items():
        for p in (p_all, p_sub):
            exp = oracle_refine(L, R, m, dr, shape, cost, p)
            np.testing.assert_array_equal(gpu_refine(engine, L, R, m, dr, shape, cost, p), exp, err_msg=name)
            # totality: invalid, or within half a disparity of the value handed in
            live = exp != (minD - 1) * 16
            assert (np.abs(exp.astype(np.int64) - m)[live] <= 8).all(), name


def test_stripes_ssd_win15(engine):
    """0 / 255 stripes of period 6 under SSD at win 15: the largest costs the stage meets.  The
    sub-pixel numerator (cm - cp) * 256 passes 2^30 here and its bound 225 * 65025 * 256 passes
    2^31, which is why the quotient is taken in 64 bits."""
    H, W, numD, win, minD = 17, 80, 6, 15, 0
    shape = (H, W, numD, win, minD)
    x = np.arange(W)
    L = np.tile(np.where(x % 6 < 3, 255, 0).astype(np.uint8), (H, 1))
    p = RefineParams(-1, 0, True)
    for pat in ((0, 0, 0, 0, 0, 255), (255, 255, 0, 0, 0, 255)):
        R = np.tile(np.array(pat, np.uint8)[x % 6], (H, 1))
        top = 0
        for d in range(numD):
            m = np.full((H, W), d * 16, np.int16)
            exp = oracle_refine(L, R, m, None, shape, "ssd", p)
            np.testing.assert_array_equal(gpu_refine(engine, L, R, m, None, shape, "ssd", p), exp, err_msg=f"{pat} d={d}")
            dm = np.full((H, W), d)
            cm = RO.window_cost(L, R, np.maximum(dm - 1, 0), win, O.COST_SSD)
            cp = RO.window_cost(L, R, np.minimum(dm + 1, numD - 1), win, O.COST_SSD)
            top = max(top, int(np.abs(cm - cp).max()) * 256)
        if pat == (0, 0, 0, 0, 0, 255):
            assert top > 2 ** 30
    exp = RO.disparity_refined(L, R, minD, numD, win, O.COST_SSD)
    np.testing.assert_array_equal(engine.disparity_refined(L, R, minD, numD, win, "ssd", RefineParams()), exp)


@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_uncorrelated_noise_and_flat_frames(engine, cost):
    H, W, numD, win, minD = 21, 90, 16, 5, 0
    rng = np.random.default_rng(9)
    L = rng.integers(0, 256, (H, W)).astype(np.uint8)
    R = rng.integers(0, 256, (H, W)).astype(np.uint8)
    inv = (minD - 1) * 16
    exp = RO.disparity_refined(L, R, minD, numD, win, COSTS[cost])
    np.testing.assert_array_equal(engine.disparity_refined(L, R, minD, numD, win, cost, RefineParams()), exp)
    band = exp[:, numD:]
    assert (band == inv).mean() > 0.3            # a large share of the pixels is rejected (0.42 / 0.44)
    flat = np.full((H, W), 97, np.uint8)
    for k in (1, 0):
        p = RefineParams(1, k, True)
        exp = RO.disparity_refined(flat, flat, minD, numD, win, COSTS[cost], min_curvature=k)
        np.testing.assert_array_equal(engine.disparity_refined(flat, flat, minD, numD, win, cost, p), exp)
        assert (exp[:, numD:] == (inv if k else minD * 16)).all()


def test_both_forms_of_the_kernel(engine):
    """The staged (LDS) form and the global-tap form, told apart by the plan query: (512, 15)
    needs 12 KiB of strips, beyond the block's budget; (16, 15) and (272, 5) fit."""
    assert E.refine_plan(512, 15)["form"] == "global" and E.refine_plan(512, 15)["lds_bytes"] > 8192
    assert E.refine_plan(16, 15)["form"] == "lds" and E.refine_plan(272, 5)["form"] == "lds"
    p = RefineParams(-1, 15 * 15 * 3, True)
    for numD, form in ((512, "global"), (16, "lds")):
        shape = (21, 150, numD, 15, -200 if numD == 512 else 0)
        H, W, _, win, minD = shape
        assert E.refine_plan(numD, win)["form"] == form
        L, R = pair(H, W, 16, 0, seed=3)
        for name, m in handed_in_maps(H, W, minD, numD, seed=2).items():
            exp = oracle_refine(L, R, m, None, shape, "sad", p)
            np.testing.assert_array_equal(gpu_refine(engine, L, R, m, None, shape, "sad", p, opitch=W + 1), exp,
                                          err_msg=f"{form} {name}")


# ------------------------------------------------------------------------------------------
# 4. composition
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_disparity_refined_is_the_chain_of_its_pieces(engine, cost):
    shape = SHAPES[1]
    H, W, numD, win, minD = shape
    L, R = pair(H, W, numD, minD)
    p = RefineParams(1, curvature_threshold(win, cost), True, speckle_window=20, speckle_range=2)
    got = engine.disparity_refined(L, R, minD, numD, win, cost, p)
    dl = engine.disparity(L, R, minD, numD, win, cost)
    dr = engine.disparity_right(L, R, minD, numD, win, cost)
    np.testing.assert_array_equal(dl, ref_maps(shape, cost)[0])
    plain = engine.refine(L, R, dl, minD, numD, win, cost, RefineParams(1, p.min_curvature, True), disp16_right=dr)
    inv = (minD - 1) * 16
    np.testing.assert_array_equal(got, engine.filter_speckles(plain, inv, 20, 32))
    np.testing.assert_array_equal(got, oracle_refine(L, R, dl, dr, shape, cost, p))
    assert (plain != got).any()                  # the speckle filter removed something
    # BGR input takes the gray conversion first
    from stereovision_amd.synthetic import to_bgr
    np.testing.assert_array_equal(engine.disparity_refined(to_bgr(L), to_bgr(R), minD, numD, win, cost, p), got)
    # without the check no right map is computed
    q = RefineParams(-1, p.min_curvature, True)
    np.testing.assert_array_equal(engine.disparity_refined(L, R, minD, numD, win, cost, q),
                                  oracle_refine(L, R, dl, None, shape, cost, q))


@pytest.mark.parametrize("cost", ["sad", "ssd", "hog"])
def test_drop_ins_with_refine(engine, monkeypatch, cost):
    from stereovision_amd.synthetic import to_bgr
    H, W, numD, win, minD = 40, 97, 16, 5, 0
    L, R = pair(H, W, numD, minD)
    p = RefineParams(1, 0, False, 12, 1) if cost == "hog" else \
        RefineParams(1, curvature_threshold(win, cost), True, speckle_window=12, speckle_range=1)
    d16 = RO.disparity_refined(L, R, minD, numD, win, COSTS[cost], p.lr_max_diff, p.min_curvature, p.subpixel,
                               p.speckle_window, p.speckle_range)
    disparity = O.disparity_f32(d16)
    for mod in (DM, FDM):
        monkeypatch.setattr(mod, "get_engine", lambda: engine)
        monkeypatch.setattr(mod, "COST", cost)
        monkeypatch.setattr(mod, "REFINE", p)
    monkeypatch.setattr(DM, "MIN_DISP", minD)
    monkeypatch.setattr(DM, "NUM_DISP", numD)
    monkeypatch.setattr(DM, "WINDOW_SIZE", win)
    dn, disp, cmap, conf = FDM.create_depth_map_stereo_scaled(to_bgr(L), to_bgr(R), minD, numD, win)
    e_dn, e_u8, e_conf = O.scaled_post(disparity, minD, numD)
    np.testing.assert_array_equal(disp, disparity)
    np.testing.assert_array_equal(dn, e_dn)
    np.testing.assert_array_equal(conf, e_conf)
    e_cmap = colormap.apply(e_u8, "jet")
    colormap.put_text(e_cmap, f"Scale:{FDM.PROCESSING_SCALE:.2f}x Disp:{numD}px")
    np.testing.assert_array_equal(cmap, e_cmap)
    assert (conf == 0).any() and (conf == 1).any()          # the stage made invalid pixels
    depth, disp, cmap = DM.create_depth_map(L, R, None, 0.2, 4.0)
    e_depth, e_norm = O.depth_post(disparity, 0.2, 4.0, minD)
    np.testing.assert_array_equal(disp, disparity)
    np.testing.assert_array_equal(depth, e_depth)
    np.testing.assert_array_equal(cmap, colormap.apply(e_norm, "turbo"))
    # None: today's path
    monkeypatch.setattr(FDM, "REFINE", None)
    dn, disp, cmap, conf = FDM.create_depth_map_stereo_scaled(L, R, minD, numD, win)
    e = O.create_depth_map_stereo_scaled(L, R, minD, numD, win, COSTS[cost])
    np.testing.assert_array_equal(disp, e[1])
    np.testing.assert_array_equal(conf, e[3])


def test_frame_pipeline_with_refine(engine, monkeypatch):
    import frame_chain as C
    from stereovision_amd import flow as F
    from stereovision_amd.frame import OUTPUT_NAMES, FusionFramePipeline
    now = [1000.0]
    monkeypatch.setattr(F.time, "time", lambda: now[0])
    p = RefineParams(1, 5 * 5 * 3, True, speckle_window=20, speckle_range=2)
    monkeypatch.setattr(FDM, "get_engine", lambda: engine)
    monkeypatch.setattr(FDM, "REFINE", p)               # the chain's drop-ins read the global
    stereo = dict(min_disp=0, num_disp=16, window_size=5)
    calib = {"img_size_proc": (64, 48)}
    pipe = FusionFramePipeline(calib, use_rectify=False, engine=engine, outputs=OUTPUT_NAMES, refine=p, **stereo)
    chain = C.HostChain(calib, use_rectify=False, **stereo)
    seen_invalid = False
    for k, (fl, fr) in enumerate(C.moving_stereo_sequence(48, 64, 6, disparity=5)):
        now[0] += 0.1
        res, exp = pipe.step(fl, fr), chain.step(fl, fr)
        for s in C.SCALARS:
            assert getattr(res, s) == exp[s], (k, s)
        for name in OUTPUT_NAMES:
            got, e = getattr(res, name), exp[name]
            assert (got is None) == (e is None), (k, name)
            if e is not None:
                np.testing.assert_array_equal(got, e, err_msg=f"frame {k}: {name}")
        seen_invalid |= bool((res.stereo_conf[:, 16:] == 0).any())
        assert (res.stereo_disparity * 16 % 16 != 0).any()   # sub-pixel values reach the outputs
    assert seen_invalid
    pipe.close()


# ------------------------------------------------------------------------------------------
# 5. argument checks: SV_EINVAL before any launch
# ------------------------------------------------------------------------------------------
def test_argument_checks(engine):
    H, W, numD, win, minD = 12, 40, 16, 5, 0
    L, R = pair(H, W, numD, minD)
    d_l, d_r = engine.upload("t_l", L), engine.upload("t_r", R)
    d_m = engine.upload("t_in", np.zeros((H, W), np.int16))
    d_o = engine.upload("t_out", np.full((H, W), SENTINEL, np.int16))
    d_dr = engine.upload("t_dr", np.zeros((H, W), np.int16))
    ok = RefineParams()
    engine.profile(True)
    before = {k: engine.profile_read(k)[1] for k in ("flip", "refine", "match", "speckle", "hog")}

    def bad(fn, *a, **kw):
        with pytest.raises(SVError) as ei:
            fn(*a, **kw)
        assert ei.value.code == -22 and E.last_error()

    def refine(l=d_l, r=d_r, pitch=W, m=d_m, dr=d_dr, mind=minD, nd=numD, w=win, cost="sad", p=ok, o=d_o, op=W):
        engine.refine_dev(l, r, H, W, pitch, m, dr, mind, nd, w, cost, p, o, op)

    def right(l=d_l, r=d_r, pitch=W, mind=minD, nd=numD, w=win, cost="sad", o=d_o, op=W):
        engine.disparity_right_dev(l, r, H, W, pitch, mind, nd, w, cost, o, op)

    def chain(l=d_l, r=d_r, pitch=W, mind=minD, nd=numD, w=win, cost="sad", p=ok, o=d_o, op=W):
        engine.disparity_refined_dev(l, r, H, W, pitch, mind, nd, w, cost, p, o, op)

    for fn in (refine, right, chain):
        bad(fn, l=0)
        bad(fn, r=0)
        bad(fn, o=0)
        bad(fn, pitch=W - 1)
        bad(fn, op=W - 1)
        bad(fn, mind=-2048)
        bad(fn, mind=2040, nd=16)
        bad(fn, w=4)
        bad(fn, w=17)
        bad(fn, nd=0)
        bad(fn, cost="sgbm")
    bad(refine, m=0)
    bad(refine, dr=d_o)                                     # the right map refined in place
    for fn in (refine, chain):
        bad(fn, cost="hog", p=RefineParams(1, 0, True))
        bad(fn, cost="hog", p=RefineParams(1, 1, False))
        bad(fn, p=RefineParams(1, -1, True))
    with pytest.raises(TypeError):
        refine(p=(1, 1, True))
    bad(engine.disparity_refined, L, R, 0, 16, 4, "sad", ok)
    bad(engine.disparity_refined, L, R, 0, 16, 5, "sgbm", ok)
    bad(engine.disparity_refined, L, R, 0, 16, 5, "hog", ok)
    with pytest.raises(SVError):
        E.refine_plan(0, 5)
    with pytest.raises(SVError):
        E.refine_plan(16, 4)
    # nothing was launched and the output is untouched
    engine.synchronize()
    after = {k: engine.profile_read(k)[1] for k in before}
    engine.profile(False)
    assert after == before
    assert (engine.to_host(d_o, (H, W), np.int16) == SENTINEL).all()
    refine()                                                # the same arguments, valid: runs
    assert (engine.to_host(d_o, (H, W), np.int16) != SENTINEL).all()
