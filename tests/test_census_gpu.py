"""The census / Hamming cost on the GPU: k_census, k_census_match and the plumbing
of cost = "census", every result array_equal to tests/sv_census_oracle.py.

Shapes are the smallest at which the kernels take another path: H < 7 and W < 9 (the whole
neighbourhood clamped), odd widths, more than one 64 x 16 transform tile and more than one
matcher block (64 - 2r columns, strips of 8 rows), windows 1..15, sweeps of 1..512 disparities
(1..4 waves of 16-disparity chunks, ragged last chunks), negative min_disp and an empty band."""
from __future__ import annotations

import functools
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("SV_WARMUP_AT_IMPORT", "0")
import sv_oracle as O  # noqa: E402
import sv_census_oracle as CO  # noqa: E402
from stereovision_amd.engine import RefineParams, SVError  # noqa: E402

pytestmark = pytest.mark.gpu

SENT64 = np.uint64(0xA5A5A5A5A5A5A5A5)
SENT16 = np.int16(0x5A5A)


class Dev:
    """Device buffers of one test, freed on exit."""

    def __init__(self, engine):
        self.e, self.ptrs = engine, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.synchronize()
        for p in self.ptrs:
            self.e.dev_free(p)

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.e.dev_alloc(a.nbytes)
        self.ptrs.append(p)
        self.e.to_device(p, a)
        return p


def pitched(a, pitch, fill=0):
    out = np.full((a.shape[0], pitch), fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


@functools.lru_cache(maxsize=None)
def image(kind, H, W, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W)).astype(np.uint8)
    if kind == "levels4":
        return (rng.integers(0, 4, (H, W)) * 64 + 17).astype(np.uint8)
    return np.full((H, W), 77, np.uint8)


@functools.lru_cache(maxsize=None)
def pair(kind, H, W, numD, minD, seed=0):
    """L and R with R(x - d) ~ L(x) for a d inside the sweep; "levels4": many ties; "flat"."""
    L = image("noise" if kind == "texture" else kind, H, W, seed)
    if kind == "flat":
        return L, L.copy()
    rng = np.random.default_rng(2000 + seed)
    d = minD + numD // 3
    fresh = image("noise" if kind == "texture" else kind, H, W, seed + 50)
    xs = np.arange(W) + d
    R = np.where((xs >= 0) & (xs < W), L[:, np.clip(xs, 0, W - 1)], fresh)
    if kind == "texture":
        R = np.clip(R.astype(np.int32) + rng.integers(-2, 3, (H, W)), 0, 255)
    else:
        R = np.where(rng.random((H, W)) < 0.1, fresh, R)
    return L, np.ascontiguousarray(R.astype(np.uint8))


# ------------------------------------------------------------------------------------------
# 1. the transform
# ------------------------------------------------------------------------------------------
T_SHAPES = [(1, 5), (3, 8), (7, 9), (20, 33), (41, 130), (24, 352)]


def gpu_census(engine, img, rows=None, pitch_extra=3, cpitch_extra=5):
    """sv_census_dev into a pitched plane with a guard row either side; returns the codes and
    checks that nothing but rows [row0, row1) x [0, W) was written."""
    H, W = img.shape
    r0, r1 = (0, H) if rows is None else rows
    pitch, cp = W + pitch_extra, W + cpitch_extra
    with Dev(engine) as d:
        dg = d.put(pitched(img, pitch, 201))
        dc = d.put(np.full((H + 2, cp), SENT64, np.uint64))
        engine.census_dev(dg, H, W, pitch, r0, r1, dc + 8 * cp, cp)
        got = engine.to_host(dc, (H + 2, cp), np.uint64)
    assert (got[0] == SENT64).all() and (got[-1] == SENT64).all(), "guard rows written"
    body = got[1:-1]
    assert (body[:, W:] == SENT64).all(), "pitch padding written"
    assert (body[:r0, :W] == SENT64).all() and (body[r1:, :W] == SENT64).all(), "rows outside the band written"
    return body[:, :W]


@pytest.mark.parametrize("kind", ["noise", "levels4", "flat"])
@pytest.mark.parametrize("shape", T_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_census_transform(engine, shape, kind):
    img = image(kind, *shape)
    np.testing.assert_array_equal(gpu_census(engine, img), CO.census(img))


def test_census_transform_row_band(engine):
    img = image("noise", 41, 130, seed=3)
    r0, r1 = 7, 29
    got = gpu_census(engine, img, rows=(r0, r1))
    np.testing.assert_array_equal(got[r0:r1], CO.census(img)[r0:r1])


def test_census_host_form(engine):
    img = image("levels4", 20, 33, seed=4)
    got = engine.census(img)
    assert got.dtype == np.uint64 and got.shape == img.shape
    np.testing.assert_array_equal(got, CO.census(img))


# ------------------------------------------------------------------------------------------
# 2. the matcher through cost = "census"
# ------------------------------------------------------------------------------------------
M_CASES = [(1, 5, 3, 1, 0), (3, 8, 4, 15, -2), (20, 33, 16, 3, 0), (40, 97, 16, 9, -3), (41, 130, 32, 15, 5),
           (24, 352, 272, 5, 0), (12, 600, 512, 7, 0), (9, 16, 16, 5, 0)]


@pytest.mark.parametrize("kind", ["texture", "levels4", "flat"])
@pytest.mark.parametrize("case", M_CASES, ids=lambda c: "H{}W{}D{}w{}m{}".format(*c))
def test_census_disparity(engine, case, kind):
    H, W, numD, win, minD = case
    L, R = pair(kind, H, W, numD, minD)
    got = engine.disparity(L, R, minD, numD, win, "census")
    exp = CO.disparity16_census(L, R, minD, numD, win)
    np.testing.assert_array_equal(got, exp)
    x0, x1 = O.valid_columns(W, minD, numD)
    if (H, W, numD) == (9, 16, 16):
        assert x1 == x0 and (got == (minD - 1) * 16).all()     # empty band: all invalid
    if kind == "flat":
        assert (got[:, x0:x1] == minD * 16).all()               # every cost ties at 0: the first minimum


@pytest.mark.parametrize("numD", [1, 5, 33, 100])
def test_census_ragged_sweeps(engine, numD):
    H, W, win, minD = 13, 150, 7, -1
    L, R = pair("texture", H, W, numD, minD, seed=numD)
    np.testing.assert_array_equal(engine.disparity(L, R, minD, numD, win, "census"),
                                  CO.disparity16_census(L, R, minD, numD, win))


def test_census_disparity_dev_pitched_band(engine):
    """Input and output pitches larger than W, a row band: nothing outside rows [row0, row1) x
    [0, W) of the map is written."""
    H, W, numD, win, minD, r0, r1 = 30, 97, 20, 9, 2, 5, 22
    L, R = pair("texture", H, W, numD, minD, seed=7)
    pitch, op = W + 7, W + 9
    with Dev(engine) as d:
        dl, dr = d.put(pitched(L, pitch, 9)), d.put(pitched(R, pitch, 250))
        do = d.put(np.full((H + 2, op), SENT16, np.int16))
        engine.disparity_dev(dl, dr, H, W, pitch, minD, numD, win, "census", r0, r1, do + 2 * op, op)
        got = engine.to_host(do, (H + 2, op), np.int16)
    exp = CO.disparity16_census(L, R, minD, numD, win)
    np.testing.assert_array_equal(got[1 + r0:1 + r1, :W], exp[r0:r1])
    got[1 + r0:1 + r1, :W] = SENT16
    assert (got == SENT16).all()


# ------------------------------------------------------------------------------------------
# 3. sv_census_match_dev on caller-supplied codes
# ------------------------------------------------------------------------------------------
def test_match_all_ones_reaches_the_cost_bound(engine):
    """64 bits set against none at win 15: every cost is 64 * 15^2 = 14400, the largest key."""
    H, W, numD, win = 20, 70, 24, 15
    CL = np.full((H, W), np.uint64(0xFFFFFFFFFFFFFFFF))
    CR = np.zeros((H, W), np.uint64)
    got = engine.census_match(CL, CR, 0, numD, win)
    np.testing.assert_array_equal(got, CO.match_codes(CL, CR, 0, numD, win))
    assert (got[:, numD:] == 0).all()
    # one zero code in the right plane lowers exactly the costs whose windows hold it
    CR2 = np.full((H, W), np.uint64(0xFFFFFFFFFFFFFFFF))
    CL2 = np.zeros((H, W), np.uint64)
    CR2[10, 30] = 0
    np.testing.assert_array_equal(engine.census_match(CL2, CR2, 0, numD, win), CO.match_codes(CL2, CR2, 0, numD, win))


def test_match_shifted_plane_first_minimum_wins(engine):
    H, W, numD, win, minD, d0, period = 16, 140, 40, 5, -4, 9, 8
    rng = np.random.default_rng(11)
    CR = rng.integers(0, 2 ** 63, (H, period), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (H, period)).astype(np.uint64)
    CR = np.ascontiguousarray(np.tile(CR, (1, W // period + 2))[:, :W])     # period-8 columns
    CL = np.ascontiguousarray(np.roll(CR, d0, axis=1))                      # CL(x) = CR(x - d0)
    got = engine.census_match(CL, CR, minD, numD, win)
    np.testing.assert_array_equal(got, CO.match_codes(CL, CR, minD, numD, win))
    # zero cost at d0 - 8, d0, d0 + 8, ...: away from the clamped borders the first of the sweep wins
    first = min(d for d in range(minD, minD + numD) if (d - d0) % period == 0)
    x0, x1 = O.valid_columns(W, minD, numD)
    assert (got[:, x0 + 3:x1 - 3] == first * 16).all()


def test_match_random_codes(engine):
    H, W, numD, win, minD = 19, 131, 40, 5, 3
    rng = np.random.default_rng(12)
    bits = [rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64) for _ in range(4)]
    CL = (bits[0] << np.uint64(32)) | bits[1]        # bits 62 and 63 in use
    CR = (bits[2] << np.uint64(32)) | bits[3]
    np.testing.assert_array_equal(engine.census_match(CL, CR, minD, numD, win), CO.match_codes(CL, CR, minD, numD, win))


@pytest.mark.parametrize("H,strip", [(1020, 32), (500, 16)])
def test_match_long_strips(engine, H, strip):
    """Strips of 32 and of 16 rows: the launcher halves the strip while a launch has fewer than
    1024 blocks, so every smaller frame here runs strips of 8.  W = 1600 at win 15 is 32 blocks a
    row (50 columns each): 1020 rows make 32 strips of 32 (the last one ragged), 500 rows 16 of 32
    and so 32 of 16.  The oracle is taken on three row bands that hold strip seams."""
    W, numD, win, minD = 1600, 20, 15, 0
    assert -(-W // (64 - 2 * (win // 2))) * -(-H // strip) >= 1024 > -(-W // 50) * -(-H // (2 * strip))
    rng = np.random.default_rng(14)
    CR = rng.integers(0, 2 ** 63, (H, W), dtype=np.uint64)
    flip = np.uint64(1) << rng.integers(0, 64, (H, W)).astype(np.uint64)
    CL = np.ascontiguousarray(np.roll(CR, 7, axis=1) ^ flip)          # CL(x) = CR(x - 7) but for one bit
    got = engine.census_match(CL, CR, minD, numD, win)
    for y0, y1 in ((0, 40), (H // 2 - 20, H // 2 + 20), (H - 40, H)):
        exp = CO.match_codes(CL, CR, minD, numD, win, rows=(y0, y1))
        np.testing.assert_array_equal(got[y0:y1], exp[y0:y1], err_msg=f"rows {y0}:{y1}")


def test_match_dev_pitched_rows(engine):
    H, W, numD, win, minD, r0, r1 = 21, 75, 12, 7, 0, 4, 15
    rng = np.random.default_rng(13)
    CL = rng.integers(0, 2 ** 62, (H, W), dtype=np.uint64)
    CR = np.ascontiguousarray(np.roll(CL, -5, axis=1))
    cp, op = W + 3, W + 6
    with Dev(engine) as d:
        dl, dr = d.put(pitched(CL, cp, SENT64)), d.put(pitched(CR, cp, SENT64))
        do = d.put(np.full((H, op), SENT16, np.int16))
        engine.census_match_dev(dl, dr, H, W, cp, minD, numD, win, r0, r1, do, op)
        got = engine.to_host(do, (H, op), np.int16)
    exp = CO.match_codes(CL, CR, minD, numD, win)
    np.testing.assert_array_equal(got[r0:r1, :W], exp[r0:r1])
    got[r0:r1, :W] = SENT16
    assert (got == SENT16).all()


# ------------------------------------------------------------------------------------------
# 4. plumbing
# ------------------------------------------------------------------------------------------
def test_batch_of_two_with_frame_strides(engine):
    H, W, numD, win, minD = 22, 90, 24, 7, -2
    pitch, op = W + 4, W + 2
    fs, ofs = pitch * H + 64, op * H + 10
    frames = [pair("texture", H, W, numD, minD, seed=20 + z) for z in range(2)]
    bl = np.full(2 * fs, 33, np.uint8)
    br = np.full(2 * fs, 44, np.uint8)
    for z, (L, R) in enumerate(frames):
        bl[z * fs:z * fs + pitch * H] = pitched(L, pitch).ravel()
        br[z * fs:z * fs + pitch * H] = pitched(R, pitch).ravel()
    with Dev(engine) as d:
        dl, dr = d.put(bl), d.put(br)
        do = d.put(np.full(2 * ofs, SENT16, np.int16))
        engine.disparity_batch_dev(dl, dr, 2, H, W, pitch, fs, minD, numD, win, "census", do, op, ofs)
        got = engine.to_host(do, (2 * ofs,), np.int16)
    for z, (L, R) in enumerate(frames):
        m = got[z * ofs:z * ofs + op * H].reshape(H, op)
        np.testing.assert_array_equal(m[:, :W], CO.disparity16_census(L, R, minD, numD, win), err_msg=str(z))
        assert (m[:, W:] == SENT16).all()
    assert (got[op * H:ofs] == SENT16).all() and (got[ofs + op * H:] == SENT16).all()


def test_row_bands_agree_with_the_full_frame(engine):
    H, W, numD, win, minD = 41, 130, 32, 15, 5
    L, R = pair("texture", H, W, numD, minD)
    full = engine.disparity(L, R, minD, numD, win, "census")
    out = np.full((H, W), SENT16, np.int16)
    for r0, r1 in ((0, 13), (13, 30), (30, 41)):
        engine.disparity_rows(L, R, minD, numD, win, r0, r1, "census", out)
    np.testing.assert_array_equal(out, full)
    np.testing.assert_array_equal(full, CO.disparity16_census(L, R, minD, numD, win))


def test_d8_index_format(engine):
    H, W, numD, win, minD = 25, 110, 48, 5, -3
    L, R = pair("texture", H, W, numD, minD, seed=31)
    with Dev(engine) as d:
        dl, dr = d.put(L), d.put(R)
        d16 = d.put(np.zeros((H, W), np.int16))
        d8 = d.put(np.zeros((H, W), np.uint8))
        engine.disparity_dev(dl, dr, H, W, W, minD, numD, win, "census", 0, H, d16, W)
        engine.median_map_dev(d16, H, W, 0, H, d8, "d8", minD, numD, cost="census")
        got = engine.to_host(d8, (H, W), np.uint8)
    med = O.median5(CO.disparity16_census(L, R, minD, numD, win)).astype(np.int32)
    np.testing.assert_array_equal(got, (med // 16 - (minD - 1)).astype(np.uint8))


def test_right_and_refined_maps(engine):
    from stereovision_amd.synthetic import stereo_pair
    H, W, numD, win, minD = 36, 120, 24, 7, 0
    L, R, _ = stereo_pair(H, W, numD, seed=41)                     # depth steps: occlusions fail the check
    np.testing.assert_array_equal(engine.disparity_right(L, R, minD, numD, win, "census"),
                                  CO.disparity16_right(L, R, minD, numD, win))
    plain = CO.disparity16_census(L, R, minD, numD, win)
    checked = CO.disparity_refined(L, R, minD, numD, win, lr_max_diff=1)
    exp = CO.disparity_refined(L, R, minD, numD, win, lr_max_diff=1, speckle_window=30, speckle_range=1)
    assert (checked != plain).any() and (exp != checked).any()    # the check and the filter both act
    np.testing.assert_array_equal(engine.disparity_refined(L, R, minD, numD, win, "census", RefineParams(1, 0, False)),
                                  checked)
    np.testing.assert_array_equal(engine.disparity_refined(L, R, minD, numD, win, "census",
                                                           RefineParams(1, 0, False, 30, 1)), exp)


@pytest.mark.parametrize("p", [RefineParams(1, 0, True), RefineParams(1, 1, False)], ids=["subpixel", "curvature"])
def test_refinement_taps_are_rejected(engine, p):
    L, R = pair("texture", 12, 40, 8, 0)
    with pytest.raises(SVError) as e:
        engine.disparity_refined(L, R, 0, 8, 5, "census", p)
    assert e.value.code == -22 and "census" in str(e.value)


def test_create_depth_map_stereo_scaled_drop_in(engine, monkeypatch):
    from stereovision_amd import fused_depth_map as FDM
    from stereovision_amd.synthetic import stereo_pair, to_bgr
    monkeypatch.setattr(FDM, "COST", "census")
    H, W, numD, win = 40, 160, 48, 5
    L, R, _ = stereo_pair(H, W, numD, seed=3)
    dn, disp, cmap, conf = FDM.create_depth_map_stereo_scaled(to_bgr(L), to_bgr(R), 0, numD, win)
    e_disp = O.disparity_f32(CO.disparity16_census(L, R, 0, numD, win))
    e_dn, _, e_conf = O.scaled_post(e_disp, 0, numD)
    np.testing.assert_array_equal(disp, e_disp)
    np.testing.assert_array_equal(dn, e_dn)
    np.testing.assert_array_equal(conf, e_conf)
    assert cmap.shape == (H, W, 3)


def test_depth_map_drop_in_and_pipeline(engine, monkeypatch):
    from stereovision_amd import depth_map as DM
    from stereovision_amd.pipeline import DepthMapPipeline
    from stereovision_amd.synthetic import stereo_pair, to_bgr
    H, W, numD, win = 32, 150, 32, 7
    L, R, _ = stereo_pair(H, W, numD, seed=5)
    e_disp = O.disparity_f32(CO.disparity16_census(L, R, 0, numD, win))
    e_depth, _ = O.depth_post(e_disp, 0.3, 2.0, 0)
    monkeypatch.setattr(DM, "COST", "census")
    monkeypatch.setattr(DM, "NUM_DISP", numD)
    monkeypatch.setattr(DM, "WINDOW_SIZE", win)
    depth, disp, _ = DM.create_depth_map(to_bgr(L), to_bgr(R))
    np.testing.assert_array_equal(disp, e_disp)
    np.testing.assert_array_equal(depth, e_depth)
    pipe = DepthMapPipeline(numD, win, cost="census", depth=1)
    try:
        depth, disp, _ = pipe.submit(to_bgr(L), to_bgr(R)).result(timeout=120)
    finally:
        pipe.close()
    np.testing.assert_array_equal(disp, e_disp)
    np.testing.assert_array_equal(depth, e_depth)


def test_row_tiled_depth_map(engine):
    from stereovision_amd.distributed import RowTiledDepthMap
    H, W, numD, win, world = 41, 130, 32, 9, 3
    L, R = pair("texture", H, W, numD, 0, seed=51)
    ref = O.disparity_f32(CO.disparity16_census(L, R, 0, numD, win))
    with Dev(engine) as d:
        dl, dr = d.put(L), d.put(R)
        disp = np.zeros((H, W), np.float32)
        for k in range(world):
            rt = RowTiledDepthMap(H, W, numD, win, cost="census", rank=k, world=world, engine=engine)
            rt.compute(dl, dr)
            engine.synchronize()
            disp[rt.r0:rt.r1] = engine.to_host(rt.disp, (H, W), np.float32)[rt.r0:rt.r1]
            rt.close()
    np.testing.assert_array_equal(disp, ref)


def test_fusion_frame_pipeline_step(engine, monkeypatch):
    import tempfile
    import frame_chain as C
    from stereovision_amd import flow as F
    from stereovision_amd import fused_depth_map as FDM
    from stereovision_amd import synthetic
    from stereovision_amd.frame import OUTPUT_NAMES, FusionFramePipeline
    monkeypatch.setattr(F.time, "time", lambda: 1000.0)
    monkeypatch.setattr(FDM, "COST", "census")          # the chain's drop-in reads it at call time
    CH, CW = 176, 240
    with tempfile.TemporaryDirectory() as t:
        path = os.path.join(t, "stereo_calibration_data.pkl")
        with open(path, "wb") as f:
            pickle.dump(synthetic.synthetic_calibration(CW, CH, 0), f)
        calib = FDM.load_stereo_calibration_with_scaling(0.5, path)
    stereo = dict(min_disp=0, num_disp=32, window_size=5)
    pipe = FusionFramePipeline(calib, engine=engine, outputs=OUTPUT_NAMES, cost="census", **stereo)
    chain = C.HostChain(calib, **stereo)
    fl, fr = C.moving_stereo_sequence(CH, CW, 1, disparity=8)[0]
    res, exp = pipe.step(fl, fr, None), chain.step(fl, fr, None)
    for s in C.SCALARS:
        assert getattr(res, s) == exp[s], s
    for name in OUTPUT_NAMES:
        got, e = getattr(res, name), exp[name]
        assert (got is None) == (e is None), name
        if e is not None:
            np.testing.assert_array_equal(got, e, err_msg=name)
    assert res.use_stereo and res.stereo_disparity.max() > 0
    # and the stereo stage is the census cost's: the drop-in's disparity equals the oracle chain's
    gl, gr = O.bgr_to_gray(res.processed_left), O.bgr_to_gray(res.processed_right)
    np.testing.assert_array_equal(res.stereo_disparity, O.disparity_f32(CO.disparity16_census(gl, gr, 0, 32, 5)))


def test_argument_errors(engine):
    H, W = 12, 40
    with Dev(engine) as d:
        dg = d.put(image("noise", H, W))
        dc = d.put(np.zeros((H, W), np.uint64))
        do = d.put(np.zeros((H, W), np.int16))

        def bad(fn, *a):
            with pytest.raises(SVError) as e:
                fn(*a)
            assert e.value.code == -22, (a, e.value)

        bad(engine.census_dev, 0, H, W, W, 0, H, dc, W)              # null pointers
        bad(engine.census_dev, dg, H, W, W, 0, H, 0, W)
        bad(engine.census_dev, dg, H, W, W - 1, 0, H, dc, W)         # pitches smaller than W
        bad(engine.census_dev, dg, H, W, W, 0, H, dc, W - 1)
        bad(engine.census_match_dev, 0, dc, H, W, W, 0, 8, 5, 0, H, do, W)
        bad(engine.census_match_dev, dc, 0, H, W, W, 0, 8, 5, 0, H, do, W)
        bad(engine.census_match_dev, dc, dc, H, W, W, 0, 8, 5, 0, H, 0, W)
        bad(engine.census_match_dev, dc, dc, H, W, W - 1, 0, 8, 5, 0, H, do, W)
        bad(engine.census_match_dev, dc, dc, H, W, W, 0, 8, 5, 0, H, do, W - 1)
        bad(engine.census_match_dev, dc, dc, H, W, W, 0, 8, 4, 0, H, do, W)      # even win
        bad(engine.census_match_dev, dc, dc, H, W, W, 0, 8, 17, 0, H, do, W)
        bad(engine.census_match_dev, dc, dc, H, W, W, 0, 513, 5, 0, H, do, W)    # num_disp = 513
        bad(engine.census_match_dev, dc, dc, H, W, W, 0, 0, 5, 0, H, do, W)
        bad(engine.census_match_dev, dc, dc, H, W, W, 2040, 16, 5, 0, H, do, W)  # the int16 range rule
        L = image("noise", H, W)
        bad(engine.disparity, L, L, 0, 513, 5, "census")
        bad(engine.disparity, L, L, 0, 8, 6, "census")
