"""The refinement stage's NumPy restatement (tests/sv_refine_oracle.py) on the CPU: the mirrored
definition of the right-referenced map against a directly written matcher, what the stage does
to an occlusion and to a flat frame, and totality on arbitrary maps."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sv_oracle as O  # noqa: E402
import sv_refine_oracle as RO  # noqa: E402


def direct_right(L, R, min_disp, num_disp, win, cost):
    """The right-referenced matcher written out: cost(x', d) = sum f(Rp(x' + i) - Lp(x' + i + d)),
    first argmin over d ascending, on the columns whose whole sweep stays a disparity of the
    image: [max(-minD, 0), W - max(minD + numD, 0))."""
    H, W = L.shape
    r = win // 2
    inv = (min_disp - 1) * 16
    out = np.full((H, W), inv, np.int16)
    x0, x1 = RO.right_valid_columns(W, min_disp, num_disp)
    if x1 <= x0:
        return out
    ys, xs = np.mgrid[0:H, x0:x1]
    best_c = np.full(ys.shape, np.iinfo(np.int64).max, np.int64)
    best_d = np.zeros(ys.shape, np.int64)
    for d in range(min_disp, min_disp + num_disp):
        c = np.zeros(ys.shape, np.int64)
        for j in range(-r, r + 1):
            yy = np.clip(ys + j, 0, H - 1)
            for i in range(-r, r + 1):
                df = R[yy, np.clip(xs + i, 0, W - 1)].astype(np.int64) - \
                    L[yy, np.clip(xs + i + d, 0, W - 1)].astype(np.int64)
                c += np.abs(df) if cost == O.COST_SAD else df * df
        m = c < best_c
        best_c[m] = c[m]
        best_d[m] = d
    out[:, x0:x1] = (best_d * 16).astype(np.int16)
    return out


@pytest.mark.parametrize("cost", [O.COST_SAD, O.COST_SSD], ids=["sad", "ssd"])
@pytest.mark.parametrize("min_disp", [-3, 0, 4])
def test_mirrored_definition_equals_the_direct_right_matcher(cost, min_disp):
    rng = np.random.default_rng(11 + min_disp)
    H, W, D, win = 13, 41, 8, 5
    bg = rng.integers(0, 256, (H, W + 16), dtype=np.uint8)
    L = np.ascontiguousarray(bg[:, 8:8 + W])
    R = np.ascontiguousarray(bg[:, 8 + min_disp + 2:8 + min_disp + 2 + W])   # true disparity minD + 2
    # coarse values too, so that cost ties occur and the first-argmin rule is exercised
    for a, b in ((L, R), (L // 64, R // 64)):
        got = RO.disparity16_right(a, b, min_disp, D, win, cost)
        np.testing.assert_array_equal(got, direct_right(a, b, min_disp, D, win, cost))
        x0, x1 = RO.right_valid_columns(W, min_disp, D)
        inv = (min_disp - 1) * 16
        assert (got[:, :x0] == inv).all() and (got[:, x1:] == inv).all() and (got[:, x0:x1] != inv).all()
    got = RO.disparity16_right(L, R, min_disp, D, win, cost)
    inner = got[3:-3, x0 + 3:x1 - 3]
    assert (inner == (min_disp + 2) * 16).mean() > 0.95


def occlusion_scenes():
    """{cost: (L, R, truth, occluded)}: a foreground patch at disparity 11 over a background at
    disparity 3; rows 8:32, columns 52:60 of the left frame show background that the patch hides
    in the right frame.  One generator across both costs: SAD takes its first background and
    foreground, SSD the next two."""
    rng = np.random.default_rng(3)
    scenes = {}
    for cost in (O.COST_SAD, O.COST_SSD):
        bg = rng.integers(0, 256, (40, 160)).astype(np.uint8)
        fg = rng.integers(0, 256, (40, 160)).astype(np.uint8)
        L = bg[:, :128].copy()
        R = bg[:, 3:131].copy()
        L[8:32, 60:90] = fg[8:32, 60:90]
        R[8:32, 49:79] = fg[8:32, 60:90]
        truth = np.full((40, 128), 3, np.int64)
        truth[8:32, 60:90] = 11
        occluded = np.zeros((40, 128), bool)
        occluded[8:32, 52:60] = True
        scenes[cost] = (L, R, truth, occluded)
    return scenes


@pytest.mark.parametrize("cost", [O.COST_SAD, O.COST_SSD], ids=["sad", "ssd"])
def test_occlusion_scene(cost):
    """Measured with the restatement: 0.953 (SAD) / 0.964 (SSD) of the occluded band invalidated,
    0.995 / 0.992 of the other pixels at x >= 16 kept, 0.997 / 0.994 of the kept pixels within half
    a pixel of the truth."""
    L, R, truth, occluded = occlusion_scenes()[cost]
    minD, numD, win = 0, 16, 5
    inv = (minD - 1) * 16
    out = RO.disparity_refined(L, R, minD, numD, win, cost, lr_max_diff=1)
    dead = out == inv
    visible = ~occluded
    visible[:, :16] = False
    invalidated = dead[occluded].mean()
    kept = (~dead)[visible].mean()
    close = (np.abs(out[visible & ~dead] / 16.0 - truth[visible & ~dead]) <= 0.5).mean()
    print(f"cost {cost}: invalidated {invalidated:.3f} kept {kept:.3f} close {close:.3f}")
    assert invalidated >= 0.90
    assert kept >= 0.98
    assert close >= 0.99
    # the plain map has no invalid pixel in the matched band: the stage is what makes them
    assert (O.disparity16(L, R, minD, numD, win, cost)[:, 16:] != inv).all()


@pytest.mark.parametrize("cost", [O.COST_SAD, O.COST_SSD], ids=["sad", "ssd"])
def test_flat_frame(cost):
    L = np.full((12, 40), 97, np.uint8)
    minD, numD, win = 0, 8, 5
    inv = (minD - 1) * 16
    out = RO.disparity_refined(L, L, minD, numD, win, cost, min_curvature=1)
    assert (out == inv).all()
    out = RO.disparity_refined(L, L, minD, numD, win, cost, min_curvature=0)
    x0, x1 = O.valid_columns(40, minD, numD)
    assert (out[:, x0:x1] == minD * 16).all() and (out[:, :x0] == inv).all() and (out[:, x1:] == inv).all()


@pytest.mark.parametrize("cost", [O.COST_SAD, O.COST_SSD], ids=["sad", "ssd"])
@pytest.mark.parametrize("min_disp,num_disp", [(0, 16), (-5, 7), (3, 1), (-2047, 16), (2032, 16)])
def test_totality_on_arbitrary_maps(cost, min_disp, num_disp):
    rng = np.random.default_rng(5)
    H, W, win = 9, 37, 5
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    inv = (min_disp - 1) * 16
    dmax = min_disp + num_disp - 1
    maps = {
        "in range": (rng.integers(min_disp, dmax + 1, (H, W)) * 16),
        "fractions": (rng.integers(min_disp, dmax + 1, (H, W)) * 16 + rng.integers(1, 16, (H, W))),
        "out of range": np.where(rng.random((H, W)) < 0.5, (dmax + 1) * 16, (min_disp - 2) * 16),
        "junk": rng.integers(-32768, 32768, (H, W)),
        "low end": np.full((H, W), min_disp * 16),
        "high end": np.full((H, W), dmax * 16),
        "holes": np.where(rng.random((H, W)) < 0.3, inv, rng.integers(min_disp, dmax + 1, (H, W)) * 16),
    }
    dR = RO.disparity16_right(L, R, min_disp, num_disp, win, cost)
    for name, m in maps.items():
        m = np.clip(m, -32768, 32767).astype(np.int16)
        for kw in (dict(), dict(lr_max_diff=-1, min_curvature=0), dict(min_curvature=0, subpixel=False)):
            out = RO.refine(L, R, m, min_disp, num_disp, win, cost, dR, **kw)
            assert out.dtype == np.int16 and out.shape == (H, W)
            v = m.astype(np.int64)
            d = v >> 4
            ok = ((v & 15) == 0) & (d >= min_disp) & (d <= dmax)
            assert (out[~ok] == inv).all(), name
            live = out != inv
            assert (np.abs(out.astype(np.int64) - v)[live] <= 8).all(), name
            if not kw.get("subpixel", True):
                assert (out[live] == m[live]).all(), name
        if name in ("fractions", "out of range"):
            assert (out == inv).all(), name
        if name in ("in range", "low end", "high end"):   # nothing rejects without the tests
            out = RO.refine(L, R, m, min_disp, num_disp, win, cost, None, lr_max_diff=-1, min_curvature=0)
            assert (out != inv).all(), name


# ------------------------------------------------------------------------------------------
# the host side: parameters, the plan query and the drop-ins' control flow (no GPU)
# ------------------------------------------------------------------------------------------
def test_refine_params_and_plan_without_gpu():
    from stereovision_amd import engine as E
    p = E.RefineParams()
    assert (p.lr_max_diff, p.min_curvature, p.subpixel, p.speckle_window, p.speckle_range) == (1, 1, True, 0, 2)
    c = E.RefineParams(2, 7, False, 30, 3).c_struct()
    assert (c.lr_max_diff, c.min_curvature, c.subpixel, c.speckle_window, c.speckle_range) == (2, 7, 0, 30, 3)
    # k_refine's strips: (4 + 2r) rows of (64 + 2r) + (64 + numD + 2r + 1) bytes
    assert E.refine_plan(96, 5) == {"lds_bytes": 8 * (68 + 165), "form": "lds"}
    assert E.refine_plan(512, 15) == {"lds_bytes": 18 * (78 + 591), "form": "global"}
    for bad in ((0, 5), (513, 5), (16, 4), (16, 17)):
        with pytest.raises(E.SVError) as ei:
            E.refine_plan(*bad)
        assert ei.value.code == -22


class RefinedOracleEngine:
    """Routes the drop-ins' refined path to the restatement (test double, CPU tests only)."""

    def __init__(self, fail=False):
        self.fail, self.calls = fail, 0

    def refined_frame(self, gl, gr, min_disp, num_disp, win, params, mode, cost="sad", cmap_bgr=None,
                      min_depth=0.0, max_depth=0.0, min_disp_global=0.0):
        from stereovision_amd.engine import POST_DEPTH, SVError
        self.calls += 1
        if self.fail:
            raise SVError("sv_disparity_refined_dev", -5, "injected")
        d16 = RO.disparity_refined(O.bgr_to_gray(gl), O.bgr_to_gray(gr), min_disp, num_disp, win,
                                   {"sad": 0, "ssd": 1}[cost], params.lr_max_diff, params.min_curvature,
                                   params.subpixel, params.speckle_window, params.speckle_range)
        disp = O.disparity_f32(d16)
        if mode == POST_DEPTH:
            a, u8 = O.depth_post(disp, min_depth, max_depth, min_disp_global)
            b = None
        else:
            a, u8, b = O.scaled_post(disp, min_disp, num_disp)
        return a, disp, u8, b, np.asarray(cmap_bgr)[u8]

    def gray(self, bgr):
        return O.bgr_to_gray(bgr)

    def __getattr__(self, name):   # the plain path must not be taken while REFINE is set
        raise AssertionError(f"unexpected engine call {name}")


def test_drop_ins_route_through_the_refined_frame(monkeypatch, capsys):
    from stereovision_amd import depth_map as DM
    from stereovision_amd import fused_depth_map as FDM
    from stereovision_amd.engine import RefineParams
    from stereovision_amd.synthetic import stereo_pair, to_bgr
    assert DM.REFINE is None and FDM.REFINE is None
    L, R, _ = stereo_pair(24, 90, 16, seed=4)
    p = RefineParams(1, 1, True, 10, 1)
    eng = RefinedOracleEngine()
    for mod in (DM, FDM):
        monkeypatch.setattr(mod, "get_engine", lambda: eng)
        monkeypatch.setattr(mod, "REFINE", p)
    monkeypatch.setattr(DM, "NUM_DISP", 16)
    monkeypatch.setattr(DM, "WINDOW_SIZE", 5)
    d16 = RO.disparity_refined(L, R, 0, 16, 5, O.COST_SAD, 1, 1, True, 10, 1)
    disparity = O.disparity_f32(d16)
    depth, disp, cmap = DM.create_depth_map(to_bgr(L), to_bgr(R), None, 0.2, 4.0)
    np.testing.assert_array_equal(disp, disparity)
    np.testing.assert_array_equal(depth, O.depth_post(disparity, 0.2, 4.0, 0)[0])
    assert cmap.shape == (24, 90, 3) and cmap.dtype == np.uint8
    dn, disp, cmap, conf = FDM.create_depth_map_stereo_scaled(L, R, 0, 16, 5)
    e_dn, _, e_conf = O.scaled_post(disparity, 0, 16)
    np.testing.assert_array_equal(disp, disparity)
    np.testing.assert_array_equal(dn, e_dn)
    np.testing.assert_array_equal(conf, e_conf)
    assert eng.calls == 2
    # the never-raise convention holds on the refined path too
    bad = RefinedOracleEngine(fail=True)
    for mod in (DM, FDM):
        monkeypatch.setattr(mod, "get_engine", lambda: bad)
    depth, disp, cmap = DM.create_depth_map(L, R)
    assert depth.shape == (24, 90) and not depth.any() and not disp.any() and cmap.shape == (24, 90, 3)
    dn, disp, cmap, conf = FDM.create_depth_map_stereo_scaled(L, R, 0, 16, 5)
    for a in (dn, disp, conf):
        assert a.shape == (24, 90) and a.dtype == np.float32 and not a.any()
    assert "injected" in capsys.readouterr().out and bad.calls == 2
