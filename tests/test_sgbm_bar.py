"""Why tests/test_sgbm_exact.py is not vacuous, derived on the CPU with the oracle alone.

The GPU file compares engine.sgbm bit for bit with oracle/sv_sgbm_oracle.py on the cases of
tests/sgbm_frames.py.  A bit-exact comparison only bites where the frames drive the kernels
to the limits their host code reasons about, and where the final map is not mostly the
invalid value.  This file asserts both, and prints the figures (pytest -s shows them):

  B1  an int32 configuration whose window cost and path costs exceed 32767;
  B2  the two last int16 configurations: window cost >= 26 000, every path cost in int16;
  B3  P2 = 32768 drives an int16 path to exactly -32768; 32769 is int32 per the host rule;
  B4  P2 = 349524: S = -3 P2 >= -2^20; the largest S of the (127, 13) ramps + 2^20 < 2^23;
  B5  band pixels with minS >= 32767 (k_sgbm_lrcheck's `minS < 32767` on its false side);
  B6  both signs of the sub-pixel numerator, and the parabola's denominator at its clamp;
  B7  >= 25 % valid band pixels for every case run with a filter on, 100 % for bare cases;
  B8  eight one-line mutants of the oracle, each of which changes the map of >= 1 case.

The host rule restated here (sv_capi.cpp, enqueue_sgbm): cap = max(preFilterCap, 15) | 1,
cmax = (2 cap + 63) win^2 must be <= 65535; path volumes are int32 iff cmax > 32767 or
P2 > 32768, else int16; P2 = max(P2, P1 + 1) < 349525.
"""
import numpy as np
import pytest

import sgbm_frames as F
import sv_sgbm_oracle as SG


def host_l32(cap, win, P2):
    cap = max(cap, 15) | 1
    cmax = (2 * cap + 63) * win * win
    assert cmax <= 65535
    return cmax > 32767 or P2 > 32768


def sgbm_dp(D):
    """sv_sgbm.hip's sgbm_dp: D padded to a multiple of both path kernels' lane plans."""
    def plan16(D):
        return next(o for o in (1, 2, 4, 8, 12, 16, 20, 24, 32) if o >= (D + 15) // 16)

    def vplan(D):
        return plan16(D) if D <= 32 else next(o for o in (2, 4, 6, 8, 10, 12, 16) if o >= (D + 31) // 32)
    lcm = int(np.lcm(plan16(D), vplan(D)))
    return (D + lcm - 1) // lcm * lcm


def params(case):
    cap = max(case.okw.get("preFilterCap", 63), 15) | 1
    p = SG.params_for(case.win)
    P1 = case.okw.get("P1", p["P1"])
    P2 = max(case.okw.get("P2", p["P2"]), P1 + 1)
    return cap, P1, P2


def block_costs(case):
    L, R = case.frames()
    cap, _, _ = params(case)
    return SG.block_cost(SG.pixel_cost(L, R, case.min_disp, case.D, cap), case.win)


def three_paths(C, P1, P2):
    """SG.aggregate with its three path volumes kept apart: (L_lr, L_rl, L_tb), int64."""
    H, Wb, D = C.shape
    C = C.astype(np.int64)
    lr, rl, tb = np.zeros_like(C), np.zeros_like(C), np.zeros_like(C)
    prev = np.zeros((H, D), np.int64)
    for x in range(Wb):
        prev = lr[:, x] = SG._step(prev, C[:, x], P1, P2)
    prev = np.zeros((H, D), np.int64)
    for x in range(Wb - 1, -1, -1):
        prev = rl[:, x] = SG._step(prev, C[:, x], P1, P2)
    prev = np.zeros((Wb, D), np.int64)
    for y in range(H):
        prev = tb[y] = SG._step(prev, C[y], P1, P2)
    return lr, rl, tb


def volumes(case):
    C = block_costs(case)
    _, P1, P2 = params(case)
    paths = three_paths(C, P1, P2)
    S = paths[0] + paths[1] + paths[2]
    np.testing.assert_array_equal(S, SG.aggregate(C, P1, P2))     # the local copy is the oracle's
    return C, paths, S


def cases(group=None, family=None, **kw):
    out = [c for c in F.CASES if (group is None or c.group == group) and (family is None or c.family == family)
           and all(c.okw.get(k) == v for k, v in kw.items())]
    assert out
    return out


def c1(family, cap, win, **fkw):
    return next(c for c in cases("c1bare", family, preFilterCap=cap) if c.win == win and
                all(c.fkw.get(k) == v for k, v in fkw.items()))


def test_b1_int32_configurations_need_int32():
    """Ramps and sawtooth at (63, 15), (127, 13): window cost and path costs beyond int16."""
    for cap, win, top in ((63, 15, 34965), (127, 13, 46878)):
        assert host_l32(cap, win, SG.params_for(win)["P2"])
        C, paths, _ = volumes(c1("ramps", cap, win))
        pmax = max(int(p.max()) for p in paths)
        print(f"B1 ramps cap {cap} win {win}: max C {C.max()} (bound {(2 * cap + 63) * win * win}), max path {pmax}")
        assert C.max() == top > 32767
        assert pmax > 32767
        C, paths, _ = volumes(c1("sawtooth", cap, win))
        assert C.max() > 32767 and max(int(p.max()) for p in paths) > 32767


def test_b2_int16_configurations_stay_in_int16_and_come_close():
    """(63, 13) and (103, 11): cmax 31 941 and 32 549, the last before the switch ((105, 11)
    has 33 033).  Every C1 frame's path costs fit int16 (what l32 = 0 rests on) and the ramps
    bring the window cost to 26 897 / 27 467."""
    assert not host_l32(103, 11, SG.params_for(11)["P2"]) and host_l32(105, 11, SG.params_for(11)["P2"])
    for cap, win, top in ((63, 13, 26897), (103, 11, 27467)):
        assert not host_l32(cap, win, SG.params_for(win)["P2"])
        lo = hi = 0
        for c in cases("c1bare", preFilterCap=cap):
            if c.win != win:
                continue
            C, paths, _ = volumes(c)
            assert C.max() <= (2 * cap + 63) * win * win
            lo = min([lo] + [int(p.min()) for p in paths])
            hi = max([hi] + [int(p.max()) for p in paths])
        C, _, _ = volumes(c1("ramps", cap, win))
        print(f"B2 cap {cap} win {win}: ramps max C {C.max()}, path costs of all C1 frames in [{lo}, {hi}]")
        assert C.max() == top >= 26000
        assert -32768 <= lo and hi <= 32767
        assert hi >= 26000                                  # and the paths come close as well


def test_b3_p2_at_the_int16_switch():
    """Flat equal frames: C = 0, every path cost is -P2.  P2 = 32768 is still int16 per the host
    rule and holds exactly -32768; 32769 selects int32."""
    for P2, l32 in ((32767, False), (32768, False), (32769, True)):
        c = next(c for c in cases("c2", "flat", P2=P2, P1=600) if c.fkw == dict(a=63, b=63))
        assert host_l32(63, c.win, P2) == l32
        C, paths, S = volumes(c)
        assert C.max() == 0
        for p in paths:
            assert p.min() == p.max() == -P2
        assert (S == -3 * P2).all()
        # every disparity ties: the first minimum wins, no parabola, the whole band valid
        out = F.expected(c)
        X0, X1 = c.band
        assert (out[:, X0:X1] == 0).all()
    print("B3 flat frames: path costs exactly -32767 / -32768 (int16) / -32769 (int32)")


def test_b4_argmin_key_and_mul24_ranges():
    """The argmin key ((S + 2^20) << 9) | d needs 0 <= S + 2^20 < 2^23, and the 24-bit
    uniqueness products |S| < 2^23."""
    c = next(c for c in cases("c2", "flat", P2=349524, P1=600) if c.fkw == dict(a=63, b=63))
    _, _, S = volumes(c)
    assert S.min() == -3 * 349524 and S.min() + (1 << 20) == 4 >= 0
    assert 3 * 349526 > 1 << 20                             # the accepted maximum is two below the first that fails
    top = 0
    for c in cases("c1bare", preFilterCap=127) + cases("c2", P2=349524):
        _, _, S = volumes(c)
        assert S.min() + (1 << 20) >= 0 and abs(S).max() < 1 << 23
        top = max(top, int(S.max()))
    _, _, S = volumes(c1("ramps", 127, 13))
    print(f"B4 min S = -3 * 349524 = {-3 * 349524}; largest S {top} (ramps 127/13: {S.max()})")
    assert S.max() + (1 << 20) < 1 << 23 and top + (1 << 20) < 1 << 23
    assert S.max() > 3 * 32767                              # well beyond three int16 paths


def test_b5_lrcheck_rule_on_its_false_side():
    """disp2cost starts at SHRT_MAX, so a pixel with minS >= 32767 never enters disp2: the
    sawtooth at (127, 13) has 225 of its 369 band pixels there (345 of 495 at 11 x 61)."""
    for c in cases("c3b", "sawtooth"):
        _, _, S = volumes(c)
        n, px = int((S.min(-1) >= 32767).sum()), S.shape[0] * S.shape[1]
        print(f"B5 {c.id}: {n} of {px} band pixels with minS >= 32767")
        assert (n, px) == ((225, 369) if c.H == 9 else (345, 495))
        assert int((S.min(-1) < 32767).sum()) > 0           # and the true side in the same frame


def test_b6_subpixel_numerator_signs_and_clamp():
    """With the first minimum at 0 < b < D-1, S[b-1] > minS and S[b+1] >= minS, so the
    denominator S[b-1] + S[b+1] - 2 minS is >= 1: max(., 1) binds only at 1, which the
    low-amplitude shifted-noise cases reach."""
    pos = neg = at1 = 0
    for c in cases(family="shifted"):
        if c.D < 3 or c.W > 3000 or c.band[0] == c.band[1]:
            continue
        C, _, S = volumes(c)
        D = c.D
        b = S.argmin(-1)
        inner = (b > 0) & (b < D - 1)
        mS = S.min(-1)
        sm = np.take_along_axis(S, np.clip(b - 1, 0, D - 1)[..., None], -1)[..., 0]
        sp = np.take_along_axis(S, np.clip(b + 1, 0, D - 1)[..., None], -1)[..., 0]
        den = sm + sp - 2 * mS
        assert (den[inner] >= 1).all()
        pos += int(((sm > sp) & inner).sum())
        neg += int(((sm < sp) & inner).sum())
        at1 += int(((den == 1) & inner).sum())
    print(f"B6 shifted-noise cases: numerator > 0 at {pos} pixels, < 0 at {neg}, denominator == 1 at {at1}")
    assert pos > 1000 and neg > 1000 and at1 >= 1


# the three shapes of test_gpu_sgbm_ragged that compared nothing: independent noise with the
# default filters leaves 0 % of the band valid (speckleWindowSize = 100 > the whole band)
OLD_RAGGED_VACUOUS = {(1, 40): 0.0, (2, 33): 0.0, (5, 17): 0.0}


def test_b7_valid_share_of_every_filtered_case():
    low = []
    shares = {}
    for c in F.CASES:
        s = F.valid_share(c, F.expected(c))
        shares.setdefault(c.group + (":bare" if c.bare else ":filtered"), []).append(s)
        if c.bare:
            assert s == 1.0, c.id                           # uniqueness 0 never fires, nothing else runs
        elif s < 0.25:
            low.append((c.id, s))
    for g, v in sorted(shares.items()):
        print(f"B7 {g}: {len(v)} cases, valid share {min(v):.2f} .. {max(v):.2f}")
    assert not low, low
    for b in F.BATCHES:
        for z, out in enumerate(F.batch_expected(b)):
            s = F.batch_valid_share(b, out)
            print(f"B7 batch {b} frame {z}: valid share {s:.2f}")
            assert s >= 0.25, (b, z)
    for H, W in F.RAGGED_SHAPES:
        rng = np.random.default_rng(H * W)                  # test_gpu_sgbm_ragged's own frames
        L = rng.integers(0, 256, (H, W), dtype=np.uint8)
        R = rng.integers(0, 256, (H, W), dtype=np.uint8)
        old = float((SG.sgbm(L, R, 0, 16, 3)[:, 16:] != -16).mean())
        L, R = F.ragged_shifted(H, W)
        new = float((SG.sgbm(L, R, 0, 16, 3, speckleWindowSize=0)[:, 16:] != -16).mean())
        print(f"B7 ragged {H}x{W}: noise + default filters {old:.2f}, shifted copy + no speckle filter {new:.2f}")
        if (H, W) in OLD_RAGGED_VACUOUS:
            assert old == OLD_RAGGED_VACUOUS[(H, W)]
        assert new >= 0.25


# invalid band pixels (of 369) at uniquenessRatio 0, 1, 50, 99, 100, per C3 frame
C3_INVALID = {("noise", 3): [0, 2, 143, 243, 243], ("noise", 13): [0, 4, 113, 238, 239],
              ("shifted", 3): [0, 2, 129, 241, 244]}


def test_c3_uniqueness_fires_and_grows_with_the_ratio():
    """Each C3 frame: no invalid pixel at u = 0; every u > 0 erases pixels, more with a larger
    u (99 -> 100 may add none: S * 1 < minS * 100 already holds nearly wherever minS > 0), the
    map of every u > 0 differs from the u = 0 map, and >= 25 % of the band stays valid at 100."""
    assert F.C3_RATIOS == (0, 1, 50, 99, 100)
    for (family, win), want in C3_INVALID.items():
        cs = [c for c in cases("c3", family) if c.win == win]
        assert [c.okw["uniquenessRatio"] for c in cs] == list(F.C3_RATIOS)
        maps = [F.expected(c) for c in cs]
        X0, X1 = cs[0].band
        n = [int((m[:, X0:X1] == -16).sum()) for m in maps]
        print(f"C3 {family} win {win}: invalid of {maps[0][:, X0:X1].size} at u = 0, 1, 50, 99, 100: {n}")
        assert n == want
        assert n[0] == 0 < n[1] < n[2] < n[3] <= n[4] <= 0.75 * maps[0][:, X0:X1].size
        for m in maps[1:]:
            assert not np.array_equal(m, maps[0])
            assert ((m == maps[0]) | (m == -16)).all()      # uniqueness only ever erases


FILTER_OFF = {"uniqueness": dict(uniquenessRatio=0), "left-right": dict(disp12MaxDiff=-1),
              "speckle": dict(speckleWindowSize=0)}
# cases per group in which switching that one filter off changes the oracle's map: (cases,
# uniqueness, left-right, speckle).  c2's four run at penalties that keep minS < 0 and show only
# that the filters erase nothing wrongly; c3 and c3b switch one filter on by design
FILTER_FIRES = {"c1filt": (54, 11, 11, 2), "c2": (4, 0, 0, 0), "c3": (12, 12, 0, 0), "c3b": (15, 3, 13, 0),
                "c4": (28, 19, 13, 18), "c5h": (5, 3, 3, 5), "c5neg": (4, 4, 4, 4), "c5pos": (2, 1, 2, 2),
                "cvwin": (5, 4, 3, 4), "cvd": (9, 8, 2, 9)}


def test_b7_filters_fire_where_they_are_on():
    """A filtered case only tests a filter that changes its map.  Per group: in how many cases
    each filter does; the companions of c4, c5h, c5neg, c5pos, cvwin and cvd (noisy frames, small
    penalties) must have every filter fire in at least one case."""
    tab = {}
    for c in F.CASES:
        if c.bare or c.W > 3000:
            continue
        L, R = c.frames()
        t = tab.setdefault(c.group, [0, 0, 0, 0])
        t[0] += 1
        for i, kw in enumerate(FILTER_OFF.values()):
            if not np.array_equal(SG.sgbm(L, R, c.min_disp, c.D, c.win, **{**c.okw, **kw}), F.expected(c)):
                t[i + 1] += 1
    for g, t in tab.items():
        print(f"B7 {g}: {t[0]} filtered cases; uniqueness fires in {t[1]}, left-right in {t[2]}, speckle in {t[3]}")
    assert {g: tuple(t) for g, t in tab.items()} == FILTER_FIRES
    for g in ("c4", "c5h", "c5neg", "c5pos", "cvwin", "cvd"):
        assert min(tab[g][1:]) >= 1, g


def test_c4_reaches_the_scalar_window_row_sums():
    """k_sgbm_vsum (the fallback of k_sgbm_vsum8) runs when win >= 11 and Wb * Dp is no
    multiple of 8: D = 5 at Wb = 25 gives an odd plane of 125."""
    odd = [c for c in cases("c4") if c.win >= 11 and ((c.band[1] - c.band[0]) * sgbm_dp(c.D)) % 2 == 1]
    assert odd and any(c.D == 5 for c in odd)
    assert [sgbm_dp(D) for D in (1, 5, 16, 17, 33, 128, 129, 500)] == [1, 5, 16, 18, 36, 128, 132, 512]
    for c in cases("c4"):
        Wb = c.band[1] - c.band[0]
        assert Wb % 2 == 1 and Wb <= 40


MUTANT_SET = [c for c in F.CASES if c.D <= 40 and c.W <= 3000]
# cases of MUTANT_SET (281) whose map each mutant changes; the counts are asserted so that this
# table stays true when the case list changes
MUTANT_FLIPS = {"last_min": 68, "sat16": 15, "uniq_le": 47, "floor_div": 171, "disp2_left": 5,
                "cost2_inf": 4, "bt_zero_edge": 126, "win_image_cols": 165}


@pytest.mark.parametrize("mutant", sorted(SG.MUTANTS))
def test_b8_mutants_are_caught(mutant):
    """Each deviation, switched on in the oracle, changes the map of at least one case the
    GPU is compared on: a kernel with that deviation could not pass test_sgbm_exact.py."""
    flipped = {}
    for c in MUTANT_SET:
        L, R = c.frames()
        out = SG.sgbm(L, R, c.min_disp, c.D, c.win, mutant=mutant, **c.okw)
        if not np.array_equal(out, F.expected(c)):
            flipped[c.group] = flipped.get(c.group, 0) + 1
    n = sum(flipped.values())
    print(f"B8 {mutant} ({SG.MUTANTS[mutant]}): {n} of {len(MUTANT_SET)} cases change {flipped}")
    assert n >= 1
    assert n == MUTANT_FLIPS[mutant] and len(MUTANT_SET) == 281


def test_mutant_hook_defaults_to_the_definition():
    c = c1("shifted", 63, 13)
    L, R = c.frames()
    np.testing.assert_array_equal(SG.sgbm(L, R, 0, 16, 13, mutant=None, **c.okw), F.expected(c))
    with pytest.raises(AssertionError):
        SG.sgbm(L, R, 0, 16, 13, mutant="no such mutant")
