"""What the frames of tests/hog_frames.py reach, shown on the CPU with the oracle alone (no
kernel runs): the GPU comparison in tests/test_hog_exact.py is only as hard as these frames.

  * the kernels' boundary constants are the oracle's, and the three formulations of the bin
    (the oracle's eight tests, k_hog_hist's four product pairs, k_hog_hist_cr's base - #{G_k <
    0} on the folded pair, restated here with its packed sign normalisation and int16 dot
    operands) agree on every reachable Sobel pair but (0, 0);
  * the boundary mosaic realises its targets, on both sides of all eight boundaries;
  * the peak frames reach magnitude 191 and window sums of 225 * 127 in one bin, and never
    more than 225 * 191 = 42,975 in the two bins of a packed dword (shares recorded below);
  * the matcher pairs tie where they claim, cost what they claim (recorded below), and name
    every plan of the HOG matcher.
"""
import os
import re

import numpy as np
import pytest

import hog_frames as F
import sv_oracle as O

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stereovision_amd", "csrc",
                   "sv_hog.hip")


def _constants():
    src = open(HIP).read()
    out = []
    for name in ("kHogCos", "kHogSin"):
        m = re.search(r"constexpr\s+int\s+%s\s*\[\s*4\s*\]\s*=\s*\{([^}]*)\}" % name, src)
        assert m, name
        out.append(np.array([int(v) for v in m.group(1).split(",")], np.int64))
    return out


def test_kernel_constants_are_the_oracles():
    kc, ks = _constants()
    np.testing.assert_array_equal(kc, O.HOG_COS[:4])
    np.testing.assert_array_equal(ks, O.HOG_SIN[:4])
    # the fold both kernels rely on: cos[7-k] = -cos[k], sin[7-k] = sin[k]
    np.testing.assert_array_equal(O.HOG_COS[4:], -O.HOG_COS[3::-1])
    np.testing.assert_array_equal(O.HOG_SIN[4:], O.HOG_SIN[3::-1])
    assert (kc > 0).all() and (ks > 0).all() and kc.max() < 1 << 15 and ks.max() < 1 << 15


def _bin_tile(gx, gy, kc, ks):
    """k_hog_hist: the flip, then four pairs of product tests (int32 products)."""
    flip = (gy < 0) | ((gy == 0) & (gx < 0))
    fx, fy = np.where(flip, -gx, gx).astype(np.int32), np.where(flip, -gy, gy).astype(np.int32)
    b = np.zeros(gx.shape, np.int64)
    for k in range(4):
        cy, sx = np.int32(kc[k]) * fy, np.int32(ks[k]) * fx
        b += (cy >= sx).astype(np.int64) + (-cy >= sx)
    return b


def _bin_cr(gx, gy, kc, ks):
    """k_hog_hist_cr: p = (gy << 16) | gx as u16 halves; flip both halves iff the signed value
    gy * 65536 + gx is negative; fold gy by the sign of gx'; four dot products of int16 pairs
    accumulated in int32; b = 4 + (gx' < 0 ? 4 : 0) - #{G_k < 0}."""
    u16 = lambda v: (v & 0xFFFF).astype(np.uint32)
    p = (u16(gy) << np.uint32(16)) | u16(gx)
    vkey = p.view(np.int32).astype(np.int64) - ((p & 0x8000).astype(np.int64) << 1)
    assert (vkey == gy * 65536 + gx).all()
    fm = np.where(vkey < 0, 0xFFFFFFFF, 0).astype(np.uint32)

    def sub_halves(a, m):   # per u16 half: a - m
        lo = ((a & 0xFFFF) - (m & 0xFFFF)) & 0xFFFF
        hi = ((a >> np.uint32(16)) - (m >> np.uint32(16))) & 0xFFFF
        return (hi << np.uint32(16)) | lo
    pn = sub_halves(p ^ fm, fm)
    gm = np.where((pn & 0x8000) != 0, 0xFFFFFFFF, 0).astype(np.uint32)   # gx' < 0
    hm = gm & np.uint32(0xFFFF0000)
    qv = sub_halves(pn ^ hm, hm)
    qx = (qv & 0xFFFF).astype(np.uint16).view(np.int16)
    qy = (qv >> np.uint32(16)).astype(np.uint16).view(np.int16)
    nneg = np.zeros(gx.shape, np.int64)
    for k in range(4):
        wx, wy = np.int16(-ks[k]), np.int16(kc[k])
        G = qx.astype(np.int32) * np.int32(wx) + qy.astype(np.int32) * np.int32(wy)
        nneg += G < 0
    return 4 + (gm & 4).astype(np.int64) - nneg


def test_three_bin_forms_agree_on_every_reachable_pair():
    kc, ks = _constants()
    gx, gy = F.reachable_pairs()
    assert gx.size == 1822741
    ref = F.oracle_bin(gx, gy)
    nz = (gx != 0) | (gy != 0)
    np.testing.assert_array_equal(_bin_tile(gx, gy, kc, ks)[nz], ref[nz])
    np.testing.assert_array_equal(_bin_cr(gx, gy, kc, ks)[nz], ref[nz])
    assert set(np.unique(ref)) == set(range(9))
    # (0, 0): the forms differ, and the magnitude is 0
    z = ~nz
    assert z.sum() == 1 and ref[z][0] == _bin_tile(gx, gy, kc, ks)[z][0] == 8 and _bin_cr(gx, gy, kc, ks)[z][0] == 4
    # the true bounds: magnitude, and so one window's sum over all bins
    assert int(((np.abs(gx) + np.abs(gy)) >> 3).max()) == 191 and F.SUM_BOUND == 42975 < 1 << 16


# ------------------------------------------------------------------------------ boundary
def test_boundary_mosaic_realises_its_targets():
    b = F.boundary()
    n_near = sum(kind == "near" for _, _, kind in b["targets"])
    assert n_near == 1044                       # reachable, magnitude > 0, within 1000 of a boundary
    assert len(b["targets"]) == 1168 and len(b["kept"]) + len(b["dropped"]) == len(b["targets"])
    # dropped: only the odd values on an axis, which no image has (gx = gy mod 2)
    assert sorted(b["dropped"]) == sorted([(1, 0, "axis"), (-1, 0, "axis"), (0, 1, "axis"), (0, -1, "axis")])
    assert len(b["dropped"]) * 20 <= len(b["targets"])          # at most 5 %
    want = np.array([(gx, gy) for gx, gy, _ in b["kept"]])
    for s, frame in enumerate(b["frames"]):
        assert frame.shape == (105, 105 + s) and (frame[:, :s] == 128).all()
        gx, gy = O.sobel(frame)
        ys, xs = np.array(b["centres"]).T
        assert (frame[ys, xs + s] == 128).all()
        np.testing.assert_array_equal(np.stack([gx[ys, xs + s], gy[ys, xs + s]], 1), want)
    # the four shifts put every target in each of a lane's four columns
    assert all({(x + s) % 4 for s in range(4)} == {0, 1, 2, 3} for _, x in b["centres"])


def test_boundary_targets_sit_on_both_sides_of_every_boundary():
    b = F.boundary()
    gx, gy = np.array([(x, y) for x, y, _ in b["kept"]], np.int64).T
    Fk = F.boundary_forms(gx, gy)
    bins = (Fk >= 0).sum(0)
    assert set(bins) == set(range(9))
    for k in range(8):
        close = np.abs(Fk[k]) < F.NEAR
        mag = (np.abs(gx) + np.abs(gy)) >> 3
        # boundary k separates bin k (F_k < 0) from bin k + 1 (F_k >= 0)
        below, above = close & (Fk[k] < 0) & (mag > 0), close & (Fk[k] >= 0) & (mag > 0)
        assert below.sum() >= 20 and above.sum() >= 20, (k, below.sum(), above.sum())
        assert set(bins[below]) == {k} and set(bins[above]) == {k + 1}
    # the axis cases of the sign normalisation, both signs, the smallest even values included
    pairs = set(zip(gx.tolist(), gy.tolist()))
    for v in (2, 4, 1020):
        assert {(v, 0), (-v, 0), (0, v), (0, -v)} <= pairs
    assert F.oracle_bin([-2], [0])[0] == 0 and F.oracle_bin([0], [-2])[0] == 4
    # the largest |gx| + |gy|
    assert sum(abs(x) + abs(y) == 1530 for x, y in pairs) >= 60


# ------------------------------------------------------------------------------ peak
# Per peak frame at win 15: the largest window sum of one bin and the largest sum of the two
# bins that share a packed dword (bins 2k and 2k + 1), as shares of 225 * 191 = 42,975:
# measured by peak_stats below and recorded (the test recomputes and compares).
SHARES = {
    "peak/per4cols/40x257p260": (0.6649, 0.6649),
    "peak/per4cols/33x249p257": (0.6649, 0.6649),
    "peak/per4cols/26x257p318": (0.6649, 0.6649),
    "peak/per4rows/40x257p260": (0.6649, 0.6649),
    "peak/per4rows/33x249p257": (0.6649, 0.6649),
    "peak/per4rows/26x257p318": (0.6649, 0.6649),
    "peak/diag_saw/40x257p260": (0.4450, 0.4450),
    "peak/diag_saw/33x249p257": (0.4450, 0.4450),
    "peak/diag_saw/26x257p318": (0.4450, 0.4450),
    "peak/diag_step/40x257p260": (0.6664, 0.6664),
    "peak/diag_step/33x249p257": (0.6664, 0.6664),
    "peak/diag_step/26x257p318": (0.6664, 0.6664),
    "peak/halves/40x257p260": (0.6649, 0.6679),
    "peak/halves/33x249p257": (0.6649, 0.6679),
    "peak/halves/26x257p318": (0.6649, 0.6679),
}


def peak_stats(f, win=15):
    h = O.hog_hist(f.image, win).astype(np.int64)
    pair = [h[2 * k] + (h[2 * k + 1] if 2 * k + 1 < 9 else 0) for k in range(5)]
    return int(h.max()), int(max(p.max() for p in pair))


PEAK = [f for f in F.HIST_FRAMES if f.group == "peak"]


def test_peak_frames_reach_the_magnitude_and_sum_bounds():
    assert {f.id for f in PEAK} == set(SHARES)
    assert {(f.H, f.W) for f in PEAK} == set(F.PEAK_SIZES) and len(PEAK) == 15
    top_mag, top_sum, top_pair = 0, 0, 0
    for f in PEAK:
        _, mag = O.hog_pixel(f.image)
        top_mag = max(top_mag, int(mag.max()))
        one, two = peak_stats(f)
        assert one <= two <= F.SUM_BOUND, f.id
        assert abs(one / F.SUM_BOUND - SHARES[f.id][0]) < 5e-5 and abs(two / F.SUM_BOUND - SHARES[f.id][1]) < 5e-5, \
            (f.id, one / F.SUM_BOUND, two / F.SUM_BOUND)
        top_sum, top_pair = max(top_sum, one), max(top_pair, two)
        if f.name == "diag_step":
            assert int(mag.max()) == 191, f.id
        if f.name in ("per4cols", "per4rows"):
            assert one == 225 * 127, f.id
        if f.name == "halves":   # both halves of dword 0 large inside one window
            h = O.hog_hist(f.image, 15).astype(np.int64)
            assert int(np.minimum(h[0], h[1]).max()) >= 8000, f.id
    assert top_mag == 191 and top_sum >= 28575 and top_pair <= F.SUM_BOUND
    assert F.HIST_SENTINEL > F.SUM_BOUND


# ------------------------------------------------------------------------------ edge
def test_edge_frames_put_the_axis_cases_on_the_image_border():
    EDGE = [f for f in F.HIST_FRAMES if f.group == "edge"]
    seen = set()
    for f in EDGE:
        (win,) = f.wins
        r = win // 2
        hl, nout = F.cr_geometry(r)
        gx, gy = O.sobel(f.image)
        for col in (0, f.W - 1):
            assert (gx[:, col] == 0).all() and (gy[:, col] > 500).any() and (gy[:, col] < -500).any(), f.id
        for row in (0, f.H - 1):
            assert (gy[row] == 0).all() and (gx[row] > 500).any() and (gx[row] < -500).any(), f.id
        x0 = (f.W - 1) // nout * nout
        seen.add((r, "j", (f.W - 1 - x0) % 4, x0 > 0))
        if x0 > 0 and f.W - 1 - (x0 - nout) < nout + 4 * hl:
            seen.add((r, "halo", (f.W - 1 - x0) // 4))
    assert {r for r, *_ in seen} == set(F.EDGE_RADII) and [F.cr_geometry(r)[0] for r in F.EDGE_RADII] == [0, 1, 1, 2]
    for r in F.EDGE_RADII:
        for j in range(4):
            assert (r, "j", j, False) in seen and (r, "j", j, True) in seen
        for lane in range(F.cr_geometry(r)[0]):
            assert (r, "halo", lane) in seen
    # every frame's two bands cut a 24-row strip and a 16-row tile
    for f in F.HIST_FRAMES:
        (a, c), (c2, z) = F.row_bands(f.H)
        assert a == 0 and c == c2 and z == f.H and c % 24 and c % 16
    assert {f.group: f.wins for f in F.HIST_FRAMES if f.group != "edge"} == {"boundary": (1, 3), "peak": (1, 7, 9, 15)}
    assert all(f.pitch > f.W for f in F.HIST_FRAMES)


# ------------------------------------------------------------------------------ matcher pairs
# The largest cost over (row, band column, disparity) of every case: measured by case_stats
# below and recorded (the test recomputes and compares).  2 * win^2 * 191 bounds them.
COSTS = {
    "noise/noise,s=-4/1x212p212/md-7,D64,w1": 120,
    "noise/noise,s=62/5x73p80/md0,D64,w7": 2302,
    "flat/flat/9x74p136/md9,D64,w15": 0,
    "high/cols_rows/9x81p84/md0,D64,w15,rows=0:4+4:9": 41910,
    "high/cols_flat/5x215p220/md-7,D64,w7": 6223,
    "noise/noise,s=4/5x245p252/md0,D96,w7,rows=1:4": 2815,
    "noise/noise,s=103/9x122p184/md9,D96,w15": 8958,
    "flat/flat/1x99p100/md-7,D96,w1": 0,
    "high/cols_rows/9x106p112/md9,D96,w15,rows=2:7": 26670,
    "high/cols_flat/5x113p176/md0,D96,w15,rows=1:4": 28575,
    "per8/per8/9x123p124/md9,D96,w15": 5749,
    "tie/tie,k=0/5x244p244/md0,D96,w7": 2550,
    "tie/tie,k=0/9x254p260/md9,D96,w15": 8243,
    "tie/tie,k=40/9x246p308/md-7,D96,w7": 3017,
    "noise/noise,s=14/9x287p348/md9,D128,w15,rows=2:7": 6966,
    "noise/noise,s=119/1x131p132/md-7,D128,w1": 111,
    "flat/flat/5x130p136/md0,D128,w7": 0,
    "high/cols_rows/9x277p340/md-7,D128,w15": 41910,
    "high/cols_flat/5x138p140/md9,D128,w7": 2667,
    "per8/per8/5x287p292/md9,D128,w1": 211,
    "noise/noise,s=-1/1x343p344/md-7,D192,w1": 120,
    "noise/noise,s=190/5x201p208/md0,D192,w7": 2966,
    "flat/flat/9x202p264/md9,D192,w15": 0,
    "high/cols_rows/9x209p212/md0,D192,w15,rows=0:4+4:9": 41910,
    "high/cols_flat/5x343p348/md-7,D192,w15,rows=1:4": 28575,
    "per8/per8/9x210p272/md9,D192,w7": 2538,
    "noise/noise,s=7/5x404p408/md0,D256,w7": 2786,
    "noise/noise,s=263/9x282p344/md9,D256,w15": 9756,
    "flat/flat/1x259p260/md-7,D256,w1": 0,
    "high/cols_rows/9x266p272/md9,D256,w15,rows=2:7": 26670,
    "high/cols_flat/5x273p336/md0,D256,w7": 6223,
    "per8/per8/5x414p416/md9,D256,w15": 6624,
    "noise/noise,s=17/9x542p604/md9,D384,w15,rows=2:7": 8083,
    "noise/noise,s=375/1x387p388/md-7,D384,w1": 111,
    "flat/flat/5x386p392/md0,D384,w7": 0,
    "high/cols_rows/9x533p596/md-7,D384,w15": 41910,
    "high/cols_flat/5x394p396/md9,D384,w15,rows=1:4": 13335,
    "per8/per8/9x398p404/md9,D384,w1": 202,
    "tie/tie,k=0/5x541p544/md9,D384,w7": 2958,
    "tie/tie,k=0/9x533p540/md-7,D384,w15": 6769,
    "tie/tie,k=40/9x534p596/md0,D384,w7": 3153,
    "noise/noise,s=2/1x662p664/md-7,D512,w1": 121,
    "noise/noise,s=510/5x521p528/md0,D512,w7": 2763,
    "flat/flat/9x522p584/md9,D512,w15": 0,
    "high/cols_rows/9x529p532/md0,D512,w15,rows=0:4+4:9": 41910,
    "high/cols_flat/5x663p668/md-7,D512,w7": 6223,
    "per8/per8/5x669p732/md9,D512,w7": 1425,
    "tie/tie,k=0/5x660p660/md-7,D512,w7": 2641,
    "tie/tie,k=0/9x661p668/md0,D512,w15": 8929,
    "tie/tie,k=40/9x671p732/md9,D512,w7": 3312,
    "noise/noise,s=10/1x212p216/md0,D61,w15": 10620,
    "noise/noise,s=68/9x73p136/md9,D61,w1": 229,
    "flat/flat/1x64p64/md-7,D61,w1": 0,
    "high/cols_rows/9x71p76/md9,D61,w15,rows=2:7": 26670,
    "high/cols_flat/5x78p140/md0,D61,w15,rows=1:4": 28575,
    "tie/tie,k=0/5x209p212/md0,D61,w7": 2455,
    "tie/tie,k=0/9x219p224/md9,D61,w15": 8062,
    "tie/tie,k=40/9x211p272/md-7,D61,w7": 2868,
    "noise/noise,s=20/5x247p308/md9,D90,w1": 270,
    "noise/noise,s=81/1x99p100/md-7,D90,w7": 1400,
    "flat/flat/5x92p96/md0,D90,w7": 0,
    "high/cols_rows/9x239p300/md-7,D90,w15": 41910,
    "high/cols_flat/5x100p100/md9,D90,w7": 2667,
    "per8/per8/5x249p256/md9,D90,w1": 221,
    "noise/noise,s=5/9x274p276/md-7,D125,w7": 3067,
    "noise/noise,s=123/5x142p148/md0,D125,w15": 7484,
    "flat/flat/9x135p196/md9,D125,w15": 0,
    "high/cols_rows/9x142p144/md0,D125,w15,rows=0:4+4:9": 41910,
    "high/cols_flat/5x276p280/md-7,D125,w15,rows=1:4": 28575,
    "per8/per8/9x143p204/md9,D125,w7": 2164,
    "tie/tie,k=0/5x273p276/md-7,D125,w7": 2537,
    "tie/tie,k=0/9x274p280/md0,D125,w15": 7508,
    "tie/tie,k=40/9x284p344/md9,D125,w7": 3611,
    "noise/noise,s=13/1x330p336/md0,D180,w15": 9255,
    "noise/noise,s=187/9x192p252/md9,D180,w1": 217,
    "flat/flat/1x183p184/md-7,D180,w1": 0,
    "high/cols_rows/9x190p196/md9,D180,w15,rows=2:7": 26670,
    "high/cols_flat/5x197p260/md0,D180,w7": 6223,
    "per8/per8/5x338p340/md9,D180,w15": 4785,
    "noise/noise,s=23/5x410p472/md9,D250,w1,rows=1:4": 277,
    "noise/noise,s=241/1x259p260/md-7,D250,w7": 2233,
    "flat/flat/5x252p256/md0,D250,w7": 0,
    "high/cols_rows/9x399p460/md-7,D250,w15": 41910,
    "high/cols_flat/5x260p260/md9,D250,w15,rows=1:4": 13335,
    "per8/per8/9x264p268/md9,D250,w1": 230,
    "tie/tie,k=0/5x407p408/md9,D250,w7": 2738,
    "tie/tie,k=0/9x399p404/md-7,D250,w15": 6146,
    "tie/tie,k=40/9x400p460/md0,D250,w7": 3352,
    "noise/noise,s=8/9x528p528/md-7,D380,w7": 2928,
    "noise/noise,s=378/5x397p404/md0,D380,w15": 7224,
    "flat/flat/9x390p452/md9,D380,w15": 0,
    "high/cols_rows/9x397p400/md0,D380,w15,rows=0:4+4:9": 41910,
    "high/cols_flat/5x531p536/md-7,D380,w7": 6223,
    "per8/per8/5x537p600/md9,D380,w7": 1579,
    "noise/noise,s=16/1x658p664/md0,D509,w15": 13455,
    "noise/noise,s=516/9x521p584/md9,D509,w1": 196,
    "flat/flat/1x512p512/md-7,D509,w1": 0,
    "high/cols_rows/9x519p524/md9,D509,w15,rows=2:7": 26670,
    "high/cols_flat/5x526p588/md0,D509,w15,rows=1:4": 28575,
    "per8/per8/9x536p536/md9,D509,w15": 6240,
    "tie/tie,k=0/5x657p660/md0,D509,w7": 2816,
    "tie/tie,k=0/9x667p672/md9,D509,w15": 10674,
    "tie/tie,k=40/9x659p720/md-7,D509,w7": 3069,
    "wide/noise,s=11/5x364p368/md0,D64,w7": 2473,
    "wide/cols_rows/9x320p320/md-7,D61,w15": 41910,
    "batch/noise,s=17/5x662p668/md0,D512,w15,nf2": 9542,
}


def case_stats(k):
    """(largest cost, fewest tying disparities at a band pixel, fewest at the planted pixels)."""
    top, ties, planted = 0, k.D, None
    for L, R in k.images():
        t = F.tie_geometry(k.W, k.D, k.min_disp, k.win, k.fkw.get("k", 0)) if k.family == "tie" else None
        for y, C in F.cost_rows(L, R, k):
            top = max(top, int(C.max()))
            n = (C == C.min(axis=1, keepdims=True)).sum(axis=1)
            ties = min(ties, int(n.min()))
            if t:
                X0 = k.band[0]
                sel = slice(t["t0"] - X0, t["t1"] - X0)
                assert (C[sel, t["d0"] - k.min_disp] == 0).all() and (C[sel, t["d1"] - k.min_disp] == 0).all()
                assert ((C[sel] == 0).sum(axis=1) == 2).all(), k.id
                planted = (int(n[sel].min()), int(n[sel].max()))
    return top, ties, planted


@pytest.fixture(scope="module")
def stats():
    return {k.id: case_stats(k) for k in F.CASES}


def test_costs_match_the_table_and_pass_15_bits(stats):
    assert set(COSTS) == set(stats)
    for cid, (top, _, _) in stats.items():
        k = F.BY_ID[cid]
        assert top == COSTS[cid], (cid, top)
        assert top < 2 * k.win * k.win * 191 <= O.max_cost(k.win, O.COST_HOG)
    high = [k for k in F.CASES if k.family == "cols_rows"]
    assert len(high) >= 14 and all(k.win == 15 and k.H == 9 for k in high)
    # 225 * 127 in bin 0 against 105 * 127 in bin 4 at every d; a band that is column W-1 alone
    # (min_disp >= 0, one matched column) sees 105 * 127 twice: L's last column has gx = 0 and
    # fills 8 of the window's 15 columns
    for k in high:
        assert COSTS[k.id] == (26670 if k.band_width == 1 and k.min_disp >= 0 else 41910), k.id
    for pl in set(F.PLANS.values()):
        assert any(COSTS[k.id] == 41910 >= 1 << 15 for k in high if F.plan_of(k.D) == pl), pl
    assert all(v < 1 << 15 for cid, v in COSTS.items() if F.BY_ID[cid].family != "cols_rows")


def test_ties_are_where_the_cases_claim(stats):
    for k in F.CASES:
        _, ties, planted = stats[k.id]
        if k.family in F.ALL_TIE:
            assert ties >= 8, (k.id, ties)
        if k.family in ("flat", "cols_flat", "cols_rows"):
            assert ties == k.D, (k.id, ties)
        if k.family == "tie":
            assert planted == (2, 2), (k.id, planted)
            t = F.tie_geometry(k.W, k.D, k.min_disp, k.win, k.fkw.get("k", 0))
            assert t["t1"] - t["t0"] >= 20 and t["d1"] - k.min_disp in (k.D - 5, 43), k.id
    assert {509, 512} <= {k.D for k in F.CASES if k.family == "tie"}


def test_table_covers_plans_windows_heights_widths_and_offsets():
    from stereovision_amd.engine import plan
    C = F.CASES
    assert sorted({k.D for k in C}) == sorted(F.D_LIST)
    named = set()
    for k in C:
        p = plan(k.D, k.win, "hog")
        assert (p["dpl"], p["lpg"]) == F.plan_of(k.D), (k.id, p)
        named.add((p["dpl"], p["lpg"]))
    assert named == {(4, 16), (6, 16), (8, 16), (6, 32), (8, 32), (6, 64), (8, 64)}
    for D, sib in F.SIBLING.items():
        assert F.plan_of(D) == F.plan_of(sib) and sib < D == F.plan_of(D)[0] * F.plan_of(D)[1]
    for pl in named:
        mine = [k for k in C if F.plan_of(k.D) == pl]
        assert {"flat", "cols_rows", "cols_flat", "noise"} <= {k.family for k in mine}, pl
        assert {k.win for k in mine} == {1, 7, 15} and {k.H for k in mine} >= {1, 5, 9}, pl
        assert {k.min_disp for k in mine} == {-7, 0, 9}, pl
        assert 1 in {k.band_width for k in mine}, pl
        assert any(k.band_width == 2 * (k.win // 2) + 3 for k in mine) and any(k.band_width >= 148 for k in mine), pl
        assert any(len(k.bands) > 1 or k.bands[0] != (0, k.H) for k in mine), pl
    assert all(k.band_width == k.W - k.D - max(k.min_disp, 0) > 0 for k in C)
    assert all(k.W <= k.D + 160 for k in C if k.group != "wide")
    # a band wider than one wave's columns at D = 64 (4 groups of 64 columns)
    assert any(k.D == 64 and k.band_width > 256 for k in C if k.group == "wide")
    assert any(k.nf == 2 and k.D == 512 and k.frame_stride() > k.pitch * k.H for k in C)
    assert any(k.family == "per8" for k in C) and all(k.min_disp == 9 for k in C if k.family == "per8")
    for k in C[::9]:   # padding differs between L and R in every padded column
        for L, R in k.frames():
            assert L.shape == (k.H, k.pitch) and (L[:, k.W:] != R[:, k.W:]).all()


if __name__ == "__main__":   # prints the SHARES and COSTS tables
    for f in PEAK:
        one, two = peak_stats(f)
        print(f'    "{f.id}": ({one / F.SUM_BOUND:.4f}, {two / F.SUM_BOUND:.4f}),')
    print()
    for k in F.CASES:
        top, ties, planted = case_stats(k)
        print(f'    "{k.id}": {top},   # ties >= {ties}' + (f", planted {planted}" if planted else ""))
