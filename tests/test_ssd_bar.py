"""What the cases of tests/ssd_frames.py reach, shown on the CPU from the frames alone (int64
NumPy, no kernel code): the GPU comparison in tests/test_ssd_exact.py is only as hard as these
frames are.

The matrix-core kind's 32-bit key of output column x and candidate x' = x - d is, before the
offset that makes it unsigned (ssd_shape's comment, sv_ssd_mfma.hip),

    key = M * (val - bias) - ix' - 2 M * Cor(x),     val = SR2(x') - 2 X(x, x'),

with SR2 and X the window sums of R'^2 and L' R' (L' = L - 128, R' = R - 128, replicate-clamped
images), ix' the column index of x' in the block, and Cor(x) the sum of L' over the window's
columns of every row that has entered the block band so far (one term per row step; it never
leaves the accumulators).  ssd_shape bounds |key| by R = M * hw + 2 M * (hb + win) * win * 128
+ the index range, hw the half-width of val about bias, and needs R < 2^31.

  * val - bias reaches -hw within 1 (L = R = 0: exactly).  Its largest value is win^2 * 48896,
    the maximum of r^2 - 2 l r over int8 pairs (l = 127, r = -128), below hw + bias = cmax =
    win^2 * 65025: cmax is the largest COST, reached at SL2 = win^2 * 127^2 > 0, so val = C -
    SL2 never attains it.  The top of the range has that much slack; the bottom has none.
  * |Cor| reaches 128 * win * (rows in the block band + win - 1) on every L = 0 frame.
  * The extremes combine at L = R = 255 (val - bias = -hw + 255 win^2, -2 M Cor negative) and
    at L = 0, R = 255: the reached half-width, as a fraction of R, is recorded per case below.
"""
import zlib

import numpy as np
import pytest

import ssd_frames as F

RANGE_FAMILIES = ("sat_lo", "sat_hi", "near_top", "near_bottom")


def _block_bands(r0, r1, hb):
    return [(y0, min(r1, y0 + hb)) for y0 in range(r0, r1, hb)]


def key_stats(k):
    """Over every frame, launch and block band of the case: min and max of val - bias, the
    largest |Cor| per block-band height, and the largest |key| / R of a launch (each launch
    against the R ssd_shape computes for its rows)."""
    H, W, D, win, md = k.H, k.W, k.D, k.win, k.min_disp
    r = win // 2
    X0, X1 = max(md + D, 0), min(W + min(md, 0), W)
    xs = np.arange(X0, X1)[:, None]
    ds = np.arange(md, md + D)[None, :]
    st = dict(vmin=None, vmax=None, cor={}, frac=0.0)
    for Lu, Ru in k.images():
        Lq, Rq = Lu.astype(np.int64) - 128, Ru.astype(np.int64) - 128
        hX = np.zeros((H, X1 - X0, D), np.int64)
        hS = np.zeros_like(hX)
        hL = np.zeros((H, X1 - X0), np.int64)
        for i in range(win):
            lc = np.clip(xs - r + i, 0, W - 1)
            rc = np.clip(xs - r + i - ds, 0, W - 1)
            lv, rv = Lq[:, lc], Rq[:, rc]          # (H, bw, 1), (H, bw, D)
            hX += lv * rv
            hS += rv * rv
            hL += lv[:, :, 0]
        T = hS - 2 * hX
        for r0, r1 in k.bands:
            s = F.shape(win, D, r1 - r0)
            M, XW = s["M"], 128 * s["xt"]
            ixp = ((xs - X0) % XW) + (md + D - 1 - ds)                 # (bw, D)
            assert ixp.min() >= 0 and ixp.max() < 32 * (4 * s["xt"] + s["nt"] - 1)
            for y0, y1 in _block_bands(r0, r1, s["hb"]):
                ys = np.arange(y0, y1)
                val = sum(T[np.clip(ys - r + j, 0, H - 1)] for j in range(win))      # (rows, bw, D)
                entered = np.clip(y0 - r + np.arange(y1 - y0 + win - 1), 0, H - 1)
                cor = np.cumsum(hL[entered], axis=0)[win - 1:]                        # (rows, bw)
                key = M * (val - s["bias"]) - ixp[None] - 2 * M * cor[:, :, None]
                vb = val - s["bias"]
                st["vmin"] = int(vb.min()) if st["vmin"] is None else min(st["vmin"], int(vb.min()))
                st["vmax"] = int(val.max()) if st["vmax"] is None else max(st["vmax"], int(val.max()))
                st["cor"][y1 - y0] = max(st["cor"].get(y1 - y0, 0), int(np.abs(cor).max()))
                assert int(np.abs(key).max()) < s["R"] < 1 << 31, (k.id, (r0, r1), (y0, y1))
                st["frac"] = max(st["frac"], int(np.abs(key).max()) / s["R"])
    return st


# The reached half-width of the 64-bit key as a fraction of ssd_shape's R, per case: measured by
# key_stats above and recorded (the test recomputes and compares).  1.0 would be the bound.
FRACTIONS = {
    "inst/sat_lo/7x65p68/md0,D32,w13": 0.9842,
    "inst/sat_hi/8x162p168/md0,D32,w15": 0.9933,
    "inst/sat_lo/9x195p260/md0,D64,w13": 0.9832,
    "inst/sat_hi/7x97p100/md0,D64,w15": 0.9933,
    "inst/sat_lo/8x226p232/md0,D96,w13": 0.9837,
    "inst/sat_hi/9x227p292/md0,D96,w15": 0.9933,
    "inst/sat_lo/7x161p164/md0,D128,w13": 0.9842,
    "inst/sat_hi/8x258p264/md0,D128,w15": 0.9933,
    "inst/sat_lo/9x291p356/md0,D160,w9": 0.9814,
    "inst/sat_hi/7x193p196/md0,D160,w11": 0.9931,
    "inst/sat_lo/8x322p328/md0,D192,w9": 0.9820,
    "inst/sat_hi/9x323p388/md0,D192,w11": 0.9931,
    "inst/sat_lo/7x257p260/md0,D224,w9": 0.9827,
    "inst/sat_hi/8x354p360/md0,D224,w11": 0.9931,
    "inst/sat_lo/9x387p452/md0,D256,w9": 0.9814,
    "inst/sat_hi/7x289p292/md0,D256,w11": 0.9931,
    "inst/sat_lo/8x194p200/md0,D64,w1": 0.9404,
    "inst/sat_hi/9x259p324/md0,D128,w3": 0.9917,
    "width/sat_lo/6x163p228/md0,D160,w9": 0.9834,
    "width/sat_hi/6x287p292/md0,D256,w11": 0.9931,
    "width/sat_lo/6x129p132/md0,D96,w13": 0.9846,
    "width/sat_hi/6x160p224/md0,D32,w15": 0.9933,
    "width/sat_lo/6x194p200/md0,D64,w13": 0.9847,
    "width/sat_lo/5x383p388/md0,D128,w15": 0.9854,
    "width/sat_hi/5x258p260/md0,D128,w15": 0.9933,
    "short/sat_hi/2x65p72/md0,D32,w13": 0.9932,
    "short/near_bottom/4x65p132/md0,D32,w13": 0.9856,
    "short/sat_hi/6x65p72/md0,D32,w13": 0.9932,
    "short/near_bottom/12x65p132/md0,D32,w13": 0.9818,
    "short/sat_lo/1x191p196/md0,D160,w9": 0.9868,
    "short/near_top/4x191p192/md0,D160,w9": 0.5971,
    "short/sat_lo/5x191p196/md0,D160,w9": 0.9841,
    "short/near_top/8x191p192/md0,D160,w9": 0.5986,
    "short/sat_lo/9x191p196/md0,D160,w9": 0.9814,
    "tall/near_bottom,L=255/63x198p204/md0,D160,w9": 0.9930,
    "tall/sat_lo/64x103p168/md0,D64,w15": 0.9618,
    "tall/near_top/64x232p232/md0,D192,w11": 0.6107,
    "tall/sat_hi/65x65p72/md0,D32,w13": 0.9932,
    "tall/sat_lo/95x167p168/md0,D128,w15": 0.9499,
    "tall/near_top/95x200p204/md0,D160,w11": 0.6163,
    "tall/near_bottom,L=255/95x65p132/md0,D32,w13": 0.9932,
    "tall/sat_hi/96x102p104/md0,D64,w15": 0.9933,
    "tall/near_top/96x295p300/md0,D256,w9": 0.6121,
    "tall/sat_lo/97x193p196/md0,D160,w9": 0.9455,
    "tall/sat_lo/129x166p172/md0,D128,w13": 0.9580,
    "tall/sat_hi/129x263p328/md0,D224,w11": 0.9931,
    "tall96/sat_lo/256x66p68/md0,D32,w9": 0.9258,
    "tall96/near_top/257x197p204/md0,D160,w9": 0.6202,
    "tall96/sat_hi/289x103p168/md0,D64,w9": 0.9930,
    "tall96/near_top/289x296p296/md0,D256,w7": 0.6284,
    "tall96/near_bottom,L=255/256x162p168/md0,D128,w5": 0.9924,
    "tall96/sat_lo/256x229p296/md0,D192,w11": 0.9528,
    "mindisp/sat_hi/8x135p140/md3,D64,w15": 0.9933,
    "mindisp/sat_hi/8x199p204/md-5,D128,w13": 0.9932,
    "mindisp/sat_lo/8x201p204/md-130,D128,w13": 0.9837,
    "mindisp/sat_lo/8x233p236/md3,D160,w11": 0.9830,
    "mindisp/sat_lo/8x105p108/md-5,D32,w13": 0.9837,
    "mindisp/sat_hi/8x107p172/md-34,D32,w13": 0.9932,
    "bands/sat_lo/21x98p100/md0,D64,w15,rows=0:1+1:21": 0.9871,
    "bands/sat_lo/150x99p104/md0,D64,w15,rows=0:20+20:130+130:150": 0.9793,
    "bands/sat_hi/21x164p228/md0,D128,w13,rows=0:1+1:21": 0.9932,
    "bands/sat_hi/150x165p168/md0,D128,w13,rows=0:20+20:130+130:150": 0.9932,
    "bands/near_top/21x293p296/md0,D256,w11,rows=0:1+1:21": 0.6000,
    "bands/near_top/150x294p300/md0,D256,w11,rows=0:20+20:130+130:150": 0.6093,
    "batch/sat_hi/9x97p100/md0,D64,w13,nf3": 0.9932,
    "batch/sat_lo/70x197p264/md0,D160,w9,nf3": 0.9417,
    "batch/near_bottom/3x34p40/md0,D32,w15,nf3": 0.9863,
    "range/near_bottom,L=0,p=0.01/64x97p100/md0,D64,w15": 0.9619,
    "range/near_bottom,L=0,p=0.01/95x66p72/md0,D32,w13": 0.9444,
    "range/near_bottom,L=0,p=0.01/256x195p260/md0,D160,w9": 0.9258,
    "range/near_bottom,L=255,p=0.01/95x166p168/md0,D128,w15": 0.9933,
    "range/near_bottom,L=255,p=0.01/64x225p232/md0,D192,w11": 0.9931,
    "range/near_bottom,L=255,p=0.01/289x66p132/md0,D32,w9": 0.9930,
    "range/near_top,L=255,p=0.01/64x131p132/md0,D96,w15": 0.5784,
    "range/near_top,L=255,p=0.01/256x262p268/md0,D224,w9": 0.5567,
    "range/near_top,L=255,p=0.01/95x193p260/md0,D160,w11": 0.5634,
    "range/near_top,L=0,p=0.01/95x98p100/md0,D64,w15": 0.6148,
    "range/near_top,L=0,p=0.01/128x291p296/md0,D256,w11": 0.6135,
    "range/near_top,L=0,p=0.01/257x166p232/md0,D128,w9": 0.6244,
    "host4/sat_lo/9x96p96/md0,D64,w15": 0.9838,
    "host4/sat_hi/10x196p200/md0,D160,w9": 0.9930,
    "host4/sat_lo/11x260p324/md0,D128,w13": 0.9823,
    "pitch/sat_lo/10x325p332/md0,D192,w9": 0.9807,
    "pitch/sat_lo/10x292p296/md0,D256,w11": 0.9819,
    "pitch/sat_lo/10x192p196/md0,D128,w15": 0.9834,
}


RANGE_CASES = [k for k in F.CASES if k.family in RANGE_FAMILIES]


@pytest.fixture(scope="module")
def stats():
    return {k.id: key_stats(k) for k in RANGE_CASES}


def test_key_halfwidth_stays_below_R_and_matches_the_table(stats):
    assert set(FRACTIONS) == set(stats)
    for cid, st in stats.items():
        k = F.BY_ID[cid]
        n = k.win * k.win
        hw = F.shape(k.win, k.D, 1)["hw"]
        assert -hw <= st["vmin"] and st["vmax"] <= n * 48896 < n * 65025, cid
        assert st["frac"] < 1, cid   # (key_stats asserts it launch by launch)
        assert abs(st["frac"] - FRACTIONS[cid]) < 5e-5, (cid, st["frac"])
    # the table comes close to the bound somewhere: a frame family that never left the middle
    # of the range would pass the line above too
    assert max(FRACTIONS.values()) > 0.95


def test_val_reaches_both_ends(stats):
    """Bottom: L = 0 against sparse {0, 1} noise has windows with at most one R pixel at 1
    (val - bias <= -hw + 1).  Top: L = 255 against sparse {0, 1} noise has an all-zero window
    (val = win^2 * 48896 exactly)."""
    lo = [k for k in RANGE_CASES if k.family == "near_bottom" and k.fkw.get("L") == 0 and k.fkw.get("p") == 0.01]
    hi = [k for k in RANGE_CASES if k.family == "near_top" and k.fkw.get("L") == 255 and k.fkw.get("p") == 0.01]
    assert len(lo) >= 3 and len(hi) >= 3
    for k in lo:
        hw = F.shape(k.win, k.D, 1)["hw"]
        assert -hw <= stats[k.id]["vmin"] <= -hw + 1, k.id
    for k in hi:
        assert stats[k.id]["vmax"] == k.win * k.win * 48896, k.id
    # the saturated frames see both ends from one launch
    for k in RANGE_CASES:
        if k.family in ("sat_lo", "sat_hi") and k.band_width >= 2 * (k.win + 1):
            n, hw = k.win * k.win, F.shape(k.win, k.D, 1)["hw"]
            st = stats[k.id]
            assert st["vmin"] <= -hw + 256 * n and st["vmax"] >= n * 48896 - 512 * n, k.id


def test_correction_term_is_maximal_at_every_band_height(stats):
    """|Cor| = 128 * win * (rows + win - 1) in every block band of every L = 0 frame; the table
    has such frames at hb = 64, hb = 96, a single band of 95 rows and a last band of one row."""
    seen = set()
    for k in RANGE_CASES:
        if k.family == "sat_lo" or (k.family.startswith("near") and k.fkw.get("L", 0) == 0):
            for rows, c in stats[k.id]["cor"].items():
                assert c == 128 * k.win * (rows + k.win - 1), (k.id, rows)
            for r0, r1 in k.bands:
                s = F.shape(k.win, k.D, r1 - r0)
                seen.add((s["hb"], r1 - r0 > s["hb"]))   # (band height, several block bands)
                if (r1 - r0) % s["hb"] == 1 and r1 - r0 > 1:
                    seen.add("last band of one row")
    assert {(64, True), (96, True), (95, False), (64, False), "last band of one row"} <= seen


def _row_costs(L, R, y, k):
    """Brute-force SSD cost volume of row y: [band column, disparity]."""
    H, W, r = k.H, k.W, k.win // 2
    X0, X1 = max(k.min_disp + k.D, 0), min(W + min(k.min_disp, 0), W)
    xs = np.arange(X0, X1)[:, None]
    ds = np.arange(k.min_disp, k.min_disp + k.D)[None, :]
    Lq, Rq = L.astype(np.int64), R.astype(np.int64)
    C = np.zeros((X1 - X0, k.D), np.int64)
    for j in range(-r, r + 1):
        yy = min(max(y + j, 0), H - 1)
        for i in range(-r, r + 1):
            d = Lq[yy, np.clip(xs + i, 0, W - 1)] - Rq[yy, np.clip(xs + i - ds, 0, W - 1)]
            C += d * d
    return C, X0, X1


PERIODIC = [k for k in F.CASES if k.family == "periodic" and k.nf == 1 and k.band_width >= 32]


@pytest.mark.parametrize("k", PERIODIC, ids=lambda k: k.id)
def test_periodic_frames_plant_ties(k):
    """At more than half of the band's pixels of the middle row at least two disparities share
    the minimum (nick: lie within 1 of it); the oracle takes the smallest.  nick: somewhere a
    candidate costs exactly 1 more than the minimum, and the map differs from the plain
    frame's, i.e. a nick decides a winner."""
    (L, R), = k.images()
    nick = bool(k.fkw.get("nick"))
    exp = F.expected(k.id)[0]
    by_one = False
    for y in range(k.H) if nick else [k.H // 2]:
        C, X0, X1 = _row_costs(L, R, y, k)
        best = C.min(axis=1, keepdims=True)
        np.testing.assert_array_equal(exp[y, X0:X1], (k.min_disp + C.argmin(axis=1)) * 16)
        by_one = by_one or bool((C == best + 1).any())
        if y == k.H // 2:
            near = (C <= best + (1 if nick else 0)).sum(axis=1)
            assert (near >= 2).sum() * 2 > X1 - X0, (near >= 2).mean()
    if nick:
        import sv_oracle_c as O
        rng = np.random.default_rng(zlib.crc32(f"{k.id}#0".encode()))
        L0, R0 = F.periodic(rng, k.H, k.W, k.win, **dict(k.fkw, nick=False))
        np.testing.assert_array_equal(L0, L)
        assert (R0 != R).any() and (np.abs(R0.astype(int) - R) <= 1).all()
        assert (O.disparity16(L0, R0, k.min_disp, k.D, k.win, 1) != exp).any()
        assert by_one


def test_table_covers_residues_heights_instances_and_paths():
    C = F.CASES
    md0 = [k for k in C if k.min_disp == 0]
    # widths
    for res in range(4):
        assert sum(k.W % 4 == res for k in C if k.group == "width") >= 2, res
    assert {1, 2, 3, 5, 31, 33, 127, 129, 130, 131} <= {k.band_width for k in md0 if F.shape(k.win, k.D, k.H)["xt"] == 1}
    assert {255, 257} <= {k.band_width for k in md0 if F.shape(k.win, k.D, k.H)["xt"] == 2}
    assert {k.pitch - F.pitch0(k.W) for k in C} == {0, 4, 64}
    # heights
    hs = {k.H for k in C}
    assert {1, 2, 4, 5, 6, 63, 64, 65, 95, 96, 97, 129} <= hs
    assert any(k.H == k.win - 1 for k in C) and any(k.H == k.win for k in C)
    assert {256, 257, 289} <= {k.H for k in C if k.win <= 9 and F.shape(k.win, k.D, k.H)["hb"] == 96}
    assert any(k.H == 256 and k.win == 11 and F.shape(11, k.D, 256)["hb"] == 64 for k in C)
    assert all(k.band_width <= 40 for k in C if k.H >= 63)
    # the 16 instances, each at W % 4 != 0 on a saturated frame; windows 1 and 3
    got = {F.instance(k.win, k.D, k.H) for k in C if k.W % 4 and k.family in ("sat_lo", "sat_hi")
           and k.bands == [(0, k.H)]}
    assert len(F.INSTANCES) == 16 and set(F.INSTANCES) <= got
    assert {(D, w) for D in (32, 64, 96, 128) for w in (13, 15)} | \
           {(D, w) for D in (160, 192, 224, 256) for w in (9, 11)} <= {(k.D, k.win) for k in C if k.W % 4}
    assert {1, 3} <= {k.win for k in C}
    assert all(F.shape(k.win, k.D, r1 - r0) for k in C for r0, r1 in k.bands)
    # min_disp, bands, batches, D >= 160
    for k in C:
        if k.group == "mindisp":
            assert k.min_disp in (-5, 3, -(k.D + 2))
    assert {m if m in (-5, 3) else "far" for m in (k.min_disp for k in C if k.group == "mindisp")} == {-5, 3, "far"}
    assert any(k.bands == [(0, 1), (1, k.H)] for k in C)
    assert any(len(k.bands) == 3 and any(r1 - r0 > 64 and r0 % 64 for r0, r1 in k.bands) for k in C)
    assert all(k.frame_stride(k.pitch) % 4 == 0 and k.frame_stride(k.pitch) > k.pitch * k.H
               for k in C if k.nf > 1) and any(k.nf == 3 for k in C)
    for g in ("bands", "batch", "pitch"):
        assert any(k.D >= 160 for k in C if k.group == g), g
    # padding differs between L and R in every padded column
    for k in C[::7]:
        for L, R in k.frames(k.pitch + 4):
            assert (L[:, k.W:] != R[:, k.W:]).all()


def test_shape_restatement_matches_the_library_query():
    """ssd_frames.shape against sv_ssd_mfma_query (host code: nothing is launched) for every
    launch of the table, at the case's pitch (the matrix-core kind) and the odd one (not)."""
    from stereovision_amd.engine import ssd_mfma_query
    for k in F.CASES:
        for r0, r1 in k.bands:
            fs = k.frame_stride(k.pitch) if k.nf > 1 else 0
            q = ssd_mfma_query(4096, 8192, k.H, k.W, k.pitch, k.min_disp, k.D, k.win, "ssd", r0, r1, k.W + 8, k.nf, fs)
            s = F.shape(k.win, k.D, r1 - r0)
            assert q["mfma"] and all(q[n] == s[n] for n in ("xt", "nt", "mb", "hb", "big")), (k.id, q, s)
            q = ssd_mfma_query(4096, 8192, k.H, k.W, F.odd_pitch(k.W), k.min_disp, k.D, k.win, "ssd", r0, r1,
                               k.W + 8, k.nf, fs)
            assert not q["mfma"], (k.id, q)
    # an odd base or frame stride alone, an empty matched band and another cost: not this kind
    assert not ssd_mfma_query(4097, 8192, 20, 200, 200, 0, 64, 9)["mfma"]
    assert not ssd_mfma_query(4096, 8192, 20, 200, 200, 0, 64, 9, n_frames=2, frame_stride=4002)["mfma"]
    assert ssd_mfma_query(4096, 8192, 20, 200, 200, 0, 64, 9, n_frames=1, frame_stride=4002)["mfma"]
    assert not ssd_mfma_query(4096, 8192, 20, 60, 60, 0, 64, 9)["mfma"]
    assert not ssd_mfma_query(4096, 8192, 20, 200, 200, 0, 64, 9, "sad")["mfma"]
    assert not ssd_mfma_query(4096, 8192, 20, 200, 200, 0, 64, 9, row0=7, row1=7)["mfma"]
    assert ssd_mfma_query(4096, 8192, 20, 300, 300, 0, 160, 13)["mfma_only"]


if __name__ == "__main__":   # prints the FRACTIONS table
    for k in RANGE_CASES:
        st = key_stats(k)
        print(f'    "{k.id}": {st["frac"]:.4f},')
