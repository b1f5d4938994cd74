"""engine.sgbm bit-exact against oracle/sv_sgbm_oracle.py on the hard frames of
tests/sgbm_frames.py: at the window-cost and path-cost bounds, the int16/int32 switch, the
argmin key's ends, ties, every ragged num_disp, bands of 0..25 columns, wholly negative and
large positive ranges, the widest frame, and with every filter off ("bare": the raw
winner-take-all + sub-pixel map, which the filters otherwise overwrite with the same invalid
value on both sides).  tests/test_sgbm_bar.py shows on the CPU that these cases reach those
limits and that each of eight one-line mutants of the oracle changes at least one of them.
"""
import numpy as np
import pytest

import sgbm_frames as F
import sv_sgbm_oracle as SG

pytestmark = pytest.mark.gpu


def run_case(engine, c):
    L, R = c.frames()
    return engine.sgbm(L, R, c.min_disp, c.D, c.win, **c.engine_kw())


def check_group(engine, group, pick=lambda c: True):
    bad = []
    n = 0
    for c in F.CASES:
        if c.group != group or not pick(c):
            continue
        n += 1
        got = run_case(engine, c)
        exp = F.expected(c)
        if not np.array_equal(got, exp):
            bad.append(f"{c.id}: {int((got != exp).sum())} of {exp.size} pixels differ")
    assert n > 0
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cap,win", F.CAP_WIN)
def test_c1_bare_every_family(engine, cap, win):
    """Raw WTA + sub-pixel map (no uniqueness, left-right check or speckle filter) of ramps,
    sawtooth, flat, shifted noise, independent noise and both stripes."""
    check_group(engine, "c1bare", lambda c: c.okw["preFilterCap"] == cap and c.win == win)


@pytest.mark.parametrize("cap,win", F.CAP_WIN)
def test_c1_default_filters(engine, cap, win):
    check_group(engine, "c1filt", lambda c: c.okw["preFilterCap"] == cap and c.win == win)


@pytest.mark.parametrize("family", ["flat", "ramps", "shifted"])
def test_c2_penalties(engine, family):
    """P2 in {32767, 32768, 32769, 349524} with P1 small and P1 = P2 - 1, P1 = 0, P1 = P2 = 0
    (P2 becomes P1 + 1); tiny penalties on low-amplitude frames (the parabola's clamp)."""
    check_group(engine, "c2", lambda c: c.family == family)
    if family == "shifted":
        check_group(engine, "c2sub")


def test_c2_p2_beyond_the_argmin_key(engine):
    L, R = F.frame("flat", 7, 49)
    with pytest.raises(Exception, match="P2 too large"):
        engine.sgbm(L, R, 0, 16, 5, P1=600, P2=349525)
    with pytest.raises(Exception, match="P2 too large"):          # P2 = max(P2, P1 + 1)
        engine.sgbm(L, R, 0, 16, 5, P1=349524, P2=10)


def test_c3_uniqueness(engine):
    """uniqueness_ratio 0, 1, 50, 99, 100 alone, on frames whose minS straddles 0: the oracle
    erases 0, 2, 143, 243, 243 of 369 band pixels on independent noise, and as many on the two
    other frames (tests/test_sgbm_bar.py asserts the counts), so each ratio has its own map."""
    check_group(engine, "c3")
    maps = {c.id: F.expected(c) for c in F.CASES if c.group == "c3" and c.family == "noise" and c.win == 3}
    assert len({m.tobytes() for m in maps.values()}) >= 4       # 99 and 100 may coincide


def test_c3b_left_right_check(engine):
    check_group(engine, "c3b")


@pytest.mark.parametrize("D", [1, 2, 3, 5, 15, 17, 31, 33, 100, 127, 128, 129, 130, 500])
def test_c4_num_disp(engine, D):
    """Every num_disp whose last lane is partly padding, D = 1..3 (no non-neighbour, no inner
    b), the scalar k_sgbm_vsum (D = 5, win 11) and the D > 128 switch, at win 3 and 11."""
    check_group(engine, "c4", lambda c: c.D == D)


@pytest.mark.parametrize("deep", ["0", "2"])
def test_c4_deep_variants(engine, monkeypatch, deep):
    """D in {129, 130, 500} again with SV_SGBM_DEEP (read per call) forcing either form of the
    vertical path + WTA; test_c4_num_disp runs the default."""
    monkeypatch.setenv("SV_SGBM_DEEP", deep)
    check_group(engine, "c4", lambda c: c.D in (129, 130, 500))


def test_c5_band_widths(engine):
    """Wb in {0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25}: around every prefetch depth."""
    check_group(engine, "c5wb")


def test_c5_heights(engine):
    check_group(engine, "c5h")


def test_c5_negative_and_large_positive_ranges(engine):
    """min_disp + D <= 0 (X0 = 0), min_disp large with a short band, and both ends of the
    int16 x16 map: min_disp = -2047 (invalid = -32768) and min_disp + D - 1 = 2047, bare and
    with every filter on (the speckle stage's new value is then -32768)."""
    check_group(engine, "c5neg")
    check_group(engine, "c5pos")
    ids = [c.id for c in F.CASES if c.group == "c5pos"]
    assert any(":m-2047:" in i for i in ids) and any(":m2032:D16:" in i for i in ids)


@pytest.mark.parametrize("cost", ["sgbm", "sad"])
@pytest.mark.parametrize("min_disp,D", [(-2048, 16), (2033, 16), (2047, 2), (-4096, 16), (4096, 1)])
def test_range_beyond_the_int16_map_is_rejected(engine, cost, min_disp, D):
    """(min_disp - 1) * 16 < -32768 or (min_disp + D - 1) * 16 > 32767 would wrap in the map."""
    L, R = F.frame("shifted", 3, 40)
    with pytest.raises(Exception, match="int16 x16 map"):
        engine.disparity(L, R, min_disp, D, 3, cost)
    if cost == "sgbm":
        with pytest.raises(Exception, match="int16 x16 map"):
            engine.sgbm(L, R, min_disp, D, 3)


@pytest.mark.parametrize("min_disp,D", [(-2047, 16), (2032, 16)])
def test_block_matcher_at_the_int16_map_edges(engine, min_disp, D):
    """The block matchers share the map and the bound: both accepted edges against the oracle."""
    import sv_oracle as O
    L, R = F.shifted_noise(2, 2100, shift=min_disp + D // 2, seed=9)
    got = engine.disparity(L, R, min_disp, D, 3, "sad")
    np.testing.assert_array_equal(got, O.disparity16(L, R, min_disp, D, 3))
    assert got.min() >= (min_disp - 1) * 16 and got.max() <= (min_disp + D - 1) * 16


def test_c5_widest_frame(engine):
    """W = 16384: k_sgbm_lrcheck's row of keys takes 128 KiB of dynamic LDS."""
    check_group(engine, "c5wide")
    L, R = F.frame("flat", 2, 16385)
    with pytest.raises(Exception, match="width beyond 16384"):
        engine.sgbm(L, R, 0, 16, 3)


@pytest.mark.parametrize("group", ["cvwin", "cvd"])
def test_variant_cases_with_the_default_switches(engine, group):
    """The cases tests/test_sgbm_variants.py runs under the A/B switches, with none set: win 1..9
    and one num_disp per lane plan of the path kernels (16, 32, 48, 128, 130, 256, 320, 384, 500)."""
    check_group(engine, group)


@pytest.mark.parametrize("fused", ["auto", "1"])
@pytest.mark.parametrize("batch", F.BATCHES, ids=lambda b: "x".join(map(str, b)))
def test_c6_batches(engine, monkeypatch, batch, fused):
    """Shifted noise and sawtooth frames through disparity_batch_dev (cost="sgbm", the
    reference's parameters) at (D 16, win 15: int32 paths) and (D 129, win 5), batches of 8
    and 3, SV_SGBM_FUSED (read per call) auto and forced."""
    if fused != "auto":
        monkeypatch.setenv("SV_SGBM_FUSED", fused)
    nf, H, W, D, win, min_disp = batch
    pitch, rows = W + 8, H + 1
    fs = rows * pitch
    Ls = np.zeros((nf, rows, pitch), np.uint8)
    Rs = np.zeros_like(Ls)
    for z, (L, R) in enumerate(F.batch_frames(*batch)):
        Ls[z, :H, :W], Rs[z, :H, :W] = L, R
    opitch, ofs = W + 4, H * (W + 4) + 16
    dL, dR = engine.dev_alloc(Ls.nbytes), engine.dev_alloc(Rs.nbytes)
    dO = engine.dev_alloc(nf * ofs * 2)
    try:
        engine.to_device(dL, Ls)
        engine.to_device(dR, Rs)
        engine.disparity_batch_dev(dL, dR, nf, H, W, pitch, fs, min_disp, D, win, "sgbm", dO, opitch, ofs)
        engine.synchronize()
        flat = engine.to_host(dO, (nf * ofs,), np.int16)
    finally:
        for p in (dL, dR, dO):
            engine.dev_free(p)
    for z, exp in enumerate(F.batch_expected(batch)):
        got = flat[z * ofs:z * ofs + H * opitch].reshape(H, opitch)[:, :W]
        np.testing.assert_array_equal(got, exp, err_msg=f"frame {z}")


# ------------------------------------------------------------------- filter_speckles, direct
def _both(engine, img, new_val, max_size, max_diff):
    """The kernels twice (equal), then against the oracle; returns the map."""
    img = np.ascontiguousarray(img, np.int16)
    a = engine.filter_speckles(img, new_val, max_size, max_diff)
    b = engine.filter_speckles(img, new_val, max_size, max_diff)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, SG.filter_speckles(img, new_val, max_size, max_diff))
    return a


@pytest.mark.parametrize("max_diff", [0, 1, 65535])
def test_c7_speckles_int16_extremes(engine, max_diff):
    """-32768, -32767 and 32767 side by side: differences of 1, 65534 and 65535 must not wrap
    in 16 bits.  Three 2x3 blocks on a background they cannot join but through max_diff."""
    img = np.full((5, 13), 0, np.int16)
    img[1:3, 1:4], img[1:3, 4:7], img[1:3, 7:10] = -32768, -32767, 32767
    out = _both(engine, img, -16, 11, max_diff)
    if max_diff == 0:                       # three islands of 6 <= 11: all gone; background 47 stays
        exp = img.copy()
        exp[1:3, 1:10] = -16
    elif max_diff == 1:                     # -32768 and -32767 join: 12 > 11 stays; 32767 alone goes
        exp = img.copy()
        exp[1:3, 7:10] = -16
    else:                                   # everything joins
        exp = img
    np.testing.assert_array_equal(out, exp)


@pytest.mark.parametrize("max_diff", [0, 1, 16, 512])
def test_c7_speckles_difference_exactly_max_diff(engine, max_diff):
    """Neighbours that differ by exactly max_diff join, by max_diff + 1 do not."""
    img = np.full((6, 8), 1000, np.int16)
    img[0:3, 0:2] = 3000                    # 6 pixels
    img[0:3, 2:4] = 3000 + max_diff         # 6 more: joins the first block (12 > 8, stays)
    img[3:6, 0:2] = 5000                    # 6 pixels
    img[3:6, 2:4] = 5000 + max_diff + 1     # 6 more, one step too far: two islands of 6, gone
    out = _both(engine, img, -16, 8, max_diff)
    exp = img.copy()
    exp[3:6, 0:4] = -16
    np.testing.assert_array_equal(out, exp)


def _corner_L(n_pixels):
    """An L-shaped region of n_pixels on a 64x64 map with its corner at (31, 31)/(32, 32):
    down column 32 from row 31 and along row 31 to the left from column 31 — pieces in three
    of the four tiles that meet there, joined only across tile borders."""
    img = np.full((64, 64), -16, np.int16)
    img[32, 32] = img[31, 32] = img[31, 31] = 640         # the corner: tiles (1,1), (0,1), (0,0)
    left = n_pixels - 3
    a = left // 2
    img[33:33 + a, 32] = 640                               # down, tile (1,1)
    img[31, 31 - (left - a):31] = 640                      # left, tile (0,0)
    assert int((img == 640).sum()) == n_pixels
    return img


@pytest.mark.parametrize("maxsize", [3, 10, 41])
def test_c7_speckles_region_of_exactly_maxsize_across_a_tile_corner(engine, maxsize):
    """maxsize pixels: erased; maxsize + 1: kept.  The answer is written out."""
    img = _corner_L(maxsize)
    out = _both(engine, img, -16, maxsize, 0)
    assert (out == -16).all()
    img = _corner_L(maxsize + 1)
    out = _both(engine, img, -16, maxsize, 0)
    np.testing.assert_array_equal(out, img)


def test_c7_speckles_four_pieces_in_four_tiles(engine):
    """A 6x6 square centred on the tile corner: 9 pixels in each of four tiles, each piece
    <= maxsize = 9..35, the whole 36 > maxsize: kept; with maxsize 36 it goes.  Beside it a
    background larger than maxsize in every tile (the skipped 'both already large' edges)."""
    img = np.full((64, 64), 320, np.int16)
    img[29:35, 29:35] = 4000
    for maxsize in (9, 20, 35):
        np.testing.assert_array_equal(_both(engine, img, -16, maxsize, 16), img)
    exp = img.copy()
    exp[29:35, 29:35] = -16
    np.testing.assert_array_equal(_both(engine, img, -16, 36, 16), exp)
    # pieces of 10 + 9 + 9 + 9 with maxsize 9: one piece is "large" on its own, the others
    # are not, so no border edge may be skipped
    img2 = np.full((64, 64), -16, np.int16)
    img2[29:35, 29:35] = 4000
    img2[28, 29] = 4000
    np.testing.assert_array_equal(_both(engine, img2, -16, 36, 16), img2)
    assert (_both(engine, img2, -16, 37, 16) == -16).all()


def test_c7_speckles_new_val_occurs_as_data(engine):
    """Pixels equal to new_val are walls: they join nothing and split what they separate."""
    img = np.full((8, 40), 500, np.int16)
    img[:, 5] = 480                          # a wall of new_val = 480 cuts off 8x5 = 40 pixels
    out = _both(engine, img, 480, 100, 32)
    exp = img.copy()
    exp[:, :5] = 480                         # 40 <= 100: gone; the right part (272) stays
    np.testing.assert_array_equal(out, exp)
    out = _both(engine, img, 481, 100, 32)   # 480 is now data within max_diff: one region of 320
    np.testing.assert_array_equal(out, img)
