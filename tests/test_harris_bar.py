"""Why the Harris kernels are held to exact equality, derived on the CPU.

The response is one fixed sequence of f32 operations (sv_oracle.harris's docstring) on three
integer box sums.  For u8 pixels |gx|, |gy| <= 4 * 255 = 1020, so a 3x3 box of products is at
most 9 * 1020^2 = 9,363,600 < 2^24 in magnitude: the int -> f32 conversion is exact, every
form of the kernel sees the same three floats and only the order of the f32 operations could
move a bit.  Both oracles fix that order, so they must agree with each other bit for bit on
every frame tests/test_harris_exact.py uses, and a kernel that follows it must agree too.
"""
import os

import numpy as np
import pytest

import harris_frames as F
import sv_oracle as O
import sv_oracle_c as C

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "golden_v1.npz")


def _tensor_sums(g):
    """The exact integer Sxx, Sxy, Syy of sv_oracle.harris (reflect-101 of the products)."""
    H, W = g.shape
    gx, gy = O.sobel(g)
    ry = O._reflect101(np.arange(-1, H + 1), H)
    rx = O._reflect101(np.arange(-1, W + 1), W)
    out = []
    for prod in (gx * gx, gx * gy, gy * gy):
        p = prod.astype(np.int64)[ry][:, rx]
        s = np.zeros((H, W), np.int64)
        for j in range(3):
            for i in range(3):
                s += p[j:j + H, i:i + W]
        out.append(s)
    return out


def _all_frames():
    """(label, frame) of every frame the GPU file compares."""
    for H, W in F.STANDALONE_SHAPES:
        for t in F.TEXTURES:
            yield f"{t} {H}x{W}", F.frame(t, H, W)
    for case in F.MEDIAN_CASES + F.SMALL_CASES:
        for z, g in enumerate(F.case_frames(case)):
            yield f"{case[4][z]} {case[0]}x{case[1]} frame {z}", g


def test_box_sums_fit_f32_exactly_and_the_bound_is_reached():
    assert F.SUM_BOUND == 9_363_600 < 1 << 24
    top = 0
    for what, g in _all_frames():
        for s in _tensor_sums(g):
            m = int(np.abs(s).max())
            assert m <= F.SUM_BOUND, what
            np.testing.assert_array_equal(s.astype(np.float32).astype(np.int64), s, err_msg=what)
            top = max(top, m)
    assert top == F.SUM_BOUND
    # the stripes are what reaches it, Sxx for columns and Syy for rows, at every shape
    for H, W in F.STANDALONE_SHAPES:
        sxx, _, _ = _tensor_sums(F.frame("vstripes", H, W))
        _, _, syy = _tensor_sums(F.frame("hstripes", H, W))
        assert sxx.max() == F.SUM_BOUND and syy.max() == F.SUM_BOUND, (H, W)


def test_one_pixel_stripes_would_be_vacuous():
    """Why the stripes and checker cells are two pixels wide: at one pixel the columns x - 1
    and x + 1 (rows y - 1 and y + 1) are equal under reflect-101 and the response is zero."""
    y, x = np.mgrid[0:16, 0:60]
    for g in ((x & 1) * 255, (y & 1) * 255, ((x + y) & 1) * 255):
        assert not O.harris(g.astype(np.uint8)).any()


def test_every_frame_has_a_telling_expected_map():
    for what, g in _all_frames():
        F.assert_not_vacuous(O.harris(g), what)


def test_oracles_agree_bit_for_bit_on_every_frame():
    for what, g in _all_frames():
        a, b = O.harris(g), C.harris(g)
        assert a.dtype == b.dtype == np.float32
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=what)


def test_golden_harris_is_the_oracle_bit_for_bit():
    """What lets test_golden_fixtures_on_gpu compare the fixture's Harris maps exactly."""
    g = np.load(GOLDEN)
    names = sorted(k[:-len("_harris")] for k in g.files if k.endswith("_harris"))
    assert names
    for n in names:
        np.testing.assert_array_equal(g[f"{n}_harris"].view(np.uint32),
                                      O.harris(g[f"{n}_left"]).view(np.uint32), err_msg=n)


@pytest.mark.parametrize("H,W", [(16, 60), (33, 504)])
def test_impulse_footprints_are_5x5(H, W):
    """An impulse's response is confined to its 5x5 neighbourhood: the impulse frames test
    neighbours, reflection and the cross term's sign, nothing further away."""
    g = F.frame("impulses", H, W)
    near = np.zeros((H, W), bool)
    for y, x in F.impulse_points(H, W):
        near[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = True
    r = O.harris(g)
    assert not r[~near].any() and r[near].any()
