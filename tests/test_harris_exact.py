"""Harris, k_median_f32 and bgr_to_gray: bit-exact against the NumPy oracle on adversarial
inputs (tests/harris_frames.py; tests/test_harris_bar.py derives why exact is the bar).

Harris inside the median launch (test_harris_in_median_launch), 2 frames per case, the case
list in harris_frames.MEDIAN_CASES in this order, (H, W, pitch - W, stride - H * pitch):

60-column waves, harris_wave<16,4> in k_median_i16<1,*> (W < 256)
   (8,60,0,0)    one wave exactly, one band of 8 rows (partial band)
   (15,61,1,0)   a second wave of one column; a band one row short; odd pitch
   (16,64,4,0)   a second wave of 4 columns; exactly one band
   (17,121,0,0)  a third wave of one column; a second band of one row; odd H * W: frame 1 of
                 the input starts at an odd address
   (33,255,1,0)  5 waves: a second Harris block with one wave; a third band of one row
   (16,61,4,3)   a frame stride that is no multiple of the pitch
   (17,255,0,0)  the partial second block at the band seam
   (33,64,1,0)   three bands, two waves
248-column waves, harris_wave4<16,4> in k_median_i16<2,*>: every W mod 4 (float4 stores only
at W % 4 == 0; the second wave starts at column 248 and holds 8..12 columns)
   (8,256,0,0) (15,257,0,0) (16,258,4,0) (17,259,1,0) (33,260,0,0)
   (17,256,4,0)  float4 stores with a pitch wider than the frame
   (16,260,1,0)  float4 stores from byte loads (odd pitch)
   (33,257,4,0)  scalar stores, three bands
the second wave starts at the seam (x0 = 248) and is not interior (x0 + 252 > W)
   (8,496,0,0) (16,497,0,0) (17,496,4,0) (33,497,1,0) (15,496,1,0)
the second wave is interior (x0 + 252 <= W): one dword load per lane-row where the frame's
base and the pitch are multiples of 4, byte loads otherwise
   (8,500,0,0) (16,504,0,0) (17,500,4,0) (33,504,4,0)  fast in both frames
   (15,500,0,0)  odd H, H * pitch % 4 == 0: fast in both frames
   (17,504,1,0)  odd H * pitch: slow in both frames (pitch % 4 != 0)
   (16,504,0,2)  stride % 4 == 2: frame 0 fast, frame 1 slow
   (15,504,4,0)  fast with a pad that is never read as data
   (33,500,0,1)  odd stride: frame 0 fast, frame 1 slow
under 8 px a side (harris_frames.SMALL_CASES): the separate Harris launch, k_harris_lds
"""
import numpy as np
import pytest

import harris_frames as F
import sv_oracle as O
import sv_oracle_c as C

pytestmark = pytest.mark.gpu


# ---- stand-alone engine.harris, default dispatch -----------------------------------------
@pytest.mark.parametrize("texture", F.TEXTURES)
@pytest.mark.parametrize("H,W", F.STANDALONE_SHAPES)
def test_harris_standalone(engine, H, W, texture):
    """k_harris_dpp<8,4> (W < 1024) and k_harris_dpp4<8,4> ((11,1030)) at the 8-row band seam
    (H 8, 16, 17), the 60-column wave seam (W 60, 61, 121), past four waves and at the 4-column
    kernel's interior fast loads and ragged last wave."""
    g = F.frame(texture, H, W)
    exp = O.harris(g)
    F.assert_not_vacuous(exp, f"{texture} {H}x{W}")
    np.testing.assert_array_equal(engine.harris(g), exp)


# ---- Harris inside the median launch -----------------------------------------------------
def _right_of(L, z):
    """A right frame the matcher finds something in: the left shifted by a few columns."""
    return np.ascontiguousarray(np.roll(L, -(3 + 2 * z), axis=1))


@pytest.mark.parametrize("case", F.MEDIAN_CASES + F.SMALL_CASES, ids=lambda c: "%dx%d+%d+%d" % c[:4])
def test_harris_in_median_launch(engine, case):
    """sv_depth_map_batch_dev with out.harris: the Harris map of each left frame equals the
    NumPy oracle bit for bit, and depth, disparity and norm stay bit-exact against the C
    oracle.  The pad columns and the gap between the frames hold noise that must never be
    read as data.  The branch each case reaches is listed in the module docstring."""
    H, W, pad, tail, tex = case
    nf, D, win = 2, 32, 7
    pitch, fstride = W + pad, H * (W + pad) + tail
    lefts = F.case_frames(case)
    rights = [_right_of(L, z) for z, L in enumerate(lefts)]
    rng = np.random.default_rng(H * 1000 + W)
    hL = rng.integers(0, 256, nf * fstride, dtype=np.uint8)
    hR = rng.integers(0, 256, nf * fstride, dtype=np.uint8)
    for z in range(nf):
        hL[z * fstride: z * fstride + H * pitch].reshape(H, pitch)[:, :W] = lefts[z]
        hR[z * fstride: z * fstride + H * pitch].reshape(H, pitch)[:, :W] = rights[z]
    n = H * W
    dL, dR = engine.dev_alloc(hL.nbytes), engine.dev_alloc(hR.nbytes)
    outs = [engine.dev_alloc(4 * n * nf), engine.dev_alloc(4 * n * nf), engine.dev_alloc(n * nf),
            engine.dev_alloc(4 * n * nf)]
    try:
        engine.to_device(dL, hL)
        engine.to_device(dR, hR)
        engine.to_device(outs[3], np.full((nf, H, W), np.nan, np.float32))   # every pixel written
        engine.depth_map_batch_dev(dL, dR, nf, H, W, pitch, fstride, 0, D, win, 0.3, 2.0, outs[0],
                                   outs[1], outs[2], d_harris=outs[3])
        depth = engine.to_host(outs[0], (nf, H, W), np.float32)
        disp = engine.to_host(outs[1], (nf, H, W), np.float32)
        norm = engine.to_host(outs[2], (nf, H, W), np.uint8)
        har = engine.to_host(outs[3], (nf, H, W), np.float32)
    finally:
        for p_ in (dL, dR, *outs):
            engine.dev_free(p_)
    for z in range(nf):
        exp = O.harris(lefts[z])
        F.assert_not_vacuous(exp, f"{tex[z]} frame {z}")
        np.testing.assert_array_equal(har[z], exp, err_msg=f"{tex[z]} frame {z}")
        e_depth, e_disp, e_norm = C.depth_map(lefts[z], rights[z], 0, D, win)
        np.testing.assert_array_equal(disp[z], e_disp, err_msg=f"frame {z}")
        np.testing.assert_array_equal(depth[z], e_depth, err_msg=f"frame {z}")
        np.testing.assert_array_equal(norm[z], e_norm, err_msg=f"frame {z}")


# ---- k_median_f32 ------------------------------------------------------------------------
MEDIAN_SHAPES = [(1, 1), (1, 7), (3, 3), (4, 70), (8, 64), (9, 65), (17, 129)]


def _median_values(kind, H, W):
    rng = np.random.default_rng([H, W, len(kind)])
    if kind == "ties":
        return rng.integers(0, 4, (H, W)).astype(np.float32)
    if kind == "constant":
        return np.full((H, W), 2.5, np.float32)
    if kind == "inf":
        a = rng.normal(size=(H, W)).astype(np.float32)
        u = rng.random((H, W))
        a[u < 0.01] = np.inf
        a[u > 0.99] = -np.inf
        return a
    if kind == "zeros":
        return np.where(rng.random((H, W)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    if kind == "subnormal":
        a = (rng.random((H, W)) * 1e-42).astype(np.float32)
        assert (a < np.finfo(np.float32).tiny).all()
        return a
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["ties", "constant", "inf", "zeros", "subnormal"])
@pytest.mark.parametrize("H,W", MEDIAN_SHAPES)
def test_median5_f32_values_and_shapes(engine, H, W, kind):
    """k_median_f32 (sv_median5_f32) against sv_oracle.median5 on and across its 64 x 8 tile and
    below the 5 x 5 window, on heavy ties, a constant, +-inf, signed zeros and subnormals (no
    NaN: the reference's medianBlur defines no answer for it).  The signed-zero maps compare by
    value: assert_array_equal takes +0.0 and -0.0 as equal, and the min/max network may return
    either of two equal elements, so which zero comes out is not specified."""
    a = _median_values(kind, H, W)
    exp = O.median5(a)
    got = engine.median5(a)
    np.testing.assert_array_equal(got, exp)
    if kind != "zeros":     # everything else also bit for bit
        np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))


# ---- bgr_to_gray -------------------------------------------------------------------------
def test_gray_every_bgr_triple(engine):
    """All 2^24 (B, G, R) triples once, as one 4096 x 4096 image, through k_gray."""
    v = np.arange(1 << 24, dtype=np.uint32)
    bgr = np.empty((1 << 24, 3), np.uint8)
    bgr[:, 0] = v & 0xFF
    bgr[:, 1] = (v >> 8) & 0xFF
    bgr[:, 2] = v >> 16
    bgr = bgr.reshape(4096, 4096, 3)
    exp = O.bgr_to_gray(bgr)
    assert exp[0, 0] == 0 and exp[-1, -1] == 255 and np.unique(exp).size == 256
    np.testing.assert_array_equal(engine.gray(bgr), exp)


@pytest.mark.parametrize("W", [1, 3, 4, 5, 63, 65, 257])
def test_gray_vector_tail_widths(engine, W):
    bgr = np.random.default_rng(W).integers(0, 256, (3, W, 3), dtype=np.uint8)
    np.testing.assert_array_equal(engine.gray(bgr), O.bgr_to_gray(bgr))
