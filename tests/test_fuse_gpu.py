"""fuse_depth_maps and its filters on the GPU, bit-exact against the NumPy restatement
(tests/sv_fuse_oracle.py).  Shapes: 8x8 (every pixel touches reflected borders on all sides,
the Gaussian radius 7 at its minimum size), 9x17, 37x70 (odd, several 16x64 tiles, partial
tiles on both axes) and the fusion app's processing size 356x633 once per function."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sv_fuse_oracle as FO  # noqa: E402
from stereovision_amd import colormap, fusion  # noqa: E402
from stereovision_amd import fused_depth_map as FDM  # noqa: E402
from stereovision_amd.engine import SVError  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = [(8, 8), (9, 17), (37, 70)]
APP = (356, 633)


def _rand(shape, seed, lo=0.0, hi=255.0):
    rng = np.random.default_rng(seed)
    return (lo + rng.random(shape) * (hi - lo)).astype(np.float32)


def _fuse_launches(engine):
    return engine.profile_read("fuse")[1]


# ---------------------------------------------------------------------------- Gaussian
@pytest.mark.parametrize("shape,k", [(s, 15) for s in SMALL + [APP]] + [((37, 70), 3), ((37, 70), 31)])
def test_gaussian_blur_bit_exact(engine, shape, k):
    x = _rand(shape, 1, -1.0, 1.0)
    got = fusion.gaussian_blur(x, k)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, FO.gauss_blur(x, k))


# ---------------------------------------------------------------------------- bilateral
@pytest.mark.parametrize("shape,d,sc,ss", [(s, 9, 75, 75) for s in SMALL + [APP]] +
                         [(s, 5, 50, 50) for s in SMALL])
def test_bilateral_random_maps_bit_exact(engine, shape, d, sc, ss):
    x = _rand(shape, 2)
    np.testing.assert_array_equal(fusion.bilateral_filter(x, d, sc, ss), FO.bilateral(x, d, sc, ss))


def test_bilateral_subnormal_table_and_last_bin(engine):
    """sigma_color 2 over [0, 255]: 39 subnormal table entries, a zero tail, and |v - c| = 255
    lands on index 4096 (the N + 2 entries suffice)."""
    x = _rand((37, 70), 3)
    x[5, 7], x[5, 8] = 0.0, 255.0
    x[20:24, 30:34] = np.float32(100.0) + _rand((4, 4), 4, 0.0, 6.0)      # some weights well above zero
    chk = {}
    exp = FO.bilateral(x, 5, 2.0, 50, check=chk)
    assert chk["max_idx"] == 4096
    np.testing.assert_array_equal(fusion.bilateral_filter(x, 5, 2.0, 50), exp)


def test_bilateral_step_edge_constant_and_sigma_radius(engine):
    step = np.full((37, 70), 40.0, np.float32)
    step[:, 33:] = 200.0
    step[18:, :10] = 90.0
    np.testing.assert_array_equal(fusion.bilateral_filter(step, 9, 75, 75), FO.bilateral(step, 9, 75, 75))
    const = np.full((9, 17), 12.5, np.float32)
    got = fusion.bilateral_filter(const, 9, 75, 75)                       # the copy path
    np.testing.assert_array_equal(got, const)
    x = _rand((37, 70), 5)
    assert FO.bilateral_radius(0, 2) == 3
    np.testing.assert_array_equal(fusion.bilateral_filter(x, 0, 30, 2), FO.bilateral(x, 0, 30, 2))
    np.testing.assert_array_equal(fusion.bilateral_filter(x, 15, 40, 3), FO.bilateral(x, 15, 40, 3))   # radius 7


# ---------------------------------------------------------------------------- fuse_depth_maps
def _scene(shape, seed):
    """Stereo in [0, 255] with ~10 % zero holes; conf = {0, 1} blobs mixed with uniform values
    (both sides of the threshold and of fw > 0.1 occur); MiDaS and flow maps."""
    H, W = shape
    rng = np.random.default_rng(seed)
    stereo = _rand(shape, seed + 100)
    stereo[rng.random(shape) < 0.1] = 0
    conf = rng.random(shape).astype(np.float32)
    conf[:, :int(0.4 * W)] = 1.0                     # wider than the blur from 37x70 on: fw reaches 0 there
    conf[:H // 2, int(0.7 * W):] = 0.0
    conf[H // 2, :3] = 0.25                          # low confidence where the blurred weight stays small
    midas = _rand(shape, seed + 200)
    flow = _rand(shape, seed + 300)
    return stereo, conf, midas, flow


def _check_fuse(res, exp):
    u8, bgr = res
    info = FDM.last_fuse_info
    np.testing.assert_array_equal(u8, exp["u8"])
    np.testing.assert_array_equal(bgr, colormap.table("jet")[u8])
    assert (info["n_midas"], info["n_hole"]) == (exp["n_midas"], exp["n_hole"])
    assert info["range"][0] == exp["range"][0] and info["range"][1] == exp["range"][1]
    assert info["smoothed"] == exp["smoothed"]
    return info


@pytest.mark.parametrize("shape", SMALL + [APP])
def test_fuse_stereo_base_both_fills(engine, shape):
    s, c, m, f = _scene(shape, 7)
    exp = FO.fuse(s, c, m, f)
    info = _check_fuse(FDM.fuse_depth_maps(s, c, m, None, f, True), exp)
    assert exp["n_midas"] > 0 and exp["n_hole"] > 0
    if shape[1] >= 70:
        # every combination of the two conditions of the MiDaS mask occurs (the smaller maps
        # are narrower than the blur: fw > 0.1 everywhere)
        fw = np.clip(FO.gauss_blur((np.float32(1) - c) * np.float32(0.9), 15), 0, 1)
        for low in (False, True):
            for big in (False, True):
                assert (((c < 0.5) == low) & ((fw > 0.1) == big)).any(), (low, big)
    assert info["mode_parts"][0] == "Stereo×0.8" and info["mode_parts"][-1] == "Flow_fill×0.5"


@pytest.mark.parametrize("shape", [(9, 17), (37, 70)])
def test_fuse_other_bases_and_switches(engine, shape, monkeypatch):
    s, c, m, f = _scene(shape, 8)
    m[1, 2] = 0.0                                                   # a hole in the MiDaS base
    # MiDaS base + flow fill; flow base; static camera (no flow)
    info = _check_fuse(FDM.fuse_depth_maps(None, None, m, None, f, True), FO.fuse(None, None, m, f))
    assert info["mode_parts"] == ["MiDaS_base", "Flow_fill×0.5"]
    info = _check_fuse(FDM.fuse_depth_maps(s, c, m, None, f, True, use_stereo=False, use_midas=False),
                       FO.fuse(None, None, None, f))
    assert info["mode_parts"] == ["Flow_base"]
    _check_fuse(FDM.fuse_depth_maps(s, c, m, None, f, False), FO.fuse(s, c, m, None))
    # stereo_conf=None: ones, the fill weight is zero everywhere
    info = _check_fuse(FDM.fuse_depth_maps(s, None, m, None, f, True), FO.fuse(s, None, m, f))
    assert info["n_midas"] == 0
    # each fill switched off
    monkeypatch.setitem(FDM.FUSION_METHODS, "use_midas_fill", False)
    _check_fuse(FDM.fuse_depth_maps(s, c, m, None, f, True), FO.fuse(s, c, m, f, use_midas_fill=False))
    monkeypatch.setitem(FDM.FUSION_METHODS, "use_midas_fill", True)
    monkeypatch.setitem(FDM.FUSION_METHODS, "use_flow_fill", False)
    info = _check_fuse(FDM.fuse_depth_maps(s, c, m, None, f, True), FO.fuse(s, c, m, f, use_flow_fill=False))
    assert info["n_hole"] == 0


def test_fuse_non_default_parameters(engine, monkeypatch):
    s, c, m, f = _scene((37, 70), 9)
    for k, v in dict(stereo_weight=1.3, midas_fill_weight=0.6, flow_fill_weight=0.3,
                     stereo_conf_threshold=0.7, flow_hole_threshold=30).items():
        monkeypatch.setitem(FDM.fusion_params, k, v)
    monkeypatch.setitem(FDM.FUSION_SMOOTHING, "midas_blend_radius", 7)
    monkeypatch.setitem(FDM.FUSION_SMOOTHING, "fusion_bilateral_d", 5)
    monkeypatch.setitem(FDM.FUSION_SMOOTHING, "fusion_bilateral_sigma", 40)
    exp = FO.fuse(s, c, m, f, stereo_weight=1.3, midas_fill_weight=0.6, flow_fill_weight=0.3,
                  stereo_conf_threshold=0.7, flow_hole_threshold=30, midas_blend_radius=7, bilateral_d=5,
                  bilateral_sigma=40)
    info = _check_fuse(FDM.fuse_depth_maps(s, c, m, None, f, True), exp)
    assert info["mode_parts"] == ["Stereo×1.3", "MiDaS_fill×0.6", "Flow_fill×0.3"]
    assert exp["range"][1] == 255.0                                 # 1.3 x stereo is clipped


def test_fuse_small_map_skips_the_bilateral(engine):
    s, c, m, f = _scene((37, 70), 10)
    k = np.float32(0.03)
    exp = FO.fuse(s * k, c, m * k, f * k)
    assert not exp["smoothed"]
    _check_fuse(FDM.fuse_depth_maps(s * k, c, m * k, None, f * k, True), exp)


# ---------------------------------------------------------------------------- errors, device variants
def test_rejected_arguments_launch_nothing(engine):
    engine.profile(True)
    try:
        engine.synchronize()
        before = _fuse_launches(engine)
        x = _rand((37, 4), 11)
        d_x = engine.upload("fuse_t_x", x)
        d_y = engine.scratch("fuse_t_y", x.nbytes)
        with pytest.raises((SVError, ValueError)):
            fusion.bilateral_filter(x, 9, 75, 75)                     # W = 4 <= radius 4
        with pytest.raises((SVError, ValueError)):
            fusion.gaussian_blur(x, 15)                               # W = 4 <= radius 7
        r, sw, lut, scale = fusion.bilateral_tables(0.0, 255.0, 9, 75, 75)
        with pytest.raises(SVError) as ei:
            engine.bilateral_f32_dev(d_x, 37, 4, r, sw, lut, scale, d_dst_f32=d_y)
        assert ei.value.code == -22 and "radius" in str(ei.value)
        with pytest.raises(SVError) as ei:
            engine.gauss_blur_f32_dev(d_x, 37, 4, fusion.gaussian_kernel(15), d_y)
        assert ei.value.code == -22
        with pytest.raises(SVError):
            engine.gauss_blur_f32_dev(d_x, 37, 4, np.ones(4, np.float32), d_y)   # even ksize
        big = _rand((37, 70), 12)
        with pytest.raises((SVError, ValueError)):
            fusion.bilateral_filter(big, 17, 75, 75)                  # radius 8
        with pytest.raises(SVError) as ei:
            engine.bilateral_f32_dev(engine.upload("fuse_t_b", big), 37, 70, 8, np.ones(196, np.float32),
                                     lut, scale, d_dst_f32=engine.scratch("fuse_t_c", big.nbytes))
        assert ei.value.code == -22
        with pytest.raises(SVError):
            engine.bilateral_f32_dev(0, 37, 70, r, sw, lut, scale, d_dst_f32=d_y)   # null source
        with pytest.raises(SVError):
            engine.fuse_blend_dev(d_y, 37, 4, 0, d_stereo=d_x, d_midas=d_x, midas_fill=True,
                                  coef=fusion.gaussian_kernel(15))    # W <= Gaussian radius
        with pytest.raises(SVError):
            engine.fuse_blend_dev(d_y, 37, 4, 1, d_stereo=d_x)        # MiDaS base without its map
        with pytest.raises(TypeError):
            fusion.bilateral_filter(big.astype(np.float64), 9, 75, 75)
        with pytest.raises(TypeError):
            fusion.gaussian_blur(big.astype(np.float64), 15)
        with pytest.raises(TypeError):
            FDM.fuse_depth_maps(big.astype(np.float64), None, None, None, None, False)
        with pytest.raises(ValueError):
            FDM.fuse_depth_maps(big, big[:, :-1], None, None, None, False)
        engine.synchronize()
        assert _fuse_launches(engine) == before
        fusion.gaussian_blur(big, 15)                                 # a good call is counted
        assert _fuse_launches(engine) == before + 1
    finally:
        engine.profile(False)


def test_device_pointer_variants_match_the_host_variants(engine):
    shape = (37, 70)
    H, W = shape
    s, c, m, f = _scene(shape, 13)
    up = engine.upload
    d_s, d_c, d_m, d_f = up("fuse_t_s", s), up("fuse_t_cf", c), up("fuse_t_m", m), up("fuse_t_f", f)
    d_fused = engine.scratch("fuse_t_fused", 4 * H * W)
    d_u8 = engine.scratch("fuse_t_u8", H * W)
    d_bgr = engine.scratch("fuse_t_bgr", 3 * H * W)
    info = fusion.fuse_maps_dev(engine, H, W, d_s, d_c, d_m, d_f, d_fused, d_u8, d_bgr, colormap.table("jet"))
    u8, bgr, hinfo = fusion.fuse_maps(s, c, m, f, cmap=colormap.table("jet"))
    np.testing.assert_array_equal(engine.to_host(d_u8, shape, np.uint8), u8)
    np.testing.assert_array_equal(engine.to_host(d_bgr, shape + (3,), np.uint8), bgr)
    assert info["range"] == hinfo["range"] and info["n_midas"] == hinfo["n_midas"]
    np.testing.assert_array_equal(u8, FO.fuse(s, c, m, f)["u8"])
    # the stand-alone filter on device pointers, and its f32 output beside the quantised ones
    d_out = engine.scratch("fuse_t_out", 4 * H * W)
    fusion.bilateral_filter_dev(engine, d_s, H, W, s.min(), s.max(), 9, 75, 75, d_out)
    host = fusion.bilateral_filter(s, 9, 75, 75)
    np.testing.assert_array_equal(engine.to_host(d_out, shape, np.float32), host)
    r, sw, lut, scale = fusion.bilateral_tables(s.min(), s.max(), 9, 75, 75)
    mn, mx = engine.bilateral_f32_dev(d_s, H, W, r, sw, lut, scale, d_dst_f32=d_out, d_dst_u8=d_u8, minmax=True)
    np.testing.assert_array_equal(engine.to_host(d_out, shape, np.float32), host)
    q = np.clip(host, np.float32(0), np.float32(255))
    np.testing.assert_array_equal(engine.to_host(d_u8, shape, np.uint8), q.astype(np.uint8))
    assert (mn, mx) == (q.min(), q.max())
    # the blend alone: the float32 map and its statistics
    st = engine.fuse_blend_dev(d_fused, H, W, 0, d_stereo=d_s, d_conf=d_c, d_midas=d_m, d_flow=d_f,
                               midas_fill=True, flow_fill=True, stereo_weight=0.8, midas_fill_weight=0.9,
                               conf_threshold=0.5, hole_threshold=15, flow_k1=0.5, flow_k2=0.5,
                               coef=fusion.gaussian_kernel(15))
    exp = FO.fuse(s, c, m, f)
    assert (st["n_midas"], st["n_hole"]) == (exp["n_midas"], exp["n_hole"])
    fused = engine.to_host(d_fused, shape, np.float32)
    assert st["min"] == fused.min() and st["max"] == fused.max()
    gb = engine.scratch("fuse_t_gb", 4 * H * W)
    engine.gauss_blur_f32_dev(d_s, H, W, fusion.gaussian_kernel(5), gb)
    np.testing.assert_array_equal(engine.to_host(gb, shape, np.float32), FO.gauss_blur(s, 5))
