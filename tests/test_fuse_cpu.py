"""Host pieces of fuse_depth_maps (no GPU): the table builders against the oracle's, the
drop-in's decisions and mode text through a host stand-in for the engine, put_text."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sv_fuse_oracle as FO  # noqa: E402
from stereovision_amd import colormap, fusion  # noqa: E402
from stereovision_amd import fused_depth_map as FDM  # noqa: E402
from stereovision_amd.engine import bilateral_tap_count  # noqa: E402


# ---------------------------------------------------------------------------- tables
@pytest.mark.parametrize("k", [3, 5, 15, 31])
def test_gaussian_kernel_matches_oracle(k):
    c = fusion.gaussian_kernel(k)
    assert c.dtype == np.float32 and c.shape == (k,)
    np.testing.assert_array_equal(c, FO.gauss_kernel(k))
    np.testing.assert_array_equal(c, c[::-1])              # the symmetric form relies on it
    assert abs(float(c.astype(np.float64).sum()) - 1.0) < 1e-6
    assert c.argmax() == k // 2


@pytest.mark.parametrize("k", [1, 2, 4, 33, -3])
def test_gaussian_kernel_rejects_bad_sizes(k):
    with pytest.raises(ValueError):
        fusion.gaussian_kernel(k)


@pytest.mark.parametrize("mn,mx,d,sc,ss", [(0.0, 255.0, 9, 75, 75), (0.0, 255.0, 5, 50, 50),
                                            (0.0, 255.0, 5, 2.0, 50), (-3.5, 17.25, 0, 10, 2),
                                            (0.0, 204.0, 9, 0, -1), (1.0, 1.5, 3, 0.01, 1)])
def test_bilateral_tables_match_oracle(mn, mx, d, sc, ss):
    r, sw, lut, scale = fusion.bilateral_tables(np.float32(mn), np.float32(mx), d, sc, ss)
    er, esw, elut, escale = FO.bilateral_tables(np.float32(mn), np.float32(mx), d, sc, ss)
    assert r == er
    assert sw.dtype == lut.dtype == np.float32 and type(scale) is np.float32
    np.testing.assert_array_equal(sw, esw)
    np.testing.assert_array_equal(lut, elut)
    assert scale == escale
    assert lut.shape == (4098,) and lut[0] == 1.0
    assert sw.size == bilateral_tap_count(r)


def test_bilateral_tap_order():
    r, sw, _, _ = fusion.bilateral_tables(0.0, 255.0, 9, 75, 75)
    assert r == 4 and sw.size == 48
    order = [(dy, dx) for dy in range(-4, 5) for dx in range(-4, 5)
             if (dy, dx) != (0, 0) and dy * dy + dx * dx <= 16]
    assert order == FO.taps(4) and len(order) == 48 and order[0] == (-4, 0) and order[1] == (-3, -2)
    exp = [np.float32(np.exp(np.float64(dy * dy + dx * dx) * (-0.5 / (75.0 * 75.0)))) for dy, dx in order]
    np.testing.assert_array_equal(sw, np.array(exp, np.float32))
    r, sw, _, _ = fusion.bilateral_tables(0.0, 255.0, 5, 50, 50)
    assert r == 2 and sw.size == 12 and len(FO.taps(2)) == 12
    assert fusion.bilateral_tables(0.0, 255.0, 0, 75, 2)[0] == 3          # round(1.5 * 2)
    assert fusion.bilateral_tables(0.0, 255.0, 1, 75, 75)[0] == 1         # max(r, 1)
    assert bilateral_tap_count(7) == 148
    with pytest.raises(ValueError):
        fusion.bilateral_tables(0.0, 255.0, 17, 75, 75)                   # radius 8


def test_bilateral_table_zero_tail():
    _, _, lut, scale = fusion.bilateral_tables(0.0, 255.0, 5, 2.0, 50)
    z = int(np.flatnonzero(lut == 0)[0])
    assert 0 < z < 4098 and np.all(lut[:z] > 0) and np.all(lut[z:] == 0)
    assert np.all(np.diff(lut[:z].astype(np.float64)) <= 0)
    tiny = float(np.finfo(np.float32).tiny)
    assert int(((lut > 0) & (lut < tiny)).sum()) == 39                    # subnormal entries are kept
    # the first zero is where the float64 value rounds to zero in float32
    v = z / float(scale)
    assert np.float32(np.exp(v * v * (-0.5 / 4.0))) == 0
    # a wide sigma never reaches zero: no tail
    assert np.all(fusion.bilateral_tables(0.0, 255.0, 9, 75, 75)[2] > 0)


# ---------------------------------------------------------------------------- drop-in
class _HostFuse:
    """The C ABI's fuse_blend / bilateral contract on host arrays: device pointers are keys
    of a dict, the arithmetic is the oracle's (to test the Python layer without a GPU)."""

    def __init__(self):
        self.bufs = {}
        self.names = {}
        self.calls = []

    def scratch(self, name, nbytes):
        return self.names.setdefault(name, len(self.names) + 1)

    def upload(self, name, a):
        p = self.scratch(name, a.nbytes)
        self.bufs[p] = np.array(a)
        return p

    def to_host(self, p, shape, dtype):
        return self.bufs[p].astype(dtype).reshape(shape)

    def fuse_blend_dev(self, d_fused, H, W, base, d_stereo=0, d_conf=0, d_midas=0, d_flow=0, midas_fill=False,
                       flow_fill=False, stereo_weight=1.0, midas_fill_weight=0.0, conf_threshold=0.0,
                       hole_threshold=0.0, flow_k1=1.0, flow_k2=0.0, coef=None, stats=True, stream=0):
        self.calls.append(("blend", base, bool(midas_fill), bool(flow_fill)))
        g = lambda p: self.bufs[p] if p else None   # noqa: E731
        f32 = np.float32
        if base == 0:
            fused = g(d_stereo) * f32(stereo_weight)
        else:
            fused = (g(d_midas) if base == 1 else g(d_flow)).copy()
        n_midas = n_hole = 0
        if midas_fill:
            conf = g(d_conf) if d_conf else np.ones((H, W), f32)
            assert coef.size == 15
            fw = np.clip(FO.gauss_blur((f32(1) - conf) * f32(midas_fill_weight), coef.size), f32(0), f32(1))
            m = (conf < f32(conf_threshold)) & (fw > f32(0.1))
            n_midas = int(m.sum())
            fused = np.where(m, fused * (f32(1) - fw) + g(d_midas) * fw, fused)
        if flow_fill:
            m = (fused < f32(hole_threshold)) | (fused == 0)
            n_hole = int(m.sum())
            fused = np.where(m, fused * f32(flow_k1) + g(d_flow) * f32(flow_k2), fused)
        self.bufs[d_fused] = fused
        return {"min": fused.min(), "max": fused.max(), "n_midas": n_midas, "n_hole": n_hole}

    def bilateral_f32_dev(self, d_src, H, W, radius, space_w, lut, scale, d_dst_f32=0, d_dst_u8=0, d_dst_bgr=0,
                          cmap=None, minmax=False, stream=0):
        self.calls.append(("bilateral", radius))
        x = self.bufs[d_src]
        if radius:
            x = FO.bilateral(x, 2 * radius + 1, 75, 75)
        q = np.clip(x, np.float32(0), np.float32(255))
        if d_dst_u8:
            self.bufs[d_dst_u8] = q.astype(np.uint8)
        if d_dst_bgr:
            self.bufs[d_dst_bgr] = np.asarray(cmap)[q.astype(np.uint8)]
        return (q.min(), q.max()) if minmax else None


def _maps(H=24, W=40, seed=0):
    rng = np.random.default_rng(seed)
    stereo = (rng.random((H, W)) * 255).astype(np.float32)
    stereo[rng.random((H, W)) < 0.1] = 0
    conf = rng.random((H, W)).astype(np.float32)
    midas = (rng.random((H, W)) * 255).astype(np.float32)
    flow = (rng.random((H, W)) * 255).astype(np.float32)
    return stereo, conf, midas, flow


@pytest.fixture
def host_engine(monkeypatch):
    eng = _HostFuse()
    monkeypatch.setattr(FDM, "get_engine", lambda *a: eng)
    return eng


def test_fuse_depth_maps_none_without_a_valid_method(host_engine):
    s, c, m, f = _maps()
    assert FDM.fuse_depth_maps(None, None, None, None, None, True) is None
    assert FDM.fuse_depth_maps(s, c, m, None, f, True, use_stereo=False, use_midas=False, use_flow=False) is None
    # the flow map alone counts only while the camera moves
    assert FDM.fuse_depth_maps(None, None, None, None, f, False) is None
    assert FDM.fuse_depth_maps(np.zeros((0, 0), np.float32), None, None, None, f, False) is None
    assert host_engine.calls == []


def test_fuse_depth_maps_stereo_base_all_fills(host_engine):
    s, c, m, f = _maps()
    u8, bgr = FDM.fuse_depth_maps(s, c, m, None, f, True)
    exp = FO.fuse(s, c, m, f)
    np.testing.assert_array_equal(u8, exp["u8"])
    np.testing.assert_array_equal(bgr, colormap.table("jet")[u8])
    info = FDM.last_fuse_info
    assert info["mode_parts"] == ["Stereo×0.8", "MiDaS_fill×0.9", "Flow_fill×0.5"]
    assert info["mode_text"] == "Stereo×0.8 + MiDaS_fill×0.9 + Flow_fill×0.5"
    assert (info["n_midas"], info["n_hole"]) == (exp["n_midas"], exp["n_hole"])
    assert info["n_midas"] > 0 and info["n_hole"] > 0
    assert info["range"] == exp["range"]
    assert host_engine.calls == [("blend", 0, True, True), ("bilateral", 4)]


def test_fuse_depth_maps_static_camera_drops_the_flow(host_engine):
    s, c, m, f = _maps()
    u8, _ = FDM.fuse_depth_maps(s, c, m, None, f, False)
    np.testing.assert_array_equal(u8, FO.fuse(s, c, m, None)["u8"])
    assert FDM.last_fuse_info["mode_parts"] == ["Stereo×0.8", "MiDaS_fill×0.9"]
    assert host_engine.calls[0] == ("blend", 0, True, False)


def test_fuse_depth_maps_other_bases_and_switches(host_engine, monkeypatch):
    s, c, m, f = _maps()
    u8, _ = FDM.fuse_depth_maps(s, c, m, None, f, True, use_stereo=False)
    np.testing.assert_array_equal(u8, FO.fuse(None, None, m, f)["u8"])
    assert FDM.last_fuse_info["mode_parts"][0] == "MiDaS_base"
    u8, _ = FDM.fuse_depth_maps(None, None, None, None, f, True)
    np.testing.assert_array_equal(u8, FO.fuse(None, None, None, f)["u8"])
    assert FDM.last_fuse_info["mode_parts"] == ["Flow_base"]
    # confident stereo everywhere: the MiDaS fill is on but changes nothing, and is not named
    u8, _ = FDM.fuse_depth_maps(s + np.float32(20), None, m, None, None, False)
    assert FDM.last_fuse_info["mode_parts"] == ["Stereo×0.8"] and FDM.last_fuse_info["n_midas"] == 0
    # the switches and weights are read at call time
    monkeypatch.setitem(FDM.FUSION_METHODS, "use_midas_fill", False)
    monkeypatch.setitem(FDM.fusion_params, "stereo_weight", 1.2)
    monkeypatch.setitem(FDM.fusion_params, "flow_fill_weight", 0.3)
    u8, _ = FDM.fuse_depth_maps(s, c, m, None, f, True)
    exp = FO.fuse(s, c, m, f, use_midas_fill=False, stereo_weight=1.2, flow_fill_weight=0.3)
    np.testing.assert_array_equal(u8, exp["u8"])
    assert FDM.last_fuse_info["mode_parts"] == ["Stereo×1.2", "Flow_fill×0.3"]
    assert host_engine.calls[-2] == ("blend", 0, False, True)


def test_fuse_depth_maps_small_map_skips_the_bilateral(host_engine):
    s, c, m, f = _maps()
    u8, _ = FDM.fuse_depth_maps(s * np.float32(0.03), c, m * np.float32(0.03), None, None, False)
    assert host_engine.calls[-1] == ("bilateral", 0) and not FDM.last_fuse_info["smoothed"]
    assert u8.max() <= 10


def test_fuse_settings_are_the_reference_defaults():
    assert FDM.FUSION_WEIGHTS == {"stereo_base": 0.8, "midas_max_fill": 0.9, "flow_max_fill": 0.5}
    assert FDM.FUSION_THRESHOLDS["stereo_low_conf"] == 0.5 and FDM.FUSION_THRESHOLDS["flow_hole_threshold"] == 15
    assert FDM.FUSION_SMOOTHING == {"midas_blend_radius": 15, "fusion_bilateral_d": 9,
                                    "fusion_bilateral_sigma": 75}
    assert FDM.FUSION_METHODS == {"use_stereo": True, "use_midas_fill": True, "use_flow_fill": True}
    assert FDM.fusion_params == {"stereo_weight": 0.8, "midas_fill_weight": 0.9, "flow_fill_weight": 0.5,
                                 "stereo_conf_threshold": 0.5, "flow_hole_threshold": 15}


def test_fuse_maps_checks_its_inputs():
    s, c, m, f = _maps()
    eng = _HostFuse()
    with pytest.raises(TypeError):
        fusion.fuse_maps(s.astype(np.float64), c, m, f, engine=eng)
    with pytest.raises(ValueError):
        fusion.fuse_maps(s, c, m[:, :-1], f, engine=eng)
    with pytest.raises(TypeError):
        fusion.fuse_maps(s, c, m, f, engine=eng, no_such_parameter=1)
    with pytest.raises(TypeError):
        fusion.bilateral_filter(s.astype(np.float64), 9, 75, 75, engine=eng)
    with pytest.raises(ValueError):
        fusion.gaussian_blur(s[:7], 15, engine=eng)              # H <= radius
    assert eng.calls == []
    assert fusion.fuse_maps(None, None, None, None, engine=eng) is None


def test_put_text_defaults_unchanged():
    import inspect
    sig = inspect.signature(colormap.put_text)
    assert list(sig.parameters) == ["img", "text", "org", "scale", "color", "thickness"]
    assert sig.parameters["org"].default == (10, 30)
    assert sig.parameters["scale"].default == 0.7
    assert sig.parameters["color"].default == (255, 255, 255)
    assert sig.parameters["thickness"].default == 2
    img = np.zeros((40, 200, 3), np.uint8)
    out = colormap.put_text(img, "x")
    assert out is img
    if colormap.cv2 is None:                                       # a no-op without cv2
        assert not img.any()
        assert not colormap.put_text(img, "x", (5, 20), scale=0.5, color=(0, 255, 0), thickness=1).any()


def test_package_exports_the_new_names():
    import stereovision_amd as sv
    for name in ("gaussian_kernel", "bilateral_tables", "gaussian_blur", "bilateral_filter",
                 "bilateral_filter_dev", "fuse_maps", "fuse_maps_dev", "fuse_depth_maps"):
        assert name in sv.__all__ and callable(getattr(sv, name))
