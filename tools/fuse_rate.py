#!/usr/bin/env python3
"""Rates of the fuse_depth_maps path: the blend and bilateral kernels alone
(HIP events around each launch, median of the runs), fuse_maps_dev on device-resident maps
and fuse_depth_maps on host arrays (wall time), at the fusion app's processing size and at
1080p, beside the NumPy restatement (tests/sv_fuse_oracle.py) on the same box.  Prints one
JSON line.  Not the bench metric."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("SV_WARMUP_AT_IMPORT", "0")
import sv_fuse_oracle as FO  # noqa: E402
from stereovision_amd import colormap, fusion  # noqa: E402
from stereovision_amd import fused_depth_map as FDM  # noqa: E402
from stereovision_amd.engine import get_engine  # noqa: E402

HBM_BYTES_PER_S = 8e12      # the roofline bench.py uses
BLEND_BYTES_PER_PX = 20     # stereo, conf, midas, flow read + fused written, 4 B each
RUNS, WARM = 25, 3


def scene(H, W, seed=0):
    rng = np.random.default_rng(seed)
    stereo = (rng.random((H, W)) * 255).astype(np.float32)
    stereo[rng.random((H, W)) < 0.1] = 0
    conf = rng.random((H, W)).astype(np.float32)
    conf[:, :W // 3] = 1.0
    conf[:H // 2, 2 * W // 3:] = 0.0
    midas = (rng.random((H, W)) * 255).astype(np.float32)
    flow = (rng.random((H, W)) * 255).astype(np.float32)
    return stereo, conf, midas, flow


def kernel_ms(eng, fn):
    """Median device time of the launches of one call (event pair around each launch)."""
    ts = []
    for i in range(WARM + RUNS):
        eng.profile_reset()
        fn()
        ms, n = eng.profile_read("fuse")
        assert n >= 1
        if i >= WARM:
            ts.append(ms)
    return statistics.median(ts)


def wall_ms(fn, runs=RUNS):
    ts = []
    for i in range(WARM + runs):
        t0 = time.perf_counter()
        fn()
        if i >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def measure(eng, H, W):
    s, c, m, f = scene(H, W)
    n = H * W
    d = {k: eng.upload(f"fr_{k}", a) for k, a in (("s", s), ("c", c), ("m", m), ("f", f))}
    d_fused = eng.scratch("fr_fused", 4 * n)
    d_u8 = eng.scratch("fr_u8", n)
    d_bgr = eng.scratch("fr_bgr", 3 * n)
    jet = colormap.table("jet")
    coef = fusion.gaussian_kernel(15)

    def blend(stats=False):
        return eng.fuse_blend_dev(d_fused, H, W, 0, d_stereo=d["s"], d_conf=d["c"], d_midas=d["m"], d_flow=d["f"],
                                  midas_fill=True, flow_fill=True, stereo_weight=0.8, midas_fill_weight=0.9,
                                  conf_threshold=0.5, hole_threshold=15, flow_k1=0.5, flow_k2=0.5, coef=coef,
                                  stats=stats)

    st = blend(True)
    r, sw, lut, scale = fusion.bilateral_tables(st["min"], st["max"], 9, 75, 75)
    eng.profile(True)
    try:
        blend_ms = kernel_ms(eng, blend)
        bil_ms = kernel_ms(eng, lambda: eng.bilateral_f32_dev(d_fused, H, W, r, sw, lut, scale, d_dst_u8=d_u8,
                                                              d_dst_bgr=d_bgr, cmap=jet, minmax=True))
        gauss_ms = kernel_ms(eng, lambda: eng.gauss_blur_f32_dev(d["c"], H, W, coef, d_fused))
    finally:
        eng.profile(False)
    dev_ms = wall_ms(lambda: fusion.fuse_maps_dev(eng, H, W, d["s"], d["c"], d["m"], d["f"], d_fused, d_u8, d_bgr, jet))
    host_ms = wall_ms(lambda: FDM.fuse_depth_maps(s, c, m, None, f, True))
    t0 = time.perf_counter()
    exp = FO.fuse(s, c, m, f)
    oracle_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    FO.bilateral(exp["f32"], 9, 75, 75)
    oracle_bil_ms = (time.perf_counter() - t0) * 1e3
    u8, _ = FDM.fuse_depth_maps(s, c, m, None, f, True)
    return {
        "size": f"{W}x{H}",
        "k_fuse_blend_ms": round(blend_ms, 4),
        "k_fuse_blend_hbm_fraction": round(BLEND_BYTES_PER_PX * n / (blend_ms * 1e-3) / HBM_BYTES_PER_S, 4),
        "k_bilateral_f32_ms": round(bil_ms, 4),
        "bilateral_taps": int(sw.size),
        "bilateral_gtaps_per_s": round(n * sw.size / (bil_ms * 1e-3) / 1e9, 2),
        "k_gauss_f32_k15_ms": round(gauss_ms, 4),
        "fuse_maps_dev_wall_ms": round(dev_ms, 3),
        "fuse_depth_maps_host_wall_ms": round(host_ms, 3),
        "numpy_oracle_fuse_ms": round(oracle_ms, 1),
        "numpy_oracle_bilateral_ms": round(oracle_bil_ms, 1),
        "bit_exact": bool(np.array_equal(u8, exp["u8"])),
    }


def main():
    eng = get_engine(0)
    sizes = [(356, 633), (1080, 1920)]
    print(json.dumps({"tool": "fuse_rate", "runs": RUNS, "results": [measure(eng, H, W) for H, W in sizes]}))


if __name__ == "__main__":
    main()
