#!/usr/bin/env python3
"""Rates of the optical-flow path: each kernel of sv_flow.hip alone (HIP events
around its launch, median of the runs), farneback_flow_dev on device-resident frames and one
OpticalFlowDepthEstimator call on a host frame (wall time), at the fusion app's processing size
and at 1080p, beside the NumPy restatement (tests/sv_flow_oracle.py) on the same box.  Prints
one JSON line.  Not the bench metric."""
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
import flow_scenes as S  # noqa: E402
import sv_flow_oracle as O  # noqa: E402
from stereovision_amd import flow as F  # noqa: E402
from stereovision_amd.engine import get_engine  # noqa: E402

HBM_BYTES_PER_S = 8e12      # the roofline bench.py uses
# algorithmic bytes per pixel: f32 image in + 5 planes out; R0 + R1 (gathered once) + flow in, M
# out; M in + flow out; flow in + depth out
BYTES_PER_PX = {"k_fb_polyexp": 24, "k_fb_update_matrices": 68, "k_fb_blur_solve": 28, "k_flow_depth": 12}
RUNS, WARM = 25, 3


def kernel_ms(eng, fn):
    ts = []
    for i in range(WARM + RUNS):
        eng.profile_reset()
        fn()
        ms, n = eng.profile_read("flow")
        assert n == 1
        if i >= WARM:
            ts.append(ms)
    return statistics.median(ts)


def wall_ms(fn, sync, runs=RUNS):
    ts = []
    for i in range(WARM + runs):
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def measure(eng, H, W):
    n = H * W
    prev, nxt = S.translated_pair(H, W, 1.5, -0.75, seed=1)
    tables = F.polyexp_tables(5, 1.2)
    d_prev, d_next = eng.upload("fr_prev", prev), eng.upload("fr_next", nxt)
    d_img = eng.upload("fr_img", prev.astype(np.float32))
    d_R0, d_R1 = eng.scratch("fr_R0", 20 * n), eng.scratch("fr_R1", 20 * n)
    d_M, d_pl = eng.scratch("fr_M", 20 * n), eng.scratch("fr_pl", 8 * n)
    d_flow, d_depth = eng.scratch("fr_flow", 8 * n), eng.scratch("fr_depth", 4 * n)
    eng.fb_polyexp_dev(d_img, H, W, 5, tables, d_R0)
    eng.fb_polyexp_dev(eng.upload("fr_img2", nxt.astype(np.float32)), H, W, 5, tables, d_R1)
    F.farneback_flow_dev(eng, d_prev, d_next, H, W, d_flow=d_flow)
    flow = eng.to_host(d_flow, (H, W, 2), np.float32)
    eng.to_device(d_pl, np.ascontiguousarray(flow.transpose(2, 0, 1)))
    Hm = np.array([[1, 0, 1.5], [0, 1, -0.75], [1e-6, -1e-6, 1.0]])
    eng.profile(True)
    try:
        ms = {
            "k_fb_polyexp": kernel_ms(eng, lambda: eng.fb_polyexp_dev(d_img, H, W, 5, tables, d_R0)),
            "k_fb_update_matrices": kernel_ms(eng, lambda: eng.fb_update_matrices_dev(d_R0, d_R1, d_pl, H, W, d_M)),
            "k_fb_blur_solve": kernel_ms(eng, lambda: eng.fb_blur_solve_dev(d_M, H, W, 15, d_pl)),
            "k_flow_depth": kernel_ms(eng, lambda: eng.flow_depth_dev(d_flow, H, W, Hm, d_depth, minmax=False)),
        }
    finally:
        eng.profile(False)
    flow_ms = wall_ms(lambda: F.farneback_flow_dev(eng, d_prev, d_next, H, W, d_flow=d_flow), eng.synchronize)
    est = F.OpticalFlowDepthEstimator(engine=eng)
    frames = [S.to_bgr(prev), S.to_bgr(nxt)]
    est(frames[0])
    k = [0]

    def step():
        k[0] ^= 1
        assert est(frames[k[0]]) is not None

    est_ms = wall_ms(step, lambda: None)
    t0 = time.perf_counter()
    exp = O.farneback(prev, nxt)
    oracle_ms = (time.perf_counter() - t0) * 1e3
    out = {"size": f"{W}x{H}"}
    for name, t in ms.items():
        out[name + "_us"] = round(t * 1e3, 1)
        out[name + "_bytes_per_px"] = BYTES_PER_PX[name]
        out[name + "_hbm_fraction"] = round(BYTES_PER_PX[name] * n / (t * 1e-3) / HBM_BYTES_PER_S, 4)
    out.update({"farneback_flow_dev_wall_ms": round(flow_ms, 3), "estimator_call_wall_ms": round(est_ms, 3),
                "numpy_oracle_farneback_ms": round(oracle_ms, 1), "bit_exact": bool(np.array_equal(flow, exp))})
    return out


def main():
    eng = get_engine(0)
    sizes = [(356, 633), (1080, 1920)]
    print(json.dumps({"tool": "flow_rate", "runs": RUNS, "results": [measure(eng, H, W) for H, W in sizes]}))


if __name__ == "__main__":
    main()
