#!/usr/bin/env python3
"""Rates of the 3D reprojection and the point cloud on device-resident maps, at the
fusion app's processing size (633x356) and at 1920x1080, with about half of the pixels valid:

  * the launches alone (HIP events around each, median of the runs): k_reproject, k_cloud_min,
    k_cloud_count, k_cloud_scan, k_cloud_emit, and their algorithmic bytes over that time as a
    fraction of HBM;
  * wall time of point_cloud_dev with the host read of N and without it (synchronised after);
  * wall time of FusionFramePipeline.step with and without cloud=, in alternating repetitions;
  * the NumPy restatement (tests/sv_cloud_oracle.py) on the same box.

Prints one JSON line and writes it to --out (default profiles/r16_cloud/cloud_rate.json).  Not the
bench metric."""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
os.environ.setdefault("SV_WARMUP_AT_IMPORT", "0")
from stereovision_amd import cloud, synthetic  # noqa: E402
from stereovision_amd import fused_depth_map as FDM  # noqa: E402
from stereovision_amd.engine import cloud_params, get_engine  # noqa: E402
from stereovision_amd.frame import FusionFramePipeline  # noqa: E402

RUNS, WARM = 25, 3
HBM_BYTES_PER_S = 8e12      # the roofline bench.py uses
CONFIGS = [(356, 633, 96, 5), (1080, 1920, 128, 9)]      # H, W and the pipeline's num_disp, window
KINDS = ("reproject", "cloud_min", "cloud_count", "cloud_scan", "cloud_emit")
TILE = 1024


def launches_ms(eng, fn):
    """{kernel id: median ms per call} of one call's launches."""
    acc = {k: [] for k in KINDS}
    for i in range(WARM + RUNS):
        eng.profile_reset()
        fn()
        eng.synchronize()
        for k in KINDS:
            ms, _ = eng.profile_read(k)
            if i >= WARM:
                acc[k].append(ms)
    return {k: statistics.median(v) for k, v in acc.items()}


def alternating_wall_ms(eng, paths, runs=RUNS):
    ts = {k: [] for k in paths}
    for i in range(WARM + runs):
        for k, fn in paths.items():
            t0 = time.perf_counter()
            fn()
            eng.synchronize()
            if i >= WARM:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: statistics.median(v) for k, v in ts.items()}


def scene(H, W, seed=0):
    """An f32 disparity map, about half of it the (min_disp - 1) marker, a Q and a BGR frame."""
    rng = np.random.default_rng(seed)
    d = rng.integers(16, 96 * 16, (H, W)).astype(np.float32) / np.float32(16)
    d[rng.random((H, W)) < 0.5] = -1.0
    f = 0.7 * W
    Q = np.array([[1, 0, 0, -W / 2 + 3.3], [0, 1, 0, -H / 2 - 1.7], [0, 0, 0, f], [0, 0, 12.5, 0.0]])
    return d, Q, rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def calibration(W, H):
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "stereo_calibration_data.pkl")
        with open(p, "wb") as f:
            pickle.dump(synthetic.synthetic_calibration(W, H, 2), f)
        return FDM.load_stereo_calibration_with_scaling(1.0, p)


def measure_kernels(eng, H, W):
    import sv_cloud_oracle as CO
    d, Q, bgr = scene(H, W)
    n = H * W
    res = {"size": f"{W}x{H}"}
    d_bgr = eng.upload("cr_bgr", bgr)
    d_xyz, d_obgr, d_idx = eng.scratch("cr_xyz", 12 * n), eng.scratch("cr_obgr", 3 * n), eng.scratch("cr_idx", 4 * n)
    d_cnt = eng.scratch("cr_cnt", 256)
    p = cloud_params(0.0, None, None, True)
    for fmt, el, arr in (("f32", 4, d), ("i16x16", 2, (d * 16).astype(np.int16))):
        d_disp = eng.upload("cr_disp_" + fmt, arr)

        def dense():
            eng.reproject_3d_dev(d_disp, fmt, H, W, W, Q, True, d_xyz)

        def cl(wait):
            return eng.point_cloud_dev(d_disp, fmt, H, W, W, Q, p, n, d_xyz, d_bgr, 3 * W, d_obgr, d_idx, d_cnt,
                                       wait=wait)

        N = cl(True)
        eng.profile(True)
        try:
            kd, kc = launches_ms(eng, dense), launches_ms(eng, lambda: cl(False))
        finally:
            eng.profile(False)
        wall = alternating_wall_ms(eng, {"with_read_of_n": lambda: cl(True), "without": lambda: cl(False)})
        nb = -(-n // TILE)
        byts = {"k_reproject": (el + 12) * n, "k_cloud_min": el * n, "k_cloud_count": el * n + 4 * nb,
                "k_cloud_scan": 8 * nb, "k_cloud_emit": el * n + 4 * nb + N * (3 + 12 + 3 + 4)}
        ms = {"k_reproject": kd["reproject"], "k_cloud_min": kc["cloud_min"], "k_cloud_count": kc["cloud_count"],
              "k_cloud_scan": kc["cloud_scan"], "k_cloud_emit": kc["cloud_emit"]}
        r = {"valid_fraction": round(N / n, 4), "points": int(N)}
        for k in ms:
            r[k + "_ms"] = round(ms[k], 4)
            r[k + "_hbm_fraction"] = round(byts[k] / (ms[k] * 1e-3) / HBM_BYTES_PER_S, 4) if ms[k] > 0 else None
        r["point_cloud_dev_wall_ms"] = {k: round(v, 4) for k, v in wall.items()}
        t0 = time.perf_counter()
        exp = CO.point_cloud(arr, Q, bgr, handle_missing=True)
        r["numpy_point_cloud_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        t0 = time.perf_counter()
        dense_exp = CO.reproject_image_to_3d(arr, Q, True)
        r["numpy_reproject_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        m = min(N, n)
        r["bit_exact"] = bool(
            N == exp[3] and np.array_equal(eng.to_host(d_xyz, (m, 3), np.float32), exp[0]) and
            np.array_equal(eng.to_host(d_obgr, (m, 3), np.uint8), exp[1]) and
            np.array_equal(eng.to_host(d_idx, (m,), np.uint32), exp[2]))
        dense()
        r["dense_bit_exact"] = bool(np.array_equal(eng.to_host(d_xyz, (H, W, 3), np.float32), dense_exp, equal_nan=True))
        res[fmt] = r
    return res


def measure_pipeline(eng, H, W, num_disp, win):
    import frame_chain as C
    calib = calibration(W, H)
    frames = C.moving_stereo_sequence(H, W, 4, disparity=20, step=(2.0, 1.0))
    stereo = dict(min_disp=0, num_disp=num_disp, window_size=win)
    pipes = {"without_cloud": FusionFramePipeline(calib, engine=eng, outputs=("fused_u8",), **stereo),
             "with_cloud": FusionFramePipeline(calib, engine=eng, outputs=("fused_u8",), cloud=cloud.CloudParams(),
                                               **stereo)}
    k = [0]
    points = []

    def step(name):
        fl, fr = frames[k[0] % len(frames)]
        r = pipes[name].step(fl, fr)
        if r.cloud is not None:
            points.append(len(r.cloud[0]))

    def both(name):
        def fn():
            step(name)
            if name == "with_cloud":
                k[0] += 1
        return fn

    wall = alternating_wall_ms(eng, {name: both(name) for name in pipes}, runs=12)
    for p in pipes.values():
        p.close()
    return {"step_wall_ms": {n: round(v, 3) for n, v in wall.items()},
            "cloud_points_median": int(statistics.median(points)) if points else 0, "pixels": H * W}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_cloud", "cloud_rate.json"))
    args = ap.parse_args()
    eng = get_engine(0)
    results = []
    for H, W, D, win in CONFIGS:
        r = measure_kernels(eng, H, W)
        r["pipeline"] = measure_pipeline(eng, H, W, D, win)
        results.append(r)
    res = {"tool": "cloud_rate", "runs": RUNS, "hbm_bytes_per_s": HBM_BYTES_PER_S, "results": results}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
