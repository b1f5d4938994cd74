#!/usr/bin/env python3
"""Rates of the refinement stage of the SAD maps on device-resident gray pairs,
at the fusion app's processing size (633x356, D=96, win 5) and at 1080p (D=128, win 9), with and
without the left-right check:

  * the launches alone (HIP events around each, median of the runs): k_flip_rows, the left and the
    right matcher run, k_refine and the speckle filter's kernels;
  * wall time per frame (match .. median + scaled post, synchronised) of the refined path, the
    plain path and cost="sgbm" at the same commit, in alternating repetitions, as medians.

Prints one JSON line and writes it to --out (default profiles/r15_refine/refine_rate.json).  Not
the bench metric."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
os.environ.setdefault("SV_WARMUP_AT_IMPORT", "0")
from stereovision_amd.engine import POST_SCALED, STAGE_ALL, RefineParams, get_engine, map_out  # noqa: E402
from stereovision_amd.synthetic import stereo_pair  # noqa: E402

RUNS, WARM = 25, 3
CONFIGS = [(356, 633, 96, 5), (1080, 1920, 128, 9)]
SPECKLE = (100, 2)          # window, range: the speckle launches are timed with these
KINDS = ("flip", "match", "refine", "speckle")


def launches_ms(eng, fn):
    """{kernel id: (median total ms per call, launches per call)} of one call's launches."""
    acc = {k: [] for k in KINDS}
    cnt = {}
    for i in range(WARM + RUNS):
        eng.profile_reset()
        fn()
        eng.synchronize()
        for k in KINDS:
            ms, n = eng.profile_read(k)
            cnt[k] = n
            if i >= WARM:
                acc[k].append(ms)
    return {k: (statistics.median(v), cnt[k]) for k, v in acc.items()}


def alternating_wall_ms(eng, paths):
    """Median wall ms of each path, the paths taking turns inside every repetition."""
    ts = {k: [] for k in paths}
    for i in range(WARM + RUNS):
        for k, fn in paths.items():
            t0 = time.perf_counter()
            fn()
            eng.synchronize()
            if i >= WARM:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: statistics.median(v) for k, v in ts.items()}


def measure(eng, H, W, D, win, check):
    L, R, _ = stereo_pair(H, W, D, seed=0)
    n = H * W
    d_l, d_r = eng.upload("rr_l", L), eng.upload("rr_r", R)
    d16 = eng.scratch("rr_d16", 2 * n)
    d_right = eng.scratch("rr_right", 2 * n)
    bufs = [eng.scratch(f"rr_o{i}", 4 * n) for i in range(3)]
    d_u8 = eng.scratch("rr_u8", n)
    out = map_out(POST_SCALED, bufs[0], bufs[1], d_u8, bufs[2])
    with_lr, no_lr = RefineParams(1, 1, True), RefineParams(-1, 1, True)
    with_speckle = RefineParams(1, 1, True, *SPECKLE)

    def refined(p):
        eng.disparity_refined_dev(d_l, d_r, H, W, W, 0, D, win, "sad", p, d16, W)
        eng.median_rows_dev(d16, H, W, 0, H, out, 0, D, "sgbm")

    def plain(cost):
        eng.depth_map_batch_ex(d_l, d_r, 1, H, W, W, n, 0, D, win, cost, STAGE_ALL, 0, out)

    eng.profile(True)
    try:
        left = launches_ms(eng, lambda: eng.disparity_dev(d_l, d_r, H, W, W, 0, D, win, "sad", 0, H, d16, W))
        right = launches_ms(eng, lambda: eng.disparity_right_dev(d_l, d_r, H, W, W, 0, D, win, "sad", d_right, W))
        ref = {name: launches_ms(eng, lambda p=p: eng.refine_dev(d_l, d_r, H, W, W, d16, d_right, 0, D, win, "sad", p,
                                                                  bufs[0], W))
               for name, p in (("lr", with_lr), ("no_lr", no_lr), ("lr_speckle", with_speckle))}
    finally:
        eng.profile(False)
    wall = alternating_wall_ms(eng, {"plain": lambda: plain("sad"), "refined_lr": lambda: refined(with_lr),
                                     "refined_no_lr": lambda: refined(no_lr),
                                     "refined_lr_speckle": lambda: refined(with_speckle),
                                     "sgbm": lambda: plain("sgbm")})
    res = {
        "size": f"{W}x{H}", "num_disp": D, "win": win,
        "k_flip_rows_ms_per_launch": round(right["flip"][0] / max(right["flip"][1], 1), 4),
        "k_flip_rows_launches": right["flip"][1],
        "match_left_ms": round(left["match"][0], 4),
        "match_right_ms": round(right["match"][0], 4),
        "k_refine_lr_ms": round(ref["lr"]["refine"][0], 4),
        "k_refine_no_lr_ms": round(ref["no_lr"]["refine"][0], 4),
        "speckle_ms": round(ref["lr_speckle"]["speckle"][0], 4),
        "k_refine_over_one_match": round(ref["lr"]["refine"][0] / left["match"][0], 3),
        "frame_wall_ms": {k: round(v, 4) for k, v in wall.items()},
        "frames_per_s": {k: round(1e3 / v, 1) for k, v in wall.items()},
    }
    if check:   # the refined map against the NumPy restatement
        import sv_refine_oracle as RO
        eng.disparity_refined_dev(d_l, d_r, H, W, W, 0, D, win, "sad", with_speckle, d16, W)
        got = eng.to_host(d16, (H, W), np.int16)
        exp = RO.disparity_refined(L, R, 0, D, win, RO.COST_SAD, 1, 1, True, *SPECKLE)
        res["bit_exact"] = bool(np.array_equal(got, exp))
        res["invalid_fraction"] = round(float((exp[:, D:] == -16).mean()), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_refine", "refine_rate.json"))
    args = ap.parse_args()
    eng = get_engine(0)
    res = {"tool": "refine_rate", "cost": "sad", "runs": RUNS,
           "results": [measure(eng, H, W, D, win, check=(H * W < 500000)) for H, W, D, win in CONFIGS]}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
