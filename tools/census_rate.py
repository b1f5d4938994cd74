#!/usr/bin/env python3
"""Rates of the census / Hamming cost on device-resident gray pairs, at the fusion
app's processing size (633x356, D=96, win 5) and at 1080p (D=128, win 9):

  * the launches alone (HIP events around each, median of the runs): k_census (both images of the
    pair in one launch) and k_census_match;
  * wall time per frame (match .. median + scaled post, synchronised) of cost="census", "sad" and
    "sgbm" at the same commit, in alternating repetitions, as medians; the census / SAD ratio and
    whether the census frame takes less time than the SGBM frame (the condition the cost is held
    to: robustness at winner-take-all price).

Prints one JSON line and writes it to --out (default profiles/r17_census/census_rate.json).  Not
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
from stereovision_amd.engine import POST_SCALED, STAGE_ALL, get_engine, map_out  # noqa: E402
from stereovision_amd.synthetic import stereo_pair  # noqa: E402

RUNS, WARM = 25, 3
CONFIGS = [(356, 633, 96, 5), (1080, 1920, 128, 9)]
KINDS = ("census", "match")
COSTS = ("census", "sad", "sgbm")


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
    d_l, d_r = eng.upload("cr_l", L), eng.upload("cr_r", R)
    d16 = eng.scratch("cr_d16", 2 * n)
    bufs = [eng.scratch(f"cr_o{i}", 4 * n) for i in range(3)]
    d_u8 = eng.scratch("cr_u8", n)
    out = map_out(POST_SCALED, bufs[0], bufs[1], d_u8, bufs[2])

    def frame(cost):
        eng.depth_map_batch_ex(d_l, d_r, 1, H, W, W, n, 0, D, win, cost, STAGE_ALL, 0, out)

    eng.profile(True)
    try:
        k = launches_ms(eng, lambda: eng.disparity_dev(d_l, d_r, H, W, W, 0, D, win, "census", 0, H, d16, W))
        sad = launches_ms(eng, lambda: eng.disparity_dev(d_l, d_r, H, W, W, 0, D, win, "sad", 0, H, d16, W))
    finally:
        eng.profile(False)
    wall = alternating_wall_ms(eng, {c: (lambda c=c: frame(c)) for c in COSTS})
    cells = n * D
    res = {
        "size": f"{W}x{H}", "num_disp": D, "win": win,
        "k_census_ms": round(k["census"][0], 4), "k_census_launches": k["census"][1],
        "k_census_match_ms": round(k["match"][0], 4), "k_census_match_launches": k["match"][1],
        "k_census_match_ns_per_kilocell": round(k["match"][0] * 1e6 / (cells / 1e3), 4),
        "sad_match_ms": round(sad["match"][0], 4),
        "frame_wall_ms": {c: round(v, 4) for c, v in wall.items()},
        "frames_per_s": {c: round(1e3 / v, 1) for c, v in wall.items()},
        "census_over_sad": round(wall["census"] / wall["sad"], 3),
        "sgbm_over_census": round(wall["sgbm"] / wall["census"], 3),
        "census_faster_than_sgbm": bool(wall["census"] < wall["sgbm"]),
    }
    if check:   # the map against the NumPy restatement
        import sv_census_oracle as CO
        eng.disparity_dev(d_l, d_r, H, W, W, 0, D, win, "census", 0, H, d16, W)
        got = eng.to_host(d16, (H, W), np.int16)
        res["bit_exact"] = bool(np.array_equal(got, CO.disparity16_census(L, R, 0, D, win)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_census", "census_rate.json"))
    args = ap.parse_args()
    eng = get_engine(0)
    res = {"tool": "census_rate", "runs": RUNS,
           "results": [measure(eng, H, W, D, win, check=(H * W < 500000)) for H, W, D, win in CONFIGS]}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
