#!/usr/bin/env python3
"""Wall time per frame of the fusion app's frame body: FusionFramePipeline.step
on host BGR camera frames beside the same frame sequence through the chain of the host-array
drop-ins (tests/frame_chain.py), on 1920x1080 camera frames at processing scale 0.33 (633x356)
and 1.0, with and without a MiDaS map, on a moving scene so the flow branch is live.  The two
run alternately on the same box; a repetition is 48 frames (the sequence, several times over).
Reports medians and ranges of the repetitions' ms per frame and the host <-> device traffic of
one steady-state frame of each.  Prints one JSON line.  Not the bench metric."""
import contextlib
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
os.environ.setdefault("SV_WARMUP_AT_IMPORT", "0")
import frame_chain as C  # noqa: E402
from stereovision_amd import fused_depth_map as FDM  # noqa: E402
from stereovision_amd import synthetic  # noqa: E402
from stereovision_amd.engine import get_engine  # noqa: E402
from stereovision_amd.frame import FusionFramePipeline  # noqa: E402

CAM_H, CAM_W = 1080, 1920
FRAMES, PASSES, REPS, WARM = 6, 8, 7, 2     # a repetition: PASSES times over the FRAMES-frame sequence


def calibration(scale):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "stereo_calibration_data.pkl")
        with open(p, "wb") as f:
            pickle.dump(synthetic.synthetic_calibration(CAM_W, CAM_H, 0), f)
        return FDM.load_stereo_calibration_with_scaling(scale, p)


def midas_map(h, w):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    return (xs * np.float32(0.4) + ys * np.float32(0.2) +
            np.random.default_rng(3).random((h, w), dtype=np.float32) * np.float32(20.0)).astype(np.float32)


def one_pass(step, frames, midas):
    t0 = time.perf_counter()                         # (every step ends in a download: the device is done)
    for _ in range(PASSES):
        for fl, fr in frames:
            step(fl, fr, midas)
    return (time.perf_counter() - t0) * 1e3 / (PASSES * len(frames))


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def measure(eng, frames, scale, with_midas):
    FDM.PROCESSING_SCALE = scale                     # the app's setting: the stereo defaults follow it
    nd, ws = FDM.scaled_stereo_params()
    calib = calibration(scale)
    pw, ph = calib["img_size_proc"]
    midas = midas_map(ph, pw) if with_midas else None
    pipe = FusionFramePipeline(calib, engine=eng)
    chain = C.HostChain(calib, min_disp=FDM.MIN_DISP_BASE, num_disp=nd, window_size=ws)
    for _ in range(WARM):
        one_pass(pipe.step, frames, midas)
        one_pass(chain.step, frames, midas)
    tp, tc = [], []
    for _ in range(REPS):                            # alternately, on the same box
        tp.append(one_pass(pipe.step, frames, midas))
        tc.append(one_pass(chain.step, frames, midas))
    fl, fr = frames[0]                               # frame_counter is even here: the occlusion check runs
    eng.copy_counters(reset=True)
    r = pipe.step(fl, fr, midas)
    cp = eng.copy_counters(reset=True)
    e = chain.step(fl, fr, midas)
    cc = eng.copy_counters(reset=True)
    out = {
        "camera": f"{CAM_W}x{CAM_H}", "processing": f"{pw}x{ph}", "scale": scale, "num_disp": nd, "window": ws,
        "midas": with_midas, "frames_per_repetition": PASSES * len(frames), "repetitions": REPS,
        "pipeline": stats(tp), "chain": stats(tc),
        "speedup_median": round(statistics.median(tc) / statistics.median(tp), 3),
        "pipeline_slowest_below_chain_fastest": bool(max(tp) < min(tc)),
        "pipeline_copies_per_frame": cp, "chain_copies_per_frame": cc,
        "flow_live": bool(e["flow_depth_raw"] is not None),
        "fused_equal": bool(np.array_equal(r.fused_u8, e["fused_u8"])),
    }
    pipe.close()
    return out


def main():
    eng = get_engine(0)
    frames = C.moving_stereo_sequence(CAM_H, CAM_W, FRAMES, disparity=60, step=(4.5, 2.25))
    with contextlib.redirect_stdout(sys.stderr):     # the loaders and the estimators announce themselves
        results = [measure(eng, frames, scale, m) for scale in (0.33, 1.0) for m in (False, True)]
    print(json.dumps({"tool": "frame_rate", "results": results}))


if __name__ == "__main__":
    main()
