"""The HOG histogram kernels against the NumPy oracle and the HOG matcher against the C oracle's
winner-take-all (first minimum), bit for bit, on the built frames of tests/hog_frames.py
(tests/test_hog_bar.py shows on the CPU what they reach).

Histograms (sv_hog_hist_dev, padded pitch): Sobel pairs on both sides of all eight bin
boundaries and on the axes of the sign normalisation, each in all four columns of a lane; the
largest magnitude (191) and window sums of 225 * 127 in one bin and in both u16 halves of a
packed dword; the axis cases on the image border, with column W-1 in each of a lane's columns
and in a halo lane.  Every frame runs whole and as two row bands whose seam cuts a 24-row strip
and a 16-row tile.  The histogram buffer lies inside a larger allocation at a byte offset that
is a multiple of 4 but not of 16; 4 KiB before it, 4 KiB after it and the rows outside the band
are filled with a sentinel and must keep it (the column-run kernel issues redundant stores past
a row's last whole chunk by design).  The same frames run in child processes with
SV_HOG_STRIP=0 (the 64x16 tile kernel) and SV_HOG_CR_ROWS=5 (strip seams every 5 rows).

Matcher (sv_disparity_dev / sv_disparity_batch_dev): every plan of k_match<COST_HOG, 5, DPL>
(4x16 .. 8x64, the last with the 8-key reduce-scatter and both permlane swaps), each at its
full D and at a D with padding disparities, windows 1 / 7 / 15, 1 / 5 / 9 rows, matched bands of
1, 2r + 3 and about 150 columns, min_disp -7 / 0 / 9, row bands, flat and periodic pairs whose
disparities all tie (at cost 0, at a high cost, at a cost above 2^15), planted ties, shifted
noise and one batch of two frames.  The output pitch exceeds W; padding columns, spare rows
and the gap between frames hold a sentinel.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import hog_exact_child as X
import hog_frames as F

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------ histograms
@pytest.mark.parametrize("group", F.HIST_GROUPS)
def test_hog_hist_frames(engine, group):
    errs, n = [], 0
    for i, f in enumerate(F.HIST_FRAMES):
        if f.group != group:
            continue
        for launch, buf in X.run_hist(engine, i):
            X.check_hist(i, launch, buf, errs, "default")
            n += 1
    assert n >= 24
    assert not errs, "\n".join(errs[:20])


@pytest.mark.parametrize("setting", ["SV_HOG_STRIP=0", "SV_HOG_CR_ROWS=5"])
def test_hog_hist_frames_under_a_switch(tmp_path, setting):
    """A fresh interpreter per setting (each is read once per process) runs every histogram
    frame and writes its allocations to a file: the tile kernel, and the column-run kernel with
    5-row strips (seams at rows that are no multiple of 4), against the oracle."""
    name, value = setting.split("=")
    out = tmp_path / "hist.bin"
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                     "hog_exact_child.py"), str(out)],
                       capture_output=True, timeout=120,
                       env=dict(os.environ, SV_WARMUP_AT_IMPORT="0", **{name: value}))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    data = np.fromfile(out, np.uint16)
    errs, off = [], 0
    for i, f in enumerate(F.HIST_FRAMES):
        n16 = X.hist_layout(i)[1]
        for launch in f.launches():
            X.check_hist(i, launch, data[off:off + n16], errs, setting)
            off += n16
    assert off == data.size
    assert not errs, "\n".join(errs[:20])


# ------------------------------------------------------------------------------ matcher
@pytest.mark.parametrize("group", F.GROUPS)
def test_hog_matcher(engine, group):
    errs = []
    for k in (c for c in F.CASES if c.group == group):
        p = engine_plan(k)
        if p != F.plan_of(k.D):
            errs.append(f"{k.id}: plan {p}, expected {F.plan_of(k.D)}")
        exp = F.expected(k.id)
        for band, buf in X.run_case(engine, k):
            maps, intact = X.split(k, band, buf)
            if not intact:
                errs.append(f"{k.id} rows {band}: sentinel overwritten outside [row0:row1, :W]")
            for z in range(k.nf):
                bad = maps[z, band[0]:band[1]] != exp[z][band[0]:band[1]]
                if bad.any():
                    y, x = np.argwhere(bad)[0]
                    errs.append(f"{k.id} rows {band} frame {z}: {int(bad.sum())} pixels differ, first at "
                                f"({band[0] + y}, {x}): got {maps[z, band[0] + y, x]}, "
                                f"oracle {exp[z][band[0] + y, x]}")
    assert not errs, "\n".join(errs[:20])


def engine_plan(k):
    from stereovision_amd.engine import plan
    p = plan(k.D, k.win, "hog")
    return p["dpl"], p["lpg"]
