"""The SSD matcher kinds against the C oracle's SSD winner-take-all (first minimum), bit for
bit, on the hard frames of tests/ssd_frames.py (tests/test_ssd_bar.py shows on the CPU what
they reach): widths that are no multiple of 4 at a padded pitch, matched bands of 1..3 columns
and one column past a tile and a block, heights below the staging distance, around one, two
and four block bands (hb = rows, 64, 96, a last band of one row), every template instance of
the matrix-core kind, both ends of its key range with the correction term at its largest,
planted ties in every register / lane half / x'-tile position, min_disp of both signs, row
bands and batches.

Each case runs twice through sv_disparity_dev / sv_disparity_batch_dev: at its 4-byte aligned
pitch, where Engine.ssd_mfma_query must say the matrix-core kind takes the call with the
expected instance, and at an odd pitch, where it must say another kind does (the ring's SSD
form, the one-row kind) or, for keys only the matrix-core kind holds, that the call is
refused.  The output buffer is filled with a sentinel first; pitch padding, the rows above and
below the band and the gap between frames must keep it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ssd_exact_child as X
import ssd_frames as F
from stereovision_amd.engine import SVError

pytestmark = pytest.mark.gpu


def _compare(k, results, errs, leg):
    exp = F.expected(k.id)
    for band, buf in results:
        maps, intact = X.split(k, band, buf)
        if not intact:
            errs.append(f"{leg} {k.id} rows {band}: sentinel overwritten outside [row0:row1, :W]")
        for z in range(k.nf):
            bad = maps[z, band[0]:band[1]] != exp[z][band[0]:band[1]]
            if bad.any():
                y, x = np.argwhere(bad)[0]
                errs.append(f"{leg} {k.id} rows {band} frame {z}: {int(bad.sum())} pixels differ, first at "
                            f"({band[0] + y}, {x}): got {maps[z, band[0] + y, x]}, oracle {exp[z][band[0] + y, x]}")


@pytest.mark.parametrize("group", F.GROUPS)
def test_ssd_mfma_leg(engine, group):
    """4-byte aligned base, pitch and frame stride: the query names the matrix-core kind and the
    case's instance (ssd_frames.shape, checked here against the library's own ssd_shape)."""
    errs = []
    for k in (c for c in F.CASES if c.group == group):
        def on_query(band, q, k=k):
            s = F.shape(k.win, k.D, band[1] - band[0])
            want = dict(mfma=True, xt=s["xt"], nt=s["nt"], mb=s["mb"], hb=s["hb"], big=s["big"])
            got = {n: q.get(n) for n in want}
            if got != want:
                errs.append(f"{k.id} rows {band}: query {q}, expected {want}")
        _compare(k, X.run_case(engine, k, k.pitch, on_query), errs, "mfma")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("group", F.GROUPS)
def test_ssd_fallback_leg(engine, group):
    """The same frames at an odd pitch: the query says the matrix-core kind does not take the
    call; another kind gives the same bytes, or (mfma_only) the call returns an error."""
    errs = []
    for k in (c for c in F.CASES if c.group == group):
        pitch = F.odd_pitch(k.W)
        qs = [X.query(engine, k, pitch, band) for band in k.bands]
        if any(q["mfma"] for q in qs):
            errs.append(f"{k.id}: query at pitch {pitch} says mfma: {qs}")
            continue
        if qs[0]["mfma_only"]:
            with pytest.raises(SVError):
                X.run_case(engine, k, pitch)
            continue
        _compare(k, X.run_case(engine, k, pitch), errs, "fallback")
    assert not errs, "\n".join(errs)


AB_CASES = [k.id for g in F.GROUPS for k in [c for c in F.CASES if c.group == g][:2]][:14]


def test_ssd_mfma_off_equals_default_and_oracle(engine):
    """SV_SSD_MFMA=0 in a child process (the switch is read once per process): the other kinds
    on 4-byte aligned images give the same buffers as the default process and the oracle.
    Cases whose keys only the matrix-core kind holds are left to the fallback leg."""
    ids = [i for i in AB_CASES
           if not X.query(engine, F.BY_ID[i], F.odd_pitch(F.BY_ID[i].W), F.BY_ID[i].bands[0])["mfma_only"]]
    assert len(ids) >= 10
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                     "ssd_exact_child.py")] + ids,
                       capture_output=True, timeout=120,
                       env=dict(os.environ, SV_SSD_MFMA="0", SV_WARMUP_AT_IMPORT="0"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    errs, off = [], 0
    for i in ids:
        k = F.BY_ID[i]
        here = X.run_case(engine, k, k.pitch)
        _compare(k, here, errs, "default")
        for _, buf in here:
            child = r.stdout[off:off + buf.nbytes]
            off += buf.nbytes
            if child != buf.tobytes():
                errs.append(f"{k.id}: SV_SSD_MFMA=0 differs from the default process")
    assert off == len(r.stdout)
    assert not errs, "\n".join(errs)


HOST_FAMILIES = ("sat_lo", "sat_hi", "periodic")


@pytest.mark.parametrize("aligned", [True, False])
def test_ssd_host_path(engine, aligned):
    """engine.disparity on contiguous frames (pitch = W): the matrix-core kind at W % 4 == 0,
    another kind otherwise (keys only the matrix-core kind holds: an error)."""
    errs, n = [], 0
    for k in F.CASES:
        if k.family not in HOST_FAMILIES or k.nf > 1 or k.bands != [(0, k.H)] or (k.W % 4 == 0) != aligned:
            continue
        q = engine.ssd_mfma_query(4096, 8192, k.H, k.W, k.W, k.min_disp, k.D, k.win, "ssd")
        assert q["mfma"] == aligned, (k.id, q)
        (L, R), = k.images()
        if q["mfma_only"] and not aligned:
            with pytest.raises(SVError):
                engine.disparity(L, R, k.min_disp, k.D, k.win, "ssd")
            continue
        n += 1
        got = engine.disparity(L, R, k.min_disp, k.D, k.win, "ssd")
        if not np.array_equal(got, F.expected(k.id)[0]):
            errs.append(f"{k.id}: {int((got != F.expected(k.id)[0]).sum())} pixels differ")
    assert n >= 3
    assert not errs, "\n".join(errs)
