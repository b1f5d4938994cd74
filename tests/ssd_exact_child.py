"""Runs cases of tests/ssd_frames.py through the device API and returns the whole output
buffers, sentinel borders included.  tests/test_ssd_exact.py imports run_case; run as a script
(ids on the command line) it writes the buffers' bytes to stdout, for the child process of the
SV_SSD_MFMA=0 comparison."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import ssd_frames as F  # noqa: E402

OPAD = 8    # out_pitch = W + OPAD
OGAP = 16   # elements between the output frames of a batch, beyond a whole frame


def geometry(k, pitch):
    """(frame stride in bytes, out pitch, rows of an output frame buffer, out frame stride):
    an output frame holds one spare row above and below the image's."""
    op = k.W + OPAD
    return k.frame_stride(pitch), op, k.H + 2, (k.H + 2) * op + OGAP


def query(e, k, pitch, band, base=(4096, 8192)):
    fs, op, _, _ = geometry(k, pitch)
    return e.ssd_mfma_query(base[0], base[1], k.H, k.W, pitch, k.min_disp, k.D, k.win, "ssd", band[0], band[1],
                            op, k.nf, fs if k.nf > 1 else 0)


def run_case(e, k, pitch, on_query=None):
    """One launch per row band of the case, each into a fresh sentinel-filled buffer.  Returns
    [(band, buffer)] with buffer an int16 array (nf, H + 2, W + OPAD) (+ the gap, checked
    here): row 1 + y of it is image row y.  on_query(band, answer): the query's answer for the
    very pointers of the launch, before it."""
    fs, op, orows, ofs = geometry(k, pitch)
    frames = k.frames(pitch)
    nin = fs * k.nf
    hostL = np.full(nin, 0xA5, np.uint8)
    hostR = np.full(nin, 0x5A, np.uint8)
    for z, (L, R) in enumerate(frames):
        hostL[z * fs:z * fs + k.H * pitch] = L.ravel()
        hostR[z * fs:z * fs + k.H * pitch] = R.ravel()
    nout = ofs * k.nf
    dL, dR, dO = e.dev_alloc(nin), e.dev_alloc(nin), e.dev_alloc(2 * nout)
    res = []
    try:
        assert dL % 4 == 0 and dR % 4 == 0
        e.to_device(dL, hostL)
        e.to_device(dR, hostR)
        for band in k.bands:
            e.to_device(dO, np.full(nout, F.SENTINEL, np.int16))
            if on_query:
                on_query(band, query(e, k, pitch, band, (dL, dR)))
            out0 = dO + 2 * op   # image row 0
            if k.nf > 1:
                assert band == (0, k.H)
                e.disparity_batch_dev(dL, dR, k.nf, k.H, k.W, pitch, fs, k.min_disp, k.D, k.win, "ssd", out0, op, ofs)
            else:
                e.disparity_dev(dL, dR, k.H, k.W, pitch, k.min_disp, k.D, k.win, "ssd", band[0], band[1], out0, op)
            e.synchronize()
            got = e.to_host(dO, (k.nf, ofs), np.int16)
            assert (got[:, orows * op:] == F.SENTINEL).all(), f"{k.id}: the gap between output frames was written"
            res.append((band, got[:, :orows * op].reshape(k.nf, orows, op).copy()))
    finally:
        for p in (dL, dR, dO):
            e.dev_free(p)
    return res


def split(k, band, buf):
    """(maps [nf, H, W] with the sentinel outside the band's rows, True if every element
    outside [row0:row1, :W] of every frame still holds the sentinel)."""
    inside = np.zeros(buf.shape, bool)
    inside[:, 1 + band[0]:1 + band[1], :k.W] = True
    intact = bool((buf[~inside] == F.SENTINEL).all())
    maps = np.full((k.nf, k.H, k.W), F.SENTINEL, np.int16)
    maps[:, band[0]:band[1]] = buf[:, 1 + band[0]:1 + band[1], :k.W]
    return maps, intact


def main(argv):
    from stereovision_amd.engine import get_engine
    e = get_engine(0)
    for cid in argv:
        k = F.BY_ID[cid]
        for _, buf in run_case(e, k, k.pitch):
            sys.stdout.buffer.write(buf.tobytes())


if __name__ == "__main__":
    main(sys.argv[1:])
