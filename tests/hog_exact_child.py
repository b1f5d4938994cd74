"""Runs the frames and cases of tests/hog_frames.py through the device API and returns the whole
output allocations, sentinel guards included.  tests/test_hog_exact.py imports run_hist,
check_hist, run_case and split; run as a script (an output path on the command line) it runs
every histogram frame and writes the allocations' bytes to that file, for the child processes
of the SV_HOG_STRIP=0 and SV_HOG_CR_ROWS comparisons (both switches are read once per process)."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import hog_frames as F  # noqa: E402

GUARD = 4096   # bytes of sentinel before and after the histogram buffer
OPAD = 8       # out_pitch = W + OPAD
OGAP = 16      # elements between the output frames of a batch, beyond a whole frame


# ------------------------------------------------------------------------------ histograms
def hist_layout(index):
    """(byte offset of the histograms in their allocation: a multiple of 4, not of 16; the
    allocation's length in u16 elements)."""
    f = F.HIST_FRAMES[index]
    off = GUARD + (4, 8, 12)[index % 3]
    return off, (off + f.H * f.W * 20 + GUARD + 16) // 2


def run_hist(e, index):
    """Every launch of HIST_FRAMES[index] through sv_hog_hist_dev, each into a freshly
    sentinel-filled allocation: [((win, row0, row1), the allocation as u16)]."""
    f = F.HIST_FRAMES[index]
    off, n16 = hist_layout(index)
    img = f.padded()
    dimg, dall = e.dev_alloc(img.nbytes), e.dev_alloc(2 * n16)
    res = []
    try:
        assert dall % 16 == 0 and (dall + off) % 4 == 0 and (dall + off) % 16
        e.to_device(dimg, img)
        fill = np.full(n16, F.HIST_SENTINEL, np.uint16)
        for win, r0, r1 in f.launches():
            e.to_device(dall, fill)
            e.hog_hist_dev(dimg, f.H, f.W, f.pitch, win, r0, r1, dall + off)
            e.synchronize()
            res.append(((win, r0, r1), e.to_host(dall, (n16,), np.uint16)))
    finally:
        e.dev_free(dimg)
        e.dev_free(dall)
    return res


def check_hist(index, launch, buf, errs, leg):
    """Compare one allocation with the oracle: the band's rows bit for bit, the pad bin 0, the
    guards before and after the buffer and the rows outside the band still the sentinel."""
    f = F.HIST_FRAMES[index]
    win, r0, r1 = launch
    off, n16 = hist_layout(index)
    assert buf.shape == (n16,)
    a, z = off // 2, off // 2 + f.H * f.W * 10
    tag = f"{leg} {f.id} win {win} rows {r0}:{r1}"
    if (buf[:a] != F.HIST_SENTINEL).any():
        errs.append(f"{tag}: {int((buf[:a] != F.HIST_SENTINEL).sum())} elements written before the buffer")
    if (buf[z:] != F.HIST_SENTINEL).any():
        errs.append(f"{tag}: {int((buf[z:] != F.HIST_SENTINEL).sum())} elements written after the buffer")
    h = buf[a:z].reshape(f.H, f.W, 10)
    if (h[:r0] != F.HIST_SENTINEL).any() or (h[r1:] != F.HIST_SENTINEL).any():
        errs.append(f"{tag}: rows outside the band written")
    if (h[r0:r1, :, 9] != 0).any():
        errs.append(f"{tag}: pad bin not 0")
    exp = F.expected_hist(index, win)[:, r0:r1]
    bad = h[r0:r1, :, :9].transpose(2, 0, 1) != exp
    if bad.any():
        b, y, x = np.argwhere(bad)[0]
        errs.append(f"{tag}: {int(bad.sum())} values differ, first at bin {b} of ({r0 + y}, {x}): got "
                    f"{h[r0 + y, x, b]}, oracle {exp[b, y, x]}")


# ------------------------------------------------------------------------------ matcher
def geometry(k):
    """(input frame stride in bytes, out pitch, rows of an output frame buffer, out frame
    stride in elements): an output frame holds one spare row above and below the image's."""
    op = k.W + OPAD
    return k.frame_stride(), op, k.H + 2, (k.H + 2) * op + OGAP


def run_case(e, k):
    """One launch per row band of the case, each into a fresh sentinel-filled buffer.  Returns
    [(band, buffer)] with buffer an int16 array (nf, H + 2, W + OPAD): row 1 + y of it is image
    row y (the gap between frames is checked here)."""
    fs, op, orows, ofs = geometry(k)
    nin = fs * k.nf
    hostL = np.full(nin, 0xA5, np.uint8)
    hostR = np.full(nin, 0x5A, np.uint8)
    for z, (L, R) in enumerate(k.frames()):
        hostL[z * fs:z * fs + k.H * k.pitch] = L.ravel()
        hostR[z * fs:z * fs + k.H * k.pitch] = R.ravel()
    nout = ofs * k.nf
    dL, dR, dO = e.dev_alloc(nin), e.dev_alloc(nin), e.dev_alloc(2 * nout)
    res = []
    try:
        e.to_device(dL, hostL)
        e.to_device(dR, hostR)
        for band in k.bands:
            e.to_device(dO, np.full(nout, F.SENTINEL, np.int16))
            out0 = dO + 2 * op   # image row 0
            if k.nf > 1:
                assert band == (0, k.H)
                e.disparity_batch_dev(dL, dR, k.nf, k.H, k.W, k.pitch, fs, k.min_disp, k.D, k.win, "hog", out0, op,
                                      ofs)
            else:
                e.disparity_dev(dL, dR, k.H, k.W, k.pitch, k.min_disp, k.D, k.win, "hog", band[0], band[1], out0, op)
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
    with open(argv[0], "wb") as out:
        for index in range(len(F.HIST_FRAMES)):
            for _, buf in run_hist(e, index):
                out.write(buf.tobytes())


if __name__ == "__main__":
    main(sys.argv[1:])
