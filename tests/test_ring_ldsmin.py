"""GPU parity of the ring kind's LDS argmin fold (sv_match_ring.hip k_match_ring LDSMIN: 32-lane
groups at win 9, i.e. 64 < D <= 128; every lane stores its 8 keys of a step pair to a per-wave
LDS scratch, lane r folds key r >> 3 of group (r >> 2) & 1) against the C oracle's
winner-take-all (first minimum), bit-exact.

The fold's switch (SV_RING_LDSMIN, on unless 0) is read once per process, and which fold a
launch took is visible only in what the library prints under SV_RING_OCC=1.  So one child
process (this file run as a script) computes every case with both set, the fixture checks that
the r 4, 32-lane launches really took the LDS fold, and the tests compare what the child wrote
with the oracle.

The cases sit where the fold can go wrong: padding-disparity keys in the scratch (D = 100), a
last wave that is partly empty and the sentinel first chunk (W = D + 7, D + 150), more than
one wave per row (W = D + 572), row counts that are no multiple of 4, ties, min_disp, a row
band and a pitched frame batch (the scratch is per wave, grid.z > 1).  D = 64 (16-lane groups)
and the other windows keep the DPP fold and run the same kernel body around it."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EDGE = [(D, extra, H) for H in (5, 23)
        for D, extra in [(64, 150), (64, 7), (100, 150), (100, 7), (128, 150), (128, 7), (128, 572)]]
TIES = [(D, kind) for D in (100, 128) for kind in ("flat", "per8")]
MIN_DISP = [-16, 5]
WINDOWS = [5, 7, 9, 11, 13, 15]
BATCH = dict(H=37, W=350, D=128, win=9, nf=3, row0=7, row1=30)


def _pair(H, W, D, seed, min_disp=0):
    from stereovision_amd.synthetic import stereo_pair
    L, R, _ = stereo_pair(H, W, D, seed=seed, min_disp=min_disp)
    return L, R


def _tie_frame(H, W, kind):
    if kind == "flat":
        return np.full((H, W), 77, np.uint8)
    return np.tile(((np.arange(W) % 8) * 30).astype(np.uint8), (H, 1))   # costs repeat every 8 d


def cases():
    """name -> (L, R, min_disp, D, win) of every single-frame case."""
    out = {}
    for D, extra, H in EDGE:
        out[f"edge_{D}_{extra}_{H}"] = (*_pair(H, D + extra, D, D + extra + H), 0, D, 9)
    for D, kind in TIES:
        f = _tie_frame(13, D + 150, kind)
        out[f"tie_{D}_{kind}"] = (f, f, 0, D, 9)
    for m in MIN_DISP:
        out[f"mind_{m}"] = (*_pair(17, 300, 128, 3, max(0, m)), m, 128, 9)
    for win in WINDOWS:
        out[f"win_{win}"] = (*_pair(23, 278, 128, win), 0, 128, win)
    return out


def _batch_frames():
    b = BATCH
    return [_pair(b["H"], b["W"], b["D"], 40 + z) for z in range(b["nf"])]


def child(path):
    """Every case through the engine of this process (SV_RING_LDSMIN as the caller set it)."""
    from stereovision_amd.engine import get_engine
    engine = get_engine(0)
    res = {k: engine.disparity(L, R, m, D, win) for k, (L, R, m, D, win) in cases().items()}
    b = BATCH
    H, W, D, win, nf = b["H"], b["W"], b["D"], b["win"], b["nf"]
    L, R = _pair(H, W, D, 21)
    res["band"] = engine.disparity_rows(L, R, 0, D, win, b["row0"], b["row1"])
    pitch = W + 16
    fs = (H + 2) * pitch
    Ls = np.zeros((nf, H + 2, pitch), np.uint8)
    Rs = np.zeros_like(Ls)
    for z, (l, r) in enumerate(_batch_frames()):
        Ls[z, :H, :W], Rs[z, :H, :W] = l, r
    opitch, ofs = W + 8, H * (W + 8) + 24
    dL, dR, dO = engine.dev_alloc(Ls.nbytes), engine.dev_alloc(Rs.nbytes), engine.dev_alloc(nf * ofs * 2)
    try:
        engine.to_device(dL, Ls)
        engine.to_device(dR, Rs)
        engine.disparity_batch_dev(dL, dR, nf, H, W, pitch, fs, 0, D, win, "sad", dO, opitch, ofs)
        engine.synchronize()
        flat = engine.to_host(dO, (nf * ofs,), np.int16)
        for z in range(nf):
            res[f"batch_{z}"] = flat[z * ofs:z * ofs + H * opitch].reshape(H, opitch)[:, :W].copy()
    finally:
        for p in (dL, dR, dO):
            engine.dev_free(p)
    np.savez(path, **res)


@pytest.fixture(scope="module")
def got(engine, tmp_path_factory):
    """What the child computed with the LDS fold on (name -> disparity map)."""
    path = str(tmp_path_factory.mktemp("ldsmin") / "out.npz")
    env = dict(os.environ, SV_RING_LDSMIN="1", SV_RING_OCC="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    launches = [ln for ln in p.stderr.splitlines() if ln.startswith("k_match_ring r=4 lpg=32 ")]
    assert launches and all(" ldsmin=1 " in ln for ln in launches), p.stderr[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def inputs():
    return cases()


def _check(got, inputs, name):
    import sv_oracle_c as C
    L, R, m, D, win = inputs[name]
    np.testing.assert_array_equal(got[name], C.disparity16(L, R, m, D, win, 0))


@pytest.mark.parametrize("D,extra,H", EDGE)
def test_ldsmin_group_widths_and_edges(got, inputs, D, extra, H):
    _check(got, inputs, f"edge_{D}_{extra}_{H}")


@pytest.mark.parametrize("D,kind", TIES)
def test_ldsmin_ties_go_to_the_smaller_disparity(got, inputs, D, kind):
    """Flat and period-8 frames: many disparities cost the same, in different lanes of a
    group; after the LDS fold the smallest index must win."""
    _check(got, inputs, f"tie_{D}_{kind}")


@pytest.mark.parametrize("min_disp", MIN_DISP)
def test_ldsmin_min_disp(got, inputs, min_disp):
    _check(got, inputs, f"mind_{min_disp}")


@pytest.mark.parametrize("win", WINDOWS)
def test_ldsmin_windows(got, inputs, win):
    """win 9 takes the LDS fold; the other radii share the kernel body and keep DPP."""
    _check(got, inputs, f"win_{win}")


def test_ldsmin_row_band_and_frame_batch(got):
    """A row band (rows [7, 30) of 37) and a pitched 3-frame batch through the device entry
    point: the emitting lanes' offsets follow the output's pitch and frame stride."""
    import sv_oracle_c as C
    b = BATCH
    H, W, D, win = b["H"], b["W"], b["D"], b["win"]
    L, R = _pair(H, W, D, 21)
    exp = C.disparity16(L, R, 0, D, win, 0)
    np.testing.assert_array_equal(got["band"][b["row0"]:b["row1"]], exp[b["row0"]:b["row1"]])
    for z, (l, r) in enumerate(_batch_frames()):
        np.testing.assert_array_equal(got[f"batch_{z}"], C.disparity16(l, r, 0, D, win, 0))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    child(sys.argv[1])
