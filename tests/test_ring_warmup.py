"""GPU parity of the ring kind's warm-up (sv_match_ring.hip k_match_ring: the first 2r steps of a
segment run as add-only chunks ahead of the loop, the cost ring starts unwritten and the last
warm-up chunk zeroes the few slots read before they are written) and of build_ring_packs' row
loads, against the C oracle's winner-take-all (first minimum), bit-exact.

Which segment width a launch took is visible only in what the library prints under
SV_RING_OCC=1, which is read once per process.  So one child process (this file run as a
script) computes every case with it set and names each case on stderr before it runs; the
fixture reads the `seg=` lines, works out the entry chunk e0 of each launch and checks that the
entry offsets the cases were chosen for really occurred.

The cases sit where the warm-up variant can go wrong:
  * the first body is entered at chunk e0 = (nit*U - Tn)/4, so the warm-up chunks land on
    different static ring slots and may wrap into the second body: win 9 with all five e0
    (W = D + 2S, S = 12 .. 28), every other window with two;
  * group widths (D = 64, 100 with padding disparities, 128, 256; the packed form at win 15);
  * ties (flat and period-8 frames: a slot that is not zeroed shows as a cost offset) and bright
    left columns (a stale ring value would change a window sum);
  * min_disp, odd heights, a row band, a pitched frame batch;
  * the SSD ring and both passes of the split ring;
  * frames a few columns wider than D + 2r (the first output follows directly on the warm-up);
  * pitched, unaligned and row-clamped inputs of the pack builder."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

E0_WIN9 = [(D, S) for D in (128,) for S in (12, 16, 20, 24, 28)] + [(100, 16)]
E0_WINDOWS = [(win, S) for win in (5, 7, 11, 13, 15) for S in (8, 12)]
WIDTHS = [(64, 9, 5), (64, 9, 23), (100, 9, 5), (100, 9, 23), (128, 9, 5), (128, 9, 23), (256, 9, 23),
          (256, 15, 23)]
TIES = [(D, kind) for D in (100, 128) for kind in ("flat", "per8")]
MIN_DISP = [-16, 5]
SSD = [(win, extra) for win in (5, 7, 9) for extra in (24, 150)]
BORDER = [(64, 9), (128, 9), (128, 11), (128, 13)]
PITCHED = [("pitched", 300, 316, 23), ("pitched_h5", 300, 316, 5), ("unaligned", 301, 303, 23)]
BATCH = dict(H=37, W=350, D=128, win=9, nf=3, row0=7, row1=30)


def e0_of(r, seg):
    """The first body's entry chunk of a segment of width seg at radius r (k_match_ring)."""
    m = 2 * r + 2
    u = m if m % 4 == 0 else 2 * m
    tn = (seg + 2 * r + 3) & ~3
    return (-(-tn // u) * u - tn) // 4


def _pair(H, W, D, seed, min_disp=0):
    from stereovision_amd.synthetic import stereo_pair
    L, R, _ = stereo_pair(H, W, D, seed=seed, min_disp=min_disp)
    return L, R


def _tie_frame(H, W, kind):
    if kind == "flat":
        return np.full((H, W), 77, np.uint8)
    return np.tile(((np.arange(W) % 8) * 30).astype(np.uint8), (H, 1))   # costs repeat every 8 d


def cases():
    """name -> (L, R, min_disp, D, win, cost) of every single-frame case on the host path."""
    out = {}
    for D, S in E0_WIN9:
        out[f"e0_9_{D}_{S}"] = (*_pair(9, D + 2 * S, D, S), 0, D, 9, "sad")
    for win, S in E0_WINDOWS:
        out[f"e0_{win}_128_{S}"] = (*_pair(9, 128 + 2 * S, 128, win + S), 0, 128, win, "sad")
    for D, win, H in WIDTHS:
        out[f"width_{D}_{win}_{H}"] = (*_pair(H, D + 150, D, D + win + H), 0, D, win, "sad")
    for D, kind in TIES:
        f = _tie_frame(13, D + 150, kind)
        out[f"tie_{D}_{kind}"] = (f, f, 0, D, 9, "sad")
    L, R = _pair(13, 290, 128, 5)
    L, R = L.copy(), R.copy()
    L[:, :140] = 250
    R[:, :14] = 3
    out["bright_left"] = (L, R, 0, 128, 9, "sad")
    for m in MIN_DISP:
        out[f"mind_{m}"] = (*_pair(17, 300, 128, 3, max(0, m)), m, 128, 9, "sad")
    for win, extra in SSD:
        out[f"ssd_{win}_{extra}"] = (*_pair(11, 100 + extra, 100, win + extra), 0, 100, win, "ssd")
    out["split_320_7"] = (*_pair(9, 320 + 150, 320, 7), 0, 320, 7, "sad")
    for D, win in BORDER:
        out[f"border_{D}_{win}"] = (*_pair(7, D + 2 * (win // 2) + 3, D, D + win), 0, D, win, "sad")
    return out


def _batch_frames():
    b = BATCH
    return [_pair(b["H"], b["W"], b["D"], 40 + z) for z in range(b["nf"])]


def _pitched_pair(W, H):
    return _pair(H, W, 128, W + H)


def _say(name):
    sys.stderr.write(f"case {name}\n")
    sys.stderr.flush()


def child(path):
    """Every case through the engine of this process."""
    from stereovision_amd.engine import get_engine
    engine = get_engine(0)
    res = {}
    for k, (L, R, m, D, win, cost) in cases().items():
        _say(k)
        res[k] = engine.disparity(L, R, m, D, win, cost)
    b = BATCH
    H, W, D, win, nf = b["H"], b["W"], b["D"], b["win"], b["nf"]
    L, R = _pair(H, W, D, 21)
    _say("band")
    res["band"] = engine.disparity_rows(L, R, 0, D, win, b["row0"], b["row1"])
    # pitched device inputs: rows of `pitch` bytes, the frame at their start
    for name, pW, pitch, pH in PITCHED:
        pl, pr = _pitched_pair(pW, pH)
        Lp = np.full((pH + 1, pitch), 200, np.uint8)
        Rp = np.full((pH + 1, pitch), 100, np.uint8)
        Lp[:pH, :pW], Rp[:pH, :pW] = pl, pr
        dL, dR, dO = engine.dev_alloc(Lp.nbytes), engine.dev_alloc(Rp.nbytes), engine.dev_alloc(pH * pW * 2)
        try:
            engine.to_device(dL, Lp)
            engine.to_device(dR, Rp)
            _say(name)
            engine.disparity_dev(dL, dR, pH, pW, pitch, 0, 128, 9, "sad", 0, pH, dO, pW)
            engine.synchronize()
            res[name] = engine.to_host(dO, (pH, pW), np.int16).copy()
        finally:
            for p in (dL, dR, dO):
                engine.dev_free(p)
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
        _say("batch")
        engine.disparity_batch_dev(dL, dR, nf, H, W, pitch, fs, 0, D, win, "sad", dO, opitch, ofs)
        engine.synchronize()
        flat = engine.to_host(dO, (nf * ofs,), np.int16)
        for z in range(nf):
            res[f"batch_{z}"] = flat[z * ofs:z * ofs + H * opitch].reshape(H, opitch)[:, :W].copy()
    finally:
        for p in (dL, dR, dO):
            engine.dev_free(p)
    np.savez(path, **res)


LAUNCH = re.compile(r"k_match_ring r=(\d+) lpg=(\d+) ldsmin=\d+ seg=(\d+) ")


@pytest.fixture(scope="module")
def run(engine, tmp_path_factory):
    """(name -> disparity map, name -> [(r, lpg, seg)] of the case's ring launches)."""
    path = str(tmp_path_factory.mktemp("warmup") / "out.npz")
    env = dict(os.environ, SV_RING_OCC="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    launches, cur = {}, None
    for ln in p.stderr.splitlines():
        if ln.startswith("case "):
            cur = ln[5:].strip()
            launches[cur] = []
            continue
        m = LAUNCH.match(ln)
        if m and cur is not None:
            launches[cur].append(tuple(int(v) for v in m.groups()))
    with np.load(path) as z:
        return {k: z[k] for k in z.files}, launches


@pytest.fixture(scope="module")
def got(run):
    return run[0]


@pytest.fixture(scope="module")
def inputs():
    return cases()


def _check(got, inputs, name):
    import sv_oracle_c as C
    L, R, m, D, win, cost = inputs[name]
    np.testing.assert_array_equal(got[name], C.disparity16(L, R, m, D, win, 1 if cost == "ssd" else 0))


def test_every_case_took_the_ring_kind(run, inputs):
    _, launches = run
    names = list(inputs) + ["band", "batch"] + [p[0] for p in PITCHED]
    assert all(launches.get(n) for n in names), {n: launches.get(n) for n in names if not launches.get(n)}
    assert sorted(lpg for _, lpg, _ in launches["split_320_7"]) == [16, 64]   # both KEYS passes


def test_entry_offsets_occurred(run):
    """win 9, 32-lane groups: all five entry chunks; every other window: two."""
    _, launches = run
    e9 = {e0_of(r, seg) for D, S in E0_WIN9 for r, lpg, seg in launches[f"e0_9_{D}_{S}"] if lpg == 32}
    assert e9 == {0, 1, 2, 3, 4}, launches
    for win in (5, 7, 11, 13, 15):
        es = {e0_of(r, seg) for w, S in E0_WINDOWS if w == win for r, _, seg in launches[f"e0_{win}_128_{S}"]}
        assert len(es) >= 2, (win, es)


@pytest.mark.parametrize("D,S", E0_WIN9)
def test_warmup_entry_offsets_win9(got, inputs, D, S):
    _check(got, inputs, f"e0_9_{D}_{S}")


@pytest.mark.parametrize("win,S", E0_WINDOWS)
def test_warmup_entry_offsets_other_windows(got, inputs, win, S):
    _check(got, inputs, f"e0_{win}_128_{S}")


@pytest.mark.parametrize("D,win,H", WIDTHS)
def test_warmup_group_widths(got, inputs, D, win, H):
    _check(got, inputs, f"width_{D}_{win}_{H}")


@pytest.mark.parametrize("D,kind", TIES)
def test_warmup_ties_go_to_the_smaller_disparity(got, inputs, D, kind):
    _check(got, inputs, f"tie_{D}_{kind}")


def test_warmup_bright_left_columns(got, inputs):
    _check(got, inputs, "bright_left")


@pytest.mark.parametrize("min_disp", MIN_DISP)
def test_warmup_min_disp(got, inputs, min_disp):
    _check(got, inputs, f"mind_{min_disp}")


@pytest.mark.parametrize("win,extra", SSD)
def test_warmup_ssd_ring(got, inputs, win, extra):
    _check(got, inputs, f"ssd_{win}_{extra}")


def test_warmup_split_ring(got, inputs):
    _check(got, inputs, "split_320_7")


@pytest.mark.parametrize("D,win", BORDER)
def test_warmup_narrow_band(got, inputs, D, win):
    """W = D + 2r + 3: one partly empty wave, the first output column right after the warm-up."""
    _check(got, inputs, f"border_{D}_{win}")


@pytest.mark.parametrize("name,W,pitch,H", PITCHED)
def test_pack_row_loads_pitched_inputs(got, name, W, pitch, H):
    """Pitch != W (both multiples of 4), an unaligned pitch (the per-column fallback), and 5
    rows (every window row clamps at the top or the bottom)."""
    import sv_oracle_c as C
    L, R = _pitched_pair(W, H)
    np.testing.assert_array_equal(got[name], C.disparity16(L, R, 0, 128, 9, 0))


def test_warmup_row_band_and_frame_batch(got):
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
