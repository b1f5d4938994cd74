"""GPU parity of the ring matcher's and the median kernel's work outside their inner loops,
bit-exact against the C oracle:

  * the pack build (sv_match_packs.h sad4_group_words: the per-row words of a 4-column group are
    built from two shared row pairs) for every radius that shares it, on aligned sources (the
    buffer row loads of build_ring_packs), on unaligned ones (build_all_packs' per-column
    form), with clamped top and bottom rows, partial last segments, widths that are no multiple
    of 4 and one or several right-image groups left of column 0 (the library's own report of
    the segment width, SV_RING_OCC, confirms that the sibling cases run two segments);
  * the invalid margins of the context's scratch map, which sv_depth_map_batch_dev writes once
    per geometry (sv_ctx::d16_margins): every change of geometry, every other writer of the
    scratch map, its release and every caller-provided map must leave the margins what the
    oracle says;
  * the median epilogue's unchecked table lookups (k_median_i16<HF, true>), which only a map
    produced by the same call's integer matcher may take: SGBM maps and maps handed in from
    outside (sub-pixel values, values beyond the table) must match the NumPy post.

Every pack case runs as a single frame with a caller's map and as a batch of two frames through
sv_depth_map_batch_dev with the scratch map, where the medians (5x5, so the margins enter) and
the f32 disparities are compared."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

MIN_DEPTH, MAX_DEPTH = 0.3, 2.0
POST_DEPTH, POST_SCALED = 1, 2   # SV_POST_*


def _pair(H, W, D, seed, min_disp=0):
    from stereovision_amd.synthetic import stereo_pair
    L, R, _ = stereo_pair(H, W, D, seed=seed, min_disp=min_disp)
    return L, R


_ORACLE = {}


def oracle16(L, R, min_disp, D, win):
    """C oracle's int16 x16 map, computed once per input pair and never modified."""
    import sv_oracle_c as C
    key = (L.tobytes(), R.tobytes(), L.shape, min_disp, D, win)
    if key not in _ORACLE:
        m = C.disparity16(L, R, min_disp, D, win, 0)
        m.setflags(write=False)
        _ORACLE[key] = m
    return _ORACLE[key]


class Dev:
    """Device buffers of one test, freed together."""

    def __init__(self, engine):
        self.e = engine
        self.ptrs = []

    def alloc(self, nbytes):
        p = self.e.dev_alloc(int(nbytes))
        self.ptrs.append(p)
        return p

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        self.e.to_device(p, a)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.e.dev_free(p)


def _pitched(frames, pitch):
    """[(L, R)] -> two arrays (nf, H + 1, pitch) with the frames at the rows' starts."""
    H, W = frames[0][0].shape
    Ls = np.full((len(frames), H + 1, pitch), 201, np.uint8)
    Rs = np.full((len(frames), H + 1, pitch), 99, np.uint8)
    for z, (l, r) in enumerate(frames):
        Ls[z, :H, :W], Rs[z, :H, :W] = l, r
    return Ls, Rs


def single_map(engine, L, R, min_disp, D, win, pitch, row0=None, row1=None, fill=None):
    """sv_disparity_dev into a caller's map (optionally pre-filled)."""
    H, W = L.shape
    Ls, Rs = _pitched([(L, R)], pitch)
    with Dev(engine) as d:
        dL, dR = d.put(Ls), d.put(Rs)
        init = np.full((H, W), 0 if fill is None else fill, np.int16)
        dO = d.put(init)
        engine.disparity_dev(dL, dR, H, W, pitch, min_disp, D, win, "sad", 0 if row0 is None else row0,
                             H if row1 is None else row1, dO, W)
        engine.synchronize()
        return engine.to_host(dO, (H, W), np.int16).copy()


def batch_run(engine, frames, min_disp, D, win, cost="sad", mode=None, pitch=None, own_map=False, fill=0x7FFF):
    """sv_depth_map_batch_dev (all stages) over `frames`; own_map: the int16 maps go to a
    caller's buffer pre-filled with `fill` (returned as "d16") instead of the scratch map."""
    from stereovision_amd.engine import STAGE_ALL, map_out
    mode = POST_DEPTH if mode is None else mode
    nf = len(frames)
    H, W = frames[0][0].shape
    pitch = W if pitch is None else pitch
    Ls, Rs = _pitched(frames, pitch)
    n = H * W
    with Dev(engine) as d:
        dL, dR = d.put(Ls), d.put(Rs)
        disp, a, b = d.alloc(nf * n * 4), d.alloc(nf * n * 4), d.alloc(nf * n * 4)
        u8, m16 = d.alloc(nf * n), d.alloc(nf * n * 2)
        d16 = d.put(np.full((nf, H, W), fill, np.int16)) if own_map else 0
        out = map_out(mode, disp, a, u8, b if mode != POST_DEPTH else 0, med16=m16, min_depth=MIN_DEPTH,
                      max_depth=MAX_DEPTH, min_disp_global=min_disp)
        engine.depth_map_batch_ex(dL, dR, nf, H, W, pitch, (H + 1) * pitch, min_disp, D, win, cost, STAGE_ALL,
                                  d16, out)
        engine.synchronize()
        res = {"disp": engine.to_host(disp, (nf, H, W), np.float32).copy(),
               "a": engine.to_host(a, (nf, H, W), np.float32).copy(),
               "u8": engine.to_host(u8, (nf, H, W), np.uint8).copy(),
               "m16": engine.to_host(m16, (nf, H, W), np.int16).copy()}
        if mode != POST_DEPTH:
            res["b"] = engine.to_host(b, (nf, H, W), np.float32).copy()
        if own_map:
            res["d16"] = engine.to_host(d16, (nf, H, W), np.int16).copy()
        return res


def expect_post(d16, mode, min_disp, D):
    """NumPy/C-oracle median + post of an int16 x16 map: (m16, disp, a, u8, b)."""
    import sv_oracle_c as C
    disp = C.median5_f32(d16)
    m16 = (disp * 16.0).astype(np.int16)
    if mode == POST_DEPTH:
        a, u8 = C.depth_post(disp, MIN_DEPTH, MAX_DEPTH, min_disp_global=min_disp)
        return m16, disp, a, u8, None
    a, u8, b = C.scaled_post(disp, min_disp, D)
    return m16, disp, a, u8, b


def check_batch(res, maps, mode, min_disp, D):
    for z, d16 in enumerate(maps):
        m16, disp, a, u8, b = expect_post(d16, mode, min_disp, D)
        np.testing.assert_array_equal(res["m16"][z], m16, err_msg=f"median map, frame {z}")
        np.testing.assert_array_equal(res["disp"][z], disp, err_msg=f"disparity, frame {z}")
        np.testing.assert_array_equal(res["a"][z], a, err_msg=f"out_a, frame {z}")
        np.testing.assert_array_equal(res["u8"][z], u8, err_msg=f"out_u8, frame {z}")
        if b is not None:
            np.testing.assert_array_equal(res["b"][z], b, err_msg=f"out_b, frame {z}")
        if "d16" in res:
            np.testing.assert_array_equal(res["d16"][z], d16, err_msg=f"int16 map, frame {z}")


# ---- ring_seg / ring_lds_bytes of sv_match_ring.hip, to find the widths that give two segments ----
def _ring_lds(lpg, seg, r):
    wc = (64 // lpg) * seg
    tn = (seg + 2 * r + 3) & ~3
    nl, nr = wc - seg + tn + 1, wc - seg + tn + 4 * lpg
    nrp = nr + (nr + 1) // 4 + 1
    return (nl + nrp + 10) * (20 if r <= 3 else 24 if r <= 5 else 28) + (2048 if (lpg == 32 and r == 4) else 0)


def _ring_seg(lpg, r, band):
    G, best, best_cost = 64 // lpg, 8, -1
    for S in range(8, 1025, 4):
        if S > 8 and _ring_lds(lpg, S, r) > 20 * 1024:
            break
        cost = -(-band // (G * S)) * ((S + 2 * r + 3) & ~3)
        if best_cost < 0 or cost <= best_cost:
            best, best_cost = S, cost
    return best


def smallest_two_segment_width(D, win):
    """Smallest W whose matched band [D, W) is wider than one segment of the width the launcher
    picks for it (so a second lane group or a second wave runs)."""
    lpg, r = (16 if D <= 64 else 32 if D <= 128 else 64), win // 2
    for W in range(D + 2 * r + 1, D + 2048):
        if W - D > _ring_seg(lpg, r, W - D):
            return W
    raise AssertionError("no width found")


PACK_WIN9 = [(H, W) for H in (12, 21) for W in (268, 396, 398)]
SIBLINGS = [(5, 64), (11, 128), (15, 256)]
BORDER = [(128, 5), (128, 16), (100, 0), (100, 5)]   # (D, min_disp)


def _pack_case(engine, H, W, D, win, min_disp, seed):
    f0, f1 = _pair(H, W, D, seed, min_disp), _pair(H, W, D, seed + 1, min_disp)
    exp0, exp1 = oracle16(*f0, min_disp, D, win), oracle16(*f1, min_disp, D, win)
    aligned = (W + 3) // 4 * 4 + 4
    unaligned = aligned + 1
    for pitch in (aligned, unaligned):
        got = single_map(engine, *f0, min_disp, D, win, pitch, fill=0x7FFF)
        np.testing.assert_array_equal(got, exp0, err_msg=f"single frame, pitch {pitch}")
        res = batch_run(engine, [f0, f1], min_disp, D, win, pitch=pitch)
        check_batch(res, [exp0, exp1], POST_DEPTH, min_disp, D)


@pytest.mark.parametrize("H,W", PACK_WIN9)
def test_pack_shapes(engine, H, W):
    """win 9, D 128: H = 21 ends in a tile with rows past the frame and clamps rows at both ends;
    W = 268 one segment, 396 two groups with a partial last segment, 398 not a multiple of 4."""
    _pack_case(engine, H, W, 128, 9, 0, 100 + H + W)


LAUNCH = re.compile(r"k_match_ring r=(\d+) lpg=(\d+) ldsmin=\d+ seg=(\d+) ")


@pytest.fixture(scope="module")
def sibling_segments():
    """(win, D) -> [(r, lpg, seg)] of the ring launches of the sibling cases, as the library
    itself reports them under SV_RING_OCC=1 (read once per process, hence one child process:
    this file run as a script).  The widths come from this file's copy of the launcher's
    segment choice; the report shows whether that copy still holds."""
    env = dict(os.environ, SV_RING_OCC="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out, cur = {}, None
    for ln in p.stderr.splitlines():
        if ln.startswith("case "):
            cur = tuple(int(v) for v in ln.split()[1:3])
            out[cur] = []
            continue
        m = LAUNCH.match(ln)
        if m and cur is not None:
            out[cur].append(tuple(int(v) for v in m.groups()))
    return out


def _child():
    from stereovision_amd.engine import get_engine
    engine = get_engine(0)
    for win, D in SIBLINGS:
        W = smallest_two_segment_width(D, win)
        sys.stderr.write(f"case {win} {D}\n")
        sys.stderr.flush()
        engine.disparity(*_pair(16, W, D, 200 + win), 0, D, win)


@pytest.mark.parametrize("win,D", SIBLINGS)
def test_pack_shapes_sibling_radii(engine, sibling_segments, win, D):
    """r 2 (one half-filled common word), r 5 (two full ones), r 7 (three, packed halves), each
    at the smallest width whose band is wider than one segment."""
    W = smallest_two_segment_width(D, win)
    launches = sibling_segments.get((win, D))
    assert launches, "the case did not take the ring kind"
    r, lpg, seg = launches[0]
    assert r == win // 2 and seg < W - D <= 2 * seg, (W, launches)   # two segments, the second partial
    _pack_case(engine, 16, W, D, win, 0, 200 + win)


@pytest.mark.parametrize("D,min_disp", BORDER)
def test_pack_shapes_border_groups(engine, D, min_disp):
    """Right-image groups left of column 0.  Groups are aligned to 4 in absolute columns and the
    right image's first pack is column D - r - (4 LPG - 1) whatever min_disp is, so no group can
    straddle column 0: what varies is how many groups lie left of it and the offset d of the
    first pack inside its group.  D = 128: column -3, one border group with one unused column
    (d = -1); D = 100: column -31 (d = -1 as well, eight border groups, padding disparities).
    min_disp > 0 moves the band and the margins, not the groups."""
    _pack_case(engine, 12, 300, D, 9, min_disp, 300 + D + min_disp)


GEOM_A = dict(H=14, W=396, D=128, win=9, min_disp=0)
GEOM_B = dict(H=14, W=268, D=64, win=5, min_disp=16)


def _geom_frames(g, seed, nf=2):
    return [_pair(g["H"], g["W"], g["D"], seed + z, g["min_disp"]) for z in range(nf)]


def _run_geom(engine, g, seed, **kw):
    frames = _geom_frames(g, seed)
    maps = [oracle16(l, r, g["min_disp"], g["D"], g["win"]) for l, r in frames]
    res = batch_run(engine, frames, g["min_disp"], g["D"], g["win"], **kw)
    check_batch(res, maps, POST_DEPTH, g["min_disp"], g["D"])


def _margin_sequence(engines):
    for k, e in enumerate(engines):
        _run_geom(e, GEOM_A, 400 + k)          # fills the scratch map's margins
    for k, e in enumerate(engines):
        _run_geom(e, GEOM_A, 410 + k)          # may leave them
    for k, e in enumerate(engines):
        _run_geom(e, GEOM_B, 420 + k)          # other geometry: other margins, other pitch
    for k, e in enumerate(engines):
        _run_geom(e, GEOM_A, 430 + k)          # B's values lie where A's margins were
    for k, e in enumerate(engines):
        _run_geom(e, GEOM_A, 440 + k, own_map=True, fill=0x7FFF)   # a caller's map: always filled
    for k, e in enumerate(engines):
        g = GEOM_A
        L, R = _pair(g["H"], g["W"], g["D"], 450 + k)
        exp = oracle16(L, R, 0, g["D"], g["win"])
        # a row band through the host entry point writes the scratch map too
        got = e.disparity_rows(L, R, 0, g["D"], g["win"], 3, 11)
        np.testing.assert_array_equal(got[3:11], exp[3:11])
        # ... and through the device entry point into a caller's map
        got = single_map(e, L, R, 0, g["D"], g["win"], g["W"], row0=3, row1=11, fill=0x7FFF)
        np.testing.assert_array_equal(got[3:11], exp[3:11])
        assert (got[:3] == 0x7FFF).all() and (got[11:] == 0x7FFF).all()
    for k, e in enumerate(engines):
        _run_geom(e, GEOM_A, 460 + k)          # after the band: filled again
    for k, e in enumerate(engines):
        # geometry B through the host entry point lands in the scratch map as well: its band
        # values lie in A's margin columns afterwards
        g = GEOM_B
        L, R = _pair(g["H"], g["W"], g["D"], 465 + k, g["min_disp"])
        np.testing.assert_array_equal(e.disparity(L, R, g["min_disp"], g["D"], g["win"]),
                                      oracle16(L, R, g["min_disp"], g["D"], g["win"]))
        _run_geom(e, GEOM_A, 466 + k)
    for k, e in enumerate(engines):
        # the scratch map released, memory of its size dirtied and freed, then A again: the
        # allocator may hand the same address back, which never held the margins
        g = GEOM_A
        _run_geom(e, g, 467 + k)
        e.release_scratch()
        n16 = 2 * g["H"] * g["W"]
        with Dev(e) as d:
            for extra in (0, 0, 64, 4096):
                d.put(np.full(n16 + extra, 0x5A5A, np.int16))
        _run_geom(e, g, 468 + k)
    for k, e in enumerate(engines):
        # a longer batch than the margins were written for, then a shorter one
        g = GEOM_A
        frames = _geom_frames(g, 470 + k, nf=3)
        maps = [oracle16(l, r, 0, g["D"], g["win"]) for l, r in frames]
        check_batch(batch_run(e, frames, 0, g["D"], g["win"]), maps, POST_DEPTH, 0, g["D"])
        check_batch(batch_run(e, frames[:1], 0, g["D"], g["win"]), maps[:1], POST_DEPTH, 0, g["D"])


def test_margin_hoisting(engine):
    _margin_sequence([engine])


def test_margin_hoisting_two_engines(engine):
    from stereovision_amd.engine import Engine
    other = Engine(0)
    try:
        _margin_sequence([engine, other])
    finally:
        other.close()


@pytest.mark.parametrize("W", [130, 256])
@pytest.mark.parametrize("mode_name", ["depth", "scaled"])
def test_epilogue_variants(engine, W, mode_name):
    from stereovision_amd.engine import STAGE_MEDIAN, map_out
    mode = POST_DEPTH if mode_name == "depth" else POST_SCALED
    H, D, win, min_disp = 20, 64, 9, 0
    frames = [_pair(H, W, D, 500 + W + z) for z in range(2)]
    # SAD through the batch entry: the call's own map, unchecked lookups
    maps = [oracle16(l, r, min_disp, D, win) for l, r in frames]
    check_batch(batch_run(engine, frames, min_disp, D, win, mode=mode), maps, mode, min_disp, D)
    # SGBM through the batch entry: sub-pixel values, so the checked form (the expectation is the
    # NumPy post of the map the call itself left in the caller's buffer)
    res = batch_run(engine, frames, min_disp, D, 5, cost="sgbm", mode=mode, own_map=True)
    assert (res["d16"] % 16 != 0).any(), "the SGBM maps should hold sub-pixel disparities"
    check_batch(res, list(res["d16"]), mode, min_disp, D)
    # a map from outside under an integer cost: values that are no multiples of 16 and values
    # below and above the table's range [(min_disp - 1) * 16, (min_disp + D) * 16)
    rng = np.random.default_rng(W + mode)
    up = rng.integers((min_disp - 1) * 16, (min_disp + D) * 16, size=(2, H, W)).astype(np.int16)
    up[0, :, ::7] = (min_disp + D + 20) * 16 + 5
    up[1, ::3, :] = (min_disp - 4) * 16 - 3
    up[1, 5:9, 40:90] = 32767
    up[0, 11:15, 10:60] = -32768
    n = H * W
    with Dev(engine) as d:
        dm = d.put(up)
        disp, a, b, u8, m16 = d.alloc(2 * n * 4), d.alloc(2 * n * 4), d.alloc(2 * n * 4), d.alloc(2 * n), d.alloc(2 * n * 2)
        out = map_out(mode, disp, a, u8, b if mode != POST_DEPTH else 0, med16=m16, min_depth=MIN_DEPTH,
                      max_depth=MAX_DEPTH, min_disp_global=min_disp)
        engine.depth_map_batch_ex(0, 0, 2, H, W, W, n, min_disp, D, win, "sad", STAGE_MEDIAN, dm, out)
        engine.synchronize()
        res = {"disp": engine.to_host(disp, (2, H, W), np.float32).copy(),
               "a": engine.to_host(a, (2, H, W), np.float32).copy(),
               "u8": engine.to_host(u8, (2, H, W), np.uint8).copy(),
               "m16": engine.to_host(m16, (2, H, W), np.int16).copy()}
        if mode != POST_DEPTH:
            res["b"] = engine.to_host(b, (2, H, W), np.float32).copy()
    check_batch(res, list(up), mode, min_disp, D)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    _child()
