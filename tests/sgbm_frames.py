"""Hard frames for the SGBM kernels, and the one list of cases the GPU is compared on.

Plain NumPy, seeded.  tests/test_sgbm_bar.py shows on the CPU, with the oracle alone, that
these frames reach the limits the host code reasons about (window cost near 2^15 and 2^16,
int16 paths near both ends, the argmin key's range, ties, both signs of the sub-pixel
numerator, the left-right rule's false side) and that every case run with a filter on keeps
>= 25 % of its band valid; tests/test_sgbm_exact.py and tests/sgbm_variant_child.py run the
same cases through the engine.  Frames are small (H <= 24, band <= ~100 columns) so the
oracle costs milliseconds per case.
"""
from __future__ import annotations

import functools

import numpy as np

import sv_sgbm_oracle as SG

BARE = dict(uniquenessRatio=0, disp12MaxDiff=-1, speckleWindowSize=0)
# oracle keyword -> engine.sgbm keyword
ENGINE_KW = {"disp12MaxDiff": "disp12_max_diff", "uniquenessRatio": "uniqueness_ratio",
             "speckleWindowSize": "speckle_window_size", "preFilterCap": "pre_filter_cap",
             "speckleRange": "speckle_range", "P1": "P1", "P2": "P2"}


# ------------------------------------------------------------------------------ frames
def slope_for(cap: int) -> int:
    """Per-column step whose x-Sobel (8 * step on identical rows) reaches the clip at cap."""
    return -(-cap // 8)


def ramps(H, W, cap=63):
    """L rises toward 255 at the right edge, R falls toward 0 there, rows identical: the
    clipped Sobel channels sit at 2*cap and 0 and the raw channels up to 255 apart."""
    s = slope_for(cap)
    t = (W - 1 - np.arange(W)) * s
    L = np.clip(255 - t, 0, 255)
    R = np.clip(t, 0, 255)
    return (np.repeat(L[None], H, 0).astype(np.uint8), np.repeat(R[None], H, 0).astype(np.uint8))


def sawtooth(H, W, cap=63):
    """The same ramps repeated with period 256 // slope: many distinct minima per row."""
    s = slope_for(cap)
    t = ((W - 1 - np.arange(W)) % (256 // s)) * s
    L = np.clip(255 - t, 0, 255)
    R = np.clip(t, 0, 255)
    return (np.repeat(L[None], H, 0).astype(np.uint8), np.repeat(R[None], H, 0).astype(np.uint8))


def flat(H, W, a=63, b=63):
    """Constants: every disparity ties.  a == b == preFilterCap (63, the value OpenCV's border
    fill puts into columns 0 and W-1 of both channels): C is 0 everywhere, L = -P2 and
    S = -3 P2; any other pair: C is one constant but for the band's last column."""
    return np.full((H, W), a, np.uint8), np.full((H, W), b, np.uint8)


def shifted_noise(H, W, shift=5, seed=0, changed=0.03, levels=256):
    """R is L moved by a whole disparity (L(x) = R(x - shift)) with a few percent of its
    pixels redrawn: unique minima and live sub-pixel parabolas.  levels < 256: grey values
    below `levels` only, so that costs are small and neighbouring S differ by 0 or 1."""
    rng = np.random.default_rng(seed)
    pad = abs(shift)
    base = rng.integers(0, levels, (H, W + 2 * pad), dtype=np.uint8)
    base = ((base.astype(np.int32) + np.roll(base, 1, 1)) // 2).astype(np.uint8)
    L = base[:, pad:pad + W].copy()
    R = base[:, pad + shift:pad + shift + W].copy()
    m = rng.random((H, W)) < changed
    R[m] = rng.integers(0, levels, int(m.sum()), dtype=np.uint8)
    return L, R


def independent_noise(H, W, seed=0):
    """Unrelated images: near-ties everywhere (uniqueness violations where minS > 0)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8))


def vstripes(H, W, lo=0, hi=255):
    """Two-level vertical stripes two pixels wide, R one pixel out of phase: the Sobel clip
    and BT's half-pixel intervals at every column, the column 0 / W-1 fill included."""
    x = np.arange(W)
    L = np.where((x // 2) % 2 == 0, lo, hi)
    R = np.where(((x + 1) // 2) % 2 == 0, lo, hi)
    return (np.repeat(L[None], H, 0).astype(np.uint8), np.repeat(R[None], H, 0).astype(np.uint8))


def hstripes(H, W, lo=0, hi=255):
    """Two-level horizontal stripes two pixels high with a column step in L: the replicated
    rows of the Sobel at the top and bottom, and windows that straddle the stripes."""
    y = np.arange(H)
    L = np.repeat(np.where((y // 2) % 2 == 0, lo, hi)[:, None], W, 1)
    R = np.repeat(np.where(((y + 1) // 2) % 2 == 0, lo, hi)[:, None], W, 1)
    L = L.copy()
    L[:, W // 2:] = 255 - L[:, W // 2:]
    return L.astype(np.uint8), R.astype(np.uint8)


FAMILIES = {"ramps": ramps, "sawtooth": sawtooth, "flat": flat, "shifted": shifted_noise,
            "noise": independent_noise, "vstripes": vstripes, "hstripes": hstripes}


def frame(family: str, H: int, W: int, **kw):
    L, R = FAMILIES[family](H, W, **kw)
    assert L.shape == R.shape == (H, W) and L.dtype == R.dtype == np.uint8
    return L, R


# ------------------------------------------------------------------------------ cases
class Case:
    """One engine.sgbm call: frame family + arguments, (min_disp, D, win) and the oracle's
    keyword parameters."""

    def __init__(self, group, family, H, W, min_disp, D, win, fkw=None, **okw):
        self.group, self.family, self.H, self.W = group, family, H, W
        self.min_disp, self.D, self.win = min_disp, D, win
        self.fkw = dict(fkw or {})
        self.okw = okw
        f = "".join(f",{k}={v}" for k, v in sorted(self.fkw.items()))
        o = "".join(f",{k}={v}" for k, v in sorted(okw.items()))
        self.id = f"{group}:{family}{f}:{H}x{W}:m{min_disp}:D{D}:w{win}{o}"

    @property
    def bare(self):
        return all(self.okw.get(k) == v for k, v in BARE.items())

    @property
    def band(self):
        X0 = max(self.min_disp + self.D, 0)
        X1 = max(self.W + min(self.min_disp, 0), X0)
        return X0, X1

    def frames(self):
        return frame(self.family, self.H, self.W, **self.fkw)

    def engine_kw(self):
        return {ENGINE_KW[k]: v for k, v in self.okw.items()}

    def __repr__(self):
        return self.id


@functools.lru_cache(maxsize=None)
def _expected(case_id: str):
    c = BY_ID[case_id]
    L, R = c.frames()
    out = SG.sgbm(L, R, c.min_disp, c.D, c.win, **c.okw)
    out.setflags(write=False)
    return out


def expected(case: Case) -> np.ndarray:
    """The oracle's map of a case: computed once per process, shared, read-only."""
    return _expected(case.id)


def valid_share(case: Case, out: np.ndarray) -> float:
    """Share of band pixels that are not the invalid value (1.0 for an empty band)."""
    X0, X1 = case.band
    if X1 == X0:
        return 1.0
    return float((out[:, X0:X1] != (case.min_disp - 1) * 16).mean())


CAP_WIN = [(63, 13), (103, 11), (105, 11), (63, 15), (127, 13), (15, 15), (63, 1)]
INT16_CONFIGS = [(63, 13), (103, 11)]          # cmax 31 941 and 32 549: the last int16 ones
INT32_CONFIGS = [(105, 11), (63, 15), (127, 13)]
C1_FRAMES = [("ramps", None), ("sawtooth", None), ("flat", dict(a=63, b=63)),
             ("flat", dict(a=255, b=0)), ("shifted", dict(shift=5, seed=1)),
             ("noise", dict(seed=2)), ("vstripes", {}), ("hstripes", {})]
# C1 with the default filters on: every family again, but for the two configurations at which
# the sawtooth's band is 0 % valid in the oracle's output (uniqueness and the speckle window
# of 100 erase it); everything else keeps >= 25 %, which test_sgbm_bar.py asserts
C1_FILTERED_SKIP = {("sawtooth", (103, 11)), ("sawtooth", (105, 11))}


# Companions run with every filter on: a third of R's pixels redrawn and small penalties, so
# that minS > 0 and uniqueness, the left-right check and the speckle filter (islands of <= 6
# pixels within one disparity) each erase pixels (test_sgbm_bar.py asserts that they do)
NOISY = dict(changed=0.2)
FILTERS = dict(P1=8, P2=32, uniquenessRatio=10, disp12MaxDiff=0, speckleWindowSize=6, speckleRange=1)
C3_RATIOS = (0, 1, 50, 99, 100)
# one num_disp per lane plan of the path kernels: 16-lane lines 1, 2, 4, 8, 12, 16, 20, 24, 32
# disparities per lane; 32-lane lines (D > 128) 6, 8, 10, 12, 16
CVD_NUM_DISP = (16, 32, 48, 128, 130, 256, 320, 384, 500)


def _fkw(family, fkw, cap):
    if fkw is None:                                   # the ramp families follow the cap
        return dict(cap=cap)
    return fkw


def _build():
    cs = []
    H1, W1 = 11, 61                                   # band 45 columns at D = 16
    # C1: bare on every family, then the default filters where the band stays valid
    for cap, win in CAP_WIN:
        for fam, fkw in C1_FRAMES:
            cs.append(Case("c1bare", fam, H1, W1, 0, 16, win, _fkw(fam, fkw, cap), preFilterCap=cap, **BARE))
        for fam, fkw in C1_FRAMES:
            if (fam, (cap, win)) not in C1_FILTERED_SKIP:
                cs.append(Case("c1filt", fam, H1, W1, 0, 16, win, _fkw(fam, fkw, cap), preFilterCap=cap))
    # C2: penalties around the int16/int32 switch and the key's end
    c2 = [("flat", dict(a=63, b=63)), ("flat", dict(a=255, b=0)), ("ramps", dict(cap=63)),
          ("shifted", dict(shift=5, seed=3))]
    for fam, fkw in c2:
        for P2 in (32767, 32768, 32769, 349524):
            cs.append(Case("c2", fam, 7, 49, 0, 16, 5, fkw, P1=600, P2=P2, **BARE))
            cs.append(Case("c2", fam, 7, 49, 0, 16, 5, fkw, P1=P2 - 1, P2=P2, **BARE))
        cs.append(Case("c2", fam, 7, 49, 0, 16, 5, fkw, P1=0, P2=2400, **BARE))
        cs.append(Case("c2", fam, 7, 49, 0, 16, 5, fkw, P1=0, P2=0, **BARE))
    # with the filters on: at these penalties minS < 0, so no filter changes a pixel of these four
    # (test_sgbm_bar.py lists what fires where); they show that the filters erase nothing wrongly
    cs.append(Case("c2", "shifted", 7, 49, 0, 16, 5, dict(shift=5, seed=3), P1=0, P2=2400, speckleWindowSize=20))
    cs.append(Case("c2", "shifted", 7, 49, 0, 16, 5, dict(shift=5, seed=3), P1=32767, P2=32768,
                   speckleWindowSize=20))
    # the uniqueness products (24-bit multiplies) on the most negative S the key can hold
    for fam, fkw in (("flat", dict(a=63, b=63)), ("shifted", dict(shift=5, seed=3))):
        cs.append(Case("c2", fam, 7, 49, 0, 16, 5, fkw, P1=600, P2=349524, uniquenessRatio=10, disp12MaxDiff=1,
                       speckleWindowSize=0))
    # tiny costs and penalties: S[b-1] + S[b+1] - 2 minS sits at 1, the parabola's clamp
    for P1, P2 in ((0, 1), (1, 2)):
        for seed in (0, 1, 2):
            cs.append(Case("c2sub", "shifted", 7, 49, 0, 16, 1, dict(shift=5, seed=seed, changed=0.2, levels=16),
                           P1=P1, P2=P2, preFilterCap=15, **BARE))
    # C3: uniqueness alone (no left-right check, no speckle filter).  S (100 - u) < minS 100 can
    # only hold where minS > 0, and the reference's P2 = 96 win^2 keeps minS negative on noise, so
    # the penalties are chosen for minS to straddle 0: invalid pixels of 369 at u = 0, 1, 50, 99,
    # 100 are 0, 2, 143, 243, 243 (independent noise), 0, 4, 113, 238, 239 (the same at cap 127,
    # win 13: S up to ~10^5 in the 24-bit products) and 0, 2, 129, 241, 244 (shifted noise with a
    # fifth of R redrawn); test_sgbm_bar.py asserts these counts
    for u in C3_RATIOS:
        cs.append(Case("c3", "noise", 9, 57, 0, 16, 3, dict(seed=4), P1=37, P2=150, uniquenessRatio=u,
                       disp12MaxDiff=-1, speckleWindowSize=0))
        cs.append(Case("c3", "noise", 9, 57, 0, 16, 13, dict(seed=4), P1=2000, P2=8000, preFilterCap=127,
                       uniquenessRatio=u, disp12MaxDiff=-1, speckleWindowSize=0))
        cs.append(Case("c3", "shifted", 9, 57, 0, 16, 3, dict(shift=5, seed=5, changed=0.2), P1=8, P2=32,
                       uniquenessRatio=u, disp12MaxDiff=-1, speckleWindowSize=0))
    # C3b: the left-right check where minS >= 32767 occurs (cap 127, win 13 on noise), and
    # where it does not
    for d12 in (0, 1, 5):
        cs.append(Case("c3b", "noise", 9, 57, 0, 16, 13, dict(seed=6), preFilterCap=127, uniquenessRatio=0,
                       disp12MaxDiff=d12, speckleWindowSize=0))
        cs.append(Case("c3b", "sawtooth", 9, 57, 0, 16, 13, dict(cap=127), preFilterCap=127, uniquenessRatio=0,
                       disp12MaxDiff=d12, speckleWindowSize=0))
        cs.append(Case("c3b", "shifted", 9, 57, 0, 16, 3, dict(shift=5, seed=7, changed=0.1), uniquenessRatio=0,
                       disp12MaxDiff=d12, speckleWindowSize=0))
        # low-amplitude noise: equal minS at several x of one right-view column (disp2 keeps the
        # rightmost); the (127, 13) sawtooth on another shape with uniqueness on as well
        cs.append(Case("c3b", "shifted", 9, 57, 0, 16, 1, dict(shift=5, seed=3, changed=0.3, levels=8),
                       preFilterCap=15, P1=1, P2=2, uniquenessRatio=0, disp12MaxDiff=d12, speckleWindowSize=0))
        cs.append(Case("c3b", "sawtooth", 11, 61, 0, 16, 13, dict(cap=127), preFilterCap=127, uniquenessRatio=10,
                       disp12MaxDiff=d12, speckleWindowSize=0))
    # C4: every lane plan's ragged end; Wb odd (<= 40).  D = 5, win 11, Wb 25: Wb * Dp odd
    # whatever Dp's lane multiple, unless Dp is even: test_sgbm_bar.py asserts one odd plane
    for D in (1, 2, 3, 5, 15, 17, 31, 33, 100, 127, 128, 129, 130, 500):
        for win in (3, 11):
            Wb = 25 if D <= 33 else 13
            sh = max(D // 2, 0)
            cs.append(Case("c4", "shifted", 6, D + Wb, 0, D, win, dict(shift=sh, seed=D), **BARE))
            cs.append(Case("c4", "shifted", 6, D + Wb, 0, D, win, dict(shift=sh, seed=D, **NOISY), **FILTERS))
    # C5: band geometry
    for Wb in (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 25):
        cs.append(Case("c5wb", "shifted", 5, 16 + Wb, 0, 16, 5, dict(shift=4, seed=Wb), **BARE))
    for Wb in (0, 1, 3, 9, 25):
        cs.append(Case("c5wb", "shifted", 5, 40 + Wb, 0, 40, 3, dict(shift=9, seed=Wb), **BARE))
    for H in (1, 2, 3, 4, 5):
        cs.append(Case("c5h", "shifted", H, 47, 0, 16, 7, dict(shift=6, seed=H), **BARE))
        cs.append(Case("c5h", "shifted", H, 47, 0, 16, 7, dict(shift=6, seed=H, **NOISY), **FILTERS))
    for m, D in ((-40, 16), (-16, 16), (-20, 16), (-8, 16)):
        cs.append(Case("c5neg", "shifted", 6, 71, m, D, 5, dict(shift=m + D // 2, seed=-m), **BARE))
        cs.append(Case("c5neg", "shifted", 6, 71, m, D, 5, dict(shift=m + D // 2, seed=-m, **NOISY), **FILTERS))
    for m, D, W in ((60, 16, 79), (300, 16, 321), (2032, 16, 2100), (-2047, 16, 61), (-2047, 16, 2100)):
        sh = m + 7
        cs.append(Case("c5pos", "shifted", 1 if W > 2000 else 5, W, m, D, 3, dict(shift=sh, seed=W), **BARE))
    # both ends of the int16 x16 map with every filter on: the speckle stage's new value is
    # -32768 at min_disp = -2047, and the disparities reach 2047 * 16 at min_disp = 2032
    for m in (2032, -2047):
        cs.append(Case("c5pos", "shifted", 3, 2100, m, 16, 3, dict(shift=m + 7, seed=abs(m), **NOISY), **FILTERS))
    # the A/B variants' cases (tests/test_sgbm_variants.py runs them in child processes with a
    # process-static switch set; test_sgbm_exact.py runs them with the defaults): every window
    # of the tiled cost kernels, and every lane plan of the unfused path kernels
    for win in (1, 3, 5, 7, 9):
        cs.append(Case("cvwin", "shifted", 9, 61, 0, 16, win, dict(shift=5, seed=win, **NOISY), **FILTERS))
        cs.append(Case("cvwin", "sawtooth", 9, 61, 0, 16, win, dict(cap=63), **BARE))
    for D in CVD_NUM_DISP:
        cs.append(Case("cvd", "shifted", 6, D + 13, 0, D, 5, dict(shift=D // 3, seed=D), **BARE))
        cs.append(Case("cvd", "shifted", 6, D + 13, 0, D, 5, dict(shift=D // 3, seed=D, **NOISY), **FILTERS))
    # the widest accepted frame
    cs.append(Case("c5wide", "shifted", 2, 16384, 0, 16, 3, dict(shift=6, seed=16384), disp12MaxDiff=1,
                   uniquenessRatio=10, speckleWindowSize=0))
    return cs


CASES = _build()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "duplicate case ids"

# the ragged shapes of tests/test_sgbm.py: (H, W) of test_gpu_sgbm_ragged; the three first had
# 0 % valid band pixels with independent noise and the default speckle window of 100
RAGGED_SHAPES = [(1, 40), (2, 33), (5, 17), (30, 20)]


def ragged_shifted(H, W):
    """The ragged shapes with R a shifted copy of L (run with speckle_window_size = 0)."""
    return shifted_noise(H, W, shift=3, seed=H * W, changed=0.0)


# C6: batches through disparity_batch_dev (cost="sgbm": the reference's parameters, no bare
# mode): (frames, H, W, D, win, min_disp); frame z alternates shifted noise and the sawtooth.
# The speckle window of 100 erases the sawtooth's small regions at most sizes: 12 x 200 keeps
# 31 % of the D = 129 band valid (6 x 170: 0 %), 9 x 77 keeps 66 % at D = 16
BATCHES = [(8, 9, 77, 16, 15, 0), (3, 9, 77, 16, 15, 0), (8, 12, 200, 129, 5, 0), (3, 12, 200, 129, 5, 0)]


def batch_frames(nf, H, W, D, win, min_disp):
    out = []
    for z in range(nf):
        if z % 2 == 0:
            out.append(shifted_noise(H, W, shift=min_disp + 3 + z, seed=50 + z))
        else:
            out.append(sawtooth(H, W, 63))
    return out


@functools.lru_cache(maxsize=None)
def batch_expected(batch):
    nf, H, W, D, win, min_disp = batch
    outs = [SG.sgbm(L, R, min_disp, D, win) for L, R in batch_frames(*batch)]
    for o in outs:
        o.setflags(write=False)
    return outs


def batch_valid_share(batch, out):
    nf, H, W, D, win, min_disp = batch
    X0, X1 = max(min_disp + D, 0), W + min(min_disp, 0)
    return float((out[:, X0:X1] != (min_disp - 1) * 16).mean())
