"""Built frames for the HOG cost, and the one list of cases the GPU is compared on.

Plain NumPy, seeded.  tests/test_hog_bar.py shows on the CPU, with the oracle alone, that the
frames reach what they claim (every bin boundary from both sides, the axis cases of the sign
normalisation, the largest magnitude, window sums near the u16 halves' bound, ties at every
disparity, costs above 2^15, every matcher plan); tests/test_hog_exact.py and
tests/hog_exact_child.py run the same frames through the engine.

Histogram frames (HIST_FRAMES), three groups:

  boundary  a mosaic of 3x3 patches at stride 3 on a background of 128, every patch centre 128
            and its eight outer pixels solved so that the centre's Sobel pair is a target
            (gx, gy): the reachable pairs within 1000 of a bin boundary (in the oracle's units
            of cos_k gy' - sin_k gx', constants scaled by 16384), the axis pairs, and pairs of
            the largest |gx| + |gy|.  Emitted with 0..3 columns of 128 in front, so that every
            target meets each of a lane's four columns.
  peak      period-4 columns / rows (every pixel magnitude 127 in one bin: window sums of
            225 * 127), the period-4 diagonal saw, diagonal steps (magnitude 191, the largest)
            and a frame whose halves fill bins 0 and 1, the two u16 halves of one packed dword.
  edge      noise with saturated border rows and columns: reflect-101 makes gx = 0 in columns
            0 and W-1 and gy = 0 in rows 0 and H-1 (the axis cases, on the kernel's code
            replication path), at widths that put column W-1 in each of a lane's four columns
            and in a halo lane of the wave before.

A Sobel pair of an 8-bit image is gx = s + q + 2u, gy = s - q + 2v with s, q, u, v differences
of two pixels each (the two diagonals, the middle row, the middle column): the reachable pairs
are those with gx = gy (mod 2), |gx| + |gy| <= 1530 and max(|gx|, |gy|) <= 1020, 1,822,741 in
all.

Matcher pairs (CASES): flat / flat, per8 / per8, per4cols / flat, per4cols / per4rows, a planted
tie and shifted noise, over every plan of the HOG matcher, with random pitch padding that
differs between L and R.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

import sv_oracle as O

SENTINEL = 0x5555        # never a map value: every output is a multiple of 16
HIST_SENTINEL = 0xBEEF   # never a histogram value: sums stay below 225 * 191 = 42,975
SUM_BOUND = 225 * 191    # the largest window sum of one bin (and of all bins together)
NEAR = 1000              # "near a boundary": min_k |cos_k gy' - sin_k gx'| < NEAR


# ------------------------------------------------------------------------------ gradient pairs
def reachable_pairs():
    """(gx, gy) int64 arrays of every Sobel pair an 8-bit image can have."""
    g = np.arange(-1020, 1021, dtype=np.int64)
    GX, GY = np.meshgrid(g, g, indexing="ij")
    m = ((GX - GY) % 2 == 0) & (np.abs(GX) + np.abs(GY) <= 1530)
    return GX[m], GY[m]


def boundary_forms(gx, gy):
    """F[k] = cos_k gy' - sin_k gx' of the sign-normalised pair, k = 0..7 (int64, [8, n])."""
    gx, gy = np.asarray(gx, np.int64), np.asarray(gy, np.int64)
    flip = (gy < 0) | ((gy == 0) & (gx < 0))
    fx, fy = np.where(flip, -gx, gx), np.where(flip, -gy, gy)
    return np.stack([O.HOG_COS[k] * fy - O.HOG_SIN[k] * fx for k in range(8)])


def oracle_bin(gx, gy):
    return (boundary_forms(gx, gy) >= 0).sum(0)


AXIS_VALUES = (1, 2, 4, 8, 14, 16, 30, 100, 254, 256, 510, 766, 1020)


def boundary_targets():
    """[(gx, gy, kind)]: kind 'near' (a), 'axis' (b), 'top' (c); no pair twice."""
    gx, gy = reachable_pairs()
    near = (np.abs(boundary_forms(gx, gy)).min(0) < NEAR) & ((np.abs(gx) + np.abs(gy)) >> 3 > 0)
    t = [(int(a), int(b), "near") for a, b in zip(gx[near], gy[near])]
    for v in AXIS_VALUES:   # (odd values on an axis are not reachable: the generator drops them)
        t += [(v, 0, "axis"), (-v, 0, "axis"), (0, v, "axis"), (0, -v, "axis")]
    for a in list(range(510, 1021, 30)):
        for sx in (1, -1):
            for sy in (1, -1):
                t.append((sx * a, sy * (1530 - a), "top"))
    seen, out = set(), []
    for a, b, kind in t:
        if (a, b) not in seen:
            seen.add((a, b))
            out.append((a, b, kind))
    return out


def solve_patch(gx, gy, rng):
    """A 3x3 uint8 patch with centre 128 whose centre has the Sobel pair (gx, gy), or None.
    gx = s + q + 2u, gy = s - q + 2v with s = p22 - p00, q = p02 - p20, u = p12 - p10, v = p21 -
    p01, each in [-255, 255]: with A = (gx + gy) / 2 = s + u + v and B = (gx - gy) / 2 = q + u -
    v, look for m = u + v near A's excess over 255 and n = u - v near B's."""
    if (gx - gy) % 2:
        return None
    A, B = (gx + gy) // 2, (gx - gy) // 2
    m0 = int(np.sign(A)) * max(0, abs(A) - 255)
    n0 = int(np.sign(B)) * max(0, abs(B) - 255)
    for dm in (0, 1, -1, 2, -2):
        for dn in (0, 1, -1, 2, -2):
            m, n = m0 + dm, n0 + dn
            if (m - n) % 2 or abs(m) + abs(n) > 510 or abs(A - m) > 255 or abs(B - n) > 255:
                continue
            u, v, s, q = (m + n) // 2, (m - n) // 2, A - m, B - n

            def two(d):   # (lo, hi) with hi - lo = d, both bytes
                lo = int(rng.integers(max(0, -d), min(255, 255 - d) + 1))
                return lo, lo + d
            p = np.full((3, 3), 128, np.int64)
            p[0, 0], p[2, 2] = two(s)
            p[2, 0], p[0, 2] = two(q)
            p[1, 0], p[1, 2] = two(u)
            p[0, 1], p[2, 1] = two(v)
            return p.astype(np.uint8)
    return None


@functools.lru_cache(maxsize=None)
def boundary():
    """dict: targets (all), kept [(gx, gy, kind)], dropped, centres [(y, x)] in the unshifted
    mosaic, frames [4 uint8 arrays] with 0..3 columns of 128 in front."""
    rng = np.random.default_rng(20240)
    targets = boundary_targets()
    kept, patches, dropped = [], [], []
    for gx, gy, kind in targets:
        p = solve_patch(gx, gy, rng)
        if p is None:
            dropped.append((gx, gy, kind))
        else:
            kept.append((gx, gy, kind))
            patches.append(p)
    order = rng.permutation(len(kept))
    side = int(np.ceil(np.sqrt(len(kept))))
    mosaic = np.full((3 * side, 3 * side), 128, np.uint8)
    centres = [None] * len(kept)
    for slot, i in enumerate(order):
        py, px = divmod(slot, side)
        mosaic[3 * py:3 * py + 3, 3 * px:3 * px + 3] = patches[i]
        centres[i] = (3 * py + 1, 3 * px + 1)
    frames = [np.concatenate([np.full((3 * side, s), 128, np.uint8), mosaic], axis=1) for s in range(4)]
    for f in frames:
        f.setflags(write=False)
    return dict(targets=targets, kept=kept, dropped=dropped, centres=centres, frames=frames)


# ------------------------------------------------------------------------------ peak patterns
def per4cols(H, W):
    """Columns 0, 0, 255, 255: gx = +-1020, gy = 0 everywhere: magnitude 127, all in bin 0."""
    return np.broadcast_to(np.where(np.arange(W) % 4 >= 2, 255, 0).astype(np.uint8)[None, :], (H, W)).copy()


def per4rows(H, W):
    """Rows 0, 0, 255, 255: gy = +-1020, gx = 0: magnitude 127 in bin 4 (rows 0 and H-1: 0)."""
    return np.broadcast_to(np.where(np.arange(H) % 4 >= 2, 255, 0).astype(np.uint8)[:, None], (H, W)).copy()


def diag_saw(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return (((x + y) % 4) * 85).astype(np.uint8)


def diag_step(H, W):
    """Diagonal stripes 4 wide: the first pixel of a bright stripe has gx = gy = 765."""
    y, x = np.mgrid[0:H, 0:W]
    return np.where((x + y) % 8 >= 4, 255, 0).astype(np.uint8)


def slant(H, W):
    """Stripes at a slope of 2: three pixels of four have magnitude 127 in bin 1."""
    y, x = np.mgrid[0:H, 0:W]
    return np.where((2 * x + y) % 8 < 4, 255, 0).astype(np.uint8)


def halves(H, W):
    """Left half bin 0 (per4cols), right half mostly bin 1 (slant): the two u16 halves of
    packed dword 0 are both large in every window over the seam."""
    g = per4cols(H, W)
    g[:, W // 2:] = slant(H, W)[:, W // 2:]
    return g


PEAK_PATTERNS = {"per4cols": per4cols, "per4rows": per4rows, "diag_saw": diag_saw, "diag_step": diag_step,
                 "halves": halves}
PEAK_SIZES = ((40, 257), (33, 249), (26, 257))   # each ends a wave in another lane


# ------------------------------------------------------------------------------ edge frames
EDGE_RADII = (0, 3, 4, 7)


def cr_geometry(r):
    """(HL, NOUT) of k_hog_hist_cr<r, 4>: halo lanes a side, columns a wave emits."""
    hl = (r + 3) // 4
    return hl, (64 - 2 * hl) * 4


def edge_widths(r):
    """Column W-1 in each of a lane's four columns inside the first wave (9..12), and just
    past a wave (NOUT + 1 .. NOUT + 4 HL, or + 4 without halo lanes): column W-1 is then j = 0..3
    of the second wave's first lanes, and sits in a halo lane of the first wave."""
    hl, nout = cr_geometry(r)
    return [9, 10, 11, 12] + [nout + i for i in range(1, 4 * max(hl, 1) + 1)]


def edge_frame(H, W, seed):
    """Noise whose two outer rows and columns follow 0, 0, 255, 255 along the border (at a random
    phase each): gy = +-1020 in the first and last columns (where gx = 0), gx = +-1020 in the
    first and last rows (where gy = 0)."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (H, W), dtype=np.uint8)
    ph = rng.integers(0, 4, 4)
    along = lambda n, p: np.where((np.arange(n) + p) % 4 >= 2, 255, 0).astype(np.uint8)
    g[:2] = along(W, ph[0])[None, :]
    g[-2:] = along(W, ph[1])[None, :]
    g[:, :2] = along(H, ph[2])[:, None]
    g[:, -2:] = along(H, ph[3])[:, None]
    return g


# ------------------------------------------------------------------------------ histogram frames
def row_bands(H):
    """Two bands whose seam cuts a 24-row strip and a 16-row tile in the middle."""
    c = 20 if H <= 48 else 52
    assert 0 < c < H and c % 24 and c % 16
    return [(0, c), (c, H)]


class HistFrame:
    def __init__(self, group, name, img, wins, pad):
        self.group, self.name, self.wins = group, name, tuple(wins)
        self.H, self.W = img.shape
        self.pitch = self.W + pad
        self.id = f"{group}/{name}/{self.H}x{self.W}p{self.pitch}"
        self._img = np.ascontiguousarray(img, np.uint8)
        self._img.setflags(write=False)

    def __repr__(self):
        return self.id

    @property
    def image(self):
        return self._img

    def padded(self):
        """(H, pitch) bytes: the image, then random padding."""
        rng = np.random.default_rng(zlib.crc32(("pad" + self.id).encode()))
        p = rng.integers(0, 256, (self.H, self.pitch), dtype=np.uint8)
        p[:, :self.W] = self._img
        return p

    def launches(self):
        """[(win, row0, row1)]: the full frame and the two bands, at every window."""
        return [(w, r0, r1) for w in self.wins for r0, r1 in [(0, self.H)] + row_bands(self.H)]


def _hist_frames():
    pads = (3, 8, 61)
    f = []
    for s, img in enumerate(boundary()["frames"]):
        f.append(HistFrame("boundary", f"shift{s}", img, (1, 3), pads[s % 3]))
    i = 0
    for name, fn in PEAK_PATTERNS.items():
        for H, W in PEAK_SIZES:
            f.append(HistFrame("peak", name, fn(H, W), (1, 7, 9, 15), pads[i % 3]))
            i += 1
    for r in EDGE_RADII:
        for W in edge_widths(r):
            f.append(HistFrame("edge", f"r{r}", edge_frame(27, W, 1000 * r + W), (2 * r + 1,), pads[i % 3]))
            i += 1
    return f


HIST_FRAMES = _hist_frames()
assert len({f.id + str(f.wins) for f in HIST_FRAMES}) == len(HIST_FRAMES)
HIST_GROUPS = ("boundary", "peak", "edge")


@functools.lru_cache(maxsize=None)
def expected_hist(index: int, win: int):
    """The oracle's [9, H, W] histograms of HIST_FRAMES[index], computed once per process."""
    h = O.hog_hist(HIST_FRAMES[index].image, win)
    h.setflags(write=False)
    return h


# ------------------------------------------------------------------------------ matcher pairs
PLANS = {64: (4, 16), 96: (6, 16), 128: (8, 16), 192: (6, 32), 256: (8, 32), 384: (6, 64), 512: (8, 64)}
SIBLING = {64: 61, 96: 90, 128: 125, 192: 180, 256: 250, 384: 380, 512: 509}   # padding disparities
D_LIST = sorted(PLANS) + sorted(SIBLING.values())


def plan_of(D):
    """(dpl, lpg) the menu gives D: the first of PLANS whose dpl * lpg holds it."""
    return PLANS[min(k for k in PLANS if k >= D)]


def _noise(rng, H, W):
    return rng.integers(0, 256, (H, W), dtype=np.uint8)


def pair_flat(rng, H, W, **_):
    return np.full((H, W), 77, np.uint8), np.full((H, W), 77, np.uint8)


def pair_per8(rng, H, W, **_):
    """One random pattern of horizontal period 8 per row, the same in L and R: away from the
    image's left and right borders the histograms, and so the costs, repeat every 8 d."""
    pat = rng.integers(0, 256, (H, 8), dtype=np.uint8)
    g = pat[:, np.arange(W) % 8]
    return g.copy(), g.copy()


def pair_cols_flat(rng, H, W, **_):
    return per4cols(H, W), np.full((H, W), 77, np.uint8)


def pair_cols_rows(rng, H, W, **_):
    return per4cols(H, W), per4rows(H, W)


def tie_geometry(W, D, min_disp, win, k):
    """The planted tie: band columns [t0, t1) whose Sobel and window support in L is copied
    into R at the disparities d0 and d0 + k.  k = 0 stands for D - 8 (the second copy's
    disparity index is D - 5, in the last lanes of a group)."""
    r = win // 2
    k = k or D - 8
    d0 = min_disp + 3
    t0 = max(min_disp + D, 0) + 10
    t1 = min(W + min(min_disp, 0), W) - r - 2
    t1 = min(t1, t0 + k - 2 * (r + 1))       # the two copies must not overlap: k >= support
    assert t1 > t0 and t0 - r - 1 - d0 - k >= 0 and d0 + k < min_disp + D
    return dict(t0=t0, t1=t1, d0=d0, d1=d0 + k, lo=t0 - r - 1, hi=t1 + r + 1)


def pair_tie(rng, H, W, D=None, min_disp=0, win=None, k=0, **_):
    t = tie_geometry(W, D, min_disp, win, k)
    L, R = _noise(rng, H, W), _noise(rng, H, W)
    for d in (t["d0"], t["d1"]):
        R[:, t["lo"] - d:t["hi"] - d] = L[:, t["lo"]:t["hi"]]
    return L, R


def pair_noise(rng, H, W, s=5, **_):
    L = _noise(rng, H, W)
    R = _noise(rng, H, W)
    if s >= 0:
        R[:, :W - s] = L[:, s:]
    else:
        R[:, -s:] = L[:, :W + s]
    return L, R


FAMILIES = {"flat": pair_flat, "per8": pair_per8, "cols_flat": pair_cols_flat, "cols_rows": pair_cols_rows,
            "tie": pair_tie, "noise": pair_noise}
ALL_TIE = ("flat", "per8", "cols_flat", "cols_rows")   # at least 8 tying disparities everywhere


def pitch0(W: int) -> int:
    return (W + 3) & ~3


class Case:
    """One sv_disparity_dev call per row band, or one sv_disparity_batch_dev call (nf > 1)."""

    def __init__(self, group, family, H, bw, D, win, min_disp=0, pad=0, bands=None, nf=1, **fkw):
        W = D + max(min_disp, 0) + bw     # bw matched columns: [max(min_disp + D, 0), W + min(min_disp, 0))
        self.group, self.family, self.H, self.W, self.D, self.win = group, family, H, W, D, win
        self.min_disp, self.nf, self.fkw = min_disp, nf, fkw
        self.pitch = pitch0(W) + pad
        self.bands = list(bands) if bands else [(0, H)]
        f = "".join(f",{k}={v}" for k, v in sorted(fkw.items()))
        b = "" if not bands else ",rows=" + "+".join(f"{a}:{z}" for a, z in self.bands)
        self.id = (f"{group}/{family}{f}/{H}x{W}p{self.pitch}/md{min_disp},D{D},w{win}{b}"
                   + (f",nf{nf}" if nf > 1 else ""))

    def __repr__(self):
        return self.id

    @property
    def band(self):
        """[X0, X1): the matched columns."""
        return O.valid_columns(self.W, self.min_disp, self.D)

    @property
    def band_width(self):
        X0, X1 = self.band
        return X1 - X0

    def frame_stride(self):
        """Bytes between the frames of a batch: a whole frame plus a gap."""
        return self.pitch * self.H + 12

    def images(self):
        """[(L, R)] per frame, contiguous H x W."""
        out = []
        for z in range(self.nf):
            rng = np.random.default_rng(zlib.crc32(f"{self.id}#{z}".encode()))
            L, R = FAMILIES[self.family](rng, self.H, self.W, D=self.D, min_disp=self.min_disp, win=self.win,
                                         **self.fkw)
            assert L.shape == R.shape == (self.H, self.W) and L.dtype == R.dtype == np.uint8
            out.append((np.ascontiguousarray(L), np.ascontiguousarray(R)))
        return out

    def frames(self):
        """[(L, R)] per frame as (H, pitch) arrays: the padding columns random, L != R there."""
        out = []
        for z, (L, R) in enumerate(self.images()):
            prng = np.random.default_rng(zlib.crc32(f"pad{self.id}#{z}".encode()))
            Lp = prng.integers(0, 256, (self.H, self.pitch), dtype=np.uint8)
            Rp = (Lp + prng.integers(1, 256, (self.H, self.pitch))).astype(np.uint8)
            Lp[:, :self.W] = L
            Rp[:, :self.W] = R
            out.append((Lp, Rp))
        return out


def _cases():
    c = []
    pads = (0, 4, 60)
    wins, Hs, mds = (1, 7, 15), (1, 5, 9), (-7, 0, 9)
    band_sets = {1: [None], 5: [None, [(1, 4)]], 9: [None, [(0, 4), (4, 9)], [(2, 7)]]}
    for i, D in enumerate(D_LIST):
        def bands(H, j):
            s = band_sets[H]
            return s[(i + j) % len(s)]
        # noise with a shift: about 150 band columns; the window, height and min_disp rotate so
        # that every plan meets each of them over its D and the sibling (i and i + 7)
        w, H, md = wins[(i + i // 7) % 3], Hs[(i + 2 * (i // 7)) % 3], mds[i % 3]
        c.append(Case("noise", "noise", H, 148 + i % 4, D, w, md, pads[i % 3], bands(H, 0), s=md + 3 + i))
        w2 = wins[(i + i // 7 + 1) % 3]
        c.append(Case("noise", "noise", Hs[(i + 1) % 3], 2 * (w2 // 2) + 3, D, w2, mds[(i + 1) % 3],
                      pads[(i + 1) % 3], s=mds[(i + 1) % 3] + D - 2))
        # flat / flat: every disparity ties at cost 0; the narrowest bands
        w = wins[(i + 2) % 3]
        c.append(Case("flat", "flat", Hs[(i + 2) % 3], (1, 2 * (w // 2) + 3, 2)[i % 3], D, w, mds[(i + 2) % 3],
                      pads[(i + 2) % 3]))
        # per4cols / per4rows at win 15, 9 rows: every disparity ties at a cost above 2^15
        c.append(Case("high", "cols_rows", 9, (17, 1, 149)[i % 3], D, 15, mds[(i + 1) % 3], pads[i % 3],
                      bands(9, 1)))
        # per4cols / flat: one high cost at every d
        c.append(Case("high", "cols_flat", 5, (151, 17, 1)[i % 3], D, (7, 15)[i % 2], mds[i % 3],
                      pads[(i + 1) % 3], bands(5, 0)))
        # per8 / per8 (min_disp 9: no candidate window touches R's right border)
        if D >= 90:
            w = (7, 15, 1)[i % 3]
            c.append(Case("per8", "per8", (5, 9)[i % 2], (148, 2 * (w // 2) + 3)[i % 2] + i % 3, D, w, 9,
                          pads[(i + 2) % 3]))
        # the planted tie: first minimum of two equal costs, 3 and D - 5 (or 3 and 43)
        if D in (509, 512, 384, 250, 125, 96, 61):
            for j, (w, k) in enumerate([(7, 0), (15, 0), (7, 40)]):
                if k == 0 and D - 8 < 2 * (w // 2 + 1) + 12:
                    continue
                c.append(Case("tie", "tie", (5, 9, 9)[j], 148 + j, D, w, mds[(i + j) % 3], pads[j], k=k))
    # a band wider than one wave's columns (D = 64: 4 groups of 64 columns)
    c.append(Case("wide", "noise", 5, 300, 64, 7, 0, 4, s=11))
    c.append(Case("wide", "cols_rows", 9, 259, 61, 15, -7, 0))
    # one batch of two frames at D = 512: padded input and output frame strides
    c.append(Case("batch", "noise", 5, 150, 512, 15, 0, 4, nf=2, s=17))
    return c


CASES = _cases()
assert len({k.id for k in CASES}) == len(CASES)
GROUPS = sorted({k.group for k in CASES})
BY_ID = {k.id: k for k in CASES}


@functools.lru_cache(maxsize=None)
def expected(case_id: str):
    """The C oracle's maps of a case, one H x W int16 array per frame: the rows of the case's
    bands hold the map, the rest the sentinel.  Computed once per process and shared."""
    import sv_oracle_c as C
    k = BY_ID[case_id]
    out = []
    for L, R in k.images():
        m = np.full((k.H, k.W), SENTINEL, np.int16)
        for r0, r1 in k.bands:
            m[r0:r1] = C.disparity16(L, R, k.min_disp, k.D, k.win, 2, rows=(r0, r1))[r0:r1]
        m.setflags(write=False)
        out.append(m)
    return tuple(out)


def cost_rows(L, R, k):
    """The oracle's HOG costs, row by row: yields (y, C[band column, disparity index])."""
    X0, X1 = k.band
    hl = O.hog_hist(L, k.win).astype(np.int64)[:, :, X0:X1]            # [9, H, bw]
    hr = O.hog_hist(R, k.win).astype(np.int64)                         # [9, H, W]
    xs = np.arange(X0, X1)[:, None]
    ds = np.arange(k.min_disp, k.min_disp + k.D)[None, :]
    cx = np.clip(xs - ds, 0, k.W - 1)
    for y in range(k.H):
        yield y, np.abs(hl[:, y, :, None] - hr[:, y][:, cx]).sum(0)
