"""Hard frames for the SSD matcher kinds, and the one list of cases the GPU is compared on.

Plain NumPy, seeded.  tests/test_ssd_bar.py shows on the CPU, from the frames alone, that the
table reaches what it claims (both ends of the matrix-core kind's key range, the correction
term at its largest, planted ties, every width residue, height and template instance);
tests/test_ssd_exact.py and tests/ssd_exact_child.py run the same cases through the engine.
Frames are small (the matched band W - D is at most 257 columns, 40 for the tall ones) so the
C oracle costs milliseconds per case.

Every frame is built at its row pitch: the padding columns [W, pitch) of every row hold
random bytes that differ between L and R and must never act as data.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

SENTINEL = 0x5555   # never a map value: every output is a multiple of 16


# ------------------------------------------------------------------------------ the shape
def shape(win: int, D: int, rows: int):
    """Restatement of ssd_shape (sv_ssd_mfma.hip) for `rows` output rows in one launch: the
    template instance (xt, nt, mb, big), the band height hb, and the key range's terms.  None:
    the matrix-core kind does not run (win, D).  tests/test_ssd_exact.py checks it against
    Engine.ssd_mfma_query case by case."""
    if win < 1 or win > 15 or win % 2 == 0 or D < 32 or D > 256 or D % 32:
        return None
    nt = D // 32 + 1
    xt = 2 if 4 <= nt <= 5 else 1
    mb = 7 if D <= 128 else 8
    M = 1 << mb
    n = win * win
    cmax, sl2 = n * 255 * 255, n * 128 * 128
    bias, hw = (cmax - sl2) // 2, (cmax + sl2 + 1) // 2
    hb = rows if rows < 96 else 64
    if rows >= 256 and win <= 9:
        hb = 96
    hb = max(hb, 1)
    cor = (hb + win) * win * 128
    R = M * hw + 2 * M * cor + 32 * (4 * xt + nt - 1) + 64
    if R >= 1 << 31:
        return None
    big = (R + M - 1) // M * M < 1 << 30
    return dict(xt=1 if big else xt, nt=nt, mb=mb, hb=hb, big=big, M=M, bias=bias, hw=hw, R=R)


def instance(win: int, D: int, rows: int):
    s = shape(win, D, rows)
    return None if s is None else (s["xt"], s["nt"], s["mb"], s["big"])


# every instance launch_ssd_mfma's switch can be handed (ssd_shape picks xt = 2 only for nt 4, 5
# without the accumulator offset: <2,2,..> and <2,3,..> of the switch are never selected)
INSTANCES = sorted({instance(w, D, 16) for D in range(32, 257, 32) for w in (9, 11, 13, 15)
                    if instance(w, D, 16)})


# ------------------------------------------------------------------------------ frames
def _two_level(rng, shp, hi, p=0.5):
    """The extreme grey level 0 (hi False) or 255 (hi True; an array picks per pixel), moved one
    level inwards with probability p: noise in {0, 1} or {254, 255}."""
    n = (rng.random(shp) < p).astype(np.int64)
    return np.where(hi, 255 - n, n).astype(np.uint8)


def _blocks(rng, H, W, win, p):
    """Vertical blocks win + 1 wide alternating between {0, 1} and {254, 255} noise."""
    hi = (np.arange(W) // (win + 1)) % 2 == 1
    return _two_level(rng, (H, W), np.broadcast_to(hi[None, :], (H, W)), p)


def sat_lo(rng, H, W, win, p=0.5, **_):
    return np.zeros((H, W), np.uint8), _blocks(rng, H, W, win, p)


def sat_hi(rng, H, W, win, p=0.5, **_):
    return np.full((H, W), 255, np.uint8), _blocks(rng, H, W, win, p)


def near_top(rng, H, W, win, L=0, p=0.5, **_):
    """L = 0 against R in {254, 255} (L = 255: R in {0, 1}): every key near the top of val."""
    return np.full((H, W), L, np.uint8), _two_level(rng, (H, W), L == 0, p)


def near_bottom(rng, H, W, win, L=0, p=0.5, **_):
    """L = 0 against R in {0, 1} (L = 255: R in {254, 255}): every key near the bottom."""
    return np.full((H, W), L, np.uint8), _two_level(rng, (H, W), L != 0, p)


def periodic(rng, H, W, win, P=8, s=1, nick=False, **_):
    """Each row its own random pattern of horizontal period P; L(x) = R(x - s): the window
    costs at d = s, s + P, ... are all zero away from the borders.  nick: sparse single R pixels
    moved by one grey level, so one of the tied candidates is cheaper by exactly 1."""
    pat = rng.integers(0, 256, (H, P), dtype=np.uint8)
    x = np.arange(W)
    R = pat[:, x % P].copy()
    L = pat[:, (x - s) % P].copy()
    if nick:
        m = rng.random((H, W)) < 1.0 / (win * win)
        R[m] = np.where(R[m] < 255, R[m] + 1, 254).astype(np.uint8)
    return L, R


def checker(rng, H, W, win, c=3, s=2, **_):
    y, x = np.mgrid[0:H, 0:W]
    T = lambda xx: ((((xx // c) + (y // c)) & 1) * 255).astype(np.uint8)
    return T(x - s), T(x)


def noise(rng, H, W, win, **_):
    return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)


FAMILIES = {"sat_lo": sat_lo, "sat_hi": sat_hi, "near_top": near_top, "near_bottom": near_bottom,
            "periodic": periodic, "checker": checker, "noise": noise}


def pitch0(W: int) -> int:
    return (W + 3) & ~3


def odd_pitch(W: int) -> int:
    """The fallback leg's pitch: odd, so no frame row but the first starts 4-byte aligned."""
    return (W | 1) + 2


# ------------------------------------------------------------------------------ cases
class Case:
    """One sv_disparity_dev / sv_disparity_batch_dev call (or one call per row band)."""

    def __init__(self, group, family, H, W, D, win, min_disp=0, pad=0, bands=None, nf=1, **fkw):
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
    def band_width(self):
        X0 = max(self.min_disp + self.D, 0)
        X1 = min(self.W + min(self.min_disp, 0), self.W)
        return max(X1 - X0, 0)

    def frame_stride(self, pitch):
        """Bytes between the frames of a batch: a whole frame plus a gap (a multiple of 4)."""
        return pitch * self.H + 8

    def frames(self, pitch=None):
        """[(L, R)] per frame as (H, pitch) arrays: columns < W the family's frame, the rest
        random padding."""
        pitch = self.pitch if pitch is None else pitch
        out = []
        for z in range(self.nf):
            rng = np.random.default_rng(zlib.crc32(f"{self.id}#{z}".encode()))
            L, R = FAMILIES[self.family](rng, self.H, self.W, self.win, **self.fkw)
            assert L.shape == R.shape == (self.H, self.W) and L.dtype == R.dtype == np.uint8
            prng = np.random.default_rng(zlib.crc32(f"pad{self.id}#{z}".encode()))
            Lp = prng.integers(0, 256, (self.H, pitch), dtype=np.uint8)
            Rp = (Lp + prng.integers(1, 256, (self.H, pitch))).astype(np.uint8)   # != Lp everywhere
            Lp[:, :self.W] = L
            Rp[:, :self.W] = R
            out.append((Lp, Rp))
        return out

    def images(self):
        """[(L, R)] per frame, contiguous H x W."""
        return [(np.ascontiguousarray(L[:, :self.W]), np.ascontiguousarray(R[:, :self.W]))
                for L, R in self.frames()]


def _cases():
    c = []
    pads = (0, 4, 64)
    sat = ("sat_lo", "sat_hi")

    # every template instance (and windows 1 and 3), each on a saturated frame at W % 4 != 0
    insts = [(D, w) for D in (32, 64, 96, 128) for w in (13, 15)] + \
            [(D, w) for D in (160, 192, 224, 256) for w in (9, 11)] + [(64, 1), (128, 3)]
    for i, (D, w) in enumerate(insts):
        bw = (33, 130, 131)[i % 3]
        c.append(Case("inst", sat[i % 2], 7 + i % 3, D + bw, D, w, pad=pads[i % 3]))

    # matched-band widths (min_disp = 0: W - D columns): 1..3 columns, one column either side of
    # a tile and of a block (128 columns; 256 for the two-x-tile form D=128 w15)
    fams = [("noise", {}), ("periodic", dict(P=8, s=2)), ("sat_lo", {}), ("checker", {}), ("sat_hi", {})]
    cfgs = [(64, 13), (96, 13), (160, 9), (32, 15), (256, 11)]   # one x-tile per wave: blocks of 128
    for i, bw in enumerate((1, 2, 3, 5, 31, 32, 33, 127, 128, 129, 130, 131)):
        D, w = cfgs[i % len(cfgs)]
        fam, kw = fams[(i + i // 5) % len(fams)]
        c.append(Case("width", fam, 6, D + bw, D, w, pad=pads[i % 3], **kw))
    for i, bw in enumerate((255, 257, 130, 3)):
        fam, kw = fams[(i + 2) % len(fams)]
        c.append(Case("width", fam, 5, [128, 96][i % 2] + bw, [128, 96][i % 2], 15, pad=pads[(i + 1) % 3], **kw))

    # heights below the DMA distance (5 steps) and around the window
    for i, H in enumerate((1, 2, 4, 5, 6, 12, 13)):
        c.append(Case("short", ("noise", "sat_hi", "near_bottom")[i % 3], H, 32 + 33, 32, 13, pad=pads[i % 3]))
    for i, H in enumerate((1, 2, 4, 5, 6, 8, 9)):
        c.append(Case("short", ("sat_lo", "noise", "near_top")[i % 3], H, 160 + 31, 160, 9, pad=pads[(i + 1) % 3]))

    # heights around one and two block bands (hb = rows below 96, then 64): saturated at
    # hb = 64, at a single band of 95 rows, and with a last band of one row (129)
    tall = {63: [("noise", 64, 15, {}), ("near_bottom", 160, 9, dict(L=255))],
            64: [("sat_lo", 64, 15, {}), ("near_top", 192, 11, {})],
            65: [("sat_hi", 32, 13, {}), ("noise", 160, 9, {})],
            95: [("sat_lo", 128, 15, {}), ("near_top", 160, 11, {}), ("near_bottom", 32, 13, dict(L=255))],
            96: [("sat_hi", 64, 15, {}), ("near_top", 256, 9, {})],
            97: [("noise", 96, 15, {}), ("sat_lo", 160, 9, {})],
            129: [("sat_lo", 128, 13, {}), ("sat_hi", 224, 11, {}), ("periodic", 64, 15, dict(P=33, s=1))]}
    i = 0
    for H, lst in tall.items():
        for fam, D, w, kw in lst:
            c.append(Case("tall", fam, H, D + (33, 38, 39, 40)[i % 4], D, w, pad=pads[i % 3], **kw))
            i += 1
    # win <= 9 from 256 rows: hb = 96 (289: a last band of one row); win 11 at 256: 4 bands of 64
    for i, (H, fam, D, w, kw) in enumerate([(256, "sat_lo", 32, 9, {}), (257, "near_top", 160, 9, {}),
                                            (289, "sat_hi", 64, 9, {}), (289, "near_top", 256, 7, {}),
                                            (256, "near_bottom", 128, 5, dict(L=255)),
                                            (256, "sat_lo", 192, 11, {}), (256, "noise", 64, 11, {})]):
        c.append(Case("tall96", fam, H, D + (34, 37, 39, 40)[i % 4], D, w, pad=pads[i % 3], **kw))

    # planted ties: inside one lane's registers and across the lane halves (P = 4, 8), across
    # x'-tiles (32, 33), in the first and the last (triangular) x'-tile (P = D - 1, s = 0)
    for i, (D, w) in enumerate([(64, 13), (128, 15), (160, 9), (96, 13), (256, 11), (32, 15)]):
        for j, (P, s) in enumerate([(4, 1), (8, 3), (32, 0), (33, 2), (D - 1, 0)]):
            if ((i + j) % 2 and P != D - 1) or s + P >= D:   # (a second tied disparity must exist)
                continue
            for nick in (False, True):
                c.append(Case("ties", "periodic", 9, D + (65, 66, 131)[(i + j) % 3], D, w,
                              pad=pads[(i + j) % 3], P=P, s=s, nick=nick))
    c.append(Case("ties", "checker", 11, 128 + 67, 128, 13, pad=4))
    c.append(Case("ties", "checker", 11, 192 + 67, 192, 9, c=4, s=3))

    # min_disp: the invalid margins on both sides, R's right border (negative values)
    for i, (D, w) in enumerate([(64, 15), (128, 13), (160, 11), (32, 13)]):
        for j, md in enumerate((-5, 3, -(D + 2))):
            fam, kw = [("noise", {}), ("sat_hi", {}), ("periodic", dict(P=8, s=2, nick=True)),
                       ("sat_lo", {})][(i + j) % 4]
            c.append(Case("mindisp", fam, 8, D + 70 + i + j, D, w, min_disp=md, pad=pads[(i + j) % 3], **kw))

    # row bands through sv_disparity_dev: the first row alone, the rest, and three unequal
    # bands whose middle one spans two 64-row block bands
    for i, (D, w, fam) in enumerate([(64, 15, "sat_lo"), (192, 9, "noise"), (128, 13, "sat_hi"),
                                     (256, 11, "near_top")]):
        c.append(Case("bands", fam, 21, D + 34 + i, D, w, pad=pads[i % 3], bands=[(0, 1), (1, 21)]))
        c.append(Case("bands", fam, 150, D + 35 + i, D, w, pad=pads[(i + 1) % 3],
                      bands=[(0, 20), (20, 130), (130, 150)]))

    # batches of 3 frames at a padded frame stride
    for i, (D, w, fam, H) in enumerate([(64, 13, "sat_hi", 9), (128, 15, "noise", 7), (160, 9, "sat_lo", 70),
                                        (224, 11, "periodic", 5), (32, 15, "near_bottom", 3)]):
        c.append(Case("batch", fam, H, D + (33, 130, 37, 131, 2)[i], D, w, pad=pads[i % 3], nf=3))

    # the ends of the key range: sparse noise (p = 0.01), so some windows sit exactly on the
    # extreme (all R pixels 0 or 255) and their neighbours one to a few units inside, at
    # hb = 64, hb = 96 and a single band of 95 rows
    for i, (fam, L, H, D, w) in enumerate([
            ("near_bottom", 0, 64, 64, 15), ("near_bottom", 0, 95, 32, 13), ("near_bottom", 0, 256, 160, 9),
            ("near_bottom", 255, 95, 128, 15), ("near_bottom", 255, 64, 192, 11), ("near_bottom", 255, 289, 32, 9),
            ("near_top", 255, 64, 96, 15), ("near_top", 255, 256, 224, 9), ("near_top", 255, 95, 160, 11),
            ("near_top", 0, 95, 64, 15), ("near_top", 0, 128, 256, 11), ("near_top", 0, 257, 128, 9)]):
        c.append(Case("range", fam, H, D + (33, 34, 35, 38)[i % 4], D, w, pad=pads[i % 3], L=L, p=0.01))

    # W % 4 == 0 frames of the families the host path (pitch = W) is run on
    for i, (fam, D, w, kw) in enumerate([("sat_lo", 64, 15, {}), ("sat_hi", 160, 9, {}), ("sat_lo", 128, 13, {}),
                                         ("periodic", 96, 15, dict(P=8, s=1)),
                                         ("periodic", 192, 11, dict(P=33, s=0, nick=True)),
                                         ("periodic", 32, 13, dict(P=4, s=2, nick=True))]):
        c.append(Case("host4", fam, 9 + i, D + (32, 36, 132)[i % 3], D, w, pad=pads[i % 3], **kw))

    # the other two pitches for D >= 160 and generic noise at W % 4 == 0
    for i, (D, w) in enumerate([(160, 11), (192, 9), (224, 9), (256, 11), (64, 13), (128, 15)]):
        c.append(Case("pitch", ("noise", "sat_lo")[i % 2], 10, D + (36, 133, 64)[i % 3], D, w, pad=(64, 4)[i % 2]))
    return c


CASES = _cases()
assert len({k.id for k in CASES}) == len(CASES)
GROUPS = sorted({k.group for k in CASES})
BY_ID = {k.id: k for k in CASES}


@functools.lru_cache(maxsize=None)
def expected(case_id: str):
    """The oracle's maps of a case, one H x W int16 array per frame: the rows of the case's
    bands hold the map, the rest the sentinel.  Computed once per process and shared."""
    import sv_oracle_c as C
    k = BY_ID[case_id]
    out = []
    for L, R in k.images():
        m = np.full((k.H, k.W), SENTINEL, np.int16)
        for r0, r1 in k.bands:
            m[r0:r1] = C.disparity16(L, R, k.min_disp, k.D, k.win, 1, rows=(r0, r1))[r0:r1]
        m.setflags(write=False)
        out.append(m)
    return tuple(out)
