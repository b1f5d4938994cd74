"""Adversarial gray frames for the bit-exact Harris tests (tests/test_harris_exact.py on the
GPU, tests/test_harris_bar.py on the CPU) and the case list both walk.

Every builder is deterministic in (H, W, seed).  The textures:

* noise     uniform u8 noise: |R| up to 3e-2, almost no pixel under 1e-4
* stereo    a synthetic.stereo_pair left frame (what the fused path was tested with)
* nearflat  100 + {0..3}: |R| ~ 1e-9, far under any absolute tolerance
* vstripes  columns 0 255 255 0 0 ... (pairs straddle the wave seams 59|60, 247|248): |gx| = 1020, Sxx reaches 9 * 1020^2, the largest box sum
            u8 pixels can give; the pattern shifts by one pixel at rows 8 and 16 (the band
            seams; at row H - 2 where the frame holds neither), which puts a cross term on
            the seam and keeps the map from being one constant
* hstripes  the same transposed: |gy| = 1020, Syy reaches the bound; shifts at columns 59,
            247 and 495 (the last column of a wave; at column W - 2 where the frame holds none)
* checker   2 x 2 cells of 0 / 255: gx, gy and the cross term all large
            (Stripes and cells are two pixels wide, not one: with one-pixel stripes the pixels
            at x - 1 and x + 1 are equal, every Sobel difference is zero under reflect-101 and
            the expected map is all zero, which would check nothing.)
* impulses  zero background, single 255 pixels: each response is a known 5x5 footprint, so a
            missing neighbour, a wrong reflected product or a wrong gx*gy sign is a few exact
            wrong values.  Impulses sit at the four corners, the middle of each border, columns
            58-61 / 246-249 / 494-497 (the 60- and 248-column wave seams) and rows 6-9 / 14-17
            (the 8- and 16-row band seams), wherever the frame holds them.
"""
import numpy as np

from stereovision_amd.synthetic import stereo_pair

TEXTURES = ("noise", "stereo", "nearflat", "vstripes", "hstripes", "checker", "impulses")

# max(Sxx, Syy, |Sxy|) over a 3x3 box of Sobel products of u8 pixels
SUM_BOUND = 9 * 1020 * 1020


def impulse_points(H, W):
    """(y, x) of the impulses of an H x W frame: seam columns on seam rows (one column per row,
    so neighbouring footprints overlap on some rows and stand alone on others), the corners
    and the middle of each border."""
    cols = [c for c in (58, 59, 60, 61, 246, 247, 248, 249, 494, 495, 496, 497) if c < W]
    rows = [r for r in (6, 7, 8, 9, 14, 15, 16, 17) if r < H]
    pts = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1),
           (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)}
    for k, c in enumerate(cols):
        if rows:
            pts.add((rows[k % len(rows)], c))
    for k, r in enumerate(rows):
        pts.add((r, cols[k % len(cols)] if cols else (3 * k + 1) % W))
    return sorted(pts)


def _shifts(idx, n, seams):
    """How many one-pixel shifts lie at or before each index."""
    at = [s for s in seams if s <= n - 2] or [n - 2]
    return sum((idx >= s).astype(np.int64) for s in at)


def frame(texture, H, W, seed=0):
    rng = np.random.default_rng([seed, H, W])
    if texture == "noise":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if texture == "stereo":
        return stereo_pair(H, W, 32, seed)[0]
    if texture == "nearflat":
        return (100 + rng.integers(0, 4, (H, W))).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    if texture == "vstripes":
        return ((((x + 1 + _shifts(y, H, (8, 16))) >> 1) & 1) * 255).astype(np.uint8)
    if texture == "hstripes":
        return ((((y + 1 + _shifts(x, W, (59, 247, 495))) >> 1) & 1) * 255).astype(np.uint8)
    if texture == "checker":
        return ((((x >> 1) + (y >> 1)) & 1) * 255).astype(np.uint8)
    if texture == "impulses":
        g = np.zeros((H, W), np.uint8)
        for py, px in impulse_points(H, W):
            g[py, px] = 255
        return g
    raise ValueError(texture)


def assert_not_vacuous(exp, what):
    """The expected map must be able to tell a right answer from zeros or a constant."""
    assert np.any(exp != 0), f"{what}: expected Harris map is all zero"
    assert np.unique(exp).size >= 5, f"{what}: expected Harris map holds under 5 distinct values"


# ---- stand-alone engine.harris -----------------------------------------------------------
# (8,8) one band, one wave; (9,61) a second band of one row and a second wave of one column;
# (16,60) exactly two bands, exactly one wave; (17,121) a third band of one row, a third wave
# of one column; (16,256) / (13,258) the 1-column kernel past 4 waves, W % 4 == 0 / 2;
# (11,1030) the 4-column kernel: interior fast loads (waves 1..3), ragged last wave of 38
# columns, W % 4 == 2 (scalar stores)
STANDALONE_SHAPES = [(8, 8), (9, 61), (16, 60), (17, 121), (16, 256), (13, 258), (11, 1030)]

# ---- Harris inside the median launch -----------------------------------------------------
# (H, W, pad, tail, textures): pitch = W + pad, frame stride = H * pitch + tail, 2 frames.
# The branch each case is there for is in test_harris_exact.py's docstring (same order).
MEDIAN_CASES = [
    # 60-column waves, k_median_i16<1, *> (W < 256)
    (8, 60, 0, 0, ("noise", "impulses")),
    (15, 61, 1, 0, ("noise", "vstripes")),
    (16, 64, 4, 0, ("stereo", "hstripes")),
    (17, 121, 0, 0, ("noise", "impulses")),
    (33, 255, 1, 0, ("noise", "checker")),
    (16, 61, 4, 3, ("nearflat", "impulses")),
    (17, 255, 0, 0, ("stereo", "impulses")),
    (33, 64, 1, 0, ("noise", "nearflat")),
    # 248-column waves, k_median_i16<2, *>: every W mod 4
    (8, 256, 0, 0, ("noise", "impulses")),
    (15, 257, 0, 0, ("noise", "vstripes")),
    (16, 258, 4, 0, ("stereo", "impulses")),
    (17, 259, 1, 0, ("noise", "hstripes")),
    (33, 260, 0, 0, ("noise", "impulses")),
    (17, 256, 4, 0, ("nearflat", "checker")),
    (16, 260, 1, 0, ("noise", "impulses")),
    (33, 257, 4, 0, ("stereo", "impulses")),
    # second wave at the seam, not interior
    (8, 496, 0, 0, ("noise", "impulses")),
    (16, 497, 0, 0, ("noise", "impulses")),
    (17, 496, 4, 0, ("stereo", "vstripes")),
    (33, 497, 1, 0, ("nearflat", "impulses")),
    (15, 496, 1, 0, ("noise", "checker")),
    # second wave interior: dword loads
    (8, 500, 0, 0, ("noise", "impulses")),
    (16, 504, 0, 0, ("noise", "impulses")),
    (17, 500, 4, 0, ("stereo", "impulses")),
    (33, 504, 4, 0, ("noise", "hstripes")),
    (15, 500, 0, 0, ("noise", "impulses")),        # odd H, H * pitch % 4 == 0: both frames fast
    (17, 504, 1, 0, ("noise", "impulses")),        # odd H * pitch; pitch % 4 != 0: both frames slow
    (16, 504, 0, 2, ("noise", "vstripes")),        # stride % 4 == 2: frame 1 slow, frame 0 fast
    (15, 504, 4, 0, ("nearflat", "impulses")),     # pitch > W, % 4 == 0: both fast, pad never read
    (33, 500, 0, 1, ("stereo", "checker")),        # odd stride: frame 1 slow, frame 0 fast
]
# under 8 px a side the Harris response takes a launch of its own (the LDS-tile kernel)
SMALL_CASES = [(7, 70, 1, 0, ("noise", "impulses")), (20, 7, 0, 0, ("noise", "impulses"))]


def case_frames(case):
    """The two left frames of a median-launch case."""
    H, W, pad, tail, tex = case
    return [frame(t, H, W, seed=z) for z, t in enumerate(tex)]
