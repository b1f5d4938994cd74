"""NumPy restatement of the census / Hamming matching cost — TEST
INFRASTRUCTURE ONLY: what sv_census_dev, sv_census_match_dev and cost = "census" of every
entry point are held bit-equal to.

Census code C(x, y), uint64: the 9-wide x 7-tall neighbourhood enumerated row-major, dy = -3..3
outer, dx = -4..4 inner, without (0, 0): k = 0..61.  Bit k is 1 iff Ip(x + dx, y + dy) < I(x, y)
(strict; Ip the replicate-clamped image).  Bits 62 and 63 are 0.

cost(x, y, d) = sum over |i|, |j| <= win // 2 of popcount(CLp(x+i, y+j) ^ CRp(x+i-d, y+j)), the
code planes with replicate-clamped coordinates (the code AT the clamped coordinate), all 64 bits
counted; d* = the first argmin over d in [minD, minD + numD); the map is the int16 x16 map of
``oracle.sv_oracle.disparity16``: d* * 16 inside valid_columns, (minD - 1) * 16 outside and on
rows that were not asked for.

The right-referenced and the refined maps compose tests/sv_refine_oracle.py with these functions
(census maps take the left-right check and the speckle filter only).
"""
from __future__ import annotations

import numpy as np

import sv_oracle as O
import sv_refine_oracle as RO

COST_CENSUS = 4
NB_RX, NB_RY = 4, 3
OFFSETS = [(dy, dx) for dy in range(-NB_RY, NB_RY + 1) for dx in range(-NB_RX, NB_RX + 1) if (dy, dx) != (0, 0)]


def census(img: np.ndarray) -> np.ndarray:
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape
    cy = np.clip(np.arange(-NB_RY, H + NB_RY), 0, H - 1)
    cx = np.clip(np.arange(-NB_RX, W + NB_RX), 0, W - 1)
    p = img[cy][:, cx]
    out = np.zeros((H, W), np.uint64)
    for k, (dy, dx) in enumerate(OFFSETS):
        nb = p[NB_RY + dy:NB_RY + dy + H, NB_RX + dx:NB_RX + dx + W]
        out |= (nb < img).astype(np.uint64) << np.uint64(k)
    return out


def popcount64(a: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(a, np.uint64).view(np.uint8).reshape(a.shape + (8,))
    return np.unpackbits(b, axis=-1).sum(-1).astype(np.int64)


def match_codes(CL: np.ndarray, CR: np.ndarray, min_disp: int, num_disp: int, win: int,
                rows: tuple[int, int] | None = None) -> np.ndarray:
    CL = np.ascontiguousarray(CL, np.uint64)
    CR = np.ascontiguousarray(CR, np.uint64)
    H, W = CL.shape
    r = win // 2
    y0, y1 = (0, H) if rows is None else rows
    invalid = (min_disp - 1) * 16
    out = np.full((H, W), invalid, np.int16)
    x0, x1 = O.valid_columns(W, min_disp, num_disp)
    if x1 <= x0 or y1 <= y0:
        return out
    best_c = np.full((y1 - y0, x1 - x0), np.iinfo(np.int64).max, np.int64)
    best_d = np.zeros((y1 - y0, x1 - x0), np.int64)
    cy = np.clip(np.arange(y0 - r, y1 + r), 0, H - 1)
    xs = np.arange(x0 - r, x1 + r)
    lp = CL[cy][:, np.clip(xs, 0, W - 1)]
    rows_r = CR[cy]
    for d in range(min_disp, min_disp + num_disp):
        rp = rows_r[:, np.clip(xs - d, 0, W - 1)]
        c = O._box_sum(popcount64(lp ^ rp), r)
        m = c < best_c
        best_c[m] = c[m]
        best_d[m] = d
    out[y0:y1, x0:x1] = (best_d * 16).astype(np.int16)
    return out


def disparity16_census(L, R, min_disp: int, num_disp: int, win: int, rows=None) -> np.ndarray:
    return match_codes(census(L), census(R), min_disp, num_disp, win, rows)


def disparity16_right(L, R, min_disp, num_disp, win):
    Lf = np.ascontiguousarray(np.asarray(L)[:, ::-1])
    Rf = np.ascontiguousarray(np.asarray(R)[:, ::-1])
    return np.ascontiguousarray(disparity16_census(Rf, Lf, min_disp, num_disp, win)[:, ::-1])


def disparity_refined(L, R, min_disp, num_disp, win, lr_max_diff=1, speckle_window=0, speckle_range=2):
    dL = disparity16_census(L, R, min_disp, num_disp, win)
    dR = disparity16_right(L, R, min_disp, num_disp, win) if lr_max_diff >= 0 else None
    return RO.refine(L, R, dL, min_disp, num_disp, win, COST_CENSUS, dR, lr_max_diff, 0, False, speckle_window,
                     speckle_range)


def kept_fraction(a: np.ndarray, b: np.ndarray, min_disp: int, num_disp: int) -> float:
    """Share of the matched band's pixels on which two maps agree."""
    x0, x1 = O.valid_columns(a.shape[1], min_disp, num_disp)
    return float((a[:, x0:x1] == b[:, x0:x1]).mean())
