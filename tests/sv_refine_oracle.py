"""NumPy restatement of the refinement stage of the winner-take-all maps —
TEST INFRASTRUCTURE ONLY: what sv_disparity_right_dev, sv_refine_dev and sv_disparity_refined
are held bit-equal to.

Notation: L, R gray u8 H x W; minD, numD, win (odd) the matcher's parameters; INV = (minD - 1) *
16; C(x, y, d) the window cost of ``oracle.sv_oracle.disparity16`` (replicate-clamped rows and
columns, right column index clip(x + i - d, 0, W - 1)), SAD or SSD.

Right-referenced map:  dR = flipx(disparity16(flipx(R), flipx(L), minD, numD, win, cost)).

Refinement of any int16 map dL, per pixel:
  0. dL is not 16 d with minD <= d <= minD + numD - 1            -> INV
  1. lr_max_diff >= 0 and a right map: x' = x - d; 0 <= x' < W, dR(x', y) != INV and
     |dR(x', y) / 16 - d| > lr_max_diff                          -> INV
  2. (SAD / SSD; needed when min_curvature > 0 or subpixel) c0 = C(d), cm = C(d - 1), cp = C(d + 1);
     d == minD: cm := cp; else d == minD + numD - 1: cp := cm; numD == 1: both c0
  3. curv = cm + cp - 2 c0; min_curvature > 0 and curv < min_curvature   -> INV
  4. subpixel: den = curv + |cp - cm|; q = trunc((cm - cp) * 256 / den) when c0 <= cm, c0 <= cp
     and den > 0, else 0; out = (d * 256 + q + 15) >> 4 (floor).  Without: out = 16 d
  5. speckle_window > 0: filterSpeckles(out, INV, speckle_window, 16 * speckle_range)
"""
from __future__ import annotations

import numpy as np

import sv_oracle as O
from sv_sgbm_oracle import filter_speckles

COST_SAD, COST_SSD, COST_HOG = O.COST_SAD, O.COST_SSD, O.COST_HOG


def disparity16_right(L, R, min_disp, num_disp, win, cost=COST_SAD):
    Lf = np.ascontiguousarray(np.asarray(L)[:, ::-1])
    Rf = np.ascontiguousarray(np.asarray(R)[:, ::-1])
    return np.ascontiguousarray(O.disparity16(Rf, Lf, min_disp, num_disp, win, cost)[:, ::-1])


def right_valid_columns(W, min_disp, num_disp):
    x0 = max(-min_disp, 0)
    return x0, max(x0, W - max(min_disp + num_disp, 0))


def window_cost(L, R, d, win, cost):
    """C(x, y, d[y, x]) for a per-pixel integer disparity array d, int64."""
    L = np.asarray(L, np.uint8)
    R = np.asarray(R, np.uint8)
    H, W = L.shape
    r = win // 2
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.asarray(d, np.int64)
    c = np.zeros((H, W), np.int64)
    for j in range(-r, r + 1):
        yy = np.clip(ys + j, 0, H - 1)
        for i in range(-r, r + 1):
            l = L[yy, np.clip(xs + i, 0, W - 1)].astype(np.int64)
            rr = R[yy, np.clip(xs + i - d, 0, W - 1)].astype(np.int64)
            df = l - rr
            c += np.abs(df) if cost == COST_SAD else df * df
    return c


def refine(L, R, dL, min_disp, num_disp, win, cost=COST_SAD, dR=None, lr_max_diff=1, min_curvature=1,
           subpixel=True, speckle_window=0, speckle_range=2):
    L = np.asarray(L, np.uint8)
    R = np.asarray(R, np.uint8)
    v = np.asarray(dL, np.int16).astype(np.int64)
    H, W = v.shape
    inv = (min_disp - 1) * 16
    dmax = min_disp + num_disp - 1
    d = v >> 4
    valid = ((v & 15) == 0) & (d >= min_disp) & (d <= dmax)                      # 0
    d = np.where(valid, d, min_disp)
    if dR is not None and lr_max_diff >= 0:                                      # 1
        vr_all = np.asarray(dR, np.int16).astype(np.int64)
        ys, xs = np.mgrid[0:H, 0:W]
        xr = xs - d
        inside = (xr >= 0) & (xr < W)
        vr = vr_all[ys, np.clip(xr, 0, W - 1)]
        valid &= ~(inside & (vr != inv) & (np.abs(vr - 16 * d) > 16 * lr_max_diff))
    out = d * 16
    if min_curvature > 0 or subpixel:                                            # 2
        if cost not in (COST_SAD, COST_SSD):
            raise ValueError("the curvature test and the sub-pixel step need SAD or SSD")
        c0 = window_cost(L, R, d, win, cost)
        if num_disp == 1:
            cm = cp = c0
        else:
            # never a cost outside the sweep: the missing side is the other one
            cm = window_cost(L, R, np.maximum(d - 1, min_disp), win, cost)
            cp = window_cost(L, R, np.minimum(d + 1, dmax), win, cost)
            cm = np.where(d == min_disp, cp, cm)
            cp = np.where((d == dmax) & (d != min_disp), cm, cp)
        curv = cm + cp - 2 * c0                                                   # 3
        if min_curvature > 0:
            valid &= curv >= min_curvature
        if subpixel:                                                              # 4
            den = curv + np.abs(cp - cm)
            ok = (c0 <= cm) & (c0 <= cp) & (den > 0)
            num = (cm - cp) * 256
            sden = np.where(ok, den, 1)
            q = np.where(ok, np.sign(num) * (np.abs(num) // sden), 0)              # truncation toward zero
            out = (d * 256 + q + 15) >> 4
    out = np.where(valid, out, inv).astype(np.int16)
    if speckle_window > 0:                                                       # 5
        out = filter_speckles(out, inv, speckle_window, 16 * speckle_range)
    return out


def disparity_refined(L, R, min_disp, num_disp, win, cost=COST_SAD, lr_max_diff=1, min_curvature=1,
                      subpixel=True, speckle_window=0, speckle_range=2):
    dL = O.disparity16(L, R, min_disp, num_disp, win, cost)
    dR = disparity16_right(L, R, min_disp, num_disp, win, cost) if lr_max_diff >= 0 else None
    return refine(L, R, dL, min_disp, num_disp, win, cost, dR, lr_max_diff, min_curvature, subpixel,
                  speckle_window, speckle_range)
