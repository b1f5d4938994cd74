"""The census / Hamming cost's definition (tests/sv_census_oracle.py), pinned without a GPU:
known answers of the transform, the strict comparison, invariance under brightness offsets, the
robustness the cost exists for (a darkened right frame keeps the census map and destroys the SAD
map), and the engine's cost parsing."""
from __future__ import annotations

import numpy as np
import pytest

import sv_oracle as O
import sv_census_oracle as CO
from stereovision_amd.synthetic import stereo_pair


def test_flat_image_gives_zero_codes():
    for v in (0, 7, 255):
        assert not CO.census(np.full((9, 13), v, np.uint8)).any()


def test_single_peak_sets_all_62_bits():
    img = np.zeros((7, 9), np.uint8)
    img[3, 4] = 200
    c = CO.census(img)
    assert c[3, 4] == np.uint64(0x3FFFFFFFFFFFFFFF)
    # every other pixel sees no darker neighbour (the peak is brighter, zeros are equal)
    c[3, 4] = 0
    assert not c.any()


def test_low_corner_sets_bit_zero():
    img = np.full((7, 9), 100, np.uint8)
    img[0, 0] = 10
    c = CO.census(img)
    assert c[3, 4] == np.uint64(1)          # (dy, dx) = (-3, -4) is k = 0
    assert CO.OFFSETS[0] == (-3, -4) and CO.OFFSETS[61] == (3, 4) and len(CO.OFFSETS) == 62
    assert CO.OFFSETS[30] == (0, -1) and CO.OFFSETS[31] == (0, 1)   # the centre is skipped


def test_equal_neighbours_give_zero_bits():
    rng = np.random.default_rng(5)
    img = (rng.integers(0, 4, (23, 31)) * 64).astype(np.uint8)   # 4 levels: many equal neighbours
    c = CO.census(img)
    H, W = img.shape
    for k, (dy, dx) in enumerate(CO.OFFSETS):
        yy = np.clip(np.arange(H) + dy, 0, H - 1)
        xx = np.clip(np.arange(W) + dx, 0, W - 1)
        nb = img[yy][:, xx]
        bit = ((c >> np.uint64(k)) & np.uint64(1)).astype(bool)
        assert not bit[nb == img].any(), k        # equal: strict comparison gives 0
        assert bit[nb < img].all() and not bit[nb > img].any(), k
    assert not (c >> np.uint64(62)).any()


def test_popcount_and_flat_match():
    a = np.array([[0, 1, 0xFFFFFFFFFFFFFFFF, 0x8000000000000001]], np.uint64)
    assert CO.popcount64(a).tolist() == [[0, 1, 64, 2]]
    flat = np.full((12, 40), 9, np.uint8)
    d = CO.disparity16_census(flat, flat, -3, 8, 5)
    x0, x1 = O.valid_columns(40, -3, 8)
    assert (d[:, x0:x1] == -3 * 16).all()         # all costs tie at 0: the first minimum
    assert (d[:, :x0] == -4 * 16).all() and (d[:, x1:] == -4 * 16).all()


def test_offset_without_saturation_leaves_the_map_equal():
    L, R, _ = stereo_pair(40, 120, 24, seed=2)
    L2 = (L // 2).astype(np.uint8)
    R2 = (R // 2 + 90).astype(np.uint8)             # <= 127 + 90: no saturation
    a = CO.disparity16_census(L2, (R // 2).astype(np.uint8), 0, 24, 7)
    b = CO.disparity16_census(L2, R2, 0, 24, 7)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(CO.census((R // 2).astype(np.uint8)), CO.census(R2))


@pytest.mark.parametrize("shape,seed,win,ref_census,ref_sad", [((96, 200, 32), 1, 7, 0.9985, 0.032),
                                                                ((64, 160, 48), 3, 5, 0.9937, 0.021)])
def test_darkened_right_frame_keeps_census_and_breaks_sad(shape, seed, win, ref_census, ref_sad):
    H, W, D = shape
    L, R, _ = stereo_pair(H, W, D, seed=seed)
    Rd = np.floor(0.5 * R.astype(np.float64) + 20).astype(np.uint8)
    kc = CO.kept_fraction(CO.disparity16_census(L, R, 0, D, win), CO.disparity16_census(L, Rd, 0, D, win), 0, D)
    ks = CO.kept_fraction(O.disparity16(L, R, 0, D, win, O.COST_SAD), O.disparity16(L, Rd, 0, D, win, O.COST_SAD), 0, D)
    print(f"kept: census {kc:.4f} (reference {ref_census}), sad {ks:.4f} (reference {ref_sad})")
    assert kc >= 0.99
    assert ks <= 0.10


def test_rows_and_right_map_compose():
    L, R, _ = stereo_pair(20, 64, 12, seed=4)
    full = CO.disparity16_census(L, R, 0, 12, 5)
    band = CO.disparity16_census(L, R, 0, 12, 5, rows=(6, 13))
    np.testing.assert_array_equal(band[6:13], full[6:13])
    assert (band[:6] == -16).all() and (band[13:] == -16).all()
    dr = CO.disparity16_right(L, R, 0, 12, 5)
    x0, x1 = 0, 64 - 12
    assert (dr[:, x1:] == -16).all() and (dr[:, x0:x1] != -16).all()
    ref = CO.disparity_refined(L, R, 0, 12, 5, lr_max_diff=1, speckle_window=0)
    assert ((ref == full) | (ref == -16)).all()


def test_engine_cost_parsing_accepts_census():
    from stereovision_amd import engine as E
    assert E.COSTS["census"] == 4 and E._cost("census") == 4 and E._cost("CENSUS") == 4
    assert E.KERNELS["census"] == 27
    assert {"sv_census_dev", "sv_census_match_dev"} <= set(E.EXPORTED)
    with pytest.raises(ValueError):
        E._cost("censu")
