"""GPU parity of the ring kind's SSD form (win 5..9, D <= 256: sv_match_ring.hip ring_ssd): the SAD
ring's packs and cost ring with Σ(L-R)² = ΣL² + ΣR² - 2ΣLR per window column, against the C
oracle's SSD winner-take-all (first minimum); north_star's "SAD/SSD over a disparity sweep".

Through engine.disparity (4-byte aligned frames, pitch = W, here a multiple of 4) the cases with
D % 32 == 0 are taken by the matrix-core kind (sv_ssd_mfma.hip) ahead of the ring; they stay as
they were, each says through Engine.ssd_mfma_query which kind it runs, and the *_odd_pitch
siblings run the same frames through sv_disparity_dev at an odd row pitch, where the ring's
SSD form takes them."""
import numpy as np
import pytest

import sv_oracle_c as C
from stereovision_amd.synthetic import stereo_pair

pytestmark = pytest.mark.gpu

RING_CASES = [(16, 5), (48, 7), (64, 9), (100, 5), (128, 7), (128, 9), (192, 9), (256, 5), (256, 9), (250, 9)]


def _mfma(engine, H, W, md, D, win, pitch=None):
    return engine.ssd_mfma_query(4096, 8192, H, W, W if pitch is None else pitch, md, D, win, "ssd")["mfma"]


def _odd_pitch_disparity(engine, L, R, md, D, win):
    """sv_disparity_dev on the frames at the odd row pitch W + 1 (W even): never the matrix-core
    kind (asked of the query with the launch's own pointers)."""
    H, W = L.shape
    P = W + 1
    assert P % 2 == 1
    rng = np.random.default_rng(W)
    Lp, Rp = (rng.integers(0, 256, (H, P), dtype=np.uint8) for _ in range(2))
    Lp[:, :W], Rp[:, :W] = L, R
    e = engine
    dL, dR, d16 = e.dev_alloc(H * P + 8), e.dev_alloc(H * P + 8), e.dev_alloc(2 * H * W)
    try:
        e.to_device(dL, Lp)
        e.to_device(dR, Rp)
        q = e.ssd_mfma_query(dL, dR, H, W, P, md, D, win, "ssd")
        assert not q["mfma"] and not q["mfma_only"]
        e.disparity_dev(dL, dR, H, W, P, md, D, win, "ssd", 0, H, d16, W)
        e.synchronize()
        return e.to_host(d16, (H, W), np.int16)
    finally:
        for p in (dL, dR, d16):
            e.dev_free(p)


@pytest.mark.parametrize("D,win", RING_CASES)
def test_ssd_ring_matches_oracle(engine, D, win):
    """D % 32 == 0: the matrix-core kind runs these (W = D + 140 is a multiple of 4); the others
    the ring."""
    H, W = 21, D + 140
    L, R, _ = stereo_pair(H, W, D, seed=D * 7 + win)
    assert _mfma(engine, H, W, 0, D, win) == (D % 32 == 0)
    np.testing.assert_array_equal(engine.disparity(L, R, 0, D, win, "ssd"), C.disparity16(L, R, 0, D, win, 1))


@pytest.mark.parametrize("D,win", [c for c in RING_CASES if c[0] % 32 == 0])
def test_ssd_ring_matches_oracle_odd_pitch(engine, D, win):
    """The D % 32 == 0 frames of test_ssd_ring_matches_oracle through the ring's SSD form."""
    H, W = 21, D + 140
    L, R, _ = stereo_pair(H, W, D, seed=D * 7 + win)
    np.testing.assert_array_equal(_odd_pitch_disparity(engine, L, R, 0, D, win), C.disparity16(L, R, 0, D, win, 1))


def test_ssd_ring_extremes_and_ties(engine):
    """Saturated contrast (255 vs 0 columns: the largest squared differences a window holds),
    flat frames (every disparity ties: the smallest wins) and a negative min_disp.  D = 128 at
    W = 400: the matrix-core kind runs these; test_ssd_ring_extremes_and_ties_odd_pitch is the
    ring's."""
    H, W, D, win = 13, 400, 128, 9
    assert _mfma(engine, H, W, 0, D, win) and _mfma(engine, H, W, -7, D, win)
    x = np.arange(W)
    stripes = np.tile(np.where((x // 3) % 2 == 0, 255, 0).astype(np.uint8), (H, 1))
    np.testing.assert_array_equal(engine.disparity(stripes, stripes[:, ::-1].copy(), 0, D, win, "ssd"),
                                  C.disparity16(stripes, stripes[:, ::-1].copy(), 0, D, win, 1))
    flat = np.full((H, W), 200, np.uint8)
    np.testing.assert_array_equal(engine.disparity(flat, flat, 0, D, win, "ssd"),
                                  C.disparity16(flat, flat, 0, D, win, 1))
    L, R, _ = stereo_pair(H, W, D, seed=5)
    np.testing.assert_array_equal(engine.disparity(L, R, -7, D, win, "ssd"), C.disparity16(L, R, -7, D, win, 1))


def test_ssd_ring_extremes_and_ties_odd_pitch(engine):
    """The frames of test_ssd_ring_extremes_and_ties through the ring's SSD form."""
    H, W, D, win = 13, 400, 128, 9
    x = np.arange(W)
    stripes = np.tile(np.where((x // 3) % 2 == 0, 255, 0).astype(np.uint8), (H, 1))
    flipped = stripes[:, ::-1].copy()
    np.testing.assert_array_equal(_odd_pitch_disparity(engine, stripes, flipped, 0, D, win),
                                  C.disparity16(stripes, flipped, 0, D, win, 1))
    flat = np.full((H, W), 200, np.uint8)
    np.testing.assert_array_equal(_odd_pitch_disparity(engine, flat, flat, 0, D, win),
                                  C.disparity16(flat, flat, 0, D, win, 1))
    L, R, _ = stereo_pair(H, W, D, seed=5)
    np.testing.assert_array_equal(_odd_pitch_disparity(engine, L, R, -7, D, win),
                                  C.disparity16(L, R, -7, D, win, 1))
