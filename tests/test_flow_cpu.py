"""The NumPy restatement of the Farneback flow (tests/sv_flow_oracle.py) and the host side of
stereovision_amd.flow, without a GPU: the level table, the polynomial expansion against exact
quadratics and a weighted least-squares fit, planted motion, the branches of the update step,
the RANSAC homography and the expected flow.  The GPU tests compare the kernels with this
restatement bit for bit, so what is checked here is that the restatement is Farneback's flow."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flow_scenes as S  # noqa: E402
import sv_flow_oracle as O  # noqa: E402
from stereovision_amd import flow as F  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)


# ---------------------------------------------------------------------------- level table
@pytest.mark.parametrize("shape,expected", [
    ((16, 16), [(16, 16, 3)]),
    ((37, 70), [(37, 70, 3)]),
    ((64, 80), [(64, 80, 3), (32, 40, 3)]),
    ((67, 133), [(67, 133, 3), (34, 66, 3)]),                      # 33.5 -> 34, 66.5 -> 66: half to even
    ((130, 150), [(130, 150, 3), (65, 75, 3), (32, 38, 9)]),
    ((356, 633), [(356, 633, 3), (178, 316, 3), (89, 158, 9), (44, 79, 19)]),
])
def test_level_table(shape, expected):
    for levels in (O.levels(*shape, 0.5, 3), F.farneback_levels(*shape, 0.5, 3)):
        assert [lv[:3] for lv in levels] == expected
        assert [lv[3] for lv in levels] == [(2.0 ** k - 1) * 0.5 for k in range(len(expected))]


def test_level_table_limits():
    assert len(F.farneback_levels(356, 633, 0.5, 0)) == 1
    assert len(F.farneback_levels(356, 633, 0.5, 1)) == 2
    assert [lv[:2] for lv in F.farneback_levels(100, 100, 0.8, 2)] == [(100, 100), (80, 80), (64, 64)]
    with pytest.raises(ValueError):                                  # sigma 7.5 -> ksize 37 > 31
        F.farneback_levels(2048, 2048, 0.5, 4)
    for bad in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            F.farneback_levels(64, 64, bad, 3)


def test_host_tables_match_the_restatement():
    for n, sigma in ((5, 1.2), (7, 1.5), (5, 1.1)):
        a, b = O.polyexp_tables(n, sigma), F.polyexp_tables(n, sigma)
        for x, y in zip(a[:3], b[:3]):
            np.testing.assert_array_equal(x, y)
        assert tuple(a[3]) == tuple(b[3])
    for k, s in ((3, 0.0), (3, 0.5), (9, 1.5), (19, 3.5)):
        np.testing.assert_array_equal(O.gauss_coef(k, s), F.gaussian_coef(k, s))
    np.testing.assert_array_equal(F.gaussian_coef(3, 0.0), np.array([0.25, 0.5, 0.25], np.float32))


@pytest.mark.parametrize("n,sigma", [(5, 1.2), (7, 1.5)])
def test_closed_form_inverse_is_the_inverse(n, sigma):
    g, _, _, ig = O.polyexp_tables(n, sigma)
    g = np.concatenate([g[:0:-1], g]).astype(np.float64)
    G = np.zeros((6, 6))
    for y in range(-n, n + 1):
        for x in range(-n, n + 1):
            v = np.array([1, x, y, x * x, y * y, x * y], np.float64)
            G += g[y + n] * g[x + n] * np.outer(v, v)
    inv = np.linalg.inv(G)
    # the table's sums take float32 products: relative 2^-24 per term
    np.testing.assert_allclose(ig, (inv[1, 1], inv[0, 3], inv[3, 3], inv[5, 5]), rtol=1e-6)


# ---------------------------------------------------------------------------- polynomial expansion
def _poly_bound(n, sigma, max_abs):
    """Every output is a fixed linear form sum c_ij I_ij of the (2n+1)^2 samples.  Each sample
    is rounded once on input and then passes at most 2n+1 float32 roundings of the vertical
    pass (the horizontal pass and the products with the inverse are float64), each relative
    eps/2, so the error is at most (2n+2) eps/2 K max|I| to first order, K = the largest sum of
    |c_ij| over the five outputs; taken as (2n+1) eps K max|I|."""
    g, xg, xxg, (ig11, ig03, ig33, ig55) = O.polyexp_tables(n, sigma)
    s_g = float(g[0]) + 2 * float(g[1:].sum())
    s_xg = 2 * float(np.abs(xg[1:]).sum())
    s_xxg = 2 * float(xxg[1:].sum())
    K = max(ig11 * s_xg * s_g, abs(ig03) * s_g * s_g + ig33 * s_xxg * s_g, ig55 * s_xg * s_xg)
    return (2 * n + 1) * EPS32 * K * max_abs


@pytest.mark.parametrize("n,sigma", [(5, 1.2), (7, 1.5)])
def test_polyexp_exact_quadratic(n, sigma):
    H, W = 40, 50
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    a, b, c, d, e, f = 3.0, 0.5, -0.25, 0.01, 0.02, -0.015
    img = (a + b * x + c * y + d * x * x + e * y * y + f * x * y).astype(np.float32)
    R = O.polyexp(img, n, sigma)
    bound = _poly_bound(n, sigma, float(np.abs(img).max()))
    # the expansion is local: about (x0, y0) the linear coefficients are the derivatives there
    # (c + 2 e y0 + f x0, b + 2 d x0 + f y0), the quadratic ones are (e, d, f) everywhere
    expected = (c + 2 * e * y + f * x, b + 2 * d * x + f * y, e + 0 * x, d + 0 * x, f + 0 * x)
    inner = (slice(n, H - n), slice(n, W - n))
    for k in range(5):
        err = float(np.abs(R[k][inner] - expected[k][inner]).max())
        print(f"polyexp n={n} plane {k}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("n,sigma", [(5, 1.2), (7, 1.5)])
def test_polyexp_equals_weighted_least_squares(n, sigma):
    rng = np.random.default_rng(11)
    img = (rng.random((33, 41)) * 255).astype(np.float32)
    R = O.polyexp(img, n, sigma)
    g = O.polyexp_tables(n, sigma)[0]
    g = np.concatenate([g[:0:-1], g]).astype(np.float64)
    v, u = np.mgrid[-n:n + 1, -n:n + 1].astype(np.float64)
    sw = np.sqrt(np.outer(g, g)).ravel()
    A = np.stack([np.ones_like(u), u, v, u * u, v * v, u * v], -1).reshape(-1, 6) * sw[:, None]
    bound = _poly_bound(n, sigma, 255.0)
    for y0, x0 in ((n, n), (16, 20), (33 - n - 1, 41 - n - 1), (12, 30)):
        patch = img[y0 - n:y0 + n + 1, x0 - n:x0 + n + 1].astype(np.float64).ravel() * sw
        r = np.linalg.lstsq(A, patch, rcond=None)[0]
        got = R[:, y0, x0]
        err = float(np.abs(got - np.array([r[2], r[1], r[4], r[3], r[5]])).max())
        print(f"polyexp n={n} at ({y0}, {x0}): max error against lstsq {err:.3e}, bound {bound:.3e}")
        assert err <= bound


# ---------------------------------------------------------------------------- planted motion
def test_translation_is_recovered():
    dx, dy = 1.5, -0.75
    prev, nxt = S.translated_pair(67, 133, dx, dy, seed=1)
    flow = O.farneback(prev, nxt)
    assert flow.shape == (67, 133, 2) and flow.dtype == np.float32
    epe = np.hypot(flow[..., 0] - dx, flow[..., 1] - dy)[16:-16, 16:-16]
    med = float(np.median(epe))
    print(f"translation ({dx}, {dy}): median endpoint error over the interior {med:.4f} px")
    # a sign flip or swapped components err by at least the motion's length
    assert med < 0.5 * float(np.hypot(dx, dy))


def test_update_takes_both_branches_and_constant_frames_give_zero_flow():
    H, W = 67, 133
    prev, nxt = S.noise_pair(H, W, seed=0)
    c = {}
    flow = O.farneback(prev, nxt, counters=c)
    assert np.all(np.isfinite(flow))
    # with a zero flow only the last row and column leave the in-image branch: per call H + W - 1
    calls = 3 * sum(h + w - 1 for h, w, _, _ in O.levels(H, W, 0.5, 3))
    print(f"noise pair: {c}, last row and column alone: {calls}")
    assert c["inside"] > 0 and c["outside"] > calls
    c = {}
    flow = O.farneback(np.full((37, 70), 9, np.uint8), np.full((37, 70), 200, np.uint8), counters=c)
    assert not flow.any()
    assert c["outside"] == 3 * (37 + 70 - 1)


def test_update_far_outside_vectors_are_defined():
    rng = np.random.default_rng(5)
    R0 = rng.standard_normal((5, 20, 24)).astype(np.float32)
    R1 = rng.standard_normal((5, 20, 24)).astype(np.float32)
    flow = np.zeros((2, 20, 24), np.float32)
    flow[0, 3, 4], flow[1, 3, 4] = 1e30, -3e9
    flow[0, 10, 10] = np.float32(24 - 1 - 10)              # exactly on the last column
    c = {}
    M = O.update_matrices(R0, R1, flow, c)
    assert np.all(np.isfinite(M[:3]))
    assert c["outside"] == (20 + 24 - 1) + 2


# ---------------------------------------------------------------------------- homography
def _planted(seed=3, n=200):
    rng = np.random.default_rng(seed)
    Ht = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [1e-5, -2e-5, 1.0]])
    src = (rng.random((n, 2)) * [1000, 700]).astype(np.float32)
    w = src[:, 0] * Ht[2, 0] + src[:, 1] * Ht[2, 1] + Ht[2, 2]
    dst = np.stack([(src[:, 0] * Ht[0, 0] + src[:, 1] * Ht[0, 1] + Ht[0, 2]) / w,
                    (src[:, 0] * Ht[1, 0] + src[:, 1] * Ht[1, 1] + Ht[1, 2]) / w], 1).astype(np.float32)
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:int(0.3 * n)]] = True
    ang = rng.random(n) * 2 * np.pi
    move = np.stack([np.cos(ang), np.sin(ang)], 1) * (20 + rng.random((n, 1)) * 30)
    dst[out] += move[out].astype(np.float32)
    return Ht, src, dst, out


def test_homography_planted_inliers():
    Ht, src, dst, out = _planted()
    Hm, mask = F.find_homography_ransac(src, dst, 3.0, 2000, 0.995)
    assert Hm.shape == (3, 3) and Hm.dtype == np.float64 and Hm[2, 2] == 1.0
    assert mask.shape == (len(src), 1) and mask.dtype == np.uint8
    np.testing.assert_array_equal(mask.ravel().astype(bool), ~out)
    s = src[~out].astype(np.float64)
    w = s[:, 0] * Hm[2, 0] + s[:, 1] * Hm[2, 1] + Hm[2, 2]
    px = (s[:, 0] * Hm[0, 0] + s[:, 1] * Hm[0, 1] + Hm[0, 2]) / w
    py = (s[:, 0] * Hm[1, 0] + s[:, 1] * Hm[1, 1] + Hm[1, 2]) / w
    err = float(np.hypot(px - dst[~out, 0], py - dst[~out, 1]).max())
    print(f"planted homography: max inlier reprojection error {err:.2e} px")
    assert err < 0.01                                       # f32 rounding below 1024 px is 6e-5 px
    H2, mask2 = F.find_homography_ransac(src, dst, 3.0, 2000, 0.995)
    assert H2.tobytes() == Hm.tobytes() and mask2.tobytes() == mask.tobytes()


def test_homography_degenerate_inputs():
    t = np.arange(50, dtype=np.float64)
    line = np.stack([t, 2 * t], 1)
    assert F.find_homography_ransac(line, line + [1.0, 0.0]) == (None, None)
    _, src, dst, _ = _planted()
    assert F.find_homography_ransac(src[:3], dst[:3]) == (None, None)
    assert F.find_homography_ransac(src[:0], dst[:0]) == (None, None)


# ---------------------------------------------------------------------------- expected flow
def test_expected_flow_identity_and_translation():
    for fn in (F.expected_flow, O.expected_flow):
        assert not fn(np.eye(3), 20, 30).any()
        e = fn(np.array([[1, 0, 2.5], [0, 1, -1.25], [0, 0, 1.0]]), 20, 30)
        assert e.dtype == np.float32 and e.shape == (20, 30, 2)
        assert (e[..., 0] == 2.5).all() and (e[..., 1] == -1.25).all()
    Hm = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [1e-4, -2e-4, 1.0]])
    np.testing.assert_array_equal(F.expected_flow(Hm, 37, 70), O.expected_flow(Hm, 37, 70))


def test_argument_errors_without_a_gpu():
    g = np.zeros((32, 32), np.uint8)
    bad = [dict(pyr_scale=1.0), dict(pyr_scale=0.0), dict(levels=-1), dict(winsize=4), dict(winsize=1),
           dict(winsize=33), dict(iterations=0), dict(poly_n=6), dict(poly_n=3), dict(flags=256), dict(flags=4)]
    for kw in bad:
        with pytest.raises(ValueError):
            F.farneback_flow(g, g, **kw)
    with pytest.raises(ValueError):
        F.farneback_flow(g[:15], g[:15])
    with pytest.raises(ValueError):
        F.farneback_flow(g, g[:, :20])
    with pytest.raises(TypeError):
        F.farneback_flow(g.astype(np.float32), g.astype(np.float32))
