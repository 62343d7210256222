"""The weighted tall-skinny product behind the covariate Gram matrix of gp_approx = "fitc" / "full_scale_vecchia"
(csrc/lowrank_gram.hip), element-wise against exact sums through the test entry GPB_TestWeightedTallSkinny:

    T = A diag(w) U (m x c),   G0 = U^T diag(w) U (c x c)

A is m x n column-major with leading dimension round_up(m, 64), the layout of the solvers' K_mn / BK.

Reference: every product a_i w_i u_i is formed in numpy.longdouble and the n products of an entry are summed by
math.fsum (each longdouble product enters as its double head plus its double tail, so nothing of it is rounded
away). Bound: |error| <= (n + 4) 2^-53 sum_i |a_i w_i u_i| per entry, the standard bound of a length-n
floating-point sum in any order (n - 1 additions, one rounding of w_i u_i and one of each product, and the
reference's own rounding): derived, not measured.

Shapes: one point range and several, n no multiple of the range length (512), of the LDS step (64) or of the
MFMA's 4; m below, at and above the 64-row workgroup tile and no multiple of 16; c = 1, odd c, c above 16 (the
second column tile) and c = 32 (the maximum).
"""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 1), (37, 333, 3), (64, 1000, 32), (50, 2049, 17), (130, 515, 2)]
U53 = 2.0 ** -53


def _hook(m, n, c, A, w, U):
    from gpboost_amd.basic import lib
    D = ctypes.POINTER(ctypes.c_double)
    f = lib().GPB_TestWeightedTallSkinny
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, D, ctypes.c_int64, D, D, D, D]
    f.restype = ctypes.c_int
    T = np.full((m, c), np.nan)
    G0 = np.full((c, c), np.nan)
    p = lambda a: a.ctypes.data_as(D)   # noqa: E731
    for a in (A, w, U):
        assert a.dtype == np.float64 and a.flags.c_contiguous
    rc = f(m, n, c, p(A), A.size, p(w), p(U), p(T), p(G0))
    assert rc == 0, lib().LGBM_GetLastError()
    return T, G0


def _inputs(m, n, c):
    rng = np.random.default_rng(20240 + 1000 * m + 10 * n + c)
    ldm = (m + 63) // 64 * 64

    def decades(shape):   # magnitudes over six decades, mixed signs
        return rng.choice([-1., 1.], size=shape) * 10. ** rng.uniform(-3., 3., size=shape)

    Am = decades((m, n))
    A = np.full((n, ldm), np.nan)   # point i's m entries contiguous; the padding rows must never be read into a sum
    A[:, :m] = Am.T
    w = 10. ** rng.uniform(-2., 2., size=n)
    U = decades((n, c))
    return Am, np.ascontiguousarray(A).ravel(), w, U


def _exact(p):
    """fsum of the longdouble products p and sum |p|: each enters as head + tail doubles (exactly)"""
    hi = p.astype(np.float64)
    lo = (p - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist()), float(np.abs(p).sum())


@pytest.mark.parametrize("m,n,c", SHAPES)
def test_weighted_tall_skinny_matches_exact_sums(m, n, c):
    Am, A, w, U = _inputs(m, n, c)
    T, G0 = _hook(m, n, c, A, w, U)
    Al, wl, Ul = Am.astype(np.longdouble), w.astype(np.longdouble), U.astype(np.longdouble)
    wU = wl[:, None] * Ul
    checked = 0
    worst = 0.
    for j in range(c):
        for i in range(m):
            ref, mag = _exact(Al[i] * wU[:, j])
            err = abs(T[i, j] - ref)
            worst = max(worst, err / (U53 * mag))
            assert err <= (n + 4) * U53 * mag, ("T", i, j, T[i, j], ref, err / (U53 * mag))
            checked += 1
        for a in range(c):
            ref, mag = _exact(Ul[:, a] * wU[:, j])
            err = abs(G0[a, j] - ref)
            worst = max(worst, err / (U53 * mag))
            assert err <= (n + 4) * U53 * mag, ("G0", a, j, G0[a, j], ref, err / (U53 * mag))
            checked += 1
    print(f"(m, n, c) = {(m, n, c)}: worst error {worst:.2f} units of 2^-53 sum|a w u| (bound {n + 4})")
    assert checked == m * c + c * c
    assert np.array_equal(G0, G0.T)
    # equal inputs give equal bits
    T2, G02 = _hook(m, n, c, A, w, U)
    assert np.array_equal(T, T2) and np.array_equal(G0, G02)


def test_weighted_tall_skinny_rejects_bad_extents():
    from gpboost_amd.basic import lib
    D = ctypes.POINTER(ctypes.c_double)
    f = lib().GPB_TestWeightedTallSkinny
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, D, ctypes.c_int64, D, D, D, D]
    f.restype = ctypes.c_int
    z = np.zeros(64 * 4)
    p = lambda a: a.ctypes.data_as(D)   # noqa: E731
    out = np.zeros(33 * 33)
    for m, n, c, a_len in [(0, 4, 1, 256), (3, 0, 1, 256), (3, 4, 0, 256), (3, 4, 33, 256), (3, 4, 1, 12), (3, 4, 1, 255)]:
        assert f(m, n, c, p(z), a_len, p(z), p(z), p(out), p(out)) == -1, (m, n, c, a_len)
        assert b"GPB_TestWeightedTallSkinny" in lib().LGBM_GetLastError()
