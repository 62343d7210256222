"""Standard errors of Gaussian Vecchia models with 65 to 128 neighbours: the wide Fisher row kernel
(vecchia_fisher_rows_wide.hip) against long-double rows through GPB_TestVecchiaFisherRows, and the public path against
the CPU oracle. Bv and Dinv take the tolerances of test_wide_factor_matches_long_double_rows. The derivative rows'
bound is measured, not derived: the same hook at m = 64 on the same coordinates is the lane-group kernel, and the wide
kernel may exceed that kernel's largest scaled error by a factor of 4 (2 for twice the summation length, 2 for the
other blocking order). The std-error tolerance is that of tests/test_gpu_stddev_vecchia.py, for the reason given
there."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

LD = np.longdouble
PARS = [0.3, 1.2, 0.15]
NAMES = ("Bv", "dBv_var", "dBv", "Dinv", "dD_var", "dD")


def _cov(ct, var, phi, P, Q):
    """(cov, dcov / dlog phi) in long double, the formulas of csrc/cov.h"""
    r = np.sqrt(((P[:, None, :] - Q[None, :, :]) ** 2).sum(-1))
    x = phi * r * r if ct == 3 else phi * r
    e = var * np.exp(-x)
    return [(e, -x * e), ((1 + x) * e, -x * x * e), ((1 + x + x * x / 3) * e, -x * x / 3 * (1 + x) * e), (e, -x * e)][ct]


def _rows_ref(xv, nbr, ct, var, phi):
    n, m = nbr.shape
    big, small = np.zeros((3, n, m), dtype=LD), np.zeros((3, n), dtype=LD)
    for i in range(n):
        k = min(i, m)
        N = xv[nbr[i, :k]]
        (c, dc), (C, dC) = _cov(ct, var, phi, N, xv[i:i + 1]), _cov(ct, var, phi, N, N)
        c, dc = c[:, 0], dc[:, 0]
        C = C + (var * (LD(np.float64(1. + 1e-10)) - 1) + 1) * np.eye(k, dtype=LD)
        C64 = C.astype(np.float64)

        def solve(b):   # numpy solves in double: refine with long-double residuals (cond(C) < 1e3)
            x = np.zeros(k, dtype=LD)
            for _ in range(3 if k else 0):
                x = x + np.linalg.solve(C64, (b - C @ x).astype(np.float64))
            return x
        a = solve(c)
        t = dC @ a
        big[:, i, :k] = -a, -solve(a), -solve(dc - t)
        small[:, i] = 1 / (var + 1 - a @ c), var - a @ c - a @ a, -(2 * (dc @ a) - t @ a)
    return dict(zip(NAMES, [*big, *small]))


@functools.lru_cache(maxsize=None)
def _run(m, n, ct, d):
    """the hook's six arrays, the long-double rows and, per output, the largest error scaled by the row's largest
    absolute entry"""
    from gpboost_amd import basic, synthetic
    X = synthetic.bench_coords(n) if d == 2 else synthetic.sim_rand_unif(n * d, 0.3).reshape(d, n).T.copy()
    _, xv, nb = O.vecchia_setup(X, m, 0, True)
    _, var, phi = O.transform(ct, PARS)
    got = dict(zip(NAMES, basic.vecchia_fisher_rows(xv, nb, ct, var, phi)))
    ref = _rows_ref(xv.astype(LD), nb, ct, LD(var), LD(phi))
    ratio = {}
    for q in NAMES:
        err, scale = np.abs(got[q] - ref[q]), np.abs(ref[q])
        if err.ndim == 2:
            err, scale = err.max(1), scale.max(1)
        ratio[q] = float((err / np.maximum(scale, LD(1e-300))).max())
    return got, ref, ratio


@pytest.mark.parametrize("m,ct,d", [(80, 0, 2), (80, 1, 2), (80, 2, 2), (80, 3, 2), (65, 0, 2), (113, 0, 2),
                                    (128, 0, 2), (100, 0, 1), (100, 0, 3)])
def test_wide_fisher_rows_match_long_double(m, ct, d):
    """The first wide m, a multiple of 16, one off a multiple of 16 and the limit; n = m + 40 holds rows with k < 64,
    64 <= k < m and full rows.

    Measured on the MI355X (largest scaled error, wide / lane-group kernel): the four derivative outputs lie between
    0.19 and 1.69 times the lane-group kernel's over the nine cases."""
    got, ref, ratio = _run(m, m + 40, ct, d)
    base = _run(64, m + 40, ct, d)[2]   # the lane-group kernel on the same coordinates
    print({q: (ratio[q], base[q]) for q in NAMES})
    np.testing.assert_allclose(got["Dinv"], ref["Dinv"].astype(float), rtol=1e-10)
    np.testing.assert_allclose(got["Bv"], ref["Bv"].astype(float), rtol=1e-8, atol=1e-11)
    for q in ("dBv_var", "dBv", "dD_var", "dD"):
        assert ratio[q] <= 4 * base[q], (q, ratio[q], base[q])
    for q in NAMES[:3]:
        assert all(np.all(got[q][i, i:] == 0.) for i in range(m)), q


@pytest.mark.parametrize("m,cov,shape,ct", [(65, "matern", 1.5, 1), (128, "exponential", 0.5, 0)])
def test_wide_std_err_matches_oracle(m, cov, shape, ct):
    from gpboost_amd import GPModel, synthetic
    from oracle.vecchia_fisher_oracle import vecchia_fisher
    n, cp = 300, [0.2, 1.1, 0.12]
    X = synthetic.bench_coords(n)
    y = synthetic.bench_spatial_gaussian_y(X)
    gm = GPModel(gp_coords=X, cov_function=cov, cov_fct_shape=shape, gp_approx="vecchia", num_neighbors=m, seed=5)
    gm.set_optim_params({"num_rand_vec_trace": 16, "seed_rand_vec_trace": 3})
    gm.neg_log_likelihood(cp, y)
    sd = gm.get_cov_pars(std_err=True)[1]
    _, xv, nb = O.vecchia_setup(X, m, 5, True)
    _, ref = vecchia_fisher(xv, nb, ct, cp, t=16, seed=3)
    np.testing.assert_allclose(sd, ref, rtol=1e-8)


def test_wide_fisher_rows_limit():
    from gpboost_amd import GPBoostError, basic, synthetic
    _, xv, nb = O.vecchia_setup(synthetic.bench_coords(131), 129, 0, True)
    with pytest.raises(GPBoostError, match=r"num_neighbors = 129 > 128"):
        basic.vecchia_fisher_rows(xv, nb, 0, 1.2, 10.)
