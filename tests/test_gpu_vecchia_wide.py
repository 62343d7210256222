"""Gaussian Vecchia models with 65 to 128 neighbours: the wide row kernel (vecchia_rows_wide.hip) against the CPU
oracle, the dense model and long-double rows. Tolerances are those of tests/test_gpu_vecchia.py (RTOL, _close) and,
for the dense identity, of tests/test_gpu_cluster.py. The oracle itself was checked at m = 128 for the four
covariances against a dense numpy slogdet / solve of the same Vecchia precision (agreement to 4e-16 relative, finite gradients)."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-6
COVS = [("exponential", 0.5, 0), ("matern", 1.5, 1), ("matern", 2.5, 2), ("gaussian", 0.5, 3)]


def _model(X, m, cov="exponential", shape=0.5, ordering="random", approx="vecchia"):
    from gpboost_amd import GPModel
    return GPModel(gp_coords=X, cov_function=cov, cov_fct_shape=shape, gp_approx=approx, num_neighbors=m,
                   vecchia_ordering=ordering, seed=0)


def _close(a, b, rtol=RTOL):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1.0))


@pytest.mark.parametrize("cov,shape,ct", COVS)
@pytest.mark.parametrize("m", [65, 80, 96, 113, 128])
def test_wide_vs_oracle_grid(cov, shape, ct, m):
    """The first wide m, a multiple of 16, one off a multiple of 16 and the limit; n = 400 holds short rows
    (k < 64, 64 <= k < m) and full rows with scattered neighbour lists."""
    from gpboost_amd import synthetic
    n = 400
    X, Y = synthetic.bench_coords(n), synthetic.bench_gaussian_y(n)
    pars = [0.3, 1.2, 0.15]
    gm = _model(X, m, cov, shape)
    perm, xv, nb = O.vecchia_setup(X, m, 0, True)
    tp = O.transform(ct, pars)
    for mode in (0, 1):
        ref = O.vecchia_nll_grad(xv, Y[perm], nb, ct, tp, mode)
        nll, g, _ = gm.neg_log_likelihood_and_grad(pars, Y, profile_sigma2=bool(mode))
        assert abs(nll - ref["nll"]) <= RTOL * abs(ref["nll"])
        assert _close(g, ref["grad"]), (m, cov, mode, g, ref["grad"])


@pytest.mark.parametrize("d", [1, 3])
def test_wide_other_dims(d):
    from gpboost_amd import synthetic
    n, m = 300, 100
    X = synthetic.sim_rand_unif(n * d, 0.3).reshape(d, n).T.copy()
    Y = synthetic.bench_gaussian_y(n)
    pars = [0.2, 1.0, 0.2]
    gm = _model(X, m)
    perm, xv, nb = O.vecchia_setup(X, m, 0, True)
    ref = O.vecchia_nll_grad(xv, Y[perm], nb, 0, O.transform(0, pars), 0)
    nll, g, _ = gm.neg_log_likelihood_and_grad(pars, Y)
    assert abs(nll - ref["nll"]) <= RTOL * abs(ref["nll"])
    assert _close(g, ref["grad"])


@pytest.mark.parametrize("m", [65, 128])
def test_wide_all_earlier_points_is_the_dense_model(m):
    """n = m + 1 without reordering: every row conditions on all earlier points, so the Vecchia likelihood is the
    exact one."""
    from gpboost_amd import synthetic
    n = m + 1
    X, Y = synthetic.bench_coords(n), synthetic.bench_gaussian_y(n)
    pars = [0.3, 1.2, 0.15]
    for prof in (False, True):
        a = _model(X, m, ordering="none").neg_log_likelihood_and_grad(pars, Y, profile_sigma2=prof)
        b = _model(X, m, approx="none").neg_log_likelihood_and_grad(pars, Y, profile_sigma2=prof)
        assert abs(a[0] - b[0]) <= 1e-9 * abs(b[0]), (a[0], b[0])
        assert _close(a[1], b[1], 1e-7), (a[1], b[1])


def test_wide_factor_matches_long_double_rows():
    from gpboost_amd import synthetic
    n, m = 300, 96
    X = synthetic.bench_coords(n)
    pars = [0.3, 1.2, 0.15]
    gm = _model(X, m)
    perm, nbr = gm.vecchia_structure()
    dinv, b = gm.vecchia_factor(pars)
    _, var, phi = O.transform(0, pars)
    xv = X[perm].astype(np.longdouble)
    cov = lambda P, Q: var * np.exp(-phi * np.sqrt(((P[:, None, :] - Q[None, :, :]) ** 2).sum(-1)))
    ref_dinv, ref_b = np.zeros(n), np.zeros((n, m))
    for i in range(n):
        k = min(i, m)
        N = xv[nbr[i, :k]]
        c = cov(N, xv[i:i + 1])[:, 0]
        C = cov(N, N) + np.eye(k, dtype=np.longdouble)
        a = np.zeros(k, dtype=np.longdouble)
        for _ in range(3 if k else 0):   # numpy solves in double: refine with long-double residuals (cond(C) < 1e3)
            a = a + np.linalg.solve(C.astype(np.float64), (c - C @ a).astype(np.float64))
        ref_dinv[i] = 1. / (var + 1. - a @ c)
        ref_b[i, :k] = -a
    np.testing.assert_allclose(dinv, ref_dinv, rtol=1e-10)
    np.testing.assert_allclose(b, ref_b, rtol=1e-8, atol=1e-11)
    assert all(np.all(b[i, i:] == 0.) for i in range(m))


def test_wide_limits():
    from gpboost_amd import synthetic
    X, Y = synthetic.bench_coords(131), synthetic.bench_gaussian_y(131)
    with pytest.raises(Exception, match=r"num_neighbors = 129 > 128"):
        _model(X, 129).neg_log_likelihood([0.3, 1.2, 0.15], Y)
    n = 100   # m = 200 is clamped to n - 1 = 99
    gm = _model(X[:n], 200, ordering="none")
    perm, xv, nb = O.vecchia_setup(X[:n], n - 1, 0, False)
    ref = O.vecchia_nll_grad(xv, Y[:n][perm], nb, 0, O.transform(0, [0.3, 1.2, 0.15]), 0)
    nll, g, _ = gm.neg_log_likelihood_and_grad([0.3, 1.2, 0.15], Y[:n])
    assert abs(nll - ref["nll"]) <= RTOL * abs(ref["nll"])
    assert _close(g, ref["grad"])
