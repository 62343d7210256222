"""Gaussian models with the Matern covariance at a general smoothness (cov_fct_shape other than 0.5, 1.5, 2.5): the
wave-per-row Vecchia kernel (num_neighbors <= 64), the wide row kernel's general-shape instantiation (65 .. 128) and
the dense path, against a plain float64 reference whose covariances come from mpmath's Bessel functions.

Reference: the neighbour sets are the model's own (vecchia_structure); every row's B and D come from a dense solve,
the likelihood is the sum over rows of (joint Gaussian nll of point and neighbours) - (nll of the neighbours), and
the gradient the same two dense terms with dSigma. mpmath takes milliseconds per Bessel value, so the 11175 pair
covariances of each point set are tabulated: tests/golden/matern_general_d<d>_nu<nu>.npz holds c and dc of
_corr(r, nu) over np.triu_indices(150, 1), r the pairwise distances of synthetic.bench_coords(150, d) computed as
np.sqrt(((X[:, None] - X[None]) ** 2).sum(-1)); every use checks a sample of the table against mpmath, and the few
covariances of the prediction test are computed on the spot. cov_pars = [0.5, 1.0, 0.2]: with the nugget every block's
condition number stays below about 200, so the reference is good to about 1e-13."""
import functools
import os

import mpmath as mp
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CP = [0.5, 1.0, 0.2]   # sigma^2, sigma_1^2, rho
N = 150


@functools.lru_cache(maxsize=None)
def _data(d):
    from gpboost_amd import synthetic
    X = synthetic.bench_coords(N, d)
    y = np.random.default_rng(7).standard_normal(N)
    return X, y


def _corr(r, nu):
    """correlation and its derivative wrt log(phi) at the distances r, from mpmath rounded to float64"""
    mp.mp.dps = 30
    phi = mp.sqrt(2 * mp.mpf(nu)) / mp.mpf(CP[2])
    k = mp.power(2, 1 - mp.mpf(nu)) / mp.gamma(nu)
    c, dc = np.ones(r.shape), np.zeros(r.shape)
    for i, j in zip(*np.triu_indices(r.shape[0], 1)):   # symmetric; the diagonal is (1, 0)
        x = phi * mp.mpf(float(r[i, j]))
        c[i, j] = c[j, i] = float(k * x ** nu * mp.besselk(nu, x))
        dc[i, j] = dc[j, i] = float(-k * x ** (nu + 1) * mp.besselk(nu - 1, x))
    return c, dc


@functools.lru_cache(maxsize=None)
def _corr_table(d, nu):
    X, _ = _data(d)
    t = np.load(os.path.join(os.path.dirname(__file__), "golden", f"matern_general_d{d}_nu{nu}.npz"))
    iu = np.triu_indices(N, 1)
    c, dc = np.eye(N), np.zeros((N, N))
    c[iu], dc[iu] = t["c"], t["dc"]
    c, dc = c + np.triu(c, 1).T, dc + dc.T
    pick = np.random.default_rng(11).choice(iu[0].size, 12, replace=False)   # the table is mpmath's: a sample
    for i, j in zip(iu[0][pick], iu[1][pick]):
        cs, ds = _corr(np.array([[0., np.sqrt(((X[i] - X[j]) ** 2).sum())], [0., 0.]]), nu)
        assert (c[i, j], dc[i, j]) == (cs[0, 1], ds[0, 1])
    return c, dc


def _gauss(y, S, dS):
    """nll of N(0, S) at y without the 2 pi term, and its derivative along each dS"""
    if y.size == 0:
        return 0., np.zeros(len(dS))
    u = np.linalg.solve(S, y)
    nll = 0.5 * np.linalg.slogdet(S)[1] + 0.5 * y @ u
    return nll, np.array([0.5 * np.trace(np.linalg.solve(S, D)) - 0.5 * u @ D @ u for D in dS])


@functools.lru_cache(maxsize=None)
def _reference(d, nu, sets):
    """sets: per row the tuple of its neighbours (all rows of the Vecchia order, or of the dense model one set each).
    Returns Dinv, the rows of B (transformed scale), and nll / gradient as functions of sigma2."""
    X, y = _data(d)
    s2, var = CP[0], CP[1] / CP[0]
    n = len(sets)
    c, dc = _corr_table(d, nu)
    Dinv, B = np.zeros(n), []

    def total(sig2):
        nll, g = 0.5 * n * np.log(2 * np.pi), np.zeros(3)
        for i, nb in enumerate(sets):
            ix = np.array(list(nb) + [i], dtype=int)
            S = sig2 * (var * c[np.ix_(ix, ix)] + np.eye(ix.size))
            dS = [S, sig2 * var * c[np.ix_(ix, ix)], sig2 * var * dc[np.ix_(ix, ix)]]
            a, ga = _gauss(y[ix], S, dS)
            k = ix.size - 1
            b, gb = _gauss(y[ix[:k]], S[:k, :k], [D[:k, :k] for D in dS])
            nll += a - b
            g += ga - gb
        return nll, g

    for i, nb in enumerate(sets):
        ix = np.array(nb, dtype=int)
        C = var * c[np.ix_(ix, ix)] + np.eye(ix.size)
        a = np.linalg.solve(C, var * c[ix, i]) if ix.size else np.zeros(0)
        B.append(-a)
        Dinv[i] = 1. / (var + 1. - var * c[ix, i] @ a)
    return Dinv, B, total


def _vecchia(d, m, nu):
    from gpboost_amd import GPModel
    X, y = _data(d)
    gm = GPModel(gp_coords=X, cov_function="matern", cov_fct_shape=nu, gp_approx="vecchia", num_neighbors=m,
                 vecchia_ordering="none")
    perm, nbr = gm.vecchia_structure()
    assert np.array_equal(perm, np.arange(N))
    sets = tuple(tuple(int(j) for j in nbr[i, :min(i, m)]) for i in range(N))
    return gm, y, nbr, sets


CASES = [(2, 1, 1), (2, 15, 1), (2, 16, 1), (2, 17, 1), (2, 30, 1), (2, 30, 0.3), (2, 30, 3.3), (2, 33, 2), (2, 64, 2),
         (2, 65, 1), (2, 80, 1), (1, 30, 1), (3, 30, 1)]


@pytest.mark.parametrize("d,m,nu", CASES)
def test_vecchia_factor_and_likelihood(d, m, nu):
    gm, y, nbr, sets = _vecchia(d, m, nu)
    Dinv_ref, B_ref, total = _reference(d, nu, sets)
    dinv, b = gm.vecchia_factor(CP)
    np.testing.assert_allclose(dinv, Dinv_ref, rtol=1e-9)
    for i in range(N):
        k = min(i, m)
        np.testing.assert_allclose(b[i, :k], B_ref[i], rtol=1e-9, atol=1e-12)
        assert np.all(b[i, k:] == 0.)
    nll_ref, g_ref = total(CP[0])
    nll, g, _ = gm.neg_log_likelihood_and_grad(CP, y, profile_sigma2=False)
    assert abs(nll - nll_ref) <= 1e-9 * abs(nll_ref)
    np.testing.assert_allclose(g, g_ref, rtol=1e-7, atol=1e-7 * np.abs(g_ref).max())
    # profiled: sigma2 = q / n with q the quadratic form at sigma2 = 1, the gradient that of the other two
    s2_ref = (N - 2. * total(1.)[1][0]) / N   # d nll / dlog sigma2 at sigma2 = 1 is (n - q) / 2
    nll_ref, g_ref = total(s2_ref)
    nll, g, s2 = gm.neg_log_likelihood_and_grad(CP, y, profile_sigma2=True)
    assert abs(s2 - s2_ref) <= 1e-9 * s2_ref
    assert abs(nll - nll_ref) <= 1e-9 * abs(nll_ref)
    np.testing.assert_allclose(g, g_ref[1:], rtol=1e-7, atol=1e-7 * np.abs(g_ref).max())


def test_dense_likelihood_and_gradient():
    from gpboost_amd import GPModel
    X, y = _data(2)
    n = 60
    gm = GPModel(gp_coords=X[:n], cov_function="matern", cov_fct_shape=1., gp_approx="none")
    sets = tuple(tuple(range(i)) for i in range(n))   # the chain rule over all earlier points is the joint density
    _, _, total = _reference(2, 1, sets)
    nll_ref, g_ref = total(CP[0])
    nll, g, _ = gm.neg_log_likelihood_and_grad(CP, y[:n], profile_sigma2=False)
    assert abs(nll - nll_ref) <= 1e-9 * abs(nll_ref)
    np.testing.assert_allclose(g, g_ref, rtol=1e-7, atol=1e-7 * np.abs(g_ref).max())


def test_vecchia_prediction_against_dense_conditionals():
    gm, y, _, _ = _vecchia(2, 15, 1)
    X, _ = _data(2)
    Xp = np.random.default_rng(3).uniform(X.min(0), X.max(0), size=(3, 2))
    mp_ = 10
    out = gm.predict(y=y, cov_pars=CP, gp_coords_pred=Xp, predict_var=True, predict_response=True,
                     num_neighbors_pred=mp_)
    s2, var = CP[0], CP[1] / CP[0]
    for p in range(3):
        nb = np.argsort(((X - Xp[p]) ** 2).sum(1), kind="stable")[:mp_]
        pts = np.vstack([X[nb], Xp[p]])
        c, _ = _corr(np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1)), 1)
        a = np.linalg.solve(var * c[:mp_, :mp_] + np.eye(mp_), var * c[:mp_, mp_])
        assert abs(out["mu"][p] - a @ y[nb]) <= 1e-8 * max(1., abs(a @ y[nb]))
        v = s2 * (var + 1. - var * c[:mp_, mp_] @ a)
        assert abs(out["var"][p] - v) <= 1e-8 * v


def test_refused_combination_names_the_shape():
    from gpboost_amd import GPModel
    from gpboost_amd.basic import GPBoostError
    X, _ = _data(2)
    with pytest.raises(GPBoostError, match="cov_fct_shape"):
        GPModel(gp_coords=X, cov_function="matern", cov_fct_shape=1., gp_approx="vecchia", num_neighbors=15,
                likelihood="bernoulli_logit")
