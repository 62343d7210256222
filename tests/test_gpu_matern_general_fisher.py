"""Standard errors of Gaussian models with the Matern covariance at a general smoothness: the wave-per-row Fisher row
kernel (vecchia_fisher_rows_bessel.hip, num_neighbors <= 64) and the wide Fisher kernel's general-shape instance
(65 .. 128) through GPB_TestVecchiaFisherRowsMatern against plain float64 rows from the mpmath tables of
test_gpu_matern_general.py, and get_cov_pars(std_err=True) for gp_approx "vecchia" (against the CPU oracle with a
scipy Bessel covariance) and "none" (against the exact Fisher information from the table).

Row tolerances are the tables' own: the block condition numbers stay below about 200 and the reference is good to
about 1e-13, so Bv and Dinv take test_vecchia_factor_and_likelihood's rtol = 1e-9, the derivative rows 1e-9 of the
row's largest entry, and dD_var / dD (cancelling sums of terms of size var) 1e-9 of var."""
import numpy as np
import pytest

from test_gpu_matern_general import CP, N, _corr_table, _data, _vecchia

pytestmark = pytest.mark.gpu

NAMES = ("Bv", "dBv_var", "dBv", "Dinv", "dD_var", "dD")


def _rows_ref(d, nu, nbr, m):
    (c, dc), var = _corr_table(d, nu), CP[1] / CP[0]
    big, small = np.zeros((3, N, m)), np.zeros((3, N))
    for i in range(N):
        k = min(i, m)
        ix = nbr[i, :k]
        C, dC = var * c[np.ix_(ix, ix)], var * dc[np.ix_(ix, ix)]   # dc has a zero diagonal
        np.fill_diagonal(C, var * (1. + 1e-10) + 1.)
        cv, dcv = var * c[ix, i], var * dc[ix, i]
        a = np.linalg.solve(C, cv) if k else np.zeros(0)
        t = dC @ a
        if k:
            big[:, i, :k] = -a, -np.linalg.solve(C, a), -np.linalg.solve(C, dcv - t)
        small[:, i] = 1. / (var + 1. - a @ cv), var - a @ cv - a @ a, -(2. * (dcv @ a) - t @ a)
    return dict(zip(NAMES, [*big, *small]))


@pytest.mark.parametrize("d,m,nu", [(2, 1, 1), (2, 15, 1), (2, 16, 1), (2, 17, 1), (2, 33, 1), (2, 64, 1), (2, 30, 0.3),
                                    (2, 30, 3.3), (1, 30, 1), (3, 30, 1), (2, 65, 1), (2, 80, 1)])
def test_fisher_rows_match_the_tables(d, m, nu):
    """One neighbour, the panel edges 15 / 16 / 17 / 33, the wave kernel's limit 64 and the wide instance (65, 80);
    N = 150 holds rows with k < m and full rows.

    Measured on the MI355X over the twelve cases (largest scaled error per output): DESIGN.md section 3."""
    from gpboost_amd import basic
    _, _, nbr, _ = _vecchia(d, m, nu)
    var, phi = CP[1] / CP[0], np.sqrt(2. * nu) / CP[2]
    got = dict(zip(NAMES, basic.vecchia_fisher_rows(_data(d)[0], nbr, 0, var, phi, shape=nu)))
    ref = _rows_ref(d, nu, nbr, m)
    err = {}
    for q in NAMES[:3]:
        err[q] = float((np.abs(got[q] - ref[q]).max(1) / np.maximum(np.abs(ref[q]).max(1), 1e-300)).max())
        assert all(np.all(got[q][i, i:] == 0.) for i in range(min(m, N))), q
    for q in ("dD_var", "dD"):
        err[q] = float(np.abs(got[q] - ref[q]).max() / var)
    err["Dinv"] = float(np.abs(got["Dinv"] / ref["Dinv"] - 1.).max())
    print((d, m, nu), err)
    np.testing.assert_allclose(got["Dinv"], ref["Dinv"], rtol=1e-9)
    np.testing.assert_allclose(got["Bv"], ref["Bv"], rtol=1e-9, atol=1e-12)
    for q in ("dBv_var", "dBv", "dD_var", "dD"):
        assert err[q] <= 1e-9, (q, err[q])


def _matern_kv(nu):
    """oracle.fitc_laplace_oracle.cov_dcov's signature for the Matern covariance of smoothness nu, with phi = 1 / rho
    (cov_type 0 of O.transform): x = sqrt(2 nu) phi r; (var, 0) at r = 0, where x^nu K_nu(x) is indeterminate"""
    from scipy.special import gamma, kv

    def cov_dcov(r, var, phi, cov_type):
        x = np.sqrt(2. * nu) * phi * np.asarray(r, float)
        xs = np.where(x > 0., x, 1.)
        k = var * 2. ** (1. - nu) / gamma(nu)
        c, dc = k * xs ** nu * kv(nu, xs), -k * xs ** (nu + 1.) * kv(nu - 1., xs)
        return np.where(x > 0., c, var), np.where(x > 0., dc, 0.)
    return cov_dcov


@pytest.mark.parametrize("m", [15, 65])
def test_vecchia_std_err_matches_oracle(m, monkeypatch):
    """the setup of test_wide_std_err_matches_oracle at nu = 1; the oracle runs with cov_type 0 (phi = 1 / rho,
    dlog phi / drho = -1 / rho) and the Bessel covariance in place of its closed forms"""
    from gpboost_amd import GPModel, synthetic
    from oracle import oracle as O
    from oracle import vecchia_fisher_oracle as VF
    n, cp = 300, [0.2, 1.1, 0.12]
    X = synthetic.bench_coords(n)
    y = synthetic.bench_spatial_gaussian_y(X)
    gm = GPModel(gp_coords=X, cov_function="matern", cov_fct_shape=1., gp_approx="vecchia", num_neighbors=m, seed=5)
    assert gm.can_calculate_standard_errors_cov_pars()
    gm.set_optim_params({"num_rand_vec_trace": 16, "seed_rand_vec_trace": 3})
    gm.neg_log_likelihood(cp, y)
    sd = gm.get_cov_pars(std_err=True)[1]
    monkeypatch.setattr(VF, "cov_dcov", _matern_kv(1.))
    _, xv, nb = O.vecchia_setup(X, m, 5, True)
    _, ref = VF.vecchia_fisher(xv, nb, 0, cp, t=16, seed=3)
    np.testing.assert_allclose(sd, ref, rtol=1e-8)


def test_dense_std_err_matches_exact_fisher_information():
    """FI_kl = tr(Sigma^-1 dSigma_k Sigma^-1 dSigma_l) / 2 on the original scale with the error variance (the formula
    in StdDevCovPars): dSigma = I, the correlation, sigma1^2 dcorr / dlog phi dlog phi / drho"""
    from gpboost_amd import GPModel
    n = 60
    X, y = _data(2)
    c, dc = (t[:n, :n] for t in _corr_table(2, 1))
    gm = GPModel(gp_coords=X[:n], cov_function="matern", cov_fct_shape=1., gp_approx="none")
    gm.neg_log_likelihood(CP, y[:n])
    sd = gm.get_cov_pars(std_err=True)[1]
    Si = np.linalg.inv(CP[0] * np.eye(n) + CP[1] * c)
    G = [Si @ D for D in (np.eye(n), c, CP[1] * dc * (-1. / CP[2]))]
    FI = np.array([[0.5 * np.trace(Gk @ Gl) for Gl in G] for Gk in G])
    np.testing.assert_allclose(sd, np.sqrt(np.diag(np.linalg.inv(FI))), rtol=1e-8)


def test_limits():
    from gpboost_amd import GPBoostError, GPModel, basic, synthetic
    from oracle import oracle as O
    _, xv, nb = O.vecchia_setup(synthetic.bench_coords(131), 129, 0, True)
    with pytest.raises(GPBoostError, match=r"num_neighbors = 129 > 128"):
        basic.vecchia_fisher_rows(xv, nb, 0, 1.2, 10., shape=1.)
    with pytest.raises(GPBoostError, match="cov_fct_shape"):
        gm = GPModel(gp_coords=_data(2)[0], cov_function="matern", cov_fct_shape=1., gp_approx="fitc")
        gm.get_cov_pars(std_err=True)
