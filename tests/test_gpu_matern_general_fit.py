"""Estimation with the general-shape Matern covariance: fit (initial range, the range transform's round trip, the
L-BFGS run) and the GLS coefficients of models with covariates, whose Gram matrices take their own way to the row
kernels (Vecchia, both kernels) and to the dense factorization."""
import numpy as np
import pytest

from test_gpu_matern_general import N, _data
from test_gpu_matern_general_ops import _device

pytestmark = pytest.mark.gpu


def _model(approx, n, nu=1., m=15, cov="matern"):
    from gpboost_amd import GPModel
    kw = dict(num_neighbors=m, vecchia_ordering="none") if approx == "vecchia" else {}
    return GPModel(gp_coords=_data(2)[0][:n], cov_function=cov, cov_fct_shape=nu, gp_approx=approx, **kw)


def test_fit_reaches_a_stationary_point():
    """nu = 1, n = 150, m = 15. The optimizer stops when an iteration lowers the nll by Delta <= delta max(|nll|, 1),
    delta = delta_rel_conv = 1e-6 (its gradient threshold, 1e-20, never acts). Near the minimum Delta = g' H^-1 g / 2
    >= |g|^2 / (2 lmax), so that setting bounds the profiled gradient by sqrt(2 lmax delta max(|nll|, 1)); lmax, the
    Hessian's largest eigenvalue in (log var, log phi), comes from central differences of the gradient."""
    y = _data(2)[1]
    gm = _model("vecchia", N).fit(y)
    assert gm.get_num_optim_iter() < 1000
    init, cp = gm.get_init_cov_pars(), gm.get_cov_pars()
    nll = gm.neg_log_likelihood(cp, y)
    assert nll <= gm.neg_log_likelihood(init, y)

    def grad(dv, dp):   # at (log var + dv, log phi + dp); phi = sqrt(2 nu) / rho
        return gm.neg_log_likelihood_and_grad([cp[0], cp[1] * np.exp(dv), cp[2] * np.exp(-dp)], y, True)[1]
    h = 1e-4
    H = np.column_stack([(grad(h, 0.) - grad(-h, 0.)) / (2 * h), (grad(0., h) - grad(0., -h)) / (2 * h)])
    lmax = np.linalg.eigvalsh(0.5 * (H + H.T)).max()
    g = np.linalg.norm(grad(0., 0.))
    print("gradient norm", g, "bound", np.sqrt(2 * lmax * 1e-6 * max(abs(nll), 1.)), "lmax", lmax)
    assert g <= np.sqrt(2 * lmax * 1e-6 * max(abs(nll), 1.))


@pytest.mark.parametrize("nu,c", [(0.3, 3.), (1., 3.), (2., 4.7), (3.3, 5.9)])
def test_initial_range(nu, c):
    """FindInitCovPar: phi = 2 c / med with c = 3, 4.7, 5.9 for nu <= 1, <= 2, above, and rho = sqrt(2 nu) / phi;
    the exponential model on the same points has rho = med / 6."""
    y = _data(2)[1]
    rho_exp = _model("vecchia", N, 0.5, cov="exponential").fit(y, params={"maxit": 1}).get_init_cov_pars()[2]
    rho = _model("vecchia", N, nu).fit(y, params={"maxit": 1}).get_init_cov_pars()[2]
    assert abs(rho - np.sqrt(2 * nu) * 6. * rho_exp / (2. * c)) <= 1e-12 * rho


@pytest.mark.parametrize("approx,m", [("vecchia", 15), ("vecchia", 65), ("none", 0)])
def test_gls_coefficients(approx, m):
    """beta = (Z' P Z)^-1 Z' P y at the fitted parameters: P = B' D^-1 B from the model's factor rows (Vecchia), or
    (var corr + I)^-1 with GPB_TestMaternGeneral's correlations (dense); both are checked against mpmath elsewhere."""
    n = 60 if approx == "none" else N
    X, y = _data(2)[0][:n], _data(2)[1][:n]
    Z = np.column_stack([np.ones(n), X[:, 0]])
    gm = _model(approx, n, 1., m).fit(y, X=Z)
    cp = gm.get_cov_pars()
    if approx == "vecchia":
        dinv, b = gm.vecchia_factor(cp)
        nbr = gm.vecchia_structure()[1]
        B = np.eye(n)
        for i in range(n):
            B[i, nbr[i, :min(i, m)]] = b[i, :min(i, m)]
        P = B.T @ (dinv[:, None] * B)
    else:
        r = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
        c = _device(1., (np.sqrt(2.) / cp[2] * r).ravel())[0].reshape(n, n)
        P = np.linalg.inv(cp[1] / cp[0] * c + np.eye(n))
    np.testing.assert_allclose(gm.get_coef(), np.linalg.solve(Z.T @ P @ Z, Z.T @ P @ y), rtol=1e-8)
