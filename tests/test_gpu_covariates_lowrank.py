"""GPU parity for linear regression covariates under the two low-rank approximations, gp_approx = "fitc" and
"full_scale_vecchia" (Gaussian likelihood, cholesky).

Reference: GPB_OptimLinRegrCoefCovPar -> OptimLinRegrCoefCovPar with optimizer_coef "wls" (re_model_template.h:
846-1700; ProfileOutCoef :2427-2445; UpdateCoefGLS :9125-9132) with X^T Psi^-1 X by the Woodbury forms of
CalcXTPsiInvX (:6078-6117), GPB_GetCoef (CalcStdDevCoef :9797-9814). Fixtures: tests/golden/golden_cov_lowrank.json
(make_golden_cov_lowrank.py, the reference itself).

Tolerances are those of test_gpu_covariates.py / test_gpu_fitc.py / test_gpu_vif.py: the objective matches the
reference to ~1e-12, so fits reproduce the iteration count, the initial values at 1e-12, the estimates at 1e-6,
the likelihood at 1e-9 and the standard deviations at 1e-5 (relative). The GLS test builds Psi densely in
numpy from the oracle's restatements (oracle.fitc_laplace_oracle's covariance, oracle/vif_oracle.py's factor)
and solves the normal equations by Cholesky; nothing of this implementation enters that side but the
parameters at which it is evaluated.
"""
import json
import os

import numpy as np
import pytest

from gpboost_amd import GPBoostError, GPModel, synthetic

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "golden_cov_lowrank.json")) as _f:
    GOLDEN = json.load(_f)
CASES = ["fitc_fit_X", "fitc_fit_X_matern15", "vif_fit_X", "vif_fit_X_gaussian"]


def _model(sp, X):
    args = dict(gp_coords=X, cov_function=sp["cov_fct"], cov_fct_shape=float(sp.get("shape", 0.5)),
                gp_approx=sp["gp_approx"], num_ind_points=int(sp["num_ind_points"]),
                ind_points_selection=sp.get("ind_points_selection", "kmeans++"), seed=0)
    if sp["gp_approx"] == "full_scale_vecchia":
        args.update(num_neighbors=int(sp["num_neighbors"]), vecchia_ordering=sp["ordering"])
    return GPModel(**args)


def _data(n, extra=0):
    Xall = synthetic.bench_coords(n + extra)
    Xc_all = synthetic.bench_covariates(n + extra, 2)
    X, Xc = Xall[:n], Xc_all[:n]
    y = synthetic.bench_gaussian_y_cov(X, Xc)
    return (X, Xc, y) if extra == 0 else (X, Xc, y, Xall[n:], Xc_all[n:])


_FITS = {}


def _fit(name):
    """The default fit of a golden case, computed once and left unchanged: (model, X, Xc, y)"""
    if name not in _FITS:
        case = GOLDEN[name]
        X, Xc, y = _data(case["n"])
        gm = _model(case["spec"], X)
        gm.fit(y, X=Xc)
        _FITS[name] = (gm, X, Xc, y)
    return _FITS[name]


@pytest.mark.parametrize("name", CASES)
def test_fit_with_covariates_matches_reference(name):
    case = GOLDEN[name]
    gm, X, Xc, y = _fit(name)
    print(name, "num_it", gm.get_num_optim_iter(), case["num_it"], "cov_pars", gm.get_cov_pars(), case["cov_pars"],
          "coef", gm.get_coef(), case["coef"], "nll", gm.get_current_neg_log_likelihood(), case["nll"],
          "sd", gm.get_coef(std_err=True)[1], case["coef_std_dev"])
    assert gm.get_num_optim_iter() == case["num_it"]
    np.testing.assert_allclose(gm.get_init_cov_pars(), case["init_cov_pars"], rtol=1e-12)
    np.testing.assert_allclose(gm.get_cov_pars(), case["cov_pars"], rtol=1e-6)
    np.testing.assert_allclose(gm.get_coef(), case["coef"], rtol=1e-6)
    assert abs(gm.get_current_neg_log_likelihood() - case["nll"]) <= 1e-9 * abs(case["nll"])
    ce = gm.get_coef(std_err=True)
    np.testing.assert_allclose(ce[0], case["coef"], rtol=1e-6)
    np.testing.assert_allclose(ce[1], case["coef_std_dev"], rtol=1e-5)
    np.testing.assert_array_equal(gm.get_response_data(), y)
    np.testing.assert_array_equal(gm.get_covariate_data(), Xc)
    assert gm.get_optim_params()["optimizer_coef"] == "wls"


def test_fitc_cov_pars_std_err_with_covariates():
    """get_cov_pars(std_err=True) of a FITC model fitted with covariates: the Fisher information does not depend on
    the response, so it equals that of a model without covariates at the same parameters."""
    gm, X, Xc, y = _fit("fitc_fit_X")
    cp = gm.get_cov_pars()
    sd = gm.get_cov_pars(std_err=True)
    np.testing.assert_array_equal(sd[0], cp)
    assert np.all(np.isfinite(sd[1])) and np.all(sd[1] > 0.)
    fresh = _model(GOLDEN["fitc_fit_X"]["spec"], X)
    fresh.neg_log_likelihood(cp, y)   # sets the parameters
    np.testing.assert_allclose(sd[1], fresh.get_cov_pars(std_err=True)[1], rtol=1e-12)


def _dense_psi(name, X, cov_pars, Z):
    """Psi on the transformed scale (nugget 1) in the model's row order, and that order, from the oracle"""
    from oracle import oracle as O
    from oracle.fitc_laplace_oracle import JITTER, _dist, cov_dcov
    from oracle.vif_oracle import vif_factor
    from scipy.linalg import cho_factor, cho_solve
    sp = GOLDEN[name]["spec"]
    ct = O.cov_code(sp["cov_fct"], float(sp.get("shape", 0.5)))
    _, var, phi = O.transform(ct, cov_pars)
    n, m = X.shape[0], Z.shape[0]
    if sp["gp_approx"] == "fitc":
        oz, _ = O.fitc_inducing_points(X, m, "kmeans++", 0)
        assert np.array_equal(Z, oz)
        K, _ = cov_dcov(_dist(X, Z), var, phi, ct)
        Ks, _ = cov_dcov(_dist(Z, Z), var, phi, ct)
        np.fill_diagonal(Ks, var * JITTER)
        low = K @ cho_solve(cho_factor(Ks, lower=True), K.T)
        d = 1. + var * JITTER - np.diag(low)   # fitc_resid_diag_ (re_model_template.h:7358-7377)
        return low + np.diag(d), np.arange(n)
    perm, oz, _ = O.vif_inducing_points(X, m, "kmeans++", 0, True)
    assert np.array_equal(Z, oz)
    xv = X[perm]
    nb = O.find_neighbors(xv, int(sp["num_neighbors"]))
    f = vif_factor(xv, nb, Z, ct, var, phi)
    Bi = np.linalg.inv(f["B"])
    return f["K"] @ cho_solve(f["cKs"], f["K"].T) + Bi @ np.diag(f["D"]) @ Bi.T, perm


@pytest.mark.parametrize("name", ["fitc_fit_X", "vif_fit_X"])
def test_coefficients_are_generalized_least_squares(name):
    from scipy.linalg import cho_factor, cho_solve
    gm, X, Xc, y = _fit(name)
    Psi, perm = _dense_psi(name, X, gm.get_cov_pars(), gm.inducing_points())
    cP = cho_factor(Psi, lower=True)
    Xv, yv = Xc[perm], y[perm]
    PiX = cho_solve(cP, Xv)
    beta = cho_solve(cho_factor(Xv.T @ PiX, lower=True), PiX.T @ yv)
    print(name, "GLS", beta, "model", gm.get_coef())
    np.testing.assert_allclose(gm.get_coef(), beta, rtol=1e-6)


@pytest.mark.parametrize("name", ["fitc_fit_X", "vif_fit_X"])
def test_predict_with_covariates_is_gp_on_residuals_plus_linear_predictor(name):
    case = GOLDEN[name]
    n, npred = case["n"], 150
    X, Xc, y, Xp, Xcp = _data(n, npred)
    gm = _model(case["spec"], X)
    gm.fit(y, X=Xc)
    beta = gm.get_coef()
    cp = gm.get_cov_pars()
    pr = gm.predict(gp_coords_pred=Xp, X_pred=Xcp, predict_var=True)
    g0 = _model(case["spec"], X)
    p0 = g0.predict(y=y - Xc @ beta, gp_coords_pred=Xp, cov_pars=cp, predict_var=True)
    np.testing.assert_allclose(pr["mu"], p0["mu"] + Xcp @ beta, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(pr["var"], p0["var"], rtol=1e-12)
    with pytest.raises(GPBoostError, match="X_pred"):
        gm.predict(gp_coords_pred=Xp)
    # the same prediction from data saved in the model (set_prediction_data with X_pred)
    gm.set_prediction_data(gp_coords_pred=Xp, X_pred=Xcp)
    ps = gm.predict(use_saved_data=True, predict_var=True)
    np.testing.assert_array_equal(ps["mu"], pr["mu"])
    np.testing.assert_array_equal(ps["var"], pr["var"])


@pytest.mark.parametrize("name", ["fitc_fit_X", "vif_fit_X"])
def test_fits_are_deterministic_and_no_factorization_goes_stale(name):
    case = GOLDEN[name]
    a, X, Xc, y = _fit(name)
    b = _model(case["spec"], X)
    b.fit(y, X=Xc)
    assert np.array_equal(a.get_cov_pars(), b.get_cov_pars())
    assert np.array_equal(a.get_coef(), b.get_coef())
    assert a.get_current_neg_log_likelihood() == b.get_current_neg_log_likelihood()
    # the model fitted with covariates, refitted without: an evaluation on it is the fresh model's, bit for bit
    cp = b.get_cov_pars()
    b.fit(y)
    fresh = _model(case["spec"], X)
    assert b.neg_log_likelihood(cp, y) == fresh.neg_log_likelihood(cp, y)
    cp2 = b.get_cov_pars()
    assert b.neg_log_likelihood(cp2, y) == fresh.neg_log_likelihood(cp2, y)


def test_gradient_descent_with_covariates_fitc():
    case = GOLDEN["fitc_fit_X"]
    X, Xc, y = _data(case["n"])
    gm = _model(case["spec"], X)
    maxit = 1000   # the default
    gm.fit(y, X=Xc, params={"optimizer_cov": "gradient_descent", "maxit": maxit})
    it = gm.get_num_optim_iter()
    nll = gm.get_current_neg_log_likelihood()
    beta, cp = gm.get_coef(), gm.get_cov_pars()
    print("gradient_descent: iterations", it, "nll", nll, "cov_pars", cp, "coef", beta)
    assert 0 < it < maxit
    g0 = _model(case["spec"], X)
    ref = g0.neg_log_likelihood(cp, y - Xc @ beta)
    assert abs(nll - ref) <= 1e-9 * abs(ref), (nll, ref)
