"""GPU: linear regression coefficients (fixed effects) of grouped random effects models under non-Gaussian likelihoods:
GPB_OptimLinRegrCoefCovPar with the coefficients inside the L-BFGS vector [log cov pars, beta, log aux pars]
(optimizer_coef = "lbfgs", optim_utils.h:243-364), GPB_GetCoef, predictions with X_pred and the extension
GPB_EvalNegLogLikelihoodGradCoef.

Identity checks against the covariate-free paths that tests/test_gpu_grouped_laplace.py verifies against the reference:
  nll(cov_pars, coef on X) = nll(cov_pars, fixed_effects = X coef): 1e-12 relative for K == 1 and cholesky, 1e-9 for
  iterative with the same seeds (both find the mode from zero; the offsets differ in the last bit, fma on the device
  against numpy's dot); grad_coef = X^T GPB_CalcGradientF at the same mode: 1e-10 of max |.|;
  predict(X_pred) of a fitted model = predict of a covariate-free model at the same parameters with
  fixed_effects = X coef, fixed_effects_pred = X_pred coef: 1e-12.
Reference fits: tests/golden/golden_grouped_coef.json (make_golden_grouped_coef.py). For such a model the reference
harness prints cov_pars, coef and their standard deviations and then stops, so the generator takes the rest from
further runs of it: the iteration count as the smallest maxit that reproduces the unrestricted fit, the optimizer's
state after every iteration from the fits at maxit = 1 .. num_it, the nll from an evaluation at the fitted parameters
(the mode found from zero). Acceptance is the project's rule for grouped Laplace fits
(tests/test_gpu_grouped_laplace.py::test_fit_matches_reference): identical num_it; cov_pars and nll at rtol 1e-6, coef
at rtol 1e-6 with atol 1e-6 max |coef|, against the reference's 1-thread run (a case is in the fixture only if four
16-thread runs of the reference reproduce that fit to 1e-7). The state after k iterations is held to the same
tolerances, widened to 10 x the distance between the reference's own 1- and 16-thread states at that k where that is
larger. The fitted shape of the gamma case is not printed by the harness and there is no reference nll for it (the
evaluation needs the shape); its initial shape (the reference's rule, with the offset F + X beta_init), its 12
iterations and the five states along them are what pins it.
The nll compared is the one evaluated from a zero mode at the fitted parameters, like the reference's. The fit's own
last value is printed beside it: it is the objective of the line search's accepted trial, whose mode finding starts
from the previous mode and may stop after one Newton step (the reference's rule at the first step: |change of the
objective| < delta_conv_mode_finding |objective|). Measured on an MI355X for k2_probit_noicpt_chol: the fit ends on
1503.3894182, evaluating again from that mode takes two more Newton steps and gives 1503.3672892, from a zero mode
five steps and 1503.3672908 (the reference's own 1503.3672908); the fitted parameters agree with the reference to
2e-13 after the same 17 iterations, so its objective values along the way were the same. The other cases: 1e-10 or
less between the two values. The R test's data adds its own tolerance: sum |error| < 1e-6, and 9 iterations
(test_GPModel_non_Gaussian_data.R:1866-1871).
Standard errors: finite differences of a gradient; the fixture holds the reference's values with 1 and 16 threads and
their relative spread, and 10 x that spread (at least 1e-6) is allowed, the GPU's order of summation being a third one.
They are taken right after the fit, as the reference takes them (its differences start from the fit's last mode).
"""
import ctypes
import json
import os

import numpy as np
import pytest

from gpboost_amd import GPBoostError, GPModel, synthetic
from gpboost_amd.basic import lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
D = ctypes.POINTER(ctypes.c_double)
TIGHT = {"cg_delta_conv": 1e-10, "num_rand_vec_trace": 50, "seed_rand_vec_trace": 1}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "golden_grouped_coef.json")) as f:
        return json.load(f)


def _covariates(n, kind):
    X = synthetic.bench_covariates(n, 2)
    return {"icpt+2": X, "icpt": X[:, :1], "2": X[:, 1:]}[kind].copy()


def _case_data(case):
    n = case["n"]
    g = synthetic.bench_groups(n, tuple(case["levels"]))
    X = _covariates(n, case["covariates"])
    y = synthetic.bench_grouped_coef_y(g, X, case["beta_data"], case["likelihood"])
    assert float(y.sum()) == case["y_sum"]
    fe = 0.5 * (synthetic.lcg_unif(n, 0.77) - 0.5) if case["offset"] else None
    return g, X, y, fe


def _model(g, likelihood, iterative=False, aux=None):
    gm = GPModel(group_data=g, likelihood=likelihood, matrix_inversion_method="iterative" if iterative else "cholesky")
    params = dict(TIGHT) if iterative else {}
    if aux is not None:
        params.update({"init_aux_pars": [aux], "estimate_aux_pars": True})
    if params:
        gm.set_optim_params(params)
    return gm


# ------------------------------------------------------------------------------------------ identities
IDENT = [("k1", 1000, (50,), False), ("k2_chol", 3001, (60, 9), False), ("k2_iter", 3001, (60, 9), True)]


@pytest.mark.parametrize("name,n,levels,iterative", IDENT)
@pytest.mark.parametrize("likelihood", ["bernoulli_logit", "poisson", "gamma"])
@pytest.mark.parametrize("with_F", [False, True])
def test_eval_at_coef_equals_eval_with_offset(name, n, levels, iterative, likelihood, with_F):
    g = synthetic.bench_groups(n, levels)
    X = synthetic.bench_covariates(n, 2)
    beta = np.array([0.3, 0.8, -0.6])
    y = synthetic.bench_grouped_coef_y(g, X, beta, likelihood)
    F = 0.5 * (synthetic.lcg_unif(n, 0.77) - 0.5) if with_F else None
    aux = 1.7 if likelihood == "gamma" else None
    cp = np.array([0.8, 0.3][:len(levels)])
    b = np.array([0.25, 0.7, -0.45])                       # a non-trivial point, not the optimum
    gm = _model(g, likelihood, iterative, aux)
    nll, gcov, gaux, gcoef = gm.neg_log_likelihood_and_grad_coef(cp, b, y, X, offset=F)
    # the verified path: the same linear predictor as an offset, then the gradient wrt F at that mode
    ref = _model(g, likelihood, iterative, aux)
    off = X @ b + (F if F is not None else 0.)
    nll_ref, grad_ref, _ = ref.neg_log_likelihood_and_grad(cp, y, fixed_effects=off)
    gf = ref.calc_gradient_f(fixed_effects=off, calc_cov_factor=False)
    tol = 1e-9 if iterative else 1e-12
    print(name, likelihood, with_F, "nll dev", abs(nll - nll_ref) / abs(nll_ref), "grad_coef dev",
          np.abs(gcoef - X.T @ gf).max() / np.abs(X.T @ gf).max())
    assert abs(nll - nll_ref) <= tol * abs(nll_ref), (nll, nll_ref)
    want = X.T @ gf
    assert np.abs(gcoef - want).max() <= (1e-9 if iterative else 1e-10) * np.abs(want).max()
    full = np.concatenate([gcov, gaux]) if gaux is not None else gcov
    np.testing.assert_allclose(full, grad_ref, rtol=1e-8 if iterative else 1e-10,
                               atol=(1e-8 if iterative else 1e-10) * np.abs(grad_ref).max())
    # equal inputs give equal bits
    nll2, _, _, gcoef2 = gm.neg_log_likelihood_and_grad_coef(cp, b, y, X, offset=F)
    assert nll2 == nll and np.array_equal(gcoef2, gcoef)


def test_grad_coef_is_the_derivative_of_the_nll():
    """central differences of the nll in each coefficient (K == 2, cholesky, Poisson): 1e-6 relative"""
    n, levels = 3001, (60, 9)
    g = synthetic.bench_groups(n, levels)
    X = synthetic.bench_covariates(n, 2)
    y = synthetic.bench_grouped_coef_y(g, X, (0.3, 0.8, -0.6), "poisson")
    gm = _model(g, "poisson")
    cp, b = np.array([0.8, 0.3]), np.array([0.25, 0.7, -0.45])
    _, _, _, gcoef = gm.neg_log_likelihood_and_grad_coef(cp, b, y, X)
    for j in range(3):
        h = 1e-5
        bp, bm = b.copy(), b.copy()
        bp[j] += h
        bm[j] -= h
        fd = (gm.neg_log_likelihood_and_grad_coef(cp, bp, y, X)[0] -
              gm.neg_log_likelihood_and_grad_coef(cp, bm, y, X)[0]) / (2 * h)
        assert fd == pytest.approx(gcoef[j], rel=1e-6, abs=1e-6 * np.abs(gcoef).max())


# ------------------------------------------------------------------------------------------ reference fits
FIT_CASES = ["k1_logit_icpt2", "k1_pois_icpt_only", "k2_probit_noicpt_chol", "k2_gamma_offset_chol",
             "k2_logit_iter_tight"]


@pytest.fixture(scope="module")
def fitted(golden):
    """every reference case fitted once, shared by the tests below"""
    out = {}
    for name in FIT_CASES:
        case = golden[name]
        g, X, y, fe = _case_data(case)
        gm = _model(g, case["likelihood"], case["iterative"] is not None, case["aux"])
        gm.fit(y, X=X, offset=fe)
        # the standard errors right after the fit, as the reference computes them (its differences start from the
        # fit's last mode, which for k2_probit_noicpt_chol is one Newton step short: 4.6e-6 in the standard errors)
        se = gm.get_coef(std_err=True) if case["iterative"] is None else None
        out[name] = (gm, g, X, y, fe, se)
    return out


@pytest.mark.parametrize("name", FIT_CASES)
def test_fit_matches_reference(golden, fitted, name):
    case = golden[name]
    gm, g, X, y, fe, _ = fitted[name]
    np.testing.assert_allclose(gm.get_init_cov_pars(), case["init_cov_pars"], rtol=1e-12)
    coef, ref = gm.get_coef(), np.asarray(case["coef"])
    print(name, "its", gm.get_num_optim_iter(), "cov dev", np.abs(gm.get_cov_pars() / case["cov_pars"] - 1).max(),
          "coef dev", np.abs(coef - ref).max() / np.abs(ref).max())
    assert gm.get_num_optim_iter() == case["num_it"]
    np.testing.assert_allclose(gm.get_cov_pars(), case["cov_pars"], rtol=1e-6)
    np.testing.assert_allclose(coef, ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())
    fit_nll = gm.get_current_neg_log_likelihood()
    # the interface around the fit
    k = ctypes.c_int(0)
    assert lib().GPB_GetNumCoef(gm.handle, ctypes.byref(k)) == 0 and k.value == X.shape[1]
    assert np.array_equal(gm.get_covariate_data(), X)
    assert gm.get_optim_params()["optimizer_coef"] == "lbfgs"
    # after the fit the offset is F + X beta: the nll from a zero mode at the fitted parameters is the reference's
    nll = gm.neg_log_likelihood(gm.get_cov_pars(), y, fixed_effects=fe)
    print(name, "nll from zero", nll, "reference", case.get("nll_at_fit"), "the fit's last value", fit_nll)
    if case["likelihood"] != "gamma":
        assert nll == pytest.approx(case["nll_at_fit"], rel=1e-6)


@pytest.mark.parametrize("name", FIT_CASES + ["rtest_probit"])
def test_optimizer_states_match_reference(golden, name):
    """the parameters after k iterations (maxit = k) against the reference's, k = 1, 2, 3, num_it / 2, num_it - 1"""
    case = golden[name]
    if name == "rtest_probit":
        g, X, y = synthetic.rtest_grouped_probit_coef()
        fe, lik, iterative = None, "bernoulli_probit", False
    else:
        g, X, y, fe = _case_data(case)
        lik, iterative = case["likelihood"], case["iterative"] is not None
    n_it, traj = case["num_it"], case["trajectory"]
    traj16 = case.get("trajectory_16", traj)
    for k in sorted({1, 2, 3, n_it // 2, n_it - 1} & set(range(1, n_it))):
        gm = _model(g, lik, iterative)
        gm.fit(y, X=X, offset=fe, params={"maxit": k})
        ref = np.asarray(traj[k - 1]["cov_pars"] + traj[k - 1]["coef"])
        ref16 = np.asarray(traj16[k - 1]["cov_pars"] + traj16[k - 1]["coef"])
        spread = np.abs(ref - ref16).max() / np.abs(ref).max()      # the reference against itself
        tol = max(1e-6, 10. * spread)
        got = np.concatenate([gm.get_cov_pars(), gm.get_coef()])
        nc = len(traj[k - 1]["cov_pars"])
        print(name, "k", k, "dev", np.abs(got / ref - 1.).max(), "reference spread", spread)
        assert gm.get_num_optim_iter() == k
        np.testing.assert_allclose(got[:nc], ref[:nc], rtol=tol)
        np.testing.assert_allclose(got[nc:], ref[nc:], rtol=tol, atol=tol * np.abs(ref[nc:]).max())


def test_initial_shape_is_found_with_the_initial_linear_predictor():
    """gamma, no init_aux_pars, maxit = 0: the shape is the reference's initial value for the offset F + X beta_init
    (re_model_template.h:1184-1198), i.e. that of a covariate-free model whose offset holds the initial intercept. The
    rule, s = log mean(y e^-F) - mean(log y - F), does not change when a constant joins F, and beta_init is zero but
    for the intercept, so the value also equals the one for F alone (to rounding); what it must not be is the value
    without F."""
    n = 1000
    g = synthetic.bench_groups(n, (50,))
    X = synthetic.bench_covariates(n, 2)
    y = synthetic.bench_grouped_coef_y(g, X, (0.5, 1.0, -0.8), "gamma")
    F = 0.5 * (synthetic.lcg_unif(n, 0.77) - 0.5)
    gm = GPModel(group_data=g, likelihood="gamma")
    gm.fit(y, X=X, offset=F, params={"maxit": 0})
    b = gm.get_coef()
    assert b[0] != 0. and np.all(b[1:] == 0.)              # the initial intercept, every other coefficient 0
    ref = GPModel(group_data=g, likelihood="gamma")
    ref.fit(y, offset=F + b[0], params={"maxit": 0})
    plain, bare = GPModel(group_data=g, likelihood="gamma"), GPModel(group_data=g, likelihood="gamma")
    plain.fit(y, offset=F, params={"maxit": 0})
    bare.fit(y, params={"maxit": 0})
    shape, want = gm.get_aux_pars()[0][0], ref.get_aux_pars()[0][0]
    shift, none = plain.get_aux_pars()[0][0], bare.get_aux_pars()[0][0]
    print("initial shape", shape, want, "offset F alone", shift, "no offset", none)
    assert shape == pytest.approx(want, rel=1e-13) and shape == pytest.approx(shift, rel=1e-13)
    assert abs(none / want - 1.) > 1e-4                    # F itself matters: var(F) = 0.02 enters s


def test_r_test_values(golden):
    """test_GPModel_non_Gaussian_data.R:1864-1871: probit, lbfgs for both, 10 groups of 10"""
    group, X, y = synthetic.rtest_grouped_probit_coef()
    assert float(y.sum()) == golden["rtest_probit"]["y_sum"]
    gm = GPModel(group_data=group, likelihood="bernoulli_probit")
    gm.fit(y, X=X, params={"optimizer_cov": "lbfgs", "optimizer_coef": "lbfgs"})
    cov, coef = gm.get_cov_pars(), gm.get_coef()
    print("rtest", cov, coef, gm.get_num_optim_iter())
    assert np.abs(cov - np.array([0.3996146704])).sum() < 1e-6            # TOLERANCE_STRICT
    assert np.abs(coef - np.array([-0.1109363315, 1.5150072519])).sum() < 1e-6
    assert gm.get_num_optim_iter() == 9
    assert gm.get_num_optim_iter() == golden["rtest_probit"]["num_it"]      # what the maxit sweep of the harness finds
    assert gm.neg_log_likelihood(cov, y) == pytest.approx(golden["rtest_probit"]["nll_at_fit"], rel=1e-6)
    gm.summary()


@pytest.mark.parametrize("name", ["k1_logit_icpt2", "k1_pois_icpt_only", "k2_probit_noicpt_chol",
                                  "k2_gamma_offset_chol"])
def test_coef_standard_errors(golden, fitted, name):
    case = golden[name]
    gm, out = fitted[name][0], fitted[name][5]
    ref, ref16 = np.asarray(case["coef_std_dev"]), np.asarray(case["coef_std_dev_16"])
    tol = max(10. * case["coef_std_dev_spread"], 1e-6)
    dev = np.abs(out[1] / ref - 1.).max()
    print(name, "std err dev", dev, "reference spread (1 vs 16 threads)", case["coef_std_dev_spread"], "allowed", tol)
    np.testing.assert_array_equal(out[0], gm.get_coef())
    assert dev <= tol and np.abs(out[1] / ref16 - 1.).max() <= tol
    # the offset of the fit was put back in place afterwards: the same bits as a fresh evaluation with y and the offset
    y, fe = fitted[name][3], fitted[name][4]
    assert gm.neg_log_likelihood(gm.get_cov_pars(), None) == gm.neg_log_likelihood(gm.get_cov_pars(), y,
                                                                                   fixed_effects=fe)


def test_standard_errors_are_refused_for_iterative(fitted):
    with pytest.raises(GPBoostError, match="iterative"):
        fitted["k2_logit_iter_tight"][0].get_coef(std_err=True)


def test_failed_fit_leaves_no_covariates_behind():
    g, X, y = _small()
    gm = GPModel(group_data=g, likelihood="bernoulli_logit")
    with pytest.raises(GPBoostError):
        gm.fit(y, X=X, params={"optimizer_coef": "wls"})
    assert not gm.has_covariates
    with pytest.raises(GPBoostError, match="does not have covariates"):
        gm.get_coef()
    gm.fit(y, X=X, params={"optimizer_coef": None})        # not sticky: None is the default again
    assert gm.has_covariates and gm.get_optim_params()["optimizer_coef"] == "lbfgs"
    gm.fit(y)                                              # and a fit without covariates drops them
    assert not gm.has_covariates and gm.get_optim_params()["optimizer_coef"] == "wls"


# ------------------------------------------------------------------------------------------ predictions
@pytest.mark.parametrize("name", ["k1_logit_icpt2", "k2_gamma_offset_chol", "k2_probit_noicpt_chol"])
@pytest.mark.parametrize("response", [False, True])
def test_predict_equals_covariate_free_model_with_offsets(golden, fitted, name, response):
    case = golden[name]
    gm, g, X, y, fe, _ = fitted[name]
    npred = 40
    gp = g[:npred].copy()
    gp[::5, 0] = 100000 + np.arange(len(gp[::5]))          # labels not seen in training
    Xp = X[-npred:] * 1.25
    fep = 0.1 * np.arange(npred) / npred if fe is not None else None
    coef = gm.get_coef()
    got = gm.predict(group_data_pred=gp, X_pred=Xp, y=y, offset=fe, offset_pred=fep, predict_var=True,
                     predict_response=response)
    aux = gm.get_aux_pars()[0][0] if case["likelihood"] == "gamma" else None
    ref = _model(g, case["likelihood"], False, aux)
    off = X @ coef + (fe if fe is not None else 0.)
    offp = Xp @ coef + (fep if fep is not None else 0.)
    want = ref.predict(group_data_pred=gp, y=y, cov_pars=gm.get_cov_pars(), offset=off, offset_pred=offp,
                       predict_var=True, predict_response=response)
    print(name, response, "mu dev", np.abs(got["mu"] - want["mu"]).max(), "var dev", np.abs(got["var"] - want["var"]).max())
    np.testing.assert_allclose(got["mu"], want["mu"], rtol=1e-12, atol=1e-12 * np.abs(want["mu"]).max())
    np.testing.assert_allclose(got["var"], want["var"], rtol=1e-12, atol=1e-12 * np.abs(want["var"]).max())
    # saved prediction data gives the same bits
    gm.set_prediction_data(group_data_pred=gp, X_pred=Xp)
    saved = gm.predict(use_saved_data=True, y=y, offset=fe, offset_pred=fep, predict_var=True,
                       predict_response=response)
    assert np.array_equal(saved["mu"], got["mu"]) and np.array_equal(saved["var"], got["var"])


def test_training_random_effects_use_the_linear_predictor(fitted):
    gm, g, X, y, fe, _ = fitted["k1_logit_icpt2"]
    got = gm.predict_training_data_random_effects()
    ref = _model(g, "bernoulli_logit")
    ref.neg_log_likelihood(gm.get_cov_pars(), y, fixed_effects=X @ gm.get_coef())
    want = ref.predict_training_data_random_effects()
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10 * np.abs(want).max())


def test_prediction_data_checks(fitted):
    gm, g, X, y, fe, _ = fitted["k1_logit_icpt2"]
    with pytest.raises(GPBoostError, match="'X_pred' is not provided but the model has covariates"):
        gm.predict(group_data_pred=g[:5], y=y)
    plain = _model(g, "bernoulli_logit")
    plain.fit(y)
    with pytest.raises(GPBoostError, match="'X_pred' is provided but the model has no covariates"):
        plain.predict(group_data_pred=g[:5], X_pred=X[:5], y=y)
    with pytest.raises(GPBoostError, match="'X_pred' is provided but the model has no covariates"):
        plain.set_prediction_data(group_data_pred=g[:5], X_pred=X[:5])


# ------------------------------------------------------------------------------------------ refusals
def _small():
    n = 300
    g = synthetic.bench_groups(n, (20,))
    X = synthetic.bench_covariates(n, 2)
    return g, X, synthetic.bench_grouped_coef_y(g, X, (0.3, 0.8, -0.6), "bernoulli_logit")


@pytest.mark.parametrize("opt", ["gradient_descent", "wls", "nelder_mead"])
def test_other_coefficient_optimizers_are_refused(opt):
    g, X, y = _small()
    gm = GPModel(group_data=g, likelihood="bernoulli_logit")
    with pytest.raises(GPBoostError, match=f"optimizer_coef = '{opt}'"):
        gm.fit(y, X=X, params={"optimizer_coef": opt})


def test_estimate_cov_par_index_with_covariates_is_refused():
    g, X, y = _small()
    gm = GPModel(group_data=g, likelihood="bernoulli_logit")
    with pytest.raises(GPBoostError, match="estimate_cov_par_index"):
        gm.fit(y, X=X, params={"estimate_cov_par_index": [1]})


def test_too_many_covariates_and_bad_values_are_refused():
    g, X, y = _small()
    n = len(y)
    gm = GPModel(group_data=g, likelihood="bernoulli_logit")
    wide = np.column_stack([np.ones(n)] + [synthetic.lcg_unif(n, 0.01 + 0.03 * k) for k in range(31)])
    with pytest.raises(GPBoostError, match="num_covariates = 32"):
        gm.fit(y, X=wide)
    for bad in (np.nan, np.inf):                            # through the C ABI: the Python layer checks X itself
        Xb = X.copy()
        Xb[7, 1] = bad
        xcol = np.ascontiguousarray(Xb.T).reshape(-1)
        ret = lib().GPB_OptimLinRegrCoefCovPar(gm.handle, y.ctypes.data_as(D), xcol.ctypes.data_as(D), ctypes.c_int(3),
                                               None)
        assert ret == -1 and b"NaN or Inf in covariate data 'X'" in lib().LGBM_GetLastError()


def test_gaussian_grouped_model_with_covariates_stays_refused():
    n = 300
    g = synthetic.bench_groups(n, (20,))
    gm = GPModel(group_data=g)
    with pytest.raises(GPBoostError, match="linear regression covariates with grouped random effects are not supported"):
        gm.fit(synthetic.bench_grouped_y(g), X=synthetic.bench_covariates(n, 2))
