"""GPU parity for grouped (crossed) random effects under the negative binomial likelihood (Laplace approximation, the
shape r as estimated auxiliary parameter) against the reference itself.

Reference path: GPB_CreateREModel with re_group_data and likelihood = "negative_binomial" -> the mode finding, gradient
and prediction functions tests/test_gpu_grouped_laplace.py names, with the likelihood's own pieces: log-likelihood
likelihoods.h:8750 and normalising constant :8448-8463, derivatives :10241, shape derivatives :10872-10885, explicit
shape gradient :10527-10538, initial shape :1087-1156, response moments :7585-7594. Fixtures:
tests/golden/golden_grouped_negbin.json (make_golden_grouped_negbin.py runs oracle/_ref/ref_harness_grouped;
tests/test_grouped_negbin_fixtures.py re-derives every Cholesky nll in numpy).

Tolerances are the project's existing bounds for this driver (tests/test_gpu_grouped_laplace.py,
tests/test_gpu_grouped_coef.py), none new: Cholesky nll 1e-9 relative, gradient (the shape entry, its last, included)
1e-7 relative with atol 1e-7 max|ref|, gradient wrt F 1e-7 max(1, max|ref|); iterative 1e-6 on both; fits: initial
covariance parameters 1e-12, equal iteration counts, parameters and fitted shape 1e-6, nll 1e-9; coefficients and
optimizer states as tests/test_gpu_grouped_coef.py; predictions 1e-6 max|ref|; training-data random effects 1e-9
max|ref|.
"""
import json
import os

import numpy as np
import pytest

from gpboost_amd import GPBoostError, GPModel, synthetic

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NB = "negative_binomial"
EVAL_CASES = ["k1_nb_aux", "k2_nb_aux_chol", "k3_nb_aux_chol", "k2_nb_offset_chol"]
ITER_CASES = ["k2_nb_aux_iter", "k2_nb_default_iter"]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "golden_grouped_negbin.json")) as f:
        return json.load(f)


def _data(case):
    g = synthetic.bench_groups(case["n"], tuple(case["levels"]))
    y = synthetic.bench_grouped_negbin_y(g)
    assert float(y.sum()) == case["y_sum"]
    fe = 0.5 * (synthetic.lcg_unif(case["n"], 0.77) - 0.5) if case["offset"] else None
    return g, y, fe


def _model(case, g, likelihood=NB):
    it = case.get("iterative")
    gm = GPModel(group_data=g, likelihood=likelihood, matrix_inversion_method="iterative" if it else "cholesky")
    params = {}
    if it:
        params = {"cg_delta_conv": float(it["cg_delta_conv"]), "num_rand_vec_trace": int(it["num_rand_vec_trace"]),
                  "seed_rand_vec_trace": int(it.get("seed_rand_vec_trace", 1))}
    if case["aux"] is not None:
        params.update({"init_aux_pars": [case["aux"]], "estimate_aux_pars": True})
    if params:
        gm.set_optim_params(params)
    return gm


@pytest.mark.parametrize("name", EVAL_CASES)
def test_nll_and_grad_match_reference(golden, name):
    case = golden[name]
    g, y, fe = _data(case)
    gm = _model(case, g)
    K = len(case["levels"])
    assert gm.num_cov_pars == K and gm.num_aux_pars == 1
    cp = np.array(case["cov_pars"])
    nll = gm.neg_log_likelihood(cp, y, fixed_effects=fe)
    nll2, grad, _ = gm.neg_log_likelihood_and_grad(cp, y, fixed_effects=fe)
    ref = np.asarray(case["grad"])   # the shape gradient is its last entry
    print(name, "nll dev", abs(nll - case["nll"]) / abs(case["nll"]), "grad dev", np.abs(grad - ref).max() / np.abs(ref).max(),
          "shape entry", grad[-1], ref[-1])
    assert abs(nll - case["nll"]) <= 1e-9 * abs(case["nll"]), (nll, case["nll"])
    assert nll2 == nll   # both start the mode finding from zero
    assert grad.shape == ref.shape == (K + 1,)
    np.testing.assert_allclose(grad, ref, rtol=1e-7, atol=1e-7 * np.abs(ref).max())
    nll3, grad3, _ = gm.neg_log_likelihood_and_grad(cp, y, fixed_effects=fe)   # equal inputs give equal bits
    assert nll3 == nll2
    np.testing.assert_array_equal(grad3, grad)
    if "grad_f" in case:
        gf = gm.calc_gradient_f(fixed_effects=fe, calc_cov_factor=False)
        rf = np.asarray(case["grad_f"])
        print(name, "grad_f dev", np.abs(gf - rf).max())
        assert np.abs(gf - rf).max() <= 1e-7 * max(1., np.abs(rf).max())


@pytest.mark.parametrize("name", ITER_CASES)
def test_iterative_nll_and_grad_match_reference(golden, name):
    case = golden[name]
    g, y, fe = _data(case)
    gm = _model(case, g)
    cp = np.array(case["cov_pars"])
    nll, grad, _ = gm.neg_log_likelihood_and_grad(cp, y, fixed_effects=fe)
    ref = np.asarray(case["grad"])
    print(name, "nll dev", abs(nll - case["nll"]) / abs(case["nll"]), "grad dev", np.abs(grad - ref).max() / np.abs(ref).max(),
          "shape entry", grad[-1], ref[-1])
    assert abs(nll - case["nll"]) <= 1e-6 * abs(case["nll"]), (nll, case["nll"])
    assert grad.shape == ref.shape
    np.testing.assert_allclose(grad, ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())
    nll3, grad3, _ = gm.neg_log_likelihood_and_grad(cp, y, fixed_effects=fe)   # equal inputs give equal bits
    assert nll3 == nll
    np.testing.assert_array_equal(grad3, grad)


@pytest.mark.parametrize("name", ["fit_k1_nb", "fit_k2_nb_chol", "fit_k2_nb_init"])
def test_fit_matches_reference(golden, name):
    """fit_k1_nb / fit_k2_nb_chol: the shape starts from the method-of-moments rule; fit_k2_nb_init: from 2"""
    case = golden[name]
    g, y, fe = _data(case)
    gm = _model(case, g)
    gm.fit(y, offset=fe)
    aux, aux_name = gm.get_aux_pars()
    print(name, "its", gm.get_num_optim_iter(), case["num_it"], "cov", gm.get_cov_pars(), case["cov_pars"], "shape", aux,
          case["aux_fit"], "nll", gm.get_current_neg_log_likelihood(), case["nll"])
    np.testing.assert_allclose(gm.get_init_cov_pars(), case["init_cov_pars"], rtol=1e-12)
    assert gm.get_num_optim_iter() == case["num_it"]
    np.testing.assert_allclose(gm.get_cov_pars(), case["cov_pars"], rtol=1e-6)
    assert abs(gm.get_current_neg_log_likelihood() - case["nll"]) <= 1e-9 * abs(case["nll"])
    assert aux_name == "shape"
    np.testing.assert_allclose(aux, case["aux_fit"], rtol=1e-6)


def _coef_data(case):
    g = synthetic.bench_groups(case["n"], tuple(case["levels"]))
    X = synthetic.bench_covariates(case["n"], 2)
    y = synthetic.bench_grouped_coef_y(g, X, case["beta_data"], NB, shape=case["data_shape"])
    assert float(y.sum()) == case["y_sum"]
    return g, X, y


def test_fit_with_covariates_matches_reference(golden):
    """num_it: with covariates the reference's harness stops before it prints its iteration count, and the fixture
    holds the count its maxit sweep defines: the smallest maxit whose fit equals the unrestricted one. The same
    definition is applied to this side. It is the optimizer's own count except where the last iteration's line search
    finds no decrease: L-BFGS then puts the parameters back, counts the iteration and stops on a zero change of the
    objective (LineSearchBacktracking.h:130-137, LBFGS.h:214-221), which no sweep can see. That is the end of this
    fit here: 11 iterations counted, 10 by the definition, the fixture's number."""
    case = golden["k2_nb_icpt2_chol"]
    g, X, y = _coef_data(case)
    gm = GPModel(group_data=g, likelihood=NB, matrix_inversion_method="cholesky")
    gm.fit(y, X=X)
    coef, ref = gm.get_coef(), np.asarray(case["coef"])
    print("its", gm.get_num_optim_iter(), "cov dev", np.abs(gm.get_cov_pars() / case["cov_pars"] - 1).max(),
          "coef dev", np.abs(coef - ref).max() / np.abs(ref).max(), "shape", gm.get_aux_pars())
    np.testing.assert_allclose(gm.get_init_cov_pars(), case["init_cov_pars"], rtol=1e-12)
    full = np.concatenate([gm.get_cov_pars(), coef])
    state = {}
    for k in (case["num_it"] - 1, case["num_it"]):
        gk = GPModel(group_data=g, likelihood=NB, matrix_inversion_method="cholesky")
        gk.fit(y, X=X, params={"maxit": k})
        assert gk.get_num_optim_iter() == k
        state[k] = np.concatenate([gk.get_cov_pars(), gk.get_coef()])
    assert np.array_equal(state[case["num_it"]], full) and not np.array_equal(state[case["num_it"] - 1], full)
    assert gm.get_num_optim_iter() in (case["num_it"], case["num_it"] + 1)   # + 1: a last iteration without a step
    np.testing.assert_allclose(gm.get_cov_pars(), case["cov_pars"], rtol=1e-6)
    np.testing.assert_allclose(coef, ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())
    assert gm.get_aux_pars()[1] == "shape"
    se = gm.get_coef(std_err=True)[1]
    rs = np.asarray(case["coef_std_dev"])
    np.testing.assert_allclose(se, rs, rtol=max(1e-6, 10. * case["coef_std_dev_spread"]))


def test_optimizer_states_with_covariates_match_reference(golden):
    """the parameters after k iterations (maxit = k), k = 1, 2, 3, num_it / 2, num_it - 1: the fitted shape is never
    printed by the reference's harness, and these states pin it (it sits in the same L-BFGS vector)"""
    case = golden["k2_nb_icpt2_chol"]
    g, X, y = _coef_data(case)
    n_it, traj, traj16 = case["num_it"], case["trajectory"], case["trajectory_16"]
    for k in sorted({1, 2, 3, n_it // 2, n_it - 1} & set(range(1, n_it))):
        gm = GPModel(group_data=g, likelihood=NB, matrix_inversion_method="cholesky")
        gm.fit(y, X=X, params={"maxit": k})
        ref = np.asarray(traj[k - 1]["cov_pars"] + traj[k - 1]["coef"])
        ref16 = np.asarray(traj16[k - 1]["cov_pars"] + traj16[k - 1]["coef"])
        spread = np.abs(ref - ref16).max() / np.abs(ref).max()
        tol = max(1e-6, 10. * spread)
        got = np.concatenate([gm.get_cov_pars(), gm.get_coef()])
        nc = len(traj[k - 1]["cov_pars"])
        print("k", k, "dev", np.abs(got / ref - 1.).max(), "reference spread", spread)
        assert gm.get_num_optim_iter() == k
        np.testing.assert_allclose(got[:nc], ref[:nc], rtol=tol)
        np.testing.assert_allclose(got[nc:], ref[nc:], rtol=tol, atol=tol * np.abs(ref[nc:]).max())


@pytest.mark.parametrize("name", ["pred_k1_nb_resp", "pred_k2_nb_chol_resp"])
def test_predictions_match_reference(golden, name):
    case = golden[name]
    g, y, _ = _data(case)
    gm = _model(case, g)
    labels = np.asarray(case["labels"])
    seen = np.array([[labels[i, k] in set(g[:, k]) for k in range(g.shape[1])] for i in range(labels.shape[0])])
    assert seen.all(axis=1).any() and (~seen).all(axis=1).any()   # seen and unseen labels
    assert g.shape[1] == 1 or (seen.any(axis=1) & ~seen.all(axis=1)).any()   # and rows mixing both
    p = gm.predict(y=y, cov_pars=case["cov_pars"], group_data_pred=labels, predict_var=True, predict_response=True)
    rm, rv = np.asarray(case["mean"]), np.asarray(case["var"])
    print(name, "mean dev", np.abs(p["mu"] - rm).max(), "var dev", np.abs(p["var"] - rv).max())
    assert np.abs(p["mu"] - rm).max() <= 1e-6 * np.abs(rm).max()
    assert np.abs(p["var"] - rv).max() <= 1e-6 * np.abs(rv).max()


def test_training_data_random_effects_match_reference(golden):
    case = golden["pred_train_k2_nb_chol"]
    g, y, _ = _data(case)
    gm = _model(case, g)
    gm.neg_log_likelihood(case["cov_pars"], y)
    out = gm.predict_training_data_random_effects()
    assert out.shape == (case["n"], len(case["levels"]))
    for k, ref in enumerate(case["level_means"]):
        _, first = np.unique(g[:, k], return_index=True)
        ref = np.asarray(ref)
        assert np.abs(out[np.sort(first), k] - ref).max() <= 1e-9 * np.abs(ref).max()


@pytest.mark.parametrize("alias", ["nbinom2", "negative_binomial_2", "negative_binomial2"])
def test_aliases_build_the_same_model(golden, alias):
    case = golden["k2_nb_aux_chol"]
    g, y, _ = _data(case)
    a = _model(case, g).neg_log_likelihood_and_grad(case["cov_pars"], y)
    b = _model(case, g, likelihood=alias).neg_log_likelihood_and_grad(case["cov_pars"], y)
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[1], b[1])


def test_large_shape_is_the_poisson_model(golden):
    """shape 1e7: the nll equals the Poisson model's to 1e-6 relative. The negative binomial density tends to the
    Poisson density as r grows: log p_nb - log p_pois = -((y - mu)^2 - y) / (2 r) + O(r^-2), which over this draw
    (n = 3001, variance mu + mu^2 / 1.5, E mu^2 about 33) sums to a few 1e-3 against an nll of several thousand. The
    device part y l - (y + r) log(e^l + r) alone has no Poisson counterpart: it becomes y l - e^l only together with
    the host's constant sum lgamma(y + r) + n (r log r - lgamma(r)), terms of size 1e11 here, so the check is also one
    of that constant's summation."""
    case = golden["k2_nb_aux_chol"]
    g, y, _ = _data(case)
    r = 1e7
    gm = GPModel(group_data=g, likelihood=NB, matrix_inversion_method="cholesky")
    gm.set_optim_params({"init_aux_pars": [r], "estimate_aux_pars": False})
    nll_nb = gm.neg_log_likelihood(case["cov_pars"], y)
    gp = GPModel(group_data=g, likelihood="poisson", matrix_inversion_method="cholesky")
    nll_p = gp.neg_log_likelihood(case["cov_pars"], y)
    print("nb", nll_nb, "poisson", nll_p, "relative difference", abs(nll_nb - nll_p) / abs(nll_p))
    assert abs(nll_nb - nll_p) <= 1e-6 * abs(nll_p), (nll_nb, nll_p)


def test_refusals():
    g = synthetic.bench_groups(600, (20, 5))
    y = synthetic.bench_grouped_negbin_y(g)
    gm = GPModel(group_data=g, likelihood=NB, matrix_inversion_method="cholesky")
    with pytest.raises(GPBoostError, match="y >= 0"):
        gm.neg_log_likelihood([0.5, 0.5], y - 1.)
    with pytest.raises(GPBoostError, match="non-integer"):
        gm.neg_log_likelihood([0.5, 0.5], y + 0.5)
    with pytest.raises(GPBoostError, match="> 0"):
        gm.set_optim_params({"init_aux_pars": [0.], "estimate_aux_pars": True})
    with pytest.raises(GPBoostError, match="> 0"):
        gm.set_optim_params({"init_aux_pars": [-1.], "estimate_aux_pars": True})
    coords = synthetic.bench_coords(600)
    with pytest.raises(GPBoostError, match="grouped random effects only"):
        GPModel(gp_coords=coords, cov_function="exponential", likelihood=NB)
    for approx in ("vecchia", "fitc", "full_scale_vecchia"):
        with pytest.raises(GPBoostError, match="grouped random effects only"):
            GPModel(gp_coords=coords, cov_function="exponential", likelihood=NB, gp_approx=approx)
    with pytest.raises(GPBoostError, match="grouped random effects only"):
        GPModel(group_data=g, gp_coords=coords, likelihood=NB, cov_function="exponential",
                matrix_inversion_method="cholesky")
    with pytest.raises(GPBoostError, match="supported: gaussian, bernoulli_logit.*negative_binomial\\)"):
        GPModel(group_data=g, likelihood="negative_binomial_1", matrix_inversion_method="cholesky")
    # what the grouped Laplace driver refuses stays refused
    gm.neg_log_likelihood([0.5, 0.5], y)
    with pytest.raises(GPBoostError, match="std_err"):
        gm.get_cov_pars(std_err=True)
    with pytest.raises(GPBoostError, match="predict_cov_mat"):
        gm.predict(group_data_pred=g[:5], predict_cov_mat=True, predict_response=False)
    gi = GPModel(group_data=g, likelihood=NB)   # iterative by default
    gi.neg_log_likelihood([0.5, 0.5], y)
    with pytest.raises(GPBoostError, match="iterative"):
        gi.predict(group_data_pred=g[:5], predict_var=True, predict_response=False)
