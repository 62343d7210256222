"""GPU parity for grouped (crossed) random effects under non-Gaussian likelihoods (Laplace approximation) against the
reference itself.

Reference path: GPB_CreateREModel with re_group_data and likelihood bernoulli_logit / bernoulli_probit / poisson / gamma ->
FindModePostRandEffCalcMLLGroupedRE (likelihoods.h:1975-2194, Cholesky branch) and, for one grouping variable,
FindModePostRandEffCalcMLLOnlyOneGroupedRECalculationsOnREScale (:2206-2293); gradients :3634-3740 / :3761-3854;
predictions :5696-5953 / :5973-6032. Fixtures: tests/golden/golden_grouped_laplace.json (make_golden_grouped_laplace.py
runs oracle/_ref/ref_harness_grouped; tests/test_grouped_laplace_fixtures.py re-derives every nll in numpy).

Tolerances are the project's bounds for its exact (Cholesky) Laplace paths (tests/test_gpu_latent_chol.py): nll 1e-9
relative, gradient 1e-7 relative with atol 1e-7 max|ref|; gradient wrt F 1e-7 max(1, max|ref|); fits as
tests/test_gpu_grouped.py::test_grouped_fit_matches_reference; predictions 1e-6 max|ref|; training-data random effects
1e-9 max|ref|. Both sides run the same Newton iterations from mode 0 with the same stopping rule.

Iterative cases (several grouping variables; the default method there): 1e-6 relative, see
test_iterative_nll_and_grad_match_reference.
"""
import json
import os
import sys

import numpy as np
import pytest

from gpboost_amd import GPBoostError, GPModel, synthetic

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

Y_OF = {"bernoulli_logit": synthetic.bench_grouped_bernoulli_y, "bernoulli_probit": synthetic.bench_grouped_bernoulli_y,
        "poisson": synthetic.bench_grouped_poisson_y, "gamma": synthetic.bench_grouped_gamma_y}
EVAL_CASES = ["k1_logit", "k1_pois", "k1_gamma_aux", "k2_logit_chol", "k2_uneven_chol", "k3_pois_chol",
              "k2_gamma_aux_chol", "k2_logit_offset_chol", "k1_logit_offset"]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "golden_grouped_laplace.json")) as f:
        return json.load(f)


def _data(case):
    g = synthetic.bench_groups(case["n"], tuple(case["levels"]))
    y = Y_OF[case["likelihood"]](g)
    fe = 0.5 * (synthetic.lcg_unif(case["n"], 0.77) - 0.5) if case["offset"] else None
    return g, y, fe


def _model(case, g):
    it = case.get("iterative")
    gm = GPModel(group_data=g, likelihood=case["likelihood"], matrix_inversion_method="iterative" if it else "cholesky")
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
    assert gm.num_cov_pars == K and gm.num_aux_pars == (1 if case["likelihood"] == "gamma" else 0)
    assert gm.cov_par_names() == [f"Group_{k + 1}" for k in range(K)]
    cp = np.array(case["cov_pars"])
    nll = gm.neg_log_likelihood(cp, y, fixed_effects=fe)
    nll2, grad, _ = gm.neg_log_likelihood_and_grad(cp, y, fixed_effects=fe)
    ref = np.asarray(case["grad"])   # the aux-parameter gradient is its last entry
    print(name, "nll dev", abs(nll - case["nll"]) / abs(case["nll"]), "grad dev", np.abs(grad - ref).max() / np.abs(ref).max())
    assert abs(nll - case["nll"]) <= 1e-9 * abs(case["nll"]), (nll, case["nll"])
    assert nll2 == nll   # both start the mode finding from zero
    assert grad.shape == ref.shape
    np.testing.assert_allclose(grad, ref, rtol=1e-7, atol=1e-7 * np.abs(ref).max())
    # equal inputs give equal bits
    nll3, grad3, _ = gm.neg_log_likelihood_and_grad(cp, y, fixed_effects=fe)
    assert nll3 == nll2
    np.testing.assert_array_equal(grad3, grad)
    if "grad_f" in case:   # the mode of the evaluation above as it stands (the reference: from zero, then CalcGradientF)
        gf = gm.calc_gradient_f(fixed_effects=fe, calc_cov_factor=False)
        rf = np.asarray(case["grad_f"])
        print(name, "grad_f dev", np.abs(gf - rf).max())
        assert np.abs(gf - rf).max() <= 1e-7 * max(1., np.abs(rf).max())


ITER_CASES = ["k2_logit_tight", "k3_probit_tight", "k2_gamma_aux_iter", "k2_logit_offset_iter", "k2_pois_default"]


@pytest.mark.parametrize("name", ITER_CASES)
def test_iterative_nll_and_grad_match_reference(golden, name):
    """matrix_inversion_method = "iterative": 1e-6 relative on the nll and the gradient (atol 1e-6 max|ref|; the aux
    gradient is the last entry), the project's bounds for iterative Laplace fixtures (tests/test_gpu_precond.py,
    tests/test_gpu_latent.py). The probes are the reference's own draws and both sides run the same stopping tests, at
    cg_delta_conv = 1e-10 and at the default 1e-2 (k2_pois_default; the argument of tests/test_gpu_grouped.py:15-21)."""
    case = golden[name]
    g, y, fe = _data(case)
    gm = _model(case, g)
    assert gm.get_optim_params()["cg_preconditioner_type"] == "ssor"
    cp = np.array(case["cov_pars"])
    nll, grad, _ = gm.neg_log_likelihood_and_grad(cp, y, fixed_effects=fe)
    ref = np.asarray(case["grad"])
    print(name, "nll dev", abs(nll - case["nll"]) / abs(case["nll"]), "grad dev", np.abs(grad - ref).max() / np.abs(ref).max())
    assert abs(nll - case["nll"]) <= 1e-6 * abs(case["nll"]), (nll, case["nll"])
    assert grad.shape == ref.shape
    np.testing.assert_allclose(grad, ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())
    nll3, grad3, _ = gm.neg_log_likelihood_and_grad(cp, y, fixed_effects=fe)   # equal inputs give equal bits
    assert nll3 == nll
    np.testing.assert_array_equal(grad3, grad)
    if "grad_f" in case:
        gf = gm.calc_gradient_f(fixed_effects=fe, calc_cov_factor=False)
        rf = np.asarray(case["grad_f"])
        print(name, "grad_f dev", np.abs(gf - rf).max())
        assert np.abs(gf - rf).max() <= 1e-7 * max(1., np.abs(rf).max())


def test_default_method_is_iterative_for_several_effects(golden):
    case = golden["k2_pois_default"]
    g, y, _ = _data(case)
    gm = GPModel(group_data=g, likelihood="poisson")   # every option at its default
    nll = gm.neg_log_likelihood(case["cov_pars"], y)
    assert abs(nll - case["nll"]) <= 1e-6 * abs(case["nll"])


@pytest.mark.parametrize("name", ["fit_k1_logit", "fit_k2_logit_chol", "fit_k2_gamma_chol", "fit_k2_pois_offset_chol",
                                  "fit_k2_logit_iter_tight"])
def test_fit_matches_reference(golden, name):
    case = golden[name]
    g, y, fe = _data(case)
    gm = _model(case, g)
    gm.fit(y, offset=fe)
    np.testing.assert_allclose(gm.get_init_cov_pars(), case["init_cov_pars"], rtol=1e-12)
    assert gm.get_num_optim_iter() == case["num_it"]
    np.testing.assert_allclose(gm.get_cov_pars(), case["cov_pars"], rtol=1e-6)
    assert abs(gm.get_current_neg_log_likelihood() - case["nll"]) <= 1e-9 * abs(case["nll"])
    if "aux_fit" in case:
        aux, aux_name = gm.get_aux_pars()
        assert aux_name == "shape"
        np.testing.assert_allclose(aux, case["aux_fit"], rtol=1e-6)


@pytest.mark.parametrize("name", ["pred_k1_logit", "pred_k1_logit_resp", "pred_k2_logit_chol", "pred_k2_logit_chol_resp",
                                  "pred_k3_pois_chol_resp", "pred_k1_probit_resp", "pred_k2_gamma_chol_resp"])
def test_predictions_match_reference(golden, name):
    case = golden[name]
    g, y, _ = _data(case)
    gm = _model(case, g)
    labels = np.asarray(case["labels"])
    seen = np.array([[labels[i, k] in set(g[:, k]) for k in range(g.shape[1])] for i in range(labels.shape[0])])
    assert seen.all(axis=1).any() and (~seen).all(axis=1).any()   # seen and unseen labels
    assert g.shape[1] == 1 or (seen.any(axis=1) & ~seen.all(axis=1)).any()   # and rows mixing both
    p = gm.predict(y=y, cov_pars=case["cov_pars"], group_data_pred=labels, predict_var=True,
                   predict_response=case["response"])
    rm, rv = np.asarray(case["mean"]), np.asarray(case["var"])
    print(name, "mean dev", np.abs(p["mu"] - rm).max(), "var dev", np.abs(p["var"] - rv).max())
    assert np.abs(p["mu"] - rm).max() <= 1e-6 * np.abs(rm).max()
    assert np.abs(p["var"] - rv).max() <= 1e-6 * np.abs(rv).max()
    # means alone (no variances asked)
    p0 = gm.predict(y=y, cov_pars=case["cov_pars"], group_data_pred=labels, predict_var=False,
                    predict_response=case["response"])
    np.testing.assert_array_equal(p0["mu"], p["mu"])
    assert p0["var"] is None


def test_iterative_prediction_means_match_reference(golden):
    case = golden["pred_k2_logit_iter"]
    g, y, _ = _data(case)
    gm = _model(case, g)
    labels = np.asarray(case["labels"])
    p = gm.predict(y=y, cov_pars=case["cov_pars"], group_data_pred=labels, predict_var=False, predict_response=False)
    rm = np.asarray(case["mean"])
    print("iterative mean dev", np.abs(p["mu"] - rm).max())
    assert np.abs(p["mu"] - rm).max() <= 1e-6 * np.abs(rm).max()
    with pytest.raises(GPBoostError, match="iterative"):   # the reference simulates them
        gm.predict(y=y, cov_pars=case["cov_pars"], group_data_pred=labels, predict_var=True, predict_response=False)
    with pytest.raises(GPBoostError, match="predict_response"):
        gm.predict(y=y, cov_pars=case["cov_pars"], group_data_pred=labels, predict_var=False, predict_response=True)


@pytest.mark.parametrize("name", ["pred_train_k1_logit", "pred_train_k2_logit_chol", "pred_train_k2_logit_iter"])
def test_training_data_random_effects_match_reference(golden, name):
    case = golden[name]
    g, y, _ = _data(case)
    gm = _model(case, g)
    gm.neg_log_likelihood(case["cov_pars"], y)
    out = gm.predict_training_data_random_effects()
    assert out.shape == (case["n"], len(case["levels"]))
    for k, ref in enumerate(case["level_means"]):
        _, first = np.unique(g[:, k], return_index=True)
        ref = np.asarray(ref)
        got = out[np.sort(first), k]
        assert np.abs(got - ref).max() <= (1e-6 if case.get("iterative") else 1e-9) * np.abs(ref).max()
        # every observation carries its level's value
        lev = {int(g[i, k]): out[i, k] for i in np.sort(first)}
        assert all(out[i, k] == lev[int(g[i, k])] for i in range(0, case["n"], 7))


def test_weighted_assembly_matches_numpy(golden):
    """Z^T W Z on the device (diagonal and CSR values: lists of 1000 observations cut into chunks, level pairs with one
    observation) against a dense numpy assembly with W at the device's own mode."""
    from grouped_laplace_restatement import LIKELIHOODS, design
    case = golden["k2_uneven_chol"]
    g, y, _ = _data(case)
    gm = _model(case, g)
    gm.neg_log_likelihood(case["cov_pars"], y)
    rowptr, col, diag, vals = gm.grouped_laplace_info()
    b_obs = gm.predict_training_data_random_effects()   # the same mode again (from zero, deterministic)
    rowptr2, col2, diag2, vals2 = gm.grouped_laplace_info()
    np.testing.assert_array_equal(diag2, diag)
    np.testing.assert_array_equal(vals2, vals)
    Z, m = design(g)
    M = Z.shape[1]
    assert rowptr.shape == (M + 1,) and rowptr[-1] == col.shape[0] == vals.shape[0]
    eta = b_obs.sum(axis=1)
    W = LIKELIHOODS[case["likelihood"]](y, eta, 1.0)[2]
    ref = Z.T @ (W[:, None] * Z)
    np.testing.assert_allclose(diag, np.diag(ref), rtol=1e-13, atol=0)
    dense = np.zeros((M, M))
    for r in range(M):
        dense[r, col[rowptr[r]:rowptr[r + 1]]] = vals[rowptr[r]:rowptr[r + 1]]
    off = ref - np.diag(np.diag(ref))
    assert np.array_equal(dense != 0, off != 0)
    print("assembly dev", np.abs(dense - off).max() / np.abs(off).max())
    np.testing.assert_allclose(dense, off, rtol=1e-13, atol=0)
    counts = np.bincount(g[:, 0])
    assert counts.min() <= 2 and np.bincount(g[:, 1]).max() >= 1000


def test_string_labels_equal_integer_labels(golden):
    case = golden["k2_logit_chol"]
    g, y, _ = _data(case)
    names = np.array([f"city_{v}" for v in g[:, 0]], dtype=object)
    gs = np.column_stack([names, g[:, 1].astype(str)])
    a = _model(case, g).neg_log_likelihood_and_grad(case["cov_pars"], y)
    b = _model(case, gs).neg_log_likelihood_and_grad(case["cov_pars"], y)
    assert a[0] == b[0]
    np.testing.assert_array_equal(a[1], b[1])


def test_warm_start_reproduces_cold_value(golden):
    """An evaluation that continues from the previous mode (as the L-BFGS objective does) gives the value of the
    evaluation from mode 0 within the nll bound."""
    case = golden["k2_logit_chol"]
    g, y, _ = _data(case)
    gm = _model(case, g)
    cold = gm.neg_log_likelihood(case["cov_pars"], y)
    gm.calc_gradient_f(calc_cov_factor=True)   # mode finding from the current mode
    warm = gm.get_current_neg_log_likelihood()
    print("warm - cold", abs(warm - cold) / abs(cold))
    assert abs(warm - cold) <= 1e-9 * abs(cold)
    assert abs(warm - case["nll"]) <= 1e-9 * abs(case["nll"])


def test_refusals():
    g = synthetic.bench_groups(600, (20, 5))
    y = synthetic.bench_grouped_bernoulli_y(g)
    with pytest.raises(GPBoostError, match="single-level grouped"):
        GPModel(group_data=g[:, :1], likelihood="bernoulli_logit", matrix_inversion_method="iterative")
    with pytest.raises(GPBoostError, match="Gaussian process beside grouped"):
        GPModel(group_data=g, gp_coords=synthetic.bench_coords(600), likelihood="poisson", cov_function="exponential",
                matrix_inversion_method="cholesky")
    with pytest.raises(GPBoostError, match="supported: gaussian, bernoulli_logit"):
        GPModel(group_data=g, likelihood="t", matrix_inversion_method="cholesky")
    gm = GPModel(group_data=g, likelihood="bernoulli_logit", matrix_inversion_method="cholesky")
    with pytest.raises(GPBoostError, match="profile_sigma2"):
        gm.neg_log_likelihood_and_grad([0.5, 0.5], y, profile_sigma2=True)
    with pytest.raises(GPBoostError, match="not supported"):
        gm.set_optim_params({"cg_preconditioner_type": "incomplete_cholesky"})
    gm.set_optim_params({"cg_preconditioner_type": None})
    with pytest.raises(GPBoostError, match="nelder_mead"):
        gm.set_optim_params({"optimizer_cov": "nelder_mead"})
    gm.set_optim_params({"optimizer_cov": "lbfgs"})
    gm.neg_log_likelihood([0.5, 0.5], y)
    assert not gm.can_calculate_standard_errors_cov_pars()
    with pytest.raises(GPBoostError, match="std_err"):
        gm.get_cov_pars(std_err=True)
    with pytest.raises(GPBoostError, match="predict_cov_mat"):
        gm.predict(group_data_pred=g[:5], predict_cov_mat=True, predict_response=False)
    with pytest.raises(GPBoostError, match="predict_var"):
        gm.predict_training_data_random_effects(predict_var=True)
    with pytest.raises(GPBoostError, match="GPB_OptimCovParBoosting"):
        gm.optim_cov_par_boosting(fixed_effects=np.zeros(600))
    with pytest.raises(GPBoostError, match="0 or 1"):
        gm.neg_log_likelihood([0.5, 0.5], y + 0.5)
    # Gaussian grouped models are as before: error term first, no aux parameters
    gg = GPModel(group_data=g, matrix_inversion_method="cholesky")
    assert gg.num_cov_pars == 3 and gg.num_aux_pars == 0 and gg.cov_par_names()[0] == "Error_term"


def test_size_smoke_gradient_agrees_in_sign_with_finite_difference():
    """n = 500000, levels (5000, 500), bernoulli_logit, every option at its default (iterative, cg_delta_conv = 1e-2): a
    finite nll and a gradient that agrees in sign with a central difference of two tight evaluations (cg_delta_conv =
    1e-10 and delta_conv_mode_finding = 1e-14 on the same probes, h = 1e-3 in the log variance)."""
    n = 500000
    g = synthetic.bench_groups(n, (5000, 500))
    y = synthetic.bench_grouped_bernoulli_y(g)
    gm = GPModel(group_data=g, likelihood="bernoulli_logit")
    cp = np.array([0.8, 0.3])
    nll, grad, _ = gm.neg_log_likelihood_and_grad(cp, y)
    assert np.isfinite(nll) and np.all(np.isfinite(grad))
    gm.set_optim_params({"cg_delta_conv": 1e-10, "delta_conv_mode_finding": 1e-14})
    h = 1e-3
    for k in range(2):
        e = np.zeros(2)
        e[k] = h
        fd = (gm.neg_log_likelihood(cp * np.exp(e), y) - gm.neg_log_likelihood(cp * np.exp(-e), y)) / (2 * h)
        print("k", k, "grad", grad[k], "fd", fd)
        assert np.sign(fd) == np.sign(grad[k])
