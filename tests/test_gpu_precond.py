"""GPU parity for cg_preconditioner_type = "pivoted_cholesky" (iterative Vecchia-Laplace models and
vecchia_latent) through the C ABI: the pivoted Cholesky of the exact covariance on the device, the
low-rank-plus-diagonal preconditioner and the CG / Lanczos runs on W^-1 + Sigma.

Fixtures: tests/golden/golden_precond.json, the reference itself at its default rank 50
(make_golden_precond.py; tests/test_precond_fixtures.py shows that no fixture's pivots depend on rounding).
Tolerances are the project's for tight (cg_delta_conv = 1e-10) iterative fixtures: nll and gradient 1e-6
relative (gradient atol 1e-6 max|ref|), gradient wrt F 1e-7 of max(1, max|ref|), predictions 1e-6 of
max|ref|. At the default cg_delta_conv = 1e-2 the gradient bound is twice the reference's own spread under
1e-14 relative moves of the covariance parameters, read from the fixture.
"""
import json
import os

import numpy as np
import pytest

from gpboost_amd import GPBoostError, GPModel, synthetic

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "golden_precond.json")) as _f:
    GOLDEN = json.load(_f)

EVAL = ["logit_short", "pois_smooth", "pois_early_stop", "gamma_aux", "gauss_latent"]


def _data(case):
    X = synthetic.bench_coords(case["n"])
    kind = case["data"]
    if kind == "bench_gauss":
        return X, synthetic.bench_gaussian_y(case["n"])
    if kind == "bench_gamma":
        return X, synthetic.bench_gamma_y(X)
    return X, (synthetic.bench_poisson_y(X) if kind == "bench_pois" else synthetic.bench_bernoulli_y(X))


def _model(X, case, dc=None, precond="pivoted_cholesky", rank=None, t=50):
    kw = dict(gp_coords=X, cov_function=case["cov_fct"], cov_fct_shape=float(case["shape"]),
              gp_approx=case.get("gp_approx", "vecchia"), num_neighbors=case["num_neighbors"],
              vecchia_ordering="random", matrix_inversion_method="iterative", seed=0)
    if case["likelihood"] != "gaussian":
        kw["likelihood"] = case["likelihood"]
    gm = GPModel(**kw)
    params = dict(num_rand_vec_trace=t, seed_rand_vec_trace=1,
                  cg_delta_conv=case.get("cg_delta_conv", 1e-10) if dc is None else dc, cg_preconditioner_type=precond)
    if rank is not None:
        params["fitc_piv_chol_preconditioner_rank"] = rank
    if case.get("aux") is not None:
        params["init_aux_pars"] = [float(case["aux"])]
        params["estimate_aux_pars"] = bool(case["estimate_aux"])
    gm.set_optim_params(params)
    return gm


def _offset(X):
    return 0.3 * np.sin(3.0 * X[:, 0]) - 0.2


@pytest.mark.parametrize("name", EVAL)
def test_nll_and_gradient_match_reference(name):
    case = GOLDEN[name]
    X, y = _data(case)
    gm = _model(X, case)
    nll, g, _ = gm.neg_log_likelihood_and_grad(case["cov_pars"], y)
    ref = np.asarray(case["grad"])
    print(name, "nll", nll, case["nll"], "grad", g, ref)
    assert abs(nll - case["nll"]) <= 1e-6 * abs(case["nll"]), (nll, case["nll"])
    np.testing.assert_allclose(g, ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())
    # the device factorisation took the pivots of the restatement and stopped where it stops
    rank, _, piv = gm.piv_chol_info()
    assert rank == case["rank"] and piv.tolist() == case["pivots"]


def test_gradient_wrt_fixed_effects_matches_reference():
    case = GOLDEN["logit_grad_f"]
    X, y = _data(case)
    F = _offset(X)
    gm = _model(X, case)
    nll, g, _ = gm.neg_log_likelihood_and_grad(case["cov_pars"], y, fixed_effects=F)
    ref = np.asarray(case["grad"])
    assert abs(nll - case["nll"]) <= 1e-6 * abs(case["nll"]), (nll, case["nll"])
    np.testing.assert_allclose(g, ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())
    gm.set_optim_params({"init_cov_pars": np.array(case["cov_pars"])})
    gf = gm.calc_gradient_f(fixed_effects=F)
    rf = np.asarray(case["grad_f"])
    print("grad_f max deviation", np.abs(gf - rf).max())
    assert np.abs(gf - rf).max() <= 1e-7 * max(1., np.abs(rf).max())


@pytest.mark.parametrize("name", ["pred_latent", "pred_response"])
def test_predictions_match_reference(monkeypatch, name):
    """Means and simulated variances on the reference's own one-thread draws (GPBOOST_AMD_PRED_DRAWS=reference,
    as tests/test_gpu_latent_pred_1t.py): every draw is solved by the CG on W^-1 + Sigma."""
    monkeypatch.setenv("GPBOOST_AMD_PRED_DRAWS", "reference")
    case = GOLDEN[name]
    X, y = _data(case)
    Xp = synthetic.lcg_unif(case["npred"] * 2, 0.713).reshape(2, case["npred"]).T.copy()
    gm = _model(X, case)
    gm.set_prediction_data(vecchia_pred_type=case["ptype"], nsim_var_pred=case["nsim"])
    pred = gm.predict(y=y, gp_coords_pred=Xp, cov_pars=case["cov_pars"], predict_var=True,
                      predict_response=case["response"])
    mu, var = np.asarray(case["mean"]), np.asarray(case["var"])
    print(name, "mean dev", np.abs(pred["mu"] - mu).max(), "var dev", np.abs(pred["var"] - var).max())
    assert np.abs(pred["mu"] - mu).max() <= 1e-6 * np.abs(mu).max()
    assert np.abs(pred["var"] - var).max() <= 1e-6 * np.abs(var).max()


def test_default_tolerance_within_reference_sensitivity():
    """cg_delta_conv = 1e-2: nll at 1e-6; the gradient within twice the reference's own largest deviation under
    1e-14 relative moves of the covariance parameters (fixture "sensitivity"; no value of this implementation
    enters the bound), as tests/test_gpu_latent.py does for the VADU preconditioner."""
    case = GOLDEN["logit_default_tol"]
    ref_g = np.asarray(case["grad"])
    spread = np.max([np.abs(np.asarray(r["grad"]) - ref_g) for r in case["sensitivity"]["runs"]], axis=0)
    X, y = _data(case)
    gm = _model(X, case)
    nll, g, _ = gm.neg_log_likelihood_and_grad(case["cov_pars"], y)
    print("default tol: nll", nll, case["nll"], "grad", g, ref_g, "spread", spread)
    assert abs(nll - case["nll"]) <= 1e-6 * abs(case["nll"]), (nll, case["nll"])
    assert np.all(np.abs(g - ref_g) <= 2 * spread), (g, ref_g, spread)


def test_rank_setting_is_used_and_solves_agree():
    """fitc_piv_chol_preconditioner_rank 8 and 64 at n = 600 (no reference fixture: the harness always runs rank
    50). With cg_delta_conv = 1e-10 every Newton step solves the same system to that residual whatever the
    preconditioner, so the latent predictive mean equals the default-rank one; the nll differs, because the
    stochastic log-determinant estimate depends on P: the rank is really used. A rank above the number of
    latent variables raises the reference's message."""
    case = GOLDEN["logit_short"]
    X, y = _data(case)
    Xp = synthetic.lcg_unif(40, 0.713).reshape(2, 20).T.copy()
    out = {}
    for rank in (None, 8, 64):
        gm = _model(X, case, rank=rank)
        nll = gm.neg_log_likelihood(case["cov_pars"], y)
        pred = gm.predict(y=y, gp_coords_pred=Xp, cov_pars=case["cov_pars"], predict_var=False, predict_response=False)
        out[rank] = (nll, np.asarray(pred["mu"]), gm.piv_chol_info()[0])
    assert out[None][2] == 50 and out[8][2] == 8 and out[64][2] == 64
    for rank in (8, 64):
        assert np.abs(out[rank][1] - out[None][1]).max() <= 1e-6 * np.abs(out[None][1]).max()
        assert out[rank][0] != out[None][0]
        assert abs(out[rank][0] - out[None][0]) < 1e-2 * abs(out[None][0])   # still an estimate of the same nll
    with pytest.raises(GPBoostError, match="cannot be larger than the dimension of the mode"):
        _model(X, case, rank=601)


def test_two_identical_calls_are_bitwise_identical():
    case = GOLDEN["logit_short"]
    X, y = _data(case)
    res = []
    for _ in range(2):
        gm = _model(X, case)
        nll, g, _ = gm.neg_log_likelihood_and_grad(case["cov_pars"], y)
        res.append((nll, np.asarray(g)))
    assert res[0][0] == res[1][0]
    assert np.array_equal(res[0][1], res[1][1])


def test_fit_converges_and_reports_its_likelihood():
    """L-BFGS on the n = 600 logit case. The reference harness's fit mode is fixed to the VADU preconditioner, so
    there is no reference fit fixture for this one; the test checks the fit's own consistency: it converges
    below maxit and the likelihood it reports is the likelihood at the parameters it returns."""
    case = GOLDEN["logit_short"]
    X, y = _data(case)
    gm = _model(X, case, dc=1e-6)
    gm.fit(y, params=dict(maxit=100))
    assert 0 < gm.get_num_optim_iter() < 100
    cp = gm.get_cov_pars()
    assert np.all(np.isfinite(cp)) and np.all(cp > 0)
    cur = gm.get_current_neg_log_likelihood()
    nll = gm.neg_log_likelihood(cp, y)
    assert abs(cur - nll) <= 1e-9 * abs(nll), (cur, nll)
    assert gm.get_optim_params()["cg_preconditioner_type"] == "pivoted_cholesky"


def test_alias_and_refusals():
    case = GOLDEN["logit_short"]
    X, y = _data(case)
    gm = _model(X, case, precond="piv_chol")
    assert gm.get_optim_params()["cg_preconditioner_type"] == "pivoted_cholesky"
    gm = _model(X, case, precond="piv_chol_on_Sigma")
    assert gm.get_optim_params()["cg_preconditioner_type"] == "pivoted_cholesky"
    for bad in ("fitc", "vecchia_response", "incomplete_cholesky", "no_such_preconditioner"):
        with pytest.raises(GPBoostError, match="vadu, pivoted_cholesky"):
            _model(X, case, precond=bad)
    # the default stays vadu
    gd = GPModel(gp_coords=X, likelihood="bernoulli_logit", cov_function="exponential", gp_approx="vecchia",
                 num_neighbors=10, matrix_inversion_method="iterative", seed=0)
    assert gd.get_optim_params()["cg_preconditioner_type"] == "vadu"
    # repeated coordinates
    Xd = np.vstack([X[:300], X[:300]])
    gr = _model(Xd, case)
    with pytest.raises(GPBoostError, match="repeated coordinates"):
        gr.neg_log_likelihood(case["cov_pars"], y)


def test_sharded_model_is_refused():
    case = GOLDEN["logit_short"]
    X, y = _data(case)
    kw = dict(gp_coords=X, likelihood="bernoulli_logit", cov_function="exponential", gp_approx="vecchia",
              num_neighbors=10, vecchia_ordering="random", matrix_inversion_method="iterative", seed=0)
    gm = GPModel(**kw)
    gm.set_distributed_host(0, 2, lambda buf: None)
    with pytest.raises(GPBoostError, match="multi-rank"):
        gm.set_optim_params(dict(cg_preconditioner_type="pivoted_cholesky"))
    gm = GPModel(**kw)   # the other order: the evaluation refuses
    gm.set_optim_params(dict(cg_preconditioner_type="pivoted_cholesky", cg_delta_conv=1e-10))
    gm.set_distributed_host(0, 2, lambda buf: None)
    with pytest.raises(GPBoostError, match="multi-rank"):
        gm.neg_log_likelihood(case["cov_pars"], y)
