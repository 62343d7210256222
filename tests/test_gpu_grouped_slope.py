"""GPU: grouped random slopes (GPModel(group_rand_coef_data=...)) against the reference's own R-test values and the dense
numpy oracles of tests/grouped_slope_cases.py (pinned to those values on the CPU by tests/test_grouped_slope_reference.py;
the oracle's two forms agree to 1e-12).

Tolerances. Gaussian cholesky, as tests/test_gpu_grouped.py: nll 1e-10 relative, gradient rtol 1e-6 with atol 1e-6 of the
largest entry, means atol 1e-10 of the largest, variances and covariances rtol 1e-9, standard deviations rtol 1e-8. R
fits at the R tests' tolerances (test_GPModel_grouped_random_effects.R: 1e-6 strict, 1e-3 medium, 1e-2 loose, 1e-1 very
loose, sums of absolute deviations). Laplace against the restatement, as tests/test_gpu_grouped_laplace.py: nll 1e-9
relative, gradient rtol 1e-7 with atol 1e-7 of the largest, grad_F 1e-7 max(1, largest). Iterative Gaussian: the
PCG-solved random-effect means atol 1e-8 of the largest; the stochastic nll and gradient within 6 standard errors of
the mean over 8 seeds. Identities at weight one: equal bits.

Not covered here: the R test's Nelder-Mead fit of the probit model (test_GPModel_non_Gaussian_data.R:880-886):
tests/test_gpu_grouped_laplace.py pins the refusal of optimizer_cov = "nelder_mead" for grouped Laplace models.
"""
import numpy as np
import pytest

import grouped_slope_cases as S
from gpboost_amd import GPBoostError, GPModel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gd():
    d = S.gaussian_data()
    d["g12"] = np.column_stack([d["group"], d["group2"]])
    return d


@pytest.fixture(scope="module")
def pdat():
    d = S.probit_data()
    d["g12"] = np.column_stack([d["group"], d["group2"]])
    return d


def _slope_model(d, method="cholesky", likelihood="gaussian", drop=None, **kw):
    return GPModel(group_data=d["g12"], group_rand_coef_data=d["x"], ind_effect_group_rand_coef=[1],
                   drop_intercept_group_rand_effect=drop, likelihood=likelihood, matrix_inversion_method=method, **kw)


def _trafo_grad(cp, Z, m, y, profile):
    return S.gaussian_nll_grad(Z, m, y, cp, "woodbury", profile)


# ------------------------------------------------------------------------------------------------ Gaussian, cholesky
@pytest.mark.parametrize("drop", [None, [True, False]])
def test_gaussian_nll_and_grad(gd, drop):
    y = gd["y_slope"] if drop is None else gd["y_drop"]
    cp = [0.1, 1.0, 2.0, 1.5] if drop is None else [0.1, 2.0, 1.5]
    gm = _slope_model(gd, drop=drop)
    comps = S.components(gd["g12"], gd["x"], [1], drop)
    Z, m = S.design(comps)
    assert gm.num_cov_pars == len(cp)
    names = ["Error_term", "Group_1", "Group_2", "Group_1_rand_coef_nb_1"]
    assert gm.cov_par_names() == (names if drop is None else [names[0], names[2], names[3]])
    ref, gref, _ = _trafo_grad(cp, Z, m, y, False)
    nll = gm.neg_log_likelihood(cp, y)
    nll2, grad, _ = gm.neg_log_likelihood_and_grad(cp, y)
    print("nll", nll, "dev", abs(nll - ref) / abs(ref), "grad dev", np.abs(grad - gref).max() / np.abs(gref).max())
    if drop is None:
        assert abs(nll - 2335.803) < 1e-2        # test_GPModel_grouped_random_effects.R:557
    assert abs(nll - ref) <= 1e-10 * abs(ref)
    assert nll2 == nll
    np.testing.assert_allclose(grad, gref, rtol=1e-6, atol=1e-6 * np.abs(gref).max())
    refp, grefp, s2p = _trafo_grad(cp, Z, m, y, True)
    nllp, gradp, s2 = gm.neg_log_likelihood_and_grad(cp, y, profile_sigma2=True)
    assert abs(nllp - refp) <= 1e-10 * abs(refp) and abs(s2 - s2p) <= 1e-10 * s2p
    np.testing.assert_allclose(gradp, grefp, rtol=1e-6, atol=1e-6 * np.abs(grefp).max())


@pytest.mark.parametrize("drop", [None, [True, False]])
def test_gaussian_predictions(gd, drop):
    y = gd["y_slope"] if drop is None else gd["y_drop"]
    cp = [0.1, 1.0, 2.0, 1.5] if drop is None else [0.1, 2.0, 1.5]
    gm = _slope_model(gd, drop=drop)
    gp = np.array([[1, 2], [1, 1], [101, 1001], [101, 7], [3, 1001], [101, 1002]])
    xp = np.array([0.0, 10.0, 0.3, -2.0, 0.5, 1.5])
    comps = S.components(gd["g12"], gd["x"], [1], drop)
    pts, same = S.pred_points(gd["g12"], gp, xp, [1], drop)
    mu, cov = S.gaussian_predict(comps, y, cp, pts, same)
    with pytest.raises(GPBoostError, match="group_rand_coef_data_pred"):    # the R test's expect_error (:541)
        gm.predict(y=y, group_data_pred=gp, cov_pars=cp)
    p = gm.predict(y=y, group_data_pred=gp, group_rand_coef_data_pred=xp, cov_pars=cp, predict_cov_mat=True)
    if drop is None:   # :544-548
        assert np.abs(p["mu"][:3] - [0.7579961, -0.2868530, 0.0]).sum() < 1e-6
        exp_cov = [0.11534086, -0.01988167, 0.0, -0.01988167, 2.4073302, 0.0, 0.0, 0.0, 3.235]
    else:              # :636-645
        assert np.abs(p["mu"][:3] - [0.8426751, -0.5964363, 0.0]).sum() < 1e-6
        exp_cov = [0.10558205, -0.01269261, 0.0, -0.01269261, 2.40180871, 0.0, 0.0, 0.0, 2.235]
    assert np.abs(p["cov"][:3, :3].ravel() - exp_cov).sum() < 1e-3
    np.testing.assert_allclose(p["mu"], mu, rtol=0, atol=1e-10 * np.abs(mu).max())
    np.testing.assert_allclose(p["cov"], cov, rtol=1e-9, atol=1e-12 * np.abs(cov).max())
    pv = gm.predict(y=y, group_data_pred=gp, group_rand_coef_data_pred=xp, cov_pars=cp, predict_var=True)
    np.testing.assert_allclose(pv["mu"], mu, rtol=0, atol=1e-10 * np.abs(mu).max())
    np.testing.assert_allclose(pv["var"], np.diag(cov), rtol=1e-9)
    # the saved-data route
    gm.set_prediction_data(group_data_pred=gp, group_rand_coef_data_pred=xp)
    ps = gm.predict(y=y, cov_pars=cp, predict_var=True, use_saved_data=True)
    np.testing.assert_array_equal(ps["mu"], pv["mu"])
    np.testing.assert_array_equal(ps["var"], pv["var"])


def test_gaussian_training_random_effects(gd):
    cp = [0.5, 1.2, 1.1, 1.1]
    gm = _slope_model(gd)
    gm.neg_log_likelihood(cp, gd["y_slope"])
    out = gm.predict_training_data_random_effects(predict_var=True)
    assert out.shape == (1000, 6)
    comps = S.components(gd["g12"], gd["x"], [1])
    b, var, m = S.gaussian_random_effects(comps, gd["y_slope"], cp)
    off = np.concatenate([[0], np.cumsum(m)])
    for c, (lev, _) in enumerate(comps):   # a slope's block holds the slope effect b, not x b
        np.testing.assert_allclose(out[:, c], b[off[c] + lev], rtol=0, atol=1e-10 * np.abs(b).max())
        np.testing.assert_allclose(out[:, 3 + c], var[off[c] + lev], rtol=1e-9)
    # the R test's consistency checks (:511-536), 1e-6 on sums of absolute deviations
    first1 = np.arange(0, 1000, 10)
    gu = np.arange(1, 101)
    gp = np.column_stack([gu, np.full(100, -1)])
    p0 = gm.predict(group_data_pred=gp, group_rand_coef_data_pred=np.zeros(100), predict_var=True, predict_response=False)
    p1 = gm.predict(group_data_pred=gp, group_rand_coef_data_pred=np.ones(100), predict_var=True, predict_response=False)
    assert np.abs(out[first1, 0] - p0["mu"]).sum() < 1e-6
    assert np.abs(out[first1, 3] - (p0["var"] - cp[2])).sum() < 1e-6
    assert np.abs(out[first1, 2] - (p1["mu"] - p0["mu"])).sum() < 1e-6
    g2u = np.arange(1, 51)
    gp2 = np.column_stack([np.full(50, -1), g2u])
    p2 = gm.predict(group_data_pred=gp2, group_rand_coef_data_pred=np.zeros(50), predict_var=True, predict_response=False)
    assert np.abs(out[:50, 1] - p2["mu"]).sum() < 1e-6
    assert np.abs(out[:50, 4] - (p2["var"] - cp[1])).sum() < 1e-6


def test_gaussian_r_fits(gd):
    y = gd["y_slope"]
    cov_pars = np.array([0.4958303, 1.2493181, 1.0543343, 1.1388604])
    init = np.full(4, np.var(y, ddof=1) / 2)
    gm = _slope_model(gd)
    gm.fit(y, params={"optimizer_cov": "gradient_descent", "init_cov_pars": init})     # :560-568
    print("gradient descent", gm.get_cov_pars(), gm.get_num_optim_iter())
    assert np.abs(gm.get_cov_pars() - cov_pars).sum() < 1e-6
    assert gm.get_num_optim_iter() == 8
    gm = _slope_model(gd)
    gm.fit(y, params={"optimizer_cov": "fisher_scoring", "maxit": 5})                  # :498-505
    exp = np.array([0.49554952, 0.02546769, 1.24880860, 0.18983953, 1.05505134, 0.22337199, 1.13840014, 0.17950490])
    got = gm.get_cov_pars(std_err=True)
    print("fisher scoring", got)
    assert np.abs(got.T.ravel() - exp).sum() < 1e-3
    assert gm.get_num_optim_iter() == 5
    # lbfgs (:577-580) and Nelder-Mead (:570-575)
    gm = _slope_model(gd)
    gm.fit(y, params={"optimizer_cov": "lbfgs"})
    print("lbfgs", gm.get_cov_pars())
    assert np.abs(gm.get_cov_pars() - cov_pars).sum() < 1e-2
    gm = _slope_model(gd)
    gm.fit(y, params={"optimizer_cov": "nelder_mead", "delta_rel_conv": 1e-6})
    print("nelder_mead", gm.get_cov_pars())
    assert np.abs(gm.get_cov_pars() - cov_pars).sum() < 1e-1


@pytest.mark.parametrize("drop", [None, [True, False]])
def test_gaussian_standard_deviations(gd, drop):
    """the Woodbury Fisher information (grouped.h, its n - M term included) on weighted Z against the dense n x n one"""
    y = gd["y_slope"] if drop is None else gd["y_drop"]
    cp = [0.5, 1.2, 1.1, 1.1] if drop is None else [0.5, 1.1, 1.1]
    gm = _slope_model(gd, drop=drop)
    gm.neg_log_likelihood(cp, y)
    got = gm.get_cov_pars(std_err=True)
    ref = S.gaussian_std_dev(S.components(gd["g12"], gd["x"], [1], drop), cp)
    print("sd", got[1], "dev", np.abs(got[1] / ref - 1).max())
    np.testing.assert_array_equal(got[0], cp)
    np.testing.assert_allclose(got[1], ref, rtol=1e-8)


def test_gaussian_r_fit_dropped_intercept(gd):
    y = gd["y_drop"]
    init = np.full(3, np.var(y, ddof=1) / 2)
    gm = _slope_model(gd, drop=[True, False])
    gm.fit(y, params={"optimizer_cov": "gradient_descent", "init_cov_pars": init})     # :598-606
    print(gm.get_cov_pars(), gm.get_num_optim_iter())
    assert np.abs(gm.get_cov_pars() - [0.5017205, 1.0818474, 1.1157430]).sum() < 1e-6
    assert gm.get_num_optim_iter() == 7
    out = gm.predict_training_data_random_effects(predict_var=True)   # :609-631
    assert out.shape == (1000, 4)
    cp = gm.get_cov_pars()
    gu = np.arange(1, 101)
    p = gm.predict(group_data_pred=np.column_stack([gu, np.full(100, -1)]), group_rand_coef_data_pred=np.ones(100),
                   predict_var=True, predict_response=False)
    first1 = np.arange(0, 1000, 10)
    assert np.abs(out[first1, 1] - p["mu"]).sum() < 1e-6
    assert np.abs(out[first1, 3] - (p["var"] - cp[1])).sum() < 1e-6


def test_one_group_with_slope_takes_the_generic_path(gd):
    """one grouping variable and a slope: two components, never the K == 1 closed form; default method iterative"""
    y = gd["y_single"] + gd["x"] * 0.3
    comps = S.components(gd["group"], gd["x"], [1])
    Z, m = S.design(comps)
    cp = [0.4, 0.9, 0.6]
    ref, gref, _ = _trafo_grad(cp, Z, m, y, False)
    gm = GPModel(group_data=gd["group"], group_rand_coef_data=gd["x"], ind_effect_group_rand_coef=[1],
                 matrix_inversion_method="cholesky")
    nll, grad, _ = gm.neg_log_likelihood_and_grad(cp, y)
    assert abs(nll - ref) <= 1e-10 * abs(ref)
    np.testing.assert_allclose(grad, gref, rtol=1e-6, atol=1e-6 * np.abs(gref).max())
    gd_ = GPModel(group_data=gd["group"], group_rand_coef_data=gd["x"], ind_effect_group_rand_coef=[1])
    assert gd_.get_optim_params()["cg_preconditioner_type"] == "ssor"     # the default there is iterative


# ------------------------------------------------------------------------------------------------ identities
def _pair(gd, lik, method, seed=3):
    """[g1, g2] with a slope x = 1 on g1 and g1's intercept dropped, and the intercept model [g2, g1]: the same Z"""
    n = gd["n"]
    a = GPModel(group_data=gd["g12"], group_rand_coef_data=np.ones(n), ind_effect_group_rand_coef=[1],
                drop_intercept_group_rand_effect=[True, False], likelihood=lik, matrix_inversion_method=method)
    b = GPModel(group_data=gd["g12"][:, ::-1], likelihood=lik, matrix_inversion_method=method)
    if method == "iterative":
        for gm in (a, b):
            gm.set_optim_params({"seed_rand_vec_trace": seed, "num_rand_vec_trace": 20})
    return a, b


@pytest.mark.parametrize("method", ["cholesky", "iterative"])
@pytest.mark.parametrize("lik", ["gaussian", "bernoulli_logit", "poisson", "gamma", "negative_binomial"])
def test_weight_one_equals_intercept_model_bitwise(gd, lik, method):
    from gpboost_amd import synthetic
    n = gd["n"]
    if lik == "gaussian":
        y, cp = gd["y_slope"], [0.3, 0.8, 1.1]
    elif lik == "bernoulli_logit":
        y, cp = (gd["y_slope"] > 0).astype(float), [0.8, 1.1]
    elif lik == "gamma":
        y, cp = 0.2 + 3 * synthetic.sim_rand_unif(n, 0.2) * (1 + (gd["y_slope"] > 0)), [0.8, 1.1]
    else:
        y, cp = np.floor(3 * synthetic.sim_rand_unif(n, 0.2) * (1 + (gd["y_slope"] > 0))), [0.8, 1.1]
    a, b = _pair(gd, lik, method)
    if lik in ("gamma", "negative_binomial"):   # the shape is estimated: the gradient ends with its entry
        for gm in (a, b):
            gm.set_optim_params({"init_aux_pars": [1.7]})
    na, ga, _ = a.neg_log_likelihood_and_grad(cp, y)
    nb, gb, _ = b.neg_log_likelihood_and_grad(cp, y)
    assert na == nb and ga.shape == (len(cp) + (lik in ("gamma", "negative_binomial")),)
    np.testing.assert_array_equal(ga, gb)
    gp = np.array([[1, 2], [5, 50], [101, 3], [7, 1001]])
    want_var = method == "cholesky"
    pa = a.predict(y=y, group_data_pred=gp, group_rand_coef_data_pred=np.ones(4), cov_pars=cp, predict_var=want_var,
                   predict_response=False)
    pb = b.predict(y=y, group_data_pred=gp[:, ::-1], cov_pars=cp, predict_var=want_var, predict_response=False)
    np.testing.assert_array_equal(pa["mu"], pb["mu"])
    if want_var:
        np.testing.assert_array_equal(pa["var"], pb["var"])
    if lik != "gaussian":
        np.testing.assert_array_equal(a.calc_gradient_f(calc_cov_factor=False), b.calc_gradient_f(calc_cov_factor=False))


def test_scaling_the_covariate_scales_the_variance(gd):
    """a slope with x = 2 and variance s is the model with x = 1 and variance 4 s"""
    n = gd["n"]
    y = gd["y_slope"]
    mk = lambda x: GPModel(group_data=gd["g12"], group_rand_coef_data=x, ind_effect_group_rand_coef=[2],   # noqa: E731
                           matrix_inversion_method="cholesky")
    n2 = mk(np.full(n, 2.0)).neg_log_likelihood([0.4, 1.0, 0.7, 0.25], y)
    n1 = mk(np.ones(n)).neg_log_likelihood([0.4, 1.0, 0.7, 1.0], y)
    assert abs(n1 - n2) <= 1e-10 * abs(n1)


# ------------------------------------------------------------------------------------------------ Gaussian, iterative
def test_gaussian_iterative(gd):
    y, cp = gd["y_slope"], [0.5, 1.2, 1.1, 1.1]
    comps = S.components(gd["g12"], gd["x"], [1])
    Z, m = S.design(comps)
    ref, gref, _ = _trafo_grad(cp, Z, m, y, False)
    b, _, m = S.gaussian_random_effects(comps, y, cp)
    off = np.concatenate([[0], np.cumsum(m)])
    vals = []
    for seed in range(1, 9):
        gm = _slope_model(gd, method="iterative")
        gm.set_optim_params({"cg_delta_conv": 1e-10, "seed_rand_vec_trace": seed})
        nll, grad, _ = gm.neg_log_likelihood_and_grad(cp, y)
        vals.append(np.concatenate([[nll], grad]))
        if seed == 1:   # the PCG-solved part
            out = gm.predict_training_data_random_effects()
            for c, (lev, _) in enumerate(comps):
                np.testing.assert_allclose(out[:, c], b[off[c] + lev], rtol=0, atol=1e-8 * np.abs(b).max())
    vals = np.array(vals)
    mean, se = vals.mean(0), vals.std(0, ddof=1) / np.sqrt(len(vals))
    want = np.concatenate([[ref], gref])
    stoch = [0, 2, 3, 4]   # the nll (log-determinant) and the traces of the three variance ratios
    ratio = np.abs(mean - want)[stoch] / se[stoch]
    print("iterative: |mean - cholesky| / standard error (nll, grad tau)", ratio, "relative se", (se / np.abs(want))[stoch])
    assert (ratio <= 6.0).all(), ratio
    # the sigma^2 entry -q / (2 sigma^2) + n / 2 has no stochastic part: the PCG solution alone
    assert np.abs(vals[:, 1] - gref[0]).max() <= 1e-8 * max(1.0, abs(gref[0]))


# ------------------------------------------------------------------------------------------------ Laplace
@pytest.mark.parametrize("method", ["cholesky", "iterative"])
def test_probit_r_values(pdat, method):
    it = method == "iterative"
    tol_nll = 1e-1 if it else 1e-3     # tolerance_loc_3
    tol_par = 1e-1 if it else 1e-6     # tolerance_loc_1
    y = pdat["y_slope"]
    gm = _slope_model(pdat, method=method, likelihood="bernoulli_probit")
    if it:
        gm.set_optim_params({"num_rand_vec_trace": 100})
    assert gm.cov_par_names() == ["Group_1", "Group_2", "Group_1_rand_coef_nb_1"]
    nll = gm.neg_log_likelihood([0.9, 0.8, 1.2], y)
    print(method, "nll", nll)
    assert abs(nll - 60.6422359) < tol_nll                                    # :897
    gp = np.array([[1, 2], [1, 1], [77, 98]])
    xp = np.array([0.0, 0.1, 0.3])
    with pytest.raises(GPBoostError, match="group_rand_coef_data_pred"):
        gm.predict(y=y, group_data_pred=gp, cov_pars=[0.9, 0.8, 1.2], predict_response=False)
    p = gm.predict(y=y, group_data_pred=gp, group_rand_coef_data_pred=xp, cov_pars=[0.9, 0.8, 1.2],
                   predict_var=not it, predict_response=False)                # :863-878
    assert np.abs(p["mu"] - [0.5195889, -0.6411954, 0.0]).sum() < 1e-3
    if not it:
        assert np.abs(p["var"] - [0.3422367, 0.3457334, 1.808]).sum() < tol_par
    gm = _slope_model(pdat, method=method, likelihood="bernoulli_probit")
    params = {"optimizer_cov": "lbfgs", "init_cov_pars": np.ones(3)}
    if it:
        params["num_rand_vec_trace"] = 100
    gm.fit(y, params=params)                                                  # :891-894
    print(method, "lbfgs", gm.get_cov_pars())
    assert np.abs(gm.get_cov_pars() - [0.3030687897, 0.9292636103, 0.3037924600]).sum() < tol_par


@pytest.mark.parametrize("method", ["cholesky", "iterative"])
def test_probit_r_gradient_descent(pdat, method):
    """test_GPModel_non_Gaussian_data.R:822-831: lr_cov = 0.2 without Nesterov acceleration, from (1, 1, 1)"""
    it = method == "iterative"
    gm = _slope_model(pdat, method=method, likelihood="bernoulli_probit")
    params = {"optimizer_cov": "gradient_descent", "init_cov_pars": np.ones(3), "lr_cov": 0.2, "use_nesterov_acc": False}
    if it:
        params["num_rand_vec_trace"] = 100
    gm.fit(pdat["y_slope"], params=params)
    print(method, gm.get_cov_pars(), gm.get_current_neg_log_likelihood(), gm.get_num_optim_iter())
    assert np.abs(gm.get_cov_pars() - [0.3060671, 0.9328884, 0.3146682]).sum() < (1e-1 if it else 1e-6)
    assert abs(gm.get_current_neg_log_likelihood() - 59.33113628) < (1e-1 if it else 1e-3)


def test_probit_r_gradient_descent_one_group_and_dropped_intercept(pdat):
    """:937-959, with Nesterov acceleration (the R package's default): one grouping variable and its slope, 100
    iterations (maxit); the dropped intercept, 18 iterations"""
    gm = GPModel(group_data=pdat["group"], group_rand_coef_data=pdat["x"], ind_effect_group_rand_coef=[1],
                 likelihood="bernoulli_probit", matrix_inversion_method="cholesky")
    gm.fit(pdat["y_one"], params={"optimizer_cov": "gradient_descent", "init_cov_pars": np.ones(2), "lr_cov": 0.1,
                                  "use_nesterov_acc": True, "maxit": 100})
    print("one group", gm.get_cov_pars(), gm.get_num_optim_iter())
    assert np.abs(gm.get_cov_pars() - [1.00742383, 0.02612587]).sum() < 1e-6
    assert gm.get_num_optim_iter() == 100
    gm = _slope_model(pdat, likelihood="bernoulli_probit", drop=[True, False])
    gm.fit(pdat["y_drop"], params={"optimizer_cov": "gradient_descent", "init_cov_pars": np.ones(2)})
    print("dropped", gm.get_cov_pars(), gm.get_num_optim_iter())
    assert np.abs(gm.get_cov_pars() - [1.0044712, 0.6549656]).sum() < 1e-3
    assert gm.get_num_optim_iter() == 18


def test_negative_binomial_slope_scaling(pdat, method="cholesky"):
    """The weighted negative-binomial shape passes (glp_nb_aux_kernel, the aux column of glp_q_kernel, Z^T dd1/dlog r)
    at weights other than one: the covariate 2 x with variance s / 4 is the model with x and s, so the nll and every
    gradient entry, the shape's included, agree at the Laplace tolerances (1e-9, 1e-7). Central differences are no
    yardstick for this entry: the library reproduces the reference's dW / dlog r (lik_device.h nb_dinfo_aux), which
    is not the derivative of W, and its values are pinned to the reference's by tests/test_gpu_grouped_negbin.py
    (measured here: shape entry -2.911 against a central difference of -3.757, and -3.072 against -3.818 for the
    same model without the slope). The weight-one identity above runs the same kernels bit for bit, iterative
    included."""
    y = S.laplace_response("poisson", pdat)
    res = []
    for f, s2 in ((1.0, [0.6, 0.9, 0.4]), (2.0, [0.6, 0.9, 0.1])):
        gm = GPModel(group_data=pdat["g12"], group_rand_coef_data=f * pdat["x"], ind_effect_group_rand_coef=[1],
                     likelihood="negative_binomial", matrix_inversion_method=method)
        gm.set_optim_params({"init_aux_pars": [1.7]})
        res.append(gm.neg_log_likelihood_and_grad(s2, y))
    (n1, g1, _), (n2, g2, _) = res
    assert g1.shape == (4,)
    print(method, "nll", n1, n2, "grad", g1, g2)
    assert abs(n1 - n2) <= 1e-9 * abs(n1)
    np.testing.assert_allclose(g2, g1, rtol=1e-7, atol=1e-7 * np.abs(g1).max())


@pytest.mark.parametrize("method", ["cholesky", "iterative"])
def test_shape_gradient_of_a_slope_model(pdat, method, lik="gamma"):
    """The shape entry of the gradient (the weighted shape-derivative kernel and traces) against central differences
    of the cholesky nll in log shape, h = 1e-3, mode finding at 1e-12. The differences carry a truncation error of
    O(h^2) = 1e-6 relative and the nll's stopping noise divided by 2 h, below 1e-5 (the argument of
    tests/test_grouped_slope_reference.py): cholesky within 2e-5 max(1, max|grad|). Iterative: a stochastic estimate,
    held to 6 standard errors of the mean over 8 seeds, plus the differences' own 2e-5."""
    y = S.laplace_response("gamma", pdat)
    s2, shape, h = np.array([0.6, 0.9, 0.4]), 1.7, 1e-3

    def model(seed=1):
        gm = _slope_model(pdat, method=method, likelihood=lik)
        gm.set_optim_params({"init_aux_pars": [shape], "estimate_aux_pars": True, "delta_conv_mode_finding": 1e-12,
                             "cg_delta_conv": 1e-10, "seed_rand_vec_trace": seed})
        return gm
    chol = _slope_model(pdat, method="cholesky", likelihood=lik)
    chol.set_optim_params({"delta_conv_mode_finding": 1e-12})
    fd = (chol.neg_log_likelihood(s2, y, aux_pars=[shape * np.exp(h)])
          - chol.neg_log_likelihood(s2, y, aux_pars=[shape * np.exp(-h)])) / (2 * h)
    if method == "cholesky":
        _, grad, _ = model().neg_log_likelihood_and_grad(s2, y)
        assert grad.shape == (4,)
        print(lik, "shape gradient", grad[3], "central difference", fd)
        assert abs(grad[3] - fd) <= 2e-5 * max(1.0, np.abs(grad).max())
    else:
        vals = np.array([model(seed).neg_log_likelihood_and_grad(s2, y)[1][3] for seed in range(1, 9)])
        se = vals.std(ddof=1) / np.sqrt(len(vals))
        print(lik, "iterative shape gradient", vals.mean(), "+-", se, "central difference (cholesky)", fd)
        assert abs(vals.mean() - fd) <= 6 * se + 2e-5 * max(1.0, abs(fd))


CASES = [("bernoulli_logit", None, None), ("poisson", None, None), ("gamma", None, None),
         ("bernoulli_probit", [True, False], None), ("bernoulli_probit", None, "one")]


@pytest.mark.parametrize("lik,drop,kind", CASES)
def test_laplace_against_restatement(pdat, lik, drop, kind):
    if kind == "one":      # one grouping variable and its slope (test_GPModel_non_Gaussian_data.R:938-941)
        groups, y, s2 = pdat["group"], pdat["y_one"], np.array([1.0, 0.4])
    elif drop:             # :951-956
        groups, y, s2 = pdat["g12"], pdat["y_drop"], np.array([0.8, 1.2])
    else:
        groups, y, s2 = pdat["g12"], S.laplace_response(lik, pdat), np.array([0.6, 0.9, 0.4])
    comps = S.components(groups, pdat["x"], [1], drop)
    gm = GPModel(group_data=groups, group_rand_coef_data=pdat["x"], ind_effect_group_rand_coef=[1],
                 drop_intercept_group_rand_effect=drop, likelihood=lik, matrix_inversion_method="cholesky")
    if lik == "gamma":
        gm.set_optim_params({"init_aux_pars": [1.7], "estimate_aux_pars": False})
    want_grad = lik != "bernoulli_probit"
    r = S.laplace(comps, y, s2, lik, aux=1.7, want_grad=want_grad)
    nll, grad, _ = gm.neg_log_likelihood_and_grad(s2, y)
    print(lik, drop, kind, "nll dev", abs(nll - r["nll"]) / abs(r["nll"]))
    assert abs(nll - r["nll"]) <= 1e-9 * abs(r["nll"])
    out = gm.predict_training_data_random_effects()
    off = np.concatenate([[0], np.cumsum(r["m"])])
    for c, (lev, _) in enumerate(comps):
        np.testing.assert_allclose(out[:, c], r["mode"][off[c] + lev], rtol=0, atol=1e-9 * np.abs(r["mode"]).max())
    if want_grad:
        print("grad dev", np.abs(grad - r["grad"]).max() / np.abs(r["grad"]).max())
        np.testing.assert_allclose(grad, r["grad"], rtol=1e-7, atol=1e-7 * np.abs(r["grad"]).max())
        gm.neg_log_likelihood_and_grad(s2, y)
        gf = gm.calc_gradient_f(calc_cov_factor=False)
        print("grad_f dev", np.abs(gf - r["grad_f"]).max())
        assert np.abs(gf - r["grad_f"]).max() <= 1e-7 * max(1.0, np.abs(r["grad_f"]).max())


def test_fit_with_covariates(pdat):
    """GLMM coefficients on a slope model: the coefficient gradient is X^T grad_F of the covariate-free path at the
    fitted offset (1e-12, the project's identity tolerance, tests/test_gpu_grouped_coef.py)"""
    n = pdat["n"]
    i = np.arange(1, n + 1)
    X = np.column_stack([np.ones(n), np.sin((i - n / 2) ** 2 * 2 * np.pi / n)])
    y = pdat["y_slope"]
    gm = _slope_model(pdat, likelihood="bernoulli_probit")
    gm.fit(y, X=X, params={"init_cov_pars": np.ones(3)})
    beta, cp = gm.get_coef(), gm.get_cov_pars()
    assert np.isfinite(beta).all() and np.isfinite(cp).all() and gm.get_num_optim_iter() > 0
    nll, gcov, gaux, gcoef = gm.neg_log_likelihood_and_grad_coef(cp, beta, y, X)
    plain = _slope_model(pdat, likelihood="bernoulli_probit")
    nll0, g0, _ = plain.neg_log_likelihood_and_grad(cp, y, fixed_effects=X @ beta)
    gf = plain.calc_gradient_f(fixed_effects=X @ beta, calc_cov_factor=False)
    assert abs(nll - nll0) <= 1e-12 * abs(nll0)
    np.testing.assert_allclose(gcov, g0, rtol=1e-12, atol=1e-12 * np.abs(g0).max())
    ref = X.T @ gf
    dev = np.abs(gcoef - ref) / (np.abs(X).T @ np.abs(gf))
    print("coefficient gradient", gcoef, "deviation / sum |X| |grad_F|", dev)
    assert (dev <= 1e-12).all()
    p = gm.predict(group_data_pred=np.array([[1, 2], [77, 98]]), group_rand_coef_data_pred=[0.1, 0.3],
                   X_pred=X[:2], predict_response=False)
    assert np.isfinite(p["mu"]).all() and abs(p["mu"][1] - X[1] @ beta) < 1e-12


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(gd):
    g12, x, n = gd["g12"], gd["x"], gd["n"]
    with pytest.raises(GPBoostError, match="drop_intercept_group_rand_effect"):     # more than one dropped intercept
        GPModel(group_data=g12, group_rand_coef_data=np.column_stack([x, x]), ind_effect_group_rand_coef=[1, 2],
                drop_intercept_group_rand_effect=[True, True])
    with pytest.raises(GPBoostError, match="drop_intercept_group_rand_effect"):     # an intercept without a slope
        GPModel(group_data=g12, group_rand_coef_data=x, ind_effect_group_rand_coef=[1],
                drop_intercept_group_rand_effect=[False, True])
    with pytest.raises(GPBoostError, match="group_rand_coef_data"):                 # the only component a slope
        GPModel(group_data=gd["group"], group_rand_coef_data=x, ind_effect_group_rand_coef=[1],
                drop_intercept_group_rand_effect=[True])
    with pytest.raises(GPBoostError, match="ind_effect_group_rand_coef"):
        GPModel(group_data=g12, group_rand_coef_data=x, ind_effect_group_rand_coef=[3])
    with pytest.raises(GPBoostError, match="ind_effect_group_rand_coef"):
        GPModel(group_data=g12, group_rand_coef_data=x, ind_effect_group_rand_coef=[0])
    bad = x.copy()
    bad[5] = np.nan
    with pytest.raises(GPBoostError, match="group_rand_coef_data"):
        GPModel(group_data=g12, group_rand_coef_data=bad, ind_effect_group_rand_coef=[1])
    bad[5] = np.inf
    with pytest.raises(GPBoostError, match="group_rand_coef_data"):
        GPModel(group_data=g12, group_rand_coef_data=bad, ind_effect_group_rand_coef=[1])
    coords = np.column_stack([x, x ** 2])
    with pytest.raises(GPBoostError, match="gp_rand_coef_data"):
        GPModel(gp_coords=coords, gp_rand_coef_data=x)
    with pytest.raises(GPBoostError, match="gp_coords"):                            # the combined model
        GPModel(group_data=g12, group_rand_coef_data=x, ind_effect_group_rand_coef=[1], gp_coords=coords,
                cov_function="exponential")
    with pytest.raises(GPBoostError, match="cluster_ids"):
        GPModel(group_data=g12, group_rand_coef_data=x, ind_effect_group_rand_coef=[1],
                cluster_ids=np.arange(n) % 2)
    gm = _slope_model(gd)
    with pytest.raises(GPBoostError, match="gp_rand_coef_data_pred"):
        gm.predict(y=gd["y_slope"], group_data_pred=g12[:2], group_rand_coef_data_pred=x[:2],
                   gp_rand_coef_data_pred=x[:2], cov_pars=[0.1, 1, 2, 1.5])
    with pytest.raises(GPBoostError, match="cluster_ids_pred"):
        gm.predict(y=gd["y_slope"], group_data_pred=g12[:2], group_rand_coef_data_pred=x[:2],
                   cluster_ids_pred=[0, 0], cov_pars=[0.1, 1, 2, 1.5])
    with pytest.raises(GPBoostError, match="covariates"):                           # Gaussian covariates stay refused
        gm.fit(gd["y_slope"], X=np.ones((n, 1)))
    it = _slope_model(gd, method="iterative")
    with pytest.raises(GPBoostError, match="iterative"):                            # and iterative predictive variances
        it.predict(y=gd["y_slope"], group_data_pred=g12[:2], group_rand_coef_data_pred=x[:2],
                   cov_pars=[0.1, 1, 2, 1.5], predict_var=True)
    plain = GPModel(group_data=g12, matrix_inversion_method="cholesky")
    with pytest.raises(GPBoostError, match="group_rand_coef_data_pred"):            # slope data for a model without
        plain.predict(y=gd["y_slope"], group_data_pred=g12[:2], group_rand_coef_data_pred=x[:2], cov_pars=[0.1, 1, 2])
