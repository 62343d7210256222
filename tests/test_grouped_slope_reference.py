"""CPU: the oracles of tests/grouped_slope_cases.py reproduce the reference's own R-test values for grouped random
slopes, so that the GPU tests (tests/test_gpu_grouped_slope.py) compare against a yardstick whose error is known.

R values: test_GPModel_grouped_random_effects.R:540-557 (nll 2335.803, predictions with a slope), :636-645 (the
dropped intercept), :164 (the single-level nll 2282.073, a check of the generator) and
test_GPModel_non_Gaussian_data.R:897 (probit nll 60.6422359 at (0.9, 0.8, 1.2)), at the R tests' tolerances: 1e-2 on
the nll, 1e-6 on the means, 1e-3 on the covariances, 1e-3 on the probit nll.

The oracle's own error: nll and gradient from the n x n Cholesky factor of Psi and from the M x M Woodbury form agree
to 1e-12 relative on every Gaussian case the GPU tests use.
"""
import numpy as np
import pytest

import grouped_slope_cases as S


@pytest.fixture(scope="module")
def gd():
    return S.gaussian_data()


def _gauss_cases(gd):
    g12 = np.column_stack([gd["group"], gd["group2"]])
    return {
        "slope": (S.components(g12, gd["x"], [1]), gd["y_slope"], [0.1, 1.0, 2.0, 1.5]),
        "drop": (S.components(g12, gd["x"], [1], [True, False]), gd["y_drop"], [0.1, 2.0, 1.5]),
        "single": (S.components(gd["group"]), gd["y_single"], [0.1, 1.0]),
        "slope_x2": (S.components(g12, 2.0 * gd["x"], [1]), gd["y_slope"], [0.5, 1.2, 0.9, 0.3]),
    }


def test_generator_and_data(gd):
    u = S.sim_rand_unif_r0(3, 0.546)
    assert u[0] == np.floor(0.546 * 134456) / 134456
    assert u[1] == ((8121 * np.floor(0.546 * 134456) + 28411) % 134456) / 134456
    assert gd["group"][[0, 9, 10, 999]].tolist() == [1, 1, 2, 100]
    assert gd["group2"][[0, 49, 50, 999]].tolist() == [1, 50, 1, 50]
    assert abs(gd["x"][0] - np.cos((1 - 500) ** 2 * 5.5 * np.pi / 1000)) == 0.0


def test_r_nll_values(gd):
    cases = _gauss_cases(gd)
    comps, y, cp = cases["slope"]
    Z, m = S.design(comps)
    assert m == [100, 50, 100]
    nll, _, _ = S.gaussian_nll_grad(Z, m, y, cp, "chol")
    print("slope nll", nll)
    assert abs(nll - 2335.803) < 1e-2           # :557
    assert abs(nll - 2335.803479) < 1e-5        # the value this restatement gave when it was written
    comps, y, cp = cases["single"]
    Z, m = S.design(comps)
    nll, _, _ = S.gaussian_nll_grad(Z, m, y, cp, "chol")
    print("single nll", nll)
    assert abs(nll - 2282.073) < 1e-2           # :164


def test_r_predictions_with_slope(gd):
    g12 = np.column_stack([gd["group"], gd["group2"]])
    gp = np.array([[1, 2], [1, 1], [101, 1001]])
    xp = np.array([0.0, 10.0, 0.3])
    comps = S.components(g12, gd["x"], [1])
    pts, same = S.pred_points(g12, gp, xp, [1])
    mu, cov = S.gaussian_predict(comps, gd["y_slope"], [0.1, 1.0, 2.0, 1.5], pts, same)
    exp_mu = np.array([0.7579961, -0.2868530, 0.0])
    exp_cov = np.array([0.11534086, -0.01988167, 0.0, -0.01988167, 2.4073302, 0.0, 0.0, 0.0, 3.235])
    print("mu", mu, "cov", cov.ravel())
    assert np.abs(mu - exp_mu).sum() < 1e-6      # :544-548
    assert np.abs(cov.ravel() - exp_cov).sum() < 1e-3
    np.testing.assert_allclose(mu[:2], [0.75799606, -0.28685298], atol=5e-9)
    np.testing.assert_allclose([cov[0, 0], cov[0, 1], cov[1, 1], cov[2, 2]],
                               [0.11534086, -0.01988167, 2.40733023, 3.235], atol=5e-9)


def test_r_predictions_dropped_intercept(gd):
    g12 = np.column_stack([gd["group"], gd["group2"]])
    gp = np.array([[1, 2], [1, 1], [101, 1001]])
    xp = np.array([0.0, 10.0, 0.3])
    drop = [True, False]
    comps = S.components(g12, gd["x"], [1], drop)
    assert len(comps) == 2 and comps[0][1] is None and comps[1][1] is not None   # [group2 intercept, slope on group]
    pts, same = S.pred_points(g12, gp, xp, [1], drop)
    mu, cov = S.gaussian_predict(comps, gd["y_drop"], [0.1, 2.0, 1.5], pts, same)
    exp_mu = np.array([0.8426751, -0.5964363, 0.0])
    exp_cov = np.array([0.10558205, -0.01269261, 0.0, -0.01269261, 2.40180871, 0.0, 0.0, 0.0, 2.235])
    print("mu", mu, "cov", cov.ravel())
    assert np.abs(mu - exp_mu).sum() < 1e-6      # :636-645
    assert np.abs(cov.ravel() - exp_cov).sum() < 1e-3


@pytest.mark.parametrize("name", ["slope", "drop", "single", "slope_x2"])
@pytest.mark.parametrize("profile", [False, True])
def test_oracle_forms_agree(gd, name, profile):
    comps, y, cp = _gauss_cases(gd)[name]
    Z, m = S.design(comps)
    n1, g1, s1 = S.gaussian_nll_grad(Z, m, y, cp, "chol", profile)
    n2, g2, s2 = S.gaussian_nll_grad(Z, m, y, cp, "woodbury", profile)
    dev = max(abs(n1 - n2) / abs(n1), np.abs(g1 - g2).max() / np.abs(g1).max(), abs(s1 - s2) / s1)
    print(name, profile, "forms differ by", dev)
    assert dev <= 1e-12


def test_gradient_is_the_derivative(gd):
    """central differences of the oracle's nll in the log parameters, as a check of the gradient formulas"""
    comps, y, cp = _gauss_cases(gd)["slope"]
    Z, m = S.design(comps)
    _, g, _ = S.gaussian_nll_grad(Z, m, y, cp, "woodbury")
    s2, tau = cp[0], np.array(cp[1:]) / cp[0]
    h = 1e-5
    for k in range(4):
        def at(e):
            ls2, lt = np.log(s2), np.log(tau).copy()
            if k == 0:
                ls2 += e
            else:
                lt[k - 1] += e
            return S.gaussian_nll_grad(Z, m, y, [np.exp(ls2)] + list(np.exp(lt) * np.exp(ls2)), "woodbury")[0]
        fd = (at(h) - at(-h)) / (2 * h)
        assert abs(fd - g[k]) <= 1e-6 * max(1.0, abs(g[k])), (k, fd, g[k])


def test_r_standard_deviations(gd):
    """the dense Fisher information gives the R test's standard deviations (:504) at the R fit's parameters, to the
    digits the R values carry (the parameters are given to 8 decimals: a relative 1e-6)"""
    g12 = np.column_stack([gd["group"], gd["group2"]])
    sd = S.gaussian_std_dev(S.components(g12, gd["x"], [1]), [0.49554952, 1.24880860, 1.05505134, 1.13840014])
    print("sd", sd)
    np.testing.assert_allclose(sd, [0.02546769, 0.18983953, 0.22337199, 0.17950490], rtol=1e-6)


def test_random_effects_equal_predictions(gd):
    """the consistency the R test checks (:511-536): predictions at x = 0 / 1 and at a new label of the other grouping
    variable give the random effects and their variances"""
    g12 = np.column_stack([gd["group"], gd["group2"]])
    comps = S.components(g12, gd["x"], [1])
    cp = [0.5, 1.2, 1.1, 1.1]
    b, var, m = S.gaussian_random_effects(comps, gd["y_slope"], cp)
    gu = np.arange(1, 101)
    gp = np.column_stack([gu, np.full(100, -1)])
    pts0, same0 = S.pred_points(g12, gp, np.zeros(100), [1])
    mu0, cov0 = S.gaussian_predict(comps, gd["y_slope"], cp, pts0, same0, predict_response=False)
    pts1, same1 = S.pred_points(g12, gp, np.ones(100), [1])
    mu1, _ = S.gaussian_predict(comps, gd["y_slope"], cp, pts1, same1, predict_response=False)
    assert np.abs(b[:100] - mu0).sum() < 1e-9
    assert np.abs(var[:100] - (np.diag(cov0) - cp[2])).sum() < 1e-9     # minus the new group2 label's variance
    assert np.abs(b[150:] - (mu1 - mu0)).sum() < 1e-9


def test_r_probit_nll():
    pd_ = S.probit_data()
    g12 = np.column_stack([pd_["group"], pd_["group2"]])
    comps = S.components(g12, pd_["x"], [1])
    r = S.laplace(comps, pd_["y_slope"], [0.9, 0.8, 1.2], "bernoulli_probit")
    print("probit nll", r["nll"], "its", r["its"])
    assert abs(r["nll"] - 60.6422359) < 1e-3     # test_GPModel_non_Gaussian_data.R:897


def test_weighted_restatement_at_weight_one_is_the_unweighted_one():
    import grouped_laplace_restatement as R
    pd_ = S.probit_data()
    g12 = np.column_stack([pd_["group"], pd_["group2"]])
    a = R.laplace_nll(g12, pd_["y_slope"], [0.7, 1.3], "bernoulli_logit")
    b = S.laplace(S.components(g12), pd_["y_slope"], [0.7, 1.3], "bernoulli_logit")
    assert a[0] == b["nll"] and a[1] == b["its"]


@pytest.mark.parametrize("lik", ["bernoulli_logit", "poisson", "gamma"])
def test_laplace_gradient_is_the_derivative(lik):
    """Central differences with h = 1e-3: their truncation error is O(h^2) = 1e-6 relative, and the restated nll
    carries the noise of its stopping rule (the Newton iteration ends once the objective stops increasing in floating
    point, which leaves about 1e-8 absolute in the nll, 1e-5 in the quotient): the bound is 2e-5 max(1, max|grad|)."""
    pd_ = S.probit_data()
    g12 = np.column_stack([pd_["group"], pd_["group2"]])
    comps = S.components(g12, pd_["x"], [1])
    y = S.laplace_response(lik, pd_)
    s2 = np.array([0.6, 0.9, 0.4])
    r = S.laplace(comps, y, s2, lik, aux=1.7, want_grad=True, delta=1e-14)
    h = 1e-3
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        fd = (S.laplace(comps, y, s2 * np.exp(e), lik, aux=1.7, delta=1e-14)["nll"]
              - S.laplace(comps, y, s2 * np.exp(-e), lik, aux=1.7, delta=1e-14)["nll"]) / (2 * h)
        assert abs(fd - r["grad"][k]) <= 2e-5 * max(1.0, np.abs(r["grad"]).max()), (lik, k, fd, r["grad"][k])
    off = np.zeros(100)
    i = 17
    off[i] = h
    fd = (S.laplace(comps, y, s2, lik, aux=1.7, offset=off, delta=1e-14)["nll"]
          - S.laplace(comps, y, s2, lik, aux=1.7, offset=-off, delta=1e-14)["nll"]) / (2 * h)
    assert abs(fd - r["grad_f"][i]) <= 2e-5 * max(1.0, np.abs(r["grad_f"]).max())
