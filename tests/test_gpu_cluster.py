"""GP models with several clusters (cluster_ids): independent realisations that share the covariance parameters.

References: exact identities (the six sums are additive over the clusters, so the clustered model equals single-cluster
GPModels combined by the same formula) and the R test's own numbers (tests/cluster_cases.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARS = [0.3, 1.2, 0.15]
GD = {"optimizer_cov": "gradient_descent", "lr_cov": 0.1, "use_nesterov_acc": True, "acc_rate_cov": 0.5,
      "delta_rel_conv": 1e-6}


def _close(a, b, rtol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1.0))


def _data(sizes):
    from gpboost_amd import synthetic
    n = int(sum(sizes))
    ids = np.repeat(np.arange(len(sizes)) + 1, sizes)
    return synthetic.bench_coords(n), synthetic.bench_gaussian_y(n), ids


DENSE_CASES = {"two": (40, 60), "mixed": (64, 65, 300, 7), "many": (25,) * 400}
VECCHIA_CASES = {"two": (40, 60), "three": (20, 31, 200)}


def _identity(X, y, ids, pars, **kw):
    """nll and gradient of both profile modes from single-cluster GPModels: at one sigma^2 the nll and the gradient
    are sums over the clusters; the profiled sigma^2 is sum_c q_c / n with q_c read off the nugget's gradient entry,
    and the profiled values are the sums at the parameters rescaled to it"""
    from gpboost_amd import GPModel
    parts = [(GPModel(gp_coords=X[r], cov_function="exponential", **kw), y[r]) for _, r in cc.split(ids)]

    def total(p):
        nll, grad = 0., np.zeros(3)
        for gm, yc in parts:
            a = gm.neg_log_likelihood_and_grad(p, yc)
            nll += a[0]
            grad += np.asarray(a[1])
        return nll, grad

    n = y.size
    nll0, g0 = total(pars)
    q = (n / 2. - g0[0]) * 2. * pars[0]
    s2 = q / n
    nll1, g1 = total([s2, pars[1] / pars[0] * s2, pars[2]])
    return (nll0, g0), (nll1, g1[1:], s2)


def _clustered(X, y, ids, pars, **kw):
    from gpboost_amd import GPModel
    gm = GPModel(gp_coords=X, cov_function="exponential", cluster_ids=ids, **kw)
    a = gm.neg_log_likelihood_and_grad(pars, y)
    b = gm.neg_log_likelihood_and_grad(pars, y, profile_sigma2=True)
    return gm, (a[0], np.asarray(a[1])), (b[0], np.asarray(b[1]), b[2])


def _assert_identity(got, want):
    (n0, g0), (n1, g1, s2) = got
    (rn0, rg0), (rn1, rg1, rs2) = want
    assert abs(n0 - rn0) <= 1e-8 * abs(rn0), (n0, rn0)
    assert _close(g0, rg0, 1e-7), (g0, rg0)
    assert abs(n1 - rn1) <= 1e-8 * abs(rn1), (n1, rn1)
    assert _close(g1, rg1, 1e-7), (g1, rg1)
    assert abs(s2 - rs2) <= 1e-8 * abs(rs2)


def test_two_clusters_construct_and_evaluate():
    """refused with "out of scope" before clusters were supported"""
    from gpboost_amd import GPModel
    X, y, ids = cc.r_data()
    gm = GPModel(gp_coords=X, cluster_ids=[1] * 40 + [2] * 60)
    assert np.isfinite(gm.neg_log_likelihood([0.1, 1., 0.15], y))
    assert gm.cluster_info() == (2, 2, 0)


@pytest.fixture(scope="module")
def dense_identity():
    out = {}
    for name, sizes in DENSE_CASES.items():
        X, y, ids = _data(sizes)
        out[name] = _identity(X, y, ids, PARS, gp_approx="none")
    return out


@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_dense_additivity(dense_identity, name):
    X, y, ids = _data(DENSE_CASES[name])
    gm, a, b = _clustered(X, y, ids, PARS, gp_approx="none")
    C = len(DENSE_CASES[name])
    small = sum(1 for s in DENSE_CASES[name] if s <= 64)
    assert gm.cluster_info() == (C, small, C - small)
    _assert_identity((a, b), dense_identity[name])
    nll = gm.neg_log_likelihood(PARS, y)
    assert abs(nll - a[0]) <= 1e-12 * abs(nll)
    assert abs(gm.get_current_neg_log_likelihood() - nll) <= 1e-12 * abs(nll)


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_gpu_cluster as T
out = {{}}
for name, sizes in T.DENSE_CASES.items():
    X, y, ids = T._data(sizes)
    gm, a, b = T._clustered(X, y, ids, T.PARS, gp_approx="none")
    out[name] = dict(info=gm.cluster_info(), a=[a[0], a[1].tolist()], b=[b[0], b[1].tolist(), b[2]])
print("RESULT " + json.dumps(out))
"""


def test_dense_additivity_without_the_batched_kernel(dense_identity):
    """GPBOOST_AMD_NO_CLUSTER_BATCH=1 (read when a model is created) in a fresh process: every cluster has an engine
    of its own, and the same identity holds"""
    env = dict(os.environ, GPBOOST_AMD_NO_CLUSTER_BATCH="1")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    for name, sizes in DENSE_CASES.items():
        o = out[name]
        assert tuple(o["info"]) == (len(sizes), 0, len(sizes))
        _assert_identity(((o["a"][0], np.array(o["a"][1])), (o["b"][0], np.array(o["b"][1]), o["b"][2])),
                         dense_identity[name])


@pytest.mark.parametrize("name", list(VECCHIA_CASES))
def test_vecchia_additivity(name):
    X, y, ids = _data(VECCHIA_CASES[name])
    kw = dict(gp_approx="vecchia", num_neighbors=30, vecchia_ordering="none")
    gm, a, b = _clustered(X, y, ids, PARS, **kw)
    _assert_identity((a, b), _identity(X, y, ids, PARS, **kw))


def test_vecchia_small_clusters_are_exact():
    """clusters of at most m + 1 points are exact under Vecchia: batched, and equal to the dense model"""
    X, y, ids = _data((20, 31, 9))
    gm, a, b = _clustered(X, y, ids, PARS, gp_approx="vecchia", num_neighbors=30, vecchia_ordering="random")
    assert gm.cluster_info() == (3, 3, 0)
    _, ad, bd = _clustered(X, y, ids, PARS, gp_approx="none")
    assert a[0] == ad[0] and np.array_equal(a[1], ad[1]) and b[0] == bd[0]


def test_interleaved_ids_equal_sorted_data():
    from gpboost_amd import GPModel
    X, y, _ = cc.r_data()
    ids = np.arange(100) % 2 + 1
    a = GPModel(gp_coords=X, cov_function="exponential", cluster_ids=ids).neg_log_likelihood(PARS, y)
    o = np.argsort(ids, kind="stable")
    b = GPModel(gp_coords=X[o], cov_function="exponential", cluster_ids=ids[o]).neg_log_likelihood(PARS, y[o])
    assert a == b
    for approx in ("none", "vecchia"):
        kw = dict(gp_approx=approx, num_neighbors=10, vecchia_ordering="none")
        a = GPModel(gp_coords=X, cov_function="matern", cov_fct_shape=1.5, cluster_ids=ids, **kw)
        b = GPModel(gp_coords=X[o], cov_function="matern", cov_fct_shape=1.5, cluster_ids=ids[o], **kw)
        va, vb = a.neg_log_likelihood(PARS, y), b.neg_log_likelihood(PARS, y[o])
        assert abs(va - vb) <= 1e-12 * abs(vb)


def test_r_dense_predictions():
    from gpboost_amd import GPModel
    X, y, ids = cc.r_data()
    gm = GPModel(gp_coords=X, cov_function="exponential", cluster_ids=ids)
    p = gm.predict(y=y, gp_coords_pred=cc.R_PRED_X, cluster_ids_pred=cc.R_PRED_IDS, cov_pars=cc.R_PARS,
                   predict_cov_mat=True)
    print("mu", p["mu"], "cov", p["cov"])
    assert np.sum(np.abs(p["mu"] - cc.R_PRED_MEAN)) < 1e-6
    assert np.sum(np.abs(p["cov"] - cc.R_PRED_COV)) < 1e-6
    p = gm.predict(y=y, gp_coords_pred=cc.R_PRED_X, cluster_ids_pred=cc.R_PRED_IDS, cov_pars=cc.R_PARS,
                   predict_var=True)
    assert np.sum(np.abs(p["mu"] - cc.R_PRED_MEAN)) < 1e-6
    assert np.sum(np.abs(p["var"] - np.diag(cc.R_PRED_COV))) < 1e-6
    # the latent process: no nugget, also for the cluster without training data
    p = gm.predict(y=y, gp_coords_pred=cc.R_PRED_X, cluster_ids_pred=cc.R_PRED_IDS, cov_pars=cc.R_PARS,
                   predict_var=True, predict_response=False)
    assert np.sum(np.abs(p["var"] - (np.diag(cc.R_PRED_COV) - 0.1))) < 1e-6
    # saved prediction data
    gm.set_prediction_data(gp_coords_pred=cc.R_PRED_X, cluster_ids_pred=cc.R_PRED_IDS)
    q = gm.predict(y=y, cov_pars=cc.R_PARS, predict_cov_mat=True, use_saved_data=True)
    assert np.sum(np.abs(q["cov"] - cc.R_PRED_COV)) < 1e-6


def test_r_dense_gradient_descent_fit():
    from gpboost_amd import GPModel
    X, y, ids = cc.r_data()
    gm = GPModel(gp_coords=X, cov_function="exponential", cluster_ids=ids)
    gm.fit(y, params=dict(GD, convergence_criterion="relative_change_in_parameters"))
    est = np.asarray(gm.get_cov_pars()).reshape(-1)[:3]
    print("iterations", gm.get_num_optim_iter(), "estimates", est, np.sum(np.abs(est - cc.R_GD_PARS)))
    assert gm.get_num_optim_iter() == cc.R_GD_ITERS
    assert np.sum(np.abs(est - cc.R_GD_PARS)) < 1e-6
    init = np.asarray(gm.get_init_cov_pars()).reshape(-1)
    t = cc.init_pars(X, y, ids)
    assert np.allclose(init, [t[0], t[1] * t[0], 1. / t[2]], rtol=1e-12)


def test_r_vecchia_predictions_and_fit():
    from gpboost_amd import GPModel
    X, y, ids = cc.r_data()
    kw = dict(gp_coords=X, cov_function="exponential", gp_approx="vecchia", num_neighbors=30, vecchia_ordering="none",
              cluster_ids=ids)
    gm = GPModel(**kw)
    gm.set_prediction_data(vecchia_pred_type="order_obs_first_cond_all", num_neighbors_pred=30)
    p = gm.predict(y=y, gp_coords_pred=cc.R_VPRED_X, cluster_ids_pred=cc.R_PRED_IDS, cov_pars=cc.R_PARS,
                   predict_cov_mat=True)
    print("mu", p["mu"], "cov", p["cov"])
    assert np.sum(np.abs(p["mu"] - cc.R_VPRED_MEAN)) < 1e-6
    assert np.sum(np.abs(p["cov"] - cc.R_VPRED_COV)) < 1e-6
    gm = GPModel(**kw)
    gm.fit(y, params=dict(GD, convergence_criterion="relative_change_in_log_likelihood"))
    print("vecchia fit nll", gm.get_current_neg_log_likelihood(), gm.get_cov_pars())
    assert abs(gm.get_current_neg_log_likelihood() - cc.R_VGD_NLL) < 1e-2


@pytest.mark.parametrize("optimizer", ["lbfgs", "nelder_mead"])
def test_other_optimizers_reach_the_optimum(optimizer):
    from gpboost_amd import GPModel
    X, y, ids = cc.r_data()
    gm = GPModel(gp_coords=X, cov_function="exponential", cluster_ids=ids)
    gm.fit(y, params={"optimizer_cov": optimizer})
    nll = gm.get_current_neg_log_likelihood()
    est = np.asarray(gm.get_cov_pars()).reshape(-1)[:3]
    print(optimizer, "nll", nll, "estimates", est, "iterations", gm.get_num_optim_iter())
    assert nll <= cc.R_GD_NLL_ORACLE + 1e-4
    if optimizer == "lbfgs":
        g = gm.neg_log_likelihood_and_grad(est, y, profile_sigma2=True)[1]
        assert np.linalg.norm(g) < 1e-3, g


def test_gradient_descent_without_nesterov_and_offset():
    from gpboost_amd import GPModel
    X, y, ids = cc.r_data()
    gm = GPModel(gp_coords=X, cov_function="exponential", cluster_ids=ids)
    gm.fit(y, params=dict(GD, use_nesterov_acc=False))
    assert gm.get_current_neg_log_likelihood() <= cc.R_GD_NLL_ORACLE + 1e-2
    off = 0.5 * np.sin(np.arange(100.))
    a = gm.neg_log_likelihood_and_grad(PARS, y + off, fixed_effects=off)
    b = gm.neg_log_likelihood_and_grad(PARS, y)
    assert abs(a[0] - b[0]) <= 1e-10 * abs(b[0]) and _close(a[1], b[1], 1e-9)


def test_string_ids_equal_integer_ids():
    from gpboost_amd import GPModel
    X, y, ids = cc.r_data()
    names = np.array(["a" if v == 1 else "b" for v in ids])
    gi = GPModel(gp_coords=X, cov_function="exponential", cluster_ids=ids)
    gs = GPModel(gp_coords=X, cov_function="exponential", cluster_ids=names)
    assert gi.neg_log_likelihood(PARS, y) == gs.neg_log_likelihood(PARS, y)
    pi = gi.predict(y=y, gp_coords_pred=cc.R_PRED_X, cluster_ids_pred=[1, 3, 1], cov_pars=cc.R_PARS,
                    predict_cov_mat=True)
    ps = gs.predict(y=y, gp_coords_pred=cc.R_PRED_X, cluster_ids_pred=["a", "new", "a"], cov_pars=cc.R_PARS,
                    predict_cov_mat=True)
    assert np.array_equal(pi["mu"], ps["mu"]) and np.array_equal(pi["cov"], ps["cov"])


def test_one_distinct_id_is_the_model_without_ids():
    from gpboost_amd import GPModel
    X, y, _ = cc.r_data()
    for kw in (dict(gp_approx="none"), dict(gp_approx="vecchia", num_neighbors=15, vecchia_ordering="random")):
        a = GPModel(gp_coords=X, cov_function="exponential", **kw)
        b = GPModel(gp_coords=X, cov_function="exponential", cluster_ids=[5] * 100, **kw)
        ra, rb = a.neg_log_likelihood_and_grad(PARS, y), b.neg_log_likelihood_and_grad(PARS, y)
        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1])
        pa = a.predict(y=y, gp_coords_pred=cc.R_PRED_X, cov_pars=cc.R_PARS, predict_var=True)
        pb = b.predict(y=y, gp_coords_pred=cc.R_PRED_X, cov_pars=cc.R_PARS, predict_var=True)
        assert np.array_equal(pa["mu"], pb["mu"]) and np.array_equal(pa["var"], pb["var"])
        assert b.cluster_info() == (1, 0, 0)


def test_refusals_name_their_option():
    from gpboost_amd import GPBoostError, GPModel
    X, y, ids = cc.r_data()
    gm = GPModel(gp_coords=X, cov_function="exponential", cluster_ids=ids)
    with pytest.raises(GPBoostError, match="cluster_ids_pred"):
        gm.predict(y=y, gp_coords_pred=cc.R_PRED_X, cov_pars=cc.R_PARS)
    with pytest.raises(GPBoostError, match="likelihood"):
        GPModel(gp_coords=X, cluster_ids=ids, likelihood="bernoulli_probit")
    for approx in ("vecchia_latent", "fitc", "full_scale_vecchia"):
        with pytest.raises(GPBoostError, match="gp_approx"):
            GPModel(gp_coords=X, cluster_ids=ids, gp_approx=approx)
    with pytest.raises(GPBoostError, match="covariates"):
        gm.fit(y, X=np.ones((100, 1)))
    with pytest.raises(GPBoostError, match="fisher_scoring"):
        gm.fit(y, params={"optimizer_cov": "fisher_scoring"})
    gm.set_optim_params({"optimizer_cov": "lbfgs"})
    gm.neg_log_likelihood(PARS, y)
    with pytest.raises(GPBoostError, match="std_err"):
        gm.get_cov_pars(std_err=True)
    with pytest.raises(GPBoostError, match="predict_training_data_random_effects"):
        gm.predict_training_data_random_effects()
    with pytest.raises(GPBoostError, match="GPB_OptimCovParBoosting"):
        gm.optim_cov_par_boosting(y=y)
    with pytest.raises(GPBoostError, match="GPB_CalcGradientF"):
        gm.calc_gradient_f(y=y)
    with pytest.raises(GPBoostError, match="multi-rank"):
        gm.set_distributed_host(0, 1, lambda buf: buf)
    with pytest.raises(GPBoostError, match="cluster"):
        GPModel(gp_coords=X, group_data=np.arange(100) % 5, cluster_ids=ids)
