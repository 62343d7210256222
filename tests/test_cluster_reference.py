"""The references of the cluster tests (tests/cluster_cases.py), checked without a GPU: the numpy restatements
reproduce the R test's numbers, and the float64 stand-in of the batched kernel is measured against longdouble."""
import numpy as np
import pytest

import cluster_cases as cc
from oracle.internal_optim_oracle import internal_optimize


def test_split_keeps_first_appearance_and_row_order():
    parts = cc.split([7, 3, 7, 7, 3, 9])
    assert [k for k, _ in parts] == [7, 3, 9]
    assert [r.tolist() for _, r in parts] == [[0, 2, 3], [1, 4], [5]]


def test_r_prediction_values():
    """test_GPModel_gaussian_process.R:599-641: mean, covariance and variances, the R test's strict 1e-6 on each sum
    of absolute differences; the unseen cluster 3 gets mean 0 and the prior variance plus the nugget"""
    X, y, ids = cc.r_data()
    mean, cov = cc.dense_predict(X, y, ids, cc.R_PARS, cc.R_PRED_X, cc.R_PRED_IDS)
    print("mean", mean, "cov", cov)
    assert np.sum(np.abs(mean - cc.R_PRED_MEAN)) < 1e-6
    assert np.sum(np.abs(cov - cc.R_PRED_COV)) < 1e-6
    assert np.sum(np.abs(np.diag(cov) - np.diag(cc.R_PRED_COV))) < 1e-6


def test_r_gradient_descent_fit():
    """the R test's gradient-descent fit by the oracle loop on the two-cluster model object: exactly 247 iterations,
    estimates within 1e-6 (summed)"""
    X, y, ids = cc.r_data()
    model = cc.ClusterSum(X, y, ids, 0)
    pars, nll, num_it = internal_optimize(model, cc.init_pars(X, y, ids), "gradient_descent", lr=0.1, acc_rate=0.5,
                                          nesterov=True, delta=1e-6, crit_params=True)
    est = np.array([pars[0], pars[1] * pars[0], cc.range_back(0, pars[2])])
    print("iterations", num_it, "estimates", est, "summed difference", np.sum(np.abs(est - cc.R_GD_PARS)), "nll", nll)
    assert num_it == cc.R_GD_ITERS
    assert np.sum(np.abs(est - cc.R_GD_PARS)) < 1e-6
    assert abs(nll - cc.R_GD_NLL_ORACLE) < 1e-6


def test_cluster_sums_are_the_sums_of_the_stand_in():
    """ClusterSum (LAPACK) and the kernel's algebra (batch_compute) agree on the six sums of the R data"""
    X, y, ids = cc.r_data()
    pars = np.array([0.1, 10., 1. / 0.15])
    a = cc.ClusterSum(X, y, ids, 0).sums(pars)
    b = np.zeros(6)
    for _, rows in cc.split(ids):
        b += cc.batch_compute(X[rows], y[rows], pars[1], pars[2], 0, 1, np.float64)[0]
    assert np.allclose(a, b, rtol=1e-10, atol=1e-10), (a, b)


@pytest.mark.parametrize("name", [c["name"] for c in cc.op_cases()])
def test_stand_in_against_longdouble(name):
    """the stand-in's own error, which sets the kernel's allowance (8 times it): Psi = var corr + I has its smallest
    eigenvalue >= 1 and its largest <= 1 + 64 var, so a backward-stable factorisation of at most 64 rows errs by a
    small multiple of 64 (1 + 64 var) 2^-53 ~ 1e-12 relative; 1e-10 of the output's largest entry bounds it with room"""
    ref, uref, info, allow, err = cc.case_reference(name)
    assert not info.any()
    scale = {k: float(np.max(np.abs(ref[:, j]))) for j, k in enumerate(cc.OUTPUTS[:6])}
    scale["u"] = float(np.max(np.abs(uref)))
    print(name, {k: (err[k], err[k] / scale[k] if scale[k] else 0.) for k in cc.OUTPUTS})
    for k in cc.OUTPUTS:
        assert np.isfinite(allow[k])
        assert err[k] <= 1e-10 * max(scale[k], 1e-300), (k, err[k], scale[k])
    c = cc._case_by_name(name)
    if not c["want_grad"]:
        assert np.all(ref[:, 2:] == 0)


def test_not_positive_definite_case_flags_one_cluster():
    ref, uref, info, allow, err = cc.case_reference("not_pd")
    assert info.tolist() == [0, 1, 0, 0]
    assert np.all(np.isfinite(ref[info == 0].astype(float)))
