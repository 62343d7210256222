"""CPU: the fixtures of the "pivoted_cholesky" preconditioner (tests/golden/golden_precond.json) are sound,
and the library's host form of the factorisation follows the rules.

A fixture is sound when its pivot sequence and rank do not depend on rounding: the numpy restatement
(tests/golden/piv_chol_restatement.py) run plain and run perturbed (covariance in longdouble, dot products
accumulated backwards) on the case's points in Vecchia order must agree, and agree with what the generator
recorded. The library's host form (GPB_PivotedCholeskyHost, the rules the device kernels follow: first
maximum in position order, the 1e-12 rule, the early stop) is compared with the restatement on the
early-stop case, on the short-range exponential case and on a still shorter range (0.02) at which far
points have l^2 below one ulp of the variance, so that remaining diagonals tie exactly after step 0 too and
the tie rule (lowest position of the permutation, not lowest row index) decides pivots.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from piv_chol_restatement import STOP_TOL, pivoted_cholesky  # noqa: E402

from gpboost_amd import synthetic  # noqa: E402
from oracle import oracle as O  # noqa: E402

with open(os.path.join(HERE, "golden", "golden_precond.json")) as _f:
    GOLDEN = json.load(_f)
RANK = 50


def _points(case):
    X = synthetic.bench_coords(case["n"])
    perm = O.vecchia_order(case["n"], 0, True)
    var, phi = O.transform_latent(O.cov_code(case["cov_fct"], case["shape"]), case["cov_pars"])
    return np.ascontiguousarray(X[perm]), float(var), float(phi)


@pytest.mark.parametrize("name", list(GOLDEN))
def test_fixture_pivots_do_not_depend_on_rounding(name):
    case = GOLDEN[name]
    xv, var, phi = _points(case)
    _, piv_a, rank_a = pivoted_cholesky(xv, case["cov_fct"], case["shape"], var, phi, RANK)
    _, piv_b, rank_b = pivoted_cholesky(xv, case["cov_fct"], case["shape"], var, phi, RANK, perturbed=True)
    assert piv_a == piv_b and rank_a == rank_b
    assert piv_a == case["pivots"] and rank_a == case["rank"]


def test_early_stop_fixture_stops_early():
    assert GOLDEN["pois_early_stop"]["rank"] < RANK
    assert all(GOLDEN[k]["rank"] == RANK for k in GOLDEN if k != "pois_early_stop")


def _host(xv, cov_code, var, phi, k):
    from gpboost_amd import basic
    n, d = xv.shape
    k = min(k, n)
    L = np.zeros((n, k))
    piv = np.zeros(k, dtype=np.int32)
    rank = ctypes.c_int(0)
    D = ctypes.POINTER(ctypes.c_double)
    ret = basic.lib().GPB_PivotedCholeskyHost(
        xv.ctypes.data_as(D), ctypes.c_int(n), ctypes.c_int(d), ctypes.c_int(cov_code), ctypes.c_double(var),
        ctypes.c_double(phi), ctypes.c_int(k), ctypes.c_double(STOP_TOL), L.ctypes.data_as(D),
        piv.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(rank))
    assert ret == 0
    return L, piv[:rank.value].tolist(), rank.value


@pytest.mark.parametrize("name", ["pois_early_stop", "logit_short"])
def test_host_factorisation_follows_the_restatement(name):
    case = GOLDEN[name]
    xv, var, phi = _points(case)
    L_ref, piv_ref, rank_ref = pivoted_cholesky(xv, case["cov_fct"], case["shape"], var, phi, RANK)
    L, piv, rank = _host(xv, O.cov_code(case["cov_fct"], case["shape"]), var, phi, RANK)
    assert rank == rank_ref and piv == piv_ref
    assert np.all(L[:, rank:] == 0.)                         # columns beyond the reached rank stay zero
    # both are float64 with forward dots; they differ by the rounding of exp / sqrt (1.1e-16), which a step
    # amplifies by at most 1 / sqrt(pivot) <= sqrt(n / STOP_TOL) < 2e4 here, over <= 50 steps: < 1e-9
    np.testing.assert_allclose(L, L_ref, rtol=0, atol=1e-9 * np.sqrt(var))
    # a valid partial factor: the Schur complement's diagonal is what the loop tracked
    resid = var - (L * L).sum(axis=1)
    assert resid.min() > -1e-12
    if rank < RANK:
        assert np.abs(np.delete(resid, piv)).sum() <= STOP_TOL


def test_host_factorisation_rank_above_n_is_clipped():
    xv = np.ascontiguousarray(synthetic.bench_coords(7))
    L, piv, rank = _host(xv, 0, 1.0, 10.0, 7)
    assert rank == 7 and sorted(piv) == list(range(7))
    S = np.exp(-10.0 * np.sqrt(((xv[:, None, :] - xv[None, :, :]) ** 2).sum(axis=2)))
    np.testing.assert_allclose(L @ L.T, S, atol=1e-12)


def test_host_factorisation_breaks_exact_ties_by_position():
    """Range 0.02 on the n = 600 points: exp(-50 r) squared is below one ulp of the variance for r > 0.37, so
    after every step most remaining diagonals are still exactly equal. First maximum in position order: the
    pivots equal the restatement's (np.argmax returns the first maximum) and are not the lowest row indices."""
    xv, _, _ = _points(GOLDEN["logit_short"])
    var, phi = (float(v) for v in O.transform_latent(0, [1.0, 0.02]))
    d0 = np.sqrt(((xv - xv[0]) ** 2).sum(axis=1))
    l = var * np.exp(-phi * d0) / np.sqrt(var)
    assert np.count_nonzero(var - l * l == var) > 100     # exact ties after step 0
    L_ref, piv_ref, rank_ref = pivoted_cholesky(xv, "exponential", 0.5, var, phi, RANK)
    L, piv, rank = _host(xv, 0, var, phi, RANK)
    assert rank == rank_ref == RANK and piv == piv_ref
    assert piv[0] == 0 and piv != sorted(piv)
    np.testing.assert_allclose(L, L_ref, rtol=0, atol=1e-9)
