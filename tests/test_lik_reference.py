"""CPU: the references and bounds of tests/lik_cases.py, without a GPU.

* A float64 stand-in (math / numpy) of the formulas lik_device.h evaluates meets every bound on the main grid and
  on the tail sets, and so do float64 stand-ins of the path kernels' derived arrays and sums. Run with -s for the
  largest error / bound per likelihood and quantity. On this suite's CPU (glibc libm): main grid at most 0.47
  (logit loglik), 0.44 (Gaussian d1), 0.37 (probit loglik), 0.34 (Poisson loglik), 0.38 (gamma loglik); tail sets at
  most 0.44 (probit dinfo at l = -38.4, y = 0) and 0.43 (gamma info at l = 745).
* The header as it was before these tests (erfc until it returns 0 and three series terms; p (1 - p), y - p and
  y l - softplus(l)) exceeds the bounds: logit info by 8e13 on the main grid (l = 35.5, y = 0) and probit info by
  2e11 on the tail set (the denormal erfc band, l = 38.5, y = 0).
* Informativeness: on the main grid no (point, quantity) has a bound above 1e-3 scale (scales: lik_cases.py).
* Every planted defect exceeds a bound somewhere.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lik_cases as lc  # noqa: E402

LIKS = sorted(lc.LIK_NAMES)


def setup_module(module):
    lc.assert_longdouble()


def _grid_ratios(si, lik, which):
    """largest error / bound per quantity of a stand-in on a grid"""
    worst = {q: 0. for q in lc.QUANTS}
    for aux, y, l, ref in lc.grid_reference(lik, which):
        got = si.points(lik, aux, y, l)
        for q in lc.QUANTS:
            worst[q] = max(worst[q], float(ref.ratios(q, got[q]).max()))
    return worst


@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("which", ["main", "tail"])
def test_standin_meets_every_bound(lik, which):
    worst = _grid_ratios(lc.StandIn(), lik, which)
    print(f"[lik reference] {lc.LIK_NAMES[lik]} {which}: " + ", ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    for q, v in worst.items():
        assert v < 1., (lc.LIK_NAMES[lik], which, q, v)


def test_original_formulas_exceed_the_bounds():
    """the header before the fixes: the one-sided logit cancellation on the main grid, the denormal erfc band of
    the probit functions on the tail set"""
    orig = lc.StandIn(original=True)
    logit = _grid_ratios(orig, lc.LOGIT, "main")
    print("[lik reference] original logit, main grid: " + ", ".join(f"{q} {v:.3g}" for q, v in logit.items()))
    for q in lc.QUANTS:
        assert logit[q] > 1e6, (q, logit[q])
    probit = _grid_ratios(orig, lc.PROBIT, "tail")
    print("[lik reference] original probit, tail set: " + ", ".join(f"{q} {v:.3g}" for q, v in probit.items()))
    for q in ("d1", "info", "dinfo"):
        assert probit[q] > 1e6, (q, probit[q])
    # the information is even in l exactly (info(l, y = 1) = info(-l, y = 0)); the original logit form is not
    l = np.array([20., 30., 36.])
    a = orig.points(lc.LOGIT, 1., np.ones(3), l)["info"]
    b = orig.points(lc.LOGIT, 1., np.zeros(3), -l)["info"]
    assert (a != b).all()
    new = lc.StandIn()
    for lik in (lc.LOGIT, lc.PROBIT):
        ls = np.concatenate([lc.MAIN_L, lc.BERNOULLI_TAIL_L])
        a = new.points(lik, 1., np.ones(ls.size), ls)["info"]
        b = new.points(lik, 1., np.zeros(ls.size), -ls)["info"]
        assert np.array_equal(a, b)


@pytest.mark.parametrize("lik", LIKS)
def test_bounds_are_informative(lik):
    worst = {q: 0. for q in lc.QUANTS}
    for aux, y, l, ref in lc.grid_reference(lik, "main"):
        for q in lc.QUANTS:
            sc, b = ref.scale(q), ref.bound[q]
            assert np.isfinite(b).all()
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(b <= 1e-3 * sc, np.where(sc > 0, b / sc, 0.), np.inf)
            worst[q] = max(worst[q], float(rel.max()))
    print(f"[lik reference] {lc.LIK_NAMES[lik]} largest bound / scale: " + ", ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    for q, v in worst.items():
        assert v <= 1e-3, (lc.LIK_NAMES[lik], q, v)


def test_tail_references_overflow_where_they_must():
    """Poisson / gamma at +-700 and +-745: the exact values beyond the double range are the infinities the test
    expects; the stand-in gives exactly those and never a NaN"""
    n_inf = 0
    for lik in (lc.POISSON, lc.GAMMA):
        for aux, y, l, ref in lc.grid_reference(lik, "tail"):
            got = lc.StandIn().points(lik, aux, y, l)
            for q in lc.QUANTS:
                assert not np.isnan(got[q]).any()
                fin = ref.representable(q)
                n_inf += int((~fin).sum())
                assert np.array_equal(np.isinf(got[q]), ~fin)
    assert n_inf > 0


@pytest.mark.parametrize("defect", lc.POINT_DEFECTS)
def test_planted_point_defect_exceeds_a_bound(defect):
    lik = {"probit-branches": lc.PROBIT, "mills": lc.PROBIT, "series-sign": lc.PROBIT, "2p-1": lc.LOGIT,
           "gamma-aux": lc.GAMMA, "poisson-dinfo-sign": lc.POISSON}[defect]
    which = "tail" if defect == "series-sign" else "main"      # the series runs past |l| = 37 only
    worst = _grid_ratios(lc.StandIn(defect=defect), lik, which)
    print(f"[lik reference] {defect}: " + ", ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    assert max(worst.values()) > 1., (defect, worst)
    clean = _grid_ratios(lc.StandIn(), lik, which)
    assert max(clean.values()) < 1.


def _prep_ratios(lik, with_offset, stored_w, n, **kw):
    idx = lc.sample_index(n, ("prep", lik))
    g = lc.gather(lc.pool(lik, with_offset), idx)
    got = lc.standin_prep(lik, g, stored_w=stored_w, **kw)
    R = lc.prep_reference(lik, with_offset, stored_w)
    out = {}
    for name in ("d1", "info", "dinfo", "rhs", "dw", "sdw", "DW", "ws", "wdw", "dpwi"):
        ref, bnd = R.arrays(name, idx)
        out[name] = lc.max_ratio(got[name], ref, bnd)
    for name in ("log_dpwi", "log_w"):
        ref, bnd = R.total(name, idx)
        out["sum " + name] = lc.max_ratio(np.array([got[name].sum()]), ref, bnd)
    return out, got, R, idx


@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("with_offset", [False, True])
def test_path_standins_meet_every_bound(lik, with_offset):
    worst = {}
    for stored_w in (False, True):
        out, _, _, _ = _prep_ratios(lik, with_offset, stored_w, 257)
        for k, v in out.items():
            worst[k] = max(worst.get(k, 0.), v)
    for kind, lam, first, cap in (("vif", 1., 1, 0), ("vif", 0.25, 0, 1), ("vif", 0.5, 0, 0), ("vif", 1., 1, 1),
                                  ("mix", 1., 0, 0), ("mix", 0.25, 0, 0)):
        idx = lc.sample_index(257, ("trial", lik))
        g = lc.gather(lc.pool(lik, with_offset), idx)
        got = lc.standin_trial(lik, g, kind, lam, first, cap)
        R = lc.trial_reference(lik, with_offset, kind, lam, first, cap)
        for name in (("trial",) if kind == "vif" else ("mnew", "anew")):
            ref, bnd = R.arrays(name, idx)
            worst[name] = max(worst.get(name, 0.), lc.max_ratio(got[name], ref, bnd))
        for name in (("loglik",) if kind == "vif" else ("loglik", "am")):
            ref, bnd = R.total(name, idx)
            worst["sum " + name] = max(worst.get("sum " + name, 0.), lc.max_ratio(np.array([got[name].sum()]), ref, bnd))
    for K in (1, 2, 3):
        idx, _, _, _ = lc.grouped_case(lik, with_offset, K, 257)
        got = lc.standin_grouped(lik, with_offset, K, 257)
        R = lc.grouped_reference(lik, with_offset, K)
        for q in lc.QUANTS:
            ref, bnd = R.arrays(q, idx)
            worst["grouped " + q] = max(worst.get("grouped " + q, 0.), lc.max_ratio(got[q], ref, bnd))
    idx, cnt, _, _ = lc.obs_case(lik, 65, with_offset)
    d1, w = lc.standin_obs(lik, 65, with_offset)
    R = lc.obs_reference(lik, with_offset, False)
    for name, got in (("d1", d1), ("info", w)):
        ref, bnd = lc.by_count(R, name, idx, cnt)
        worst["obs " + name] = lc.max_ratio(got, ref, bnd)
    print(f"[lik reference] {lc.LIK_NAMES[lik]} offset {int(with_offset)} paths: " +
          ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v < 1., (lc.LIK_NAMES[lik], with_offset, k, v)


@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("defect", ["dropped", "twice"])
def test_planted_offset_defect_exceeds_a_bound(lik, defect):
    out, _, _, _ = _prep_ratios(lik, True, False, 64, offset=defect)
    names = ("d1",) if lik == lc.GAUSSIAN else ("d1", "info")      # the Gaussian information does not depend on l
    for name in names:
        assert out[name] > 1., (lc.LIK_NAMES[lik], defect, name, out[name])


@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("defect", ["row-y", "drop-last"])
def test_planted_obsmap_defect_exceeds_a_bound(lik, defect):
    idx, cnt, _, _ = lc.obs_case(lik, 65, True)
    d1, w = lc.standin_obs(lik, 65, True, defect=defect)
    R = lc.obs_reference(lik, True, False)
    ref, bnd = lc.by_count(R, "d1", idx, cnt)
    assert lc.max_ratio(d1, ref, bnd) > 1., (lc.LIK_NAMES[lik], defect)
    # rows with one observation of their own are not changed by dropping the last of several
    if defect == "drop-last":
        one = cnt == 1
        assert lc.max_ratio(d1[one], ref[one], bnd[one]) < 1.


@pytest.mark.parametrize("lik", LIKS)
@pytest.mark.parametrize("n", [65, 257, 1000, lc.WRAP_N])
def test_dropped_end_of_a_sum_exceeds_its_bound(lik, n):
    """a block reduction that loses its last term, at sizes that are no multiple of the block; at the size where the
    grid-stride loop wraps, one that loses the wrapped pass (the last 257 terms: with (n - 1) U sum |term| over
    262401 terms a single small term is below any bound of a sum)"""
    idx = lc.sample_index(n, ("trial", lik))
    g = lc.gather(lc.pool(lik, True), idx)
    got = lc.standin_trial(lik, g, "mix", 0.25, 0, 0)
    R = lc.trial_reference(lik, True, "mix", 0.25, 0, 0)
    lost = 257 if n == lc.WRAP_N else 1
    for name in ("loglik", "am"):
        ref, bnd = R.total(name, idx)
        assert lc.max_ratio(np.array([math.fsum(got[name])]), ref, bnd) < 1., (name, n)
        assert lc.max_ratio(np.array([math.fsum(got[name][:-lost])]), ref, bnd) > 1., (name, n)
