"""CPU: the references and bounds of tests/lik_nb_cases.py (negative binomial likelihood layer), without a GPU.

* A float64 stand-in (math) of the nb_* formulas of csrc/lik_device.h meets every bound of the seven quantities on the
  main grid (MAIN_L x y in {0, 1, 2, 7, 50, 1e4} x r in {0.05, 1, 2.5, 400}) and on the tail set l = +-700, +-745,
  1000, where all seven are finite and the information is not negative. Run with -s for the largest error / bound;
  on this suite's CPU (glibc libm): main grid at most 0.34 (loglik), tail set at most 0.31 (d1, info).
* The definitions as they are written (d1 and the information through mu / (mu + r)) are the seeded defect that
  shows the test can fail: d1 exceeds its bound 6.6e4 times on the main grid (the naive information is a product
  without cancellation and stays accurate there), and neither is finite on the tail set.
* Informativeness: on the main grid no (point, quantity) has a bound above 1e-3 scale (scales: lik_nb_cases.py);
  the largest bound / scale is 1.4e-13 (aux_term).
* The host's sums over the table of distinct responses (lgamma and the AS 103 digamma, ascending values) meet their
  bounds against mpmath, on the fixtures' own draw and on a table with large counts.
* The grouped observation pass's stand-in (eta formed as the kernels form it) meets the pool bounds.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lik_cases as lc  # noqa: E402
import lik_nb_cases as nb  # noqa: E402


def setup_module(module):
    lc.assert_longdouble()


def _grid_ratios(which, naive=False):
    worst = {q: 0. for q in nb.NB_QUANTS}
    for r, y, ls, ref in nb.grid_reference(which):
        got = nb.standin_block(r, y, ls, naive)
        for q in nb.NB_QUANTS:
            worst[q] = max(worst[q], float(ref.ratios(q, got[q]).max()))
    return worst


@pytest.mark.parametrize("which", ["main", "tail"])
def test_standin_meets_every_bound(which):
    worst = _grid_ratios(which)
    print(f"[lik nb reference] {which}: " + ", ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    for q, v in worst.items():
        assert v < 1., (which, q, v)


def test_tail_values_are_finite_and_the_information_is_not_negative():
    for r, y, ls, ref in nb.grid_reference("tail"):
        got = nb.standin_block(r, y, ls)
        for q in nb.NB_QUANTS:
            assert np.isfinite(got[q]).all(), (r, y, q, got[q])
            assert all(abs(v) <= lc.DBL_MAX for v in ref.exact_mp[q])
        assert (got["info"] >= 0.).all()


def test_naive_form_exceeds_the_bounds():
    """mu / (mu + r): on the main grid d1 = y - (y + r) p has lost 1 - p for l >> log r (the naive information is a
    product without cancellation and stays accurate there); on the tail set e^l overflows in both"""
    main = _grid_ratios("main", naive=True)
    print("[lik nb reference] naive, main grid: " + ", ".join(f"{q} {v:.3g}" for q, v in main.items()))
    assert main["d1"] > 1e3, main
    tail = _grid_ratios("tail", naive=True)
    assert tail["d1"] == np.inf and tail["info"] == np.inf
    clean = _grid_ratios("main")
    assert max(clean.values()) < 1.


def test_bounds_are_informative():
    worst = {q: 0. for q in nb.NB_QUANTS}
    for r, y, ls, ref in nb.grid_reference("main"):
        for q in nb.NB_QUANTS:
            sc, b = ref.scale(q), ref.bound[q]
            assert np.isfinite(b).all()
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(b <= 1e-3 * sc, np.where(sc > 0, b / sc, 0.), np.inf)
            worst[q] = max(worst[q], float(rel.max()))
    print("[lik nb reference] largest bound / scale: " + ", ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    for q, v in worst.items():
        assert v <= 1e-3, (q, v)


@pytest.mark.parametrize("r", [0.05, 1.5, 2.0, 400., 1e7])
def test_host_table_sums_meet_their_bounds(r):
    from gpboost_amd import synthetic
    draws = [synthetic.bench_grouped_negbin_y(synthetic.bench_groups(3001, (60, 9))),
             np.array([0., 0., 1., 7., 7., 7., 1e4, 123456., 2. ** 31])]
    for y in draws:
        sl, sd = nb.table_sums64(y, r)
        (el, bl), (ed, bd) = nb.table_reference(y, r)
        rl, rd = lc.max_ratio([sl], el, bl), lc.max_ratio([sd], ed, bd)
        print(f"[lik nb reference] table sums r = {r:g}, {len(np.unique(y))} distinct of {y.size}: lgamma {rl:.3g}, "
              f"digamma {rd:.3g}; bound / |sum| {bl / abs(float(el)):.3g}, {bd / abs(float(ed)):.3g}")
        assert rl < 1. and rd < 1.
        assert bl <= 1e-12 * max(abs(float(el)), y.size) and bd <= 1e-12 * max(abs(float(ed)), y.size)


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("with_offset", [False, True])
def test_grouped_standin_meets_the_pool_bounds(K, with_offset):
    n = 257
    idx, _, _, eta = nb.eta64(with_offset, K, n)
    y = nb.pool(with_offset)["y"][idx]
    R = nb.grouped_reference(with_offset, K)
    rows =[nb.standin(nb.NB_PATH_AUX, float(y[i]), float(eta[i])) for i in range(n)]
    for q in nb.NB_QUANTS:
        ref, bnd = R.arrays(q, idx)
        v = lc.max_ratio(np.array([row[q] for row in rows]), ref, bnd)
        assert v < 1., (q, v)
    for q in ("loglik", "aux_term"):   # the sums in any order
        tot, bnd = R.total(q, idx)
        assert lc.max_ratio([sum(row[q] for row in rows)], tot, bnd) < 1.
