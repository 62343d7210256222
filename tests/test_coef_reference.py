"""CPU: the cases and bounds of tests/coef_cases.py hold for a float64 numpy evaluation of the three passes of the
coefficient layer (offset F + X beta, gradient X^T gF, the four step-cap sums), in numpy's own order of summation; the
bounds are informative (a small fraction of the scale) and planted defects exceed them, so the GPU test that shares
the cases (tests/test_gpu_coef_ops.py) is not vacuous. Run with -s for the largest error / bound per quantity.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coef_cases as cc  # noqa: E402

_worst = {}


def setup_module(module):
    cc.assert_longdouble()


def teardown_module(module):
    for key in sorted(_worst):
        print(f"[coef reference] largest error / bound, {key}: {_worst[key]:.3g}")


def _cases():
    return [pytest.param(n, p, f, id=f"n{n}-p{p}-F{int(f)}") for n in cc.NS for p in cc.PS for f in (False, True)]


@pytest.mark.parametrize("n,p,with_F", _cases())
def test_numpy_float64_meets_every_bound(n, p, with_F):
    c = cc.make_case(n, p, with_F)
    ref = cc.reference(c)
    got = cc.numpy_eval(c)
    for q in ("eta0", "g", "mom"):
        r = cc.max_ratio(got[q], ref[q][0], ref[q][1])
        _worst[q] = max(_worst.get(q, 0.), r)
        assert r < 1., (c["name"], q, r)


def test_bounds_are_informative():
    """every bound is below 1e-10 of its scale (gamma_{70032} = 7.8e-12), and above zero wherever the scale is"""
    for c in cc.all_cases():
        ref = cc.reference(c)
        for q in ("eta0", "g", "mom"):
            _, bnd, scale = ref[q]
            assert np.all(bnd <= 1e-10 * scale), (c["name"], q)
            assert np.all((bnd > 0) == (scale > 0)), (c["name"], q)


def test_cancelling_case_true_sum_is_1e12_of_the_terms():
    c = cc.make_cancelling_case()
    ref = cc.reference(c)
    g, _, terms = ref["g"]
    rel = np.abs(g) / terms
    assert np.all((rel > 1e-13) & (rel < 1e-11)), rel
    mom, _, msc = ref["mom"]
    assert np.all(np.abs(mom[:2]) / msc[:2] < 1e-11) and np.all(np.abs(mom[:2]) > 0)
    # numpy float64 meets the bound; a relative check at 1e-6 against the true sum would be 1e6 times tighter than
    # the arithmetic can give, one against the terms 1e6 times looser than the bound
    got = cc.numpy_eval(c)
    for q in ("g", "mom"):
        r = cc.max_ratio(got[q], ref[q][0], ref[q][1])
        _worst["cancelling " + q] = r
        assert r < 1., (q, r)
    garbage = np.asarray(ref["g"][0], dtype=np.float64) + 1e-9 * np.asarray(terms, dtype=np.float64)
    assert cc.max_ratio(garbage, ref["g"][0], ref["g"][1]) > 1.


@pytest.mark.parametrize("n,p", [(65, 5), (4097, 31), (70001, 2)])
def test_planted_defects_exceed_the_bounds(n, p):
    c = cc.make_case(n, p, True)
    ref = cc.reference(c)
    X = c["X"]
    # float32 accumulation
    e32 = (X.astype(np.float32) @ c["beta"].astype(np.float32)).astype(np.float64) + c["F"]
    assert cc.max_ratio(e32, *ref["eta0"][:2]) > 1.
    # the last row left out of the sums (a tile tail dropped)
    g_drop = X[:-1].T @ c["gF"][:-1]
    assert cc.max_ratio(g_drop, *ref["g"][:2]) > 1.
    a, b = X[:-1] @ c["dir"], X[:-1] @ c["beta"]
    m_drop = np.array([a.sum(), b.sum(), (a * a).sum(), (a * b).sum()])
    assert cc.max_ratio(m_drop, *ref["mom"][:2]) > 1.
    # a column read at the wrong stride (p + 1 instead of p) for p > 1
    if p > 1:
        flat = X.reshape(-1)
        Xw = np.stack([flat[np.minimum(np.arange(n) * (p + 1) + j, flat.size - 1)] for j in range(p)], axis=1)
        assert cc.max_ratio(Xw @ c["beta"] + c["F"], *ref["eta0"][:2]) > 1.
    # F forgotten
    assert cc.max_ratio(X @ c["beta"], *ref["eta0"][:2]) > 1.
