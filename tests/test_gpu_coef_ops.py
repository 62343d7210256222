"""GPU: the three passes of the coefficient layer (csrc/coef_kernels.hip) through GPB_TestCoefOps on the cases of
tests/coef_cases.py: the offset F + X beta, the gradient X^T gF and the four step-cap sums against longdouble
references and the derived bounds (none tuned to a kernel; tests/test_coef_reference.py holds a float64 numpy
evaluation to the same bounds and shows that planted defects exceed them). n in {1, 63, 64, 65, 257, 4097, 70001}
crosses the tile of 256 rows, one and several blocks and the tail tile; p in {1, 2, 5, 31} the even / odd LDS strides
and the widest matrix. Outputs start as NaN between guard bands. Two consecutive runs give the same bits.
Run with -s for the largest error / bound per quantity and case.

Largest error / bound measured on an MI355X (58 tests in 1.2 s): offset .66 (n = 70001, p = 2, with F), gradient .32
and step sums .38 (both at n = p = 1); the cancelling case: gradient 0 (the pairs cancel exactly), step sums 2.7e-4.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coef_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu
_worst = {}


def setup_module(module):
    cc.assert_longdouble()


def teardown_module(module):
    for key in sorted(_worst):
        print(f"[coef ops] largest error / bound, {key}: {_worst[key][0]:.3g} ({_worst[key][1]})")


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _check(c):
    ref = cc.reference(c)
    got = cc.device_eval(c)
    again = cc.device_eval(c)
    for q in ("eta0", "g", "mom"):
        r = cc.max_ratio(got[q], ref[q][0], ref[q][1])
        print(f"{c['name']} {q}: error / bound {r:.3g}")
        if r > _worst.get(q, (0., ""))[0]:
            _worst[q] = (r, c["name"])
        assert r < 1., (c["name"], q, r)
        assert _same_bits(got[q], again[q]), (c["name"], q)


@pytest.mark.parametrize("n", cc.NS)
@pytest.mark.parametrize("p", cc.PS)
@pytest.mark.parametrize("with_F", [False, True])
def test_passes_meet_every_bound_and_repeat_bitwise(n, p, with_F):
    _check(cc.make_case(n, p, with_F))


def test_cancelling_sums_meet_the_bound():
    """the true sums are 1e-12 of sum |terms|: the check is the bound, not a relative error"""
    _check(cc.make_cancelling_case())


def test_outputs_are_optional_and_refusals_name_the_limit():
    c = cc.make_case(65, 5, True)
    from gpboost_amd import basic
    import ctypes
    D = ctypes.POINTER(ctypes.c_double)
    X = np.ascontiguousarray(c["X"])
    g = np.full(5, np.nan)
    ret = basic.lib().GPB_TestCoefOps(ctypes.c_int(65), ctypes.c_int(5), X.ctypes.data_as(D), None, None, None,
                                      np.ascontiguousarray(c["gF"]).ctypes.data_as(D), None, g.ctypes.data_as(D), None)
    assert ret == 0
    assert _same_bits(g, cc.device_eval(c)["g"])
    big = np.ones((4, 32))
    ret = basic.lib().GPB_TestCoefOps(ctypes.c_int(4), ctypes.c_int(32), big.ctypes.data_as(D), None, None, None,
                                      np.ones(4).ctypes.data_as(D), None, np.zeros(32).ctypes.data_as(D), None)
    assert ret == -1 and b"outside [1, 31]" in basic.lib().LGBM_GetLastError()
