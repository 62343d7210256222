"""The device evaluation of the general-shape Matern covariance (csrc/cov.h matern_general, through
GPB_TestMaternGeneral) against mpmath's Bessel functions at 50 digits.

Tolerance: the host form of the same function (cov.h compiled into a stand-alone program, hipcc -O2, run on the CPU)
against the same reference over this grid is off by at most 5.4e-14 at x = 1e-150 (dc at nu = 0.3: the rounding of
the exponent of (x/2)^nu) and by at most 2.6e-15 at every other x. The device gets 4 times the
figure of its x for FMA contraction and its own exp."""
import ctypes

import mpmath as mp
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_TINY, TOL = 4 * 5.4e-14, 4 * 2.6e-15   # x = 1e-150, every other x
NUS = [0.3, 0.75, 1, 2, 3.3, 0.5, 1.5, 2.5]
XS = [0, 1e-150, 1e-8, 1e-3, 0.5, 1.999, 2, 2.001, 5, 30, 200, 700, 800]


def _device(nu, xs):
    from gpboost_amd.basic import lib
    fn = lib().GPB_TestMaternGeneral
    D = ctypes.POINTER(ctypes.c_double)
    fn.argtypes = [ctypes.c_double, ctypes.c_int, D, D, D]
    x = np.asarray(xs, dtype=np.float64)
    c, dc = np.full(x.size, np.nan), np.full(x.size, np.nan)
    assert fn(float(nu), x.size, x.ctypes.data_as(D), c.ctypes.data_as(D), dc.ctypes.data_as(D)) == 0
    return c, dc


@pytest.mark.parametrize("nu", NUS)
def test_matern_general_against_mpmath(nu):
    mp.mp.dps = 50
    c, dc = _device(nu, XS)
    k = mp.power(2, 1 - mp.mpf(nu)) / mp.gamma(nu)
    for x, cv, dv in zip(XS, c, dc):
        if x == 0:
            assert (cv, dv) == (1., 0.)
            continue
        xm = mp.mpf(x)
        refs = (k * xm ** nu * mp.besselk(nu, xm), -k * xm ** (nu + 1) * mp.besselk(nu - 1, xm))
        for name, v, r in zip(("c", "dc"), (cv, dv), refs):
            if abs(r) < 1e-290:
                assert np.isfinite(v) and abs(v) <= 1e-290, (nu, x, name, v)
            else:
                err = float(abs(mp.mpf(float(v)) - r) / abs(r))
                print(f"nu={nu} x={x} {name} rel err {err:.2e}")
                assert err <= (TOL_TINY if x == 1e-150 else TOL), (nu, x, name, v, mp.nstr(r, 17), err)
