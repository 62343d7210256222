"""CPU: the host side of the coefficient layer (csrc/coef.cpp) through GPB_TestCoefHost, against a numpy restatement
written from the reference: intercept detection (re_model_template.h:976-1000: the first column all of whose entries
equal its first one by TwoNumbersAreEqual, |a - b| < 1e-10 max(1, |a|, |b|)), centring and scaling (:1084-1107: every
other column minus its mean, over its population standard deviation; nothing when the intercept is the only column),
TransformCoef / TransformBackCoef (:7273-7315), FindInitialIntercept (likelihoods.h:747-802),
FindConstantsCapTooLargeLearningRateCoef (:1658-1685) and MaximalLearningRateCoef (re_model_template.h:4952-4981).
No device call is made.
"""
import ctypes
import math

import numpy as np
import pytest
from statistics import NormalDist

D = ctypes.POINTER(ctypes.c_double)
LOGIT, PROBIT, POISSON, GAMMA = 1, 2, 3, 4
C_MAX_CHANGE_COEF = 10.


def _dp(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(D) if a is not None else None


def hook(op, lik=0, n=0, p=0, X=None, y=None, F=None, inp=None, out_len=1):
    from gpboost_amd import basic
    keep = [np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in (X, y, F, inp)]
    out = np.full(out_len, np.nan)
    ret = basic.lib().GPB_TestCoefHost(ctypes.c_int(op), ctypes.c_int(lik), ctypes.c_int(n), ctypes.c_int(p),
                                       *[a.ctypes.data_as(D) if a is not None else None for a in keep],
                                       out.ctypes.data_as(D))
    if ret != 0:
        raise RuntimeError(basic.lib().LGBM_GetLastError().decode())
    return out


# ------------------------------------------------------------------------------------------ restatement
def two_numbers_equal(a, b):
    return abs(a - b) < 1e-10 * max(1.0, abs(a), abs(b))


def scaling_restated(X):
    n, p = X.shape
    icol = -1
    for j in range(p):
        if all(two_numbers_equal(X[i, j], X[0, j]) for i in range(1, n)):
            icol = j
            break
    scaled = not (icol >= 0 and p == 1)
    loc, scale, Xs = np.zeros(p), np.ones(p), X.copy()
    if scaled:
        for j in range(p):
            if j != icol:
                loc[j] = X[:, j].mean()
                cen = X[:, j] - loc[j]
                scale[j] = math.sqrt((cen ** 2).sum() / n)
                Xs[:, j] = cen / scale[j]
    return icol, scaled, loc, scale, Xs


def transform_restated(b, icol, loc, scale):
    t = np.array(b, dtype=np.float64)
    for j in range(len(t)):
        if j != icol:
            if icol >= 0:
                t[icol] += t[j] * loc[j]
            t[j] *= scale[j]
    if icol >= 0:
        t[icol] *= scale[icol]
    return t


def transform_back_restated(b, icol, loc, scale):
    o = np.array(b, dtype=np.float64)
    if icol >= 0:
        o[icol] /= scale[icol]
    for j in range(len(o)):
        if j != icol:
            o[j] /= scale[j]
            if icol >= 0:
                o[icol] -= o[j] * loc[j]
    return o


def lib_scaling(X):
    n, p = X.shape
    out = hook(0, n=n, p=p, X=X.T.reshape(-1), out_len=2 + 2 * p + n * p)
    return int(out[0]), bool(out[1]), out[2:2 + p], out[2 + p:2 + 2 * p], out[2 + 2 * p:].reshape(n, p)


def _design(kind, n=57, seed=3):
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, 3)) * np.array([1., 40., 0.02]) + np.array([0., -7., 3.])
    one = np.ones((n, 1))
    if kind == "intercept_first":
        return np.hstack([one, Z])
    if kind == "intercept_last":
        return np.hstack([Z, one])
    if kind == "none":
        return Z
    if kind == "constant_2p5":                # a constant column that is not 1 still counts as the intercept
        return np.hstack([Z[:, :1], np.full((n, 1), 2.5), Z[:, 1:]])
    if kind == "only_intercept":
        return one
    if kind == "nearly_constant":             # within TwoNumbersAreEqual of its first entry
        c = 1.0 + 3e-11 * rng.standard_normal((n, 1))
        return np.hstack([c, Z])
    if kind == "not_quite_constant":          # one entry 3e-10 away: no intercept
        c = np.ones((n, 1))
        c[n // 2] += 3e-10
        return np.hstack([c, Z[:, :1]])
    raise ValueError(kind)


KINDS = ["intercept_first", "intercept_last", "none", "constant_2p5", "only_intercept", "nearly_constant",
         "not_quite_constant"]
EXPECT_ICOL = {"intercept_first": 0, "intercept_last": 3, "none": -1, "constant_2p5": 1, "only_intercept": 0,
               "nearly_constant": 0, "not_quite_constant": -1}


@pytest.mark.parametrize("kind", KINDS)
def test_intercept_detection_and_scaling(kind):
    X = _design(kind)
    icol, scaled, loc, scale, Xs = lib_scaling(X)
    ricol, rscaled, rloc, rscale, rXs = scaling_restated(X)
    assert icol == ricol == EXPECT_ICOL[kind]
    assert scaled == rscaled == (kind != "only_intercept")
    # sums over at most 57 terms: the library adds in index order, numpy pairwise; n ulp covers both
    n = X.shape[0]
    tol = 4 * n * np.finfo(np.float64).eps
    np.testing.assert_allclose(loc, rloc, rtol=tol, atol=tol * np.abs(X).max())
    np.testing.assert_allclose(scale, rscale, rtol=tol)
    np.testing.assert_allclose(Xs, rXs, rtol=0, atol=tol * np.abs(X).max() / rscale.min())
    if icol >= 0:
        assert loc[icol] == 0. and scale[icol] == 1.
        assert np.array_equal(Xs[:, icol], X[:, icol])         # the intercept column stays as given
    if scaled and kind != "not_quite_constant":   # (its column of spread 3e-10 around 1 is centred with cancellation)
        others = [j for j in range(X.shape[1]) if j != icol]
        assert np.allclose(Xs[:, others].mean(axis=0), 0., atol=1e-9)
        assert np.allclose((Xs[:, others] ** 2).mean(axis=0), 1., rtol=1e-9)


@pytest.mark.parametrize("kind", KINDS)
def test_transform_coef_and_round_trip(kind):
    X = _design(kind)
    n, p = X.shape
    icol, scaled, loc, scale, _ = lib_scaling(X)
    rng = np.random.default_rng(11)
    b = rng.standard_normal(p) * np.array([3., 0.1, 50., 1.][:p])
    t = hook(1, n=n, p=p, X=X.T.reshape(-1), inp=b, out_len=p)
    o = hook(2, n=n, p=p, X=X.T.reshape(-1), inp=b, out_len=p)
    if not scaled:
        assert np.array_equal(t, b) and np.array_equal(o, b)
        return
    # the same operations in the same order on the library's own loc / scale: bit for bit
    assert np.array_equal(t, transform_restated(b, icol, loc, scale))
    assert np.array_equal(o, transform_back_restated(b, icol, loc, scale))
    # TransformBackCoef(TransformCoef(b)) = b to 4 ulp of the largest quantity that enters each entry
    back = hook(2, n=n, p=p, X=X.T.reshape(-1), inp=t, out_len=p)
    ulp = np.finfo(np.float64).eps
    mag = np.abs(b).copy()
    if icol >= 0:
        mag[icol] = abs(b[icol]) + np.sum(np.abs(b * loc))
    assert np.all(np.abs(back - b) <= 4 * ulp * mag), (back - b, mag)
    # the linear predictor is the same on both scales: X b = Xs TransformCoef(b) when the constant column is 1
    if icol < 0 or np.all(X[:, icol] == 1.):
        _, _, _, _, Xs = lib_scaling(X)
        if icol >= 0:
            np.testing.assert_allclose(Xs @ t, X @ b, rtol=1e-10, atol=1e-10 * np.abs(X @ b).max())


def _intercept_restated(lik, y, F, var):
    n = len(y)
    if lik in (LOGIT, PROBIT):
        swy = float(np.sum(y))
        pavg = swy / n if swy > 0 else 0.5
        pavg = min(max(pavg, 1e-12), 1 - 1e-12)
        v = math.log(pavg / (1 - pavg)) if lik == LOGIT else NormalDist().inv_cdf(pavg)
        return min(max(v, -3.), 3.)
    avg = float(np.mean(y if F is None else y / np.exp(F)))
    return math.log(max(avg, 1e-12)) - 0.5 * var


@pytest.mark.parametrize("lik", [LOGIT, PROBIT, POISSON, GAMMA])
@pytest.mark.parametrize("with_F", [False, True])
def test_initial_intercept(lik, with_F):
    rng = np.random.default_rng(5 + lik)
    n = 211
    F = rng.standard_normal(n) * 0.7 if with_F else None
    if lik in (LOGIT, PROBIT):
        ys = [(rng.uniform(size=n) < q).astype(float) for q in (0.5, 0.2, 0.93)]
    elif lik == POISSON:
        ys = [rng.poisson(3.0, size=n).astype(float), np.zeros(n)]          # all zero: the 1e-12 floor
    else:
        ys = [rng.gamma(2.0, 1.5, size=n)]
    for y in ys:
        for var in (0.5, 2.0):
            got = hook(3, lik=lik, n=n, y=y, F=F, inp=[var])[0]
            want = _intercept_restated(lik, y, F, var)
            assert got == pytest.approx(want, rel=1e-12, abs=1e-12), (lik, with_F, var)


@pytest.mark.parametrize("lik", [LOGIT, PROBIT])
def test_initial_intercept_is_clipped_to_3(lik):
    n = 1000
    y = np.zeros(n)
    y[0] = 1.                                  # pavg = 0.001: logit -6.9, probit -3.09
    assert hook(3, lik=lik, n=n, y=y, inp=[1.0])[0] == -3.0
    assert hook(3, lik=lik, n=n, y=1. - y, inp=[1.0])[0] == 3.0
    assert hook(3, lik=lik, n=n, y=np.ones(n), inp=[1.0])[0] == 3.0          # pavg clipped to 1 - 1e-12
    # all zero: the reference's swy > 0 test fails and pavg is 0.5
    assert hook(3, lik=lik, n=n, y=np.zeros(n), inp=[1.0])[0] == 0.0
    # just inside the clip
    y = np.zeros(n)
    y[:60] = 1.
    want = math.log(0.06 / 0.94) if lik == LOGIT else NormalDist().inv_cdf(0.06)
    assert hook(3, lik=lik, n=n, y=y, inp=[1.0])[0] == pytest.approx(want, rel=1e-13)


def test_probit_quantile_over_its_range():
    """the initial probit intercept is the normal quantile of mean(y) wherever it is inside +-3"""
    n = 4000
    for k in (6, 40, 300, 1000, 2000, 2900, 3700, 3990):
        y = np.zeros(n)
        y[:k] = 1.
        assert hook(3, lik=PROBIT, n=n, y=y, inp=[1.0])[0] == pytest.approx(NormalDist().inv_cdf(k / n), rel=1e-13)


def test_cap_constants():
    rng = np.random.default_rng(8)
    y = rng.gamma(2.0, 3.0, size=300)
    for lik in (LOGIT, PROBIT):
        assert list(hook(4, lik=lik, n=300, y=(y > 5).astype(float), out_len=2)) == [1., 1.]
    for lik in (POISSON, GAMMA):
        yy = np.floor(y) if lik == POISSON else y
        mean, sec = yy.mean(), (yy ** 2).mean()
        got = hook(4, lik=lik, n=300, y=yy, out_len=2)
        assert got[0] == pytest.approx(abs(math.log(mean)), rel=1e-12)
        assert got[1] == pytest.approx(abs(math.log(sec - mean * mean)), rel=1e-10)
    # a constant response: variance 0, SafeLog gives -inf, the constant is +inf (no variance cap)
    got = hook(4, lik=POISSON, n=10, y=np.full(10, 2.), out_len=2)
    assert got[0] == pytest.approx(math.log(2.)) and got[1] == math.inf


def _cap_restated(mom, n, C_mu, C_sigma2):
    mean_c, mean_l = mom[0] / n, mom[1] / n
    var_c = mom[2] / n - mean_c * mean_c
    cov = mom[3] / n - mean_c * mean_l
    with np.errstate(divide="ignore", invalid="ignore"):
        lr_mu = np.float64(C_mu * C_MAX_CHANGE_COEF) / np.float64(abs(mean_c))
        lr_var = (abs(cov) + np.sqrt(np.float64(cov * cov + 4 * var_c * C_sigma2 * C_MAX_CHANGE_COEF))) / 2 / np.float64(var_c)
    return lr_mu, lr_var


@pytest.mark.parametrize("mom,n,C_mu,C_sigma2", [
    ([12.0, 30.0, 40.0, 55.0], 10, 1., 1.),             # both caps finite, the mean cap binds
    ([0.5, 30.0, 400.0, 55.0], 10, 1., 1.),             # the variance cap binds
    ([-12.0, 30.0, 40.0, -55.0], 10, 0.7, 2.3),         # signs: |mean change|, |cov|
    ([0.0, 3.0, 9.0, 1.0], 10, 1., 1.),                 # mean change 0: the mean cap is +inf
    ([20.0, 5.0, 40.0 + 1e-13, 10.0], 10, 1., 1.),      # an intercept-only direction: var_lp_change ~ 1e-14
])
def test_step_cap_from_moments(mom, n, C_mu, C_sigma2):
    got = hook(5, n=n, inp=list(mom) + [C_mu, C_sigma2])[0]
    lr_mu, lr_var = _cap_restated(mom, n, C_mu, C_sigma2)
    want = min(lr_mu, lr_var)
    assert math.isfinite(got) and got > 0
    assert got == pytest.approx(want, rel=1e-14)


def test_step_cap_with_zero_variance_of_the_change():
    """var_lp_change exactly 0 (a direction along the intercept alone, cov 0): 0 / 0 in the variance cap. std::min
    keeps its first argument against a NaN, so the mean cap is returned, as the reference's std::min({mu, var})."""
    mom = [20.0, 5.0, 40.0, 10.0]                       # mean 2, second moment 4: variance 0; cov = 1 - 2 * 0.5 = 0
    got = hook(5, n=10, inp=mom + [1., 1.])[0]
    assert got == pytest.approx(1. * C_MAX_CHANGE_COEF / 2.0, rel=1e-15)
    # variance 0 with a non-zero covariance term: |cov| / 0 = +inf, the mean cap again
    mom = [20.0, 5.0, 40.0, 30.0]
    assert hook(5, n=10, inp=mom + [1., 1.])[0] == pytest.approx(5.0, rel=1e-15)


def test_refusals_name_the_limit():
    with pytest.raises(RuntimeError, match="num_covariates = 32"):
        hook(0, n=3, p=32, X=np.ones(96), out_len=200)
    X = np.ones(6)
    X[4] = np.nan
    with pytest.raises(RuntimeError, match="NaN or Inf in covariate data"):
        hook(0, n=3, p=2, X=X, out_len=20)
