"""Cases, references and error bounds of the three device passes of the coefficient layer (csrc/coef_kernels.hip),
shared by tests/test_gpu_coef_ops.py (GPB_TestCoefOps on the device) and tests/test_coef_reference.py (CPU: a float64
numpy evaluation meets every bound, the bounds are informative, planted defects exceed them).

Reference: numpy longdouble (64-bit significand; its own error, (n + p) 2^-64 sum |terms|, is 2^-11 of the bounds).

Bounds, u = 2^-53, gamma_k = k u / (1 - k u):
  offset      |eta0_i - exact| <= gamma_{p+1} (|F_i| + sum_j |X_ij beta_j|)            p products, p additions
  reductions  |sum - exact|    <= gamma_{n+p} sum_i |terms_i|                           any order of summation
with the terms
  g_j                 X_ij gF_i
  sum (X dir)_i       sum_j |X_ij dir_j|                    = A_i
  sum (X beta)_i      sum_j |X_ij beta_j|                   = B_i
  sum (X dir)_i^2     A_i^2
  sum (X dir)(X beta) A_i B_i
No bound is tuned to what a kernel gives.

The cancelling cases: pairs of rows whose terms are equal and opposite, plus one term of about 1e-12 of sum |terms|,
which is then the whole true sum. A relative-error check would pass any garbage of size 1e-12 sum |terms| there (or
demand the impossible); the bound is the check.
"""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from latent_ops_cases import LD, assert_longdouble  # noqa: E402,F401

U = 2.0 ** -53
NS = (1, 63, 64, 65, 257, 4097, 70001)
PS = (1, 2, 5, 31)
MAX_P = 31


def gamma(k):
    return k * U / (1.0 - k * U)


def make_case(n, p, with_F, seed=0):
    """X row-major n x p of mixed magnitudes, beta, dir, F (or None) and gF"""
    rng = np.random.default_rng(1000003 * n + 101 * p + 7 * int(with_F) + seed)
    X = rng.standard_normal((n, p)) * np.exp(rng.uniform(-3., 3., size=(1, p)))
    X[:, 0] = 1.0 if p > 1 else X[:, 0]          # an intercept column beside the others
    beta = rng.standard_normal(p) * np.exp(rng.uniform(-2., 2., size=p))
    dirv = rng.standard_normal(p) * np.exp(rng.uniform(-2., 2., size=p))
    F = rng.standard_normal(n) * 3. if with_F else None
    gF = rng.standard_normal(n) * np.exp(rng.uniform(-4., 4., size=n))
    return dict(n=n, p=p, X=np.ascontiguousarray(X), beta=beta, dir=dirv, F=F, gF=gF, name=f"n{n}_p{p}_F{int(with_F)}")


def make_cancelling_case(n=4097, p=2):
    """n odd: rows 2k and 2k + 1 carry equal values, gF and dir's effect alternate in sign, so every pair cancels
    exactly in exact arithmetic; the last row carries about 1e-12 of sum |terms| and is the whole true sum."""
    assert n % 2 == 1
    rng = np.random.default_rng(4242)
    half = (n - 1) // 2
    v = rng.uniform(0.5, 2.0, size=(half, p))
    X = np.zeros((n, p))
    X[0:n - 1:2] = v
    X[1:n - 1:2] = -v                       # (X w)_{2k+1} = -(X w)_{2k} for every w
    gF = np.ones(n)                         # X_ij gF_i alternates with X
    beta = rng.uniform(0.5, 1.5, size=p)
    dirv = rng.uniform(0.5, 1.5, size=p)
    tiny = 1e-12 * float(np.abs(v).sum()) * 2. / p
    X[n - 1] = tiny
    return dict(n=n, p=p, X=np.ascontiguousarray(X), beta=beta, dir=dirv, F=None, gF=gF, name=f"cancel_n{n}_p{p}")


def all_cases():
    for n in NS:
        for p in PS:
            for with_F in (False, True):
                yield make_case(n, p, with_F)
    yield make_cancelling_case()


def reference(c):
    """Exact values (longdouble) and the bounds: dict of name -> (ref, bound, scale)"""
    n, p = c["n"], c["p"]
    X = c["X"].astype(LD)
    b, d = c["beta"].astype(LD), c["dir"].astype(LD)
    F = c["F"].astype(LD) if c["F"] is not None else np.zeros(n, dtype=LD)
    g = c["gF"].astype(LD)
    Xb, Xd = X * b, X * d
    B, A = np.abs(Xb).sum(axis=1), np.abs(Xd).sum(axis=1)
    lp_b, lp_d = Xb.sum(axis=1), Xd.sum(axis=1)
    out = {}
    sc = np.abs(F) + B
    out["eta0"] = (F + lp_b, gamma(p + 1) * sc, sc)
    terms = np.abs(X * g[:, None]).sum(axis=0)
    out["g"] = ((X * g[:, None]).sum(axis=0), gamma(n + p) * terms, terms)
    mom = np.array([lp_d.sum(), lp_b.sum(), (lp_d * lp_d).sum(), (lp_d * lp_b).sum()], dtype=LD)
    msc = np.array([A.sum(), B.sum(), (A * A).sum(), (A * B).sum()], dtype=LD)
    out["mom"] = (mom, gamma(n + p) * msc, msc)
    return out


def max_ratio(got, ref, bnd):
    """largest |got - ref| / bound; a zero bound needs an exact result"""
    got = np.asarray(got, dtype=np.float64).astype(LD)
    err = np.abs(got - ref)
    if not np.all(np.isfinite(got.astype(np.float64))):
        return float("inf")
    r = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), np.where(err > 0, np.inf, 0.))
    return float(np.max(r))


def numpy_eval(c):
    """float64 numpy stand-in of the three passes (the CPU check of the bounds)"""
    X = c["X"]
    eta0 = X @ c["beta"] + (c["F"] if c["F"] is not None else 0.)
    g = X.T @ c["gF"]
    a, b = X @ c["dir"], X @ c["beta"]
    mom = np.array([a.sum(), b.sum(), (a * a).sum(), (a * b).sum()])
    return dict(eta0=eta0, g=g, mom=mom)


# ------------------------------------------------------------------------------------------ the device hook
def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else None


GUARD = 8


def device_eval(c):
    """GPB_TestCoefOps; outputs start as NaN between guard bands that must come back untouched"""
    from gpboost_amd import basic
    n, p = c["n"], c["p"]
    X = np.ascontiguousarray(c["X"], dtype=np.float64)
    bufs = {k: np.full(m + 2 * GUARD, np.nan) for k, m in (("eta0", n), ("g", p), ("mom", 4))}
    for bfr in bufs.values():
        bfr[:GUARD] = -777.
        bfr[-GUARD:] = -777.
    views = {k: v[GUARD:-GUARD] for k, v in bufs.items()}
    ret = basic.lib().GPB_TestCoefOps(
        ctypes.c_int(n), ctypes.c_int(p), _dp(X), _dp(np.ascontiguousarray(c["beta"])),
        _dp(np.ascontiguousarray(c["dir"])), _dp(np.ascontiguousarray(c["F"])) if c["F"] is not None else None,
        _dp(np.ascontiguousarray(c["gF"])), _dp(views["eta0"]), _dp(views["g"]), _dp(views["mom"]))
    if ret != 0:
        raise RuntimeError(basic.lib().LGBM_GetLastError().decode())
    for k, bfr in bufs.items():
        assert np.all(bfr[:GUARD] == -777.) and np.all(bfr[-GUARD:] == -777.), f"{k}: guard band overwritten"
    return {k: v.copy() for k, v in views.items()}
