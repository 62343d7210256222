"""Cases, exact references and error bounds of the negative binomial likelihood layer (the nb_* functions of
csrc/lik_device.h, glp_obs_kernel's negative binomial branch and glp_nb_aux_kernel of csrc/grouped_laplace.hip, and
the host's sums over the table of distinct responses), shared by tests/test_lik_nb_reference.py (CPU) and
tests/test_gpu_lik_nb_ops.py (GPU). The error algebra (class E, e_exp, e_log, e_log1p, const, the sigmoid and
softplus of the header, to_ld / to_bound, PoolRef) is that of tests/lik_cases.py, imported, with its assumed budgets
(2 ulp for exp / log / log1p) and its MARGIN.

Seven per-sample quantities at shape r, response y and location l, mu = e^l:
    loglik      y l - (y + r) log(mu + r)                     (no normalising constant)
    d1          y - (y + r) mu / (mu + r)
    info        (y + r) mu r / (mu + r)^2
    dinfo       -(y + r) mu r (mu - r) / (mu + r)^3
    dd1_aux     mu r / (mu + r)^2 (y - mu)                    d d1 / dlog r
    dinfo_aux   -mu r / (mu + r)^2 (y (r - mu) - 2 r mu) / (y + r)     d info / dlog r as the reference has it
    aux_term    log(mu + r) + (y + r) / (mu + r)              the per-observation part of the explicit shape gradient
Exact reference: these closed forms in mpmath at 80 digits (e^1000 is an ordinary mpf). Bound: the running error
bound of the header's own formulas in t = l - log r, p = sigmoid(t), q = sigmoid(-t).

Informativeness scale (asserted by test_lik_nb_reference.py, bound <= 1e-3 scale on the main grid): |exact|, and for
the quantities that cross 0 inside the grid the information beside it, the scale a Newton step divides by: d1 and
dd1_aux (0 at mu = y), dinfo (0 at mu = r), dinfo_aux; for loglik and aux_term, whose log(mu + r) crosses 0 at mu + r
= 1, max(|exact|, r): the value's own size away from that crossing.

Host sums: sum_v c_v lgamma(v + r) and sum_v c_v digamma(v + r) over the distinct responses ascending. digamma is
Algorithm AS 103 (recurrence to x >= 8.5, then five terms of the asymptotic series; the first dropped term
691 / (32760 x^12) is added to its bound); lgamma is the C library's, with an ASSUMED budget of UF_LGAMMA ulp of
max(|value|, 1) (its error near its zeros at 1 and 2 is absolute, not relative).
"""
import ctypes
import functools
import math
import os
import sys

import mpmath
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lik_cases as lc  # noqa: E402
from lik_cases import (DBL_MAX, E, LD, MAIN_L, POOL, TINY, U, PoolRef, e_exp, e_log, e_sum,  # noqa: E402,F401
                       f_sigmoid, f_softplus, mpf, to_bound, to_ld)

NB = 5
NB_QUANTS = ("loglik", "d1", "info", "dinfo", "dd1_aux", "dinfo_aux", "aux_term")
POINT_QUANTS = NB_QUANTS[:4]
AUX_QUANTS = NB_QUANTS[4:]
NB_Y = (0., 1., 2., 7., 50., 1e4)
NB_R = (0.05, 1., 2.5, 400.)
NB_TAIL_L = np.array([700., -700., 745., -745., 1000.])
NB_PATH_AUX = 2.5
UF_LGAMMA = 8


def formulas(r, y, l, lf):
    """the nb_* functions of lik_device.h over E; l: E of the location, lf: the float64 location the device holds"""
    log_r = e_log(E(r))
    t = l - log_r
    tf = lf - math.log(r)
    p, q = f_sigmoid(t, tf), f_sigmoid(-t, -tf)
    sp, sm = f_softplus(t, tf), f_softplus(-t, -tf)
    pq = p * q
    return dict(loglik=-y * sm - r * (log_r + sp), d1=y * q - r * p, info=(y + r) * pq, dinfo=-(y + r) * pq * (p - q),
                dd1_aux=p * (y * q - r * p), dinfo_aux=-(p * r) * (y * (q - p) - 2 * (r * p)) / (y + r),
                aux_term=log_r + sp + (y + r) * q / r)


def exact(r, y, l):
    l, r, y = mpf(l), mpf(r), mpf(y)
    mu = mpmath.exp(l)
    s = mu + r
    k = mu * r / (s * s)
    log_s = mpmath.log(r) + mpmath.log1p(mu / r)   # log(mu + r); 80 digits do not hold 1 + e^-700
    return dict(loglik=y * l - (y + r) * log_s, d1=y - (y + r) * mu / s, info=(y + r) * k,
                dinfo=-(y + r) * k * (mu - r) / s, dd1_aux=k * (y - mu),
                dinfo_aux=-k * (y * (r - mu) - 2 * r * mu) / (y + r), aux_term=log_s + (y + r) / s)


@functools.lru_cache(maxsize=None)
def point_reference(r, y, mode, offset=None):
    if offset is None:
        l, lf = E(mode), mode
    else:
        l, lf = E(mode) + E(offset), mode + offset
    ex = exact(r, y, mpf(mode) + (0 if offset is None else mpf(offset)))
    fm = formulas(r, y, l, lf)
    return ex, {q: fm[q].e for q in NB_QUANTS}


class Ref:
    """exact values (longdouble), bounds (float64) and scales of a block of points at one (r, y)"""

    def __init__(self, r, y, ls):
        n = len(ls)
        self.r = r
        self.exact = {q: np.zeros(n, LD) for q in NB_QUANTS}
        self.bound = {q: np.zeros(n) for q in NB_QUANTS}
        self.exact_mp = {q: [None] * n for q in NB_QUANTS}
        for i in range(n):
            ex, bd = point_reference(float(r), float(y), float(ls[i]))
            for q in NB_QUANTS:
                self.exact[q][i] = to_ld(ex[q])
                self.bound[q][i] = to_bound(bd[q])
                self.exact_mp[q][i] = ex[q]

    def ratios(self, q, got):
        """|got - exact| / bound (0 / 0 = 0); inf where got is not finite (every exact value here is a double)"""
        got = np.asarray(got)
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs(got.astype(LD) - self.exact[q])
        with np.errstate(divide="ignore", invalid="ignore"):
            rr = np.where(err == 0, LD(0), err / self.bound[q].astype(LD)).astype(float)
        rr[~np.isfinite(got)] = np.inf
        return rr

    def scale(self, q):
        s = np.array([float(abs(v)) for v in self.exact_mp[q]])
        if q in ("d1", "dinfo", "dd1_aux", "dinfo_aux"):
            s = np.maximum(s, np.array([float(abs(v)) for v in self.exact_mp["info"]]))
        if q in ("loglik", "aux_term"):
            s = np.maximum(s, self.r)
        return s


def grid(which="main"):
    ls = MAIN_L if which == "main" else NB_TAIL_L
    return [(r, y, ls.copy()) for r in NB_R for y in NB_Y]


@functools.lru_cache(maxsize=None)
def grid_reference(which):
    return [(r, y, ls, Ref(r, y, ls)) for r, y, ls in grid(which)]


# ------------------------------------------------------------------------------------------ float64 stand-in
def _sp(x):
    return math.log1p(math.exp(-abs(x))) + max(x, 0.)


def standin(r, y, l, naive=False):
    """the header's formulas in float64 (math); naive: d1 and info through mu / (mu + r) as the definitions are
    written (the seeded defect: 1 - p has no digit left for l >> log r, and e^l overflows)"""
    log_r = math.log(r)
    t = l - log_r
    p, q = lc._sigmoid64(t), lc._sigmoid64(-t)
    out = dict(loglik=-y * _sp(-t) - r * (log_r + _sp(t)), d1=y * q - r * p, info=(y + r) * (p * q),
               dinfo=-(y + r) * (p * q) * (p - q), dd1_aux=p * (y * q - r * p),
               dinfo_aux=-(p * r) * (y * (q - p) - 2. * (r * p)) / (y + r), aux_term=log_r + _sp(t) + (y + r) * q / r)
    if naive:
        mu = lc._exp64(l)
        with np.errstate(all="ignore"):
            pn = np.float64(mu) / (np.float64(mu) + r)
            out["d1"] = float(y - (y + r) * pn)
            out["info"] = float((y + r) * np.float64(mu) * r / ((np.float64(mu) + r) * (np.float64(mu) + r)))
    return out


def standin_block(r, y, ls, naive=False):
    rows = [standin(float(r), float(y), float(l), naive) for l in ls]
    return {q: np.array([row[q] for row in rows]) for q in NB_QUANTS}


# ------------------------------------------------------------------------------------------ host table sums
def digamma_asa103(x):
    """float64 copy of digamma_asa103 (csrc/laplace_newton.h)"""
    if x <= 0.000001:
        return -0.57721566490153286060 - 1.0 / x + 1.6449340668482264365 * x
    value, x2 = 0., x
    while x2 < 8.5:
        value = value - 1.0 / x2
        x2 = x2 + 1.0
    r = 1.0 / x2
    value = value + math.log(x2) - 0.5 * r
    r = r * r
    return value - r * (1.0 / 12.0 - r * (1.0 / 120.0 - r * (1.0 / 252.0 - r * (1.0 / 240.0 - r * (1.0 / 132.0)))))


def e_digamma(x):
    """the algorithm over E at the double x > 1e-6 (every table entry is y + r >= r), with its truncation"""
    value, x2, xf = E(0), E(x), x
    while xf < 8.5:
        value = value - 1 / x2
        x2 = x2 + 1
        xf = xf + 1.0
    r = 1 / x2
    value = value + e_log(x2) - r.half()
    r2 = r * r
    series = r2 * (lc.const(mpf(1) / 12) - r2 * (lc.const(mpf(1) / 120) - r2 * (lc.const(mpf(1) / 252) - r2 * (
        lc.const(mpf(1) / 240) - r2 * lc.const(mpf(1) / 132)))))
    out = value - series
    return E(out.v, out.e + mpf(691) / 32760 / x2.v ** 12)


def table_of(y):
    vals, cnt = np.unique(np.asarray(y, dtype=np.float64), return_counts=True)
    return vals, cnt.astype(np.float64)


def table_sums64(y, r):
    """the host's SumOverY in float64: ascending distinct values, c_v f(v + r) added in that order"""
    vals, cnt = table_of(y)
    sl = sd = 0.
    for v, c in zip(vals, cnt):
        sl += c * math.lgamma(v + r)
        sd += c * digamma_asa103(v + r)
    return sl, sd


def table_reference(y, r):
    """exact sum_i lgamma(y_i + r), sum_i digamma(y_i + r) at the doubles y_i + r and their bounds"""
    vals, cnt = table_of(y)
    tl, td = [], []
    for v, c in zip(vals, cnt):
        x = float(v + r)                                  # the double the host passes on
        lg = mpmath.loggamma(mpf(x))
        tl.append(E(lg, UF_LGAMMA * 2 * U * max(abs(lg), 1)) * float(c))
        dg = e_digamma(x)
        td.append(E(mpmath.digamma(mpf(x)), dg.e + abs(dg.v - mpmath.digamma(mpf(x)))) * float(c))
    sl, sd = e_sum(tl), e_sum(td)
    return (to_ld(sl.v), to_bound(sl.e)), (to_ld(sd.v), to_bound(sd.e))


# ------------------------------------------------------------------------------------------ path cases
@functools.lru_cache(maxsize=None)
def pool(with_offset):
    """POOL samples: counts with a few large ones, moderate locations (|mode + offset| <= 7)"""
    r = np.random.default_rng(lc._stable_seed("nb-pool", with_offset))
    y = r.negative_binomial(1.5, 0.3, POOL).astype(float)
    y[:3] = (0., 1., 250.)
    return dict(y=y, mode=r.uniform(-3., 3., POOL), off=r.uniform(-4., 4., POOL) if with_offset else None)


@functools.lru_cache(maxsize=None)
def grouped_reference(with_offset, K):
    """eta = F + sum_k b[level_k] as lik_cases.grouped_reference, then the seven quantities per pool sample"""
    pl, R = pool(with_offset), PoolRef()
    _, _, b, lev = lc.grouped_case(NB, with_offset, K, POOL)
    for k in range(POOL):
        y = float(pl["y"][k])
        f0 = float(pl["off"][k]) if with_offset else 0.
        eta, etaf, etax = E(f0), f0, mpf(f0)
        for j in range(K):
            bj = float(b[lev[j, k]])
            eta, etaf, etax = eta + E(bj), etaf + bj, etax + mpf(bj)
        ex = exact(NB_PATH_AUX, y, etax)
        fm = formulas(NB_PATH_AUX, y, eta, etaf)
        for q in NB_QUANTS:
            R.put(q, k, ex[q], fm[q].e)
    return R


def eta64(with_offset, K, n):
    """the float64 eta the kernels form (F first, then the effects in order) for the n entries of a grouped case"""
    pl = pool(with_offset)
    idx, glev, b, _ = lc.grouped_case(NB, with_offset, K, n)
    eta = pl["off"][idx].copy() if with_offset else np.zeros(n)
    for j in range(K):
        eta = eta + b[glev[j]]
    return idx, glev, b, eta


# ------------------------------------------------------------------------------------------ the hooks
def _lib():
    lib = lc._lib()
    if not getattr(lib, "_lik_nb_typed", False):
        c = ctypes
        Dp = c.POINTER(c.c_double)
        lib.GPB_TestLikAuxPoint.argtypes = [c.c_int, c.c_double, c.c_int, Dp, Dp, Dp, Dp, Dp, c.POINTER(c.c_int)]
        lib._lik_nb_typed = True
    return lib


def point_hook(r, y, loc):
    """GPB_TestLikPoint and GPB_TestLikAuxPoint at likelihood 5: dict of the seven quantities"""
    y, loc = np.ascontiguousarray(y, dtype=np.float64), np.ascontiguousarray(loc, dtype=np.float64)
    out = lc.point_hook(NB, r, y, loc)
    assert np.isnan(out.pop("dinfo_lowrank")).all()      # the low-rank path does not have this likelihood
    n = y.size
    aux = {q: np.full(n, lc.SENTINEL) for q in AUX_QUANTS}
    g = ctypes.c_int(-1)
    lc._check(_lib().GPB_TestLikAuxPoint(NB, r, n, lc._dp(y), lc._dp(loc), *[lc._dp(aux[q]) for q in AUX_QUANTS],
                                         ctypes.byref(g)))
    assert g.value == 0, "a guard word of the shape outputs changed"
    out.update(aux)
    return out
