"""Cases, exact references and error bounds of the likelihood-layer tests, shared by tests/test_gpu_lik_ops.py (the
device functions of csrc/lik_device.h and the per-sample kernels of the Laplace paths through GPB_TestLikPoint /
GPB_TestLikPath) and tests/test_lik_reference.py (CPU: a float64 stand-in of the header's formulas meets every
bound, the bounds are informative, planted defects exceed them).

Exact reference: mpmath at 80 digits. The probit quantities come from erfc directly (Phi(x) = erfc(-x / sqrt 2) / 2,
r = phi / Phi; y = 0 by the symmetry l -> -l of the y = 1 closed forms, not by a second set of formulas), the logit,
Poisson, gamma and Gaussian ones from their closed forms.

Bound: a first-order running error bound, carried in mpmath beside the value of the very formula lik_device.h
evaluates (class E: a value and a bound on the float64 result's distance from it).
  + - * / sqrt      half an ulp of the result: U |z|, U = 2^-53, plus 2^-1075 where the result may be a denormal
  exp log log1p     UF_ELEM = 2 ulp of the result (2^-52 |z| each), erfc UF_ERFC = 8 ulp. No copy of the HIP math
                    API accuracy table is at hand, so these budgets are ASSUMED, not measured.
  constants         a literal of the header is the double next to the real constant: U |c|
  series branch     normal_log_cdf past u = 37 keeps 1 - 1/u^2 + ... + 10395/u^12; the first dropped term
                    135135 / u^14 is added to the series' bound (relative in Phi)
  sums              the per-term bounds plus (terms - 1) U sum |term|
  propagation       first order: |f'(x)| e_x through a function, |y| e_x + |x| e_y through a product, ...
The whole bound is multiplied by MARGIN = 2 for the different association order of fused code (fma contraction).
No bound is tuned to what a kernel or the stand-in gives.

Informativeness (asserted by test_lik_reference.py): on the main grid no (point, quantity) has a bound above
1e-3 scale, scale = |exact|; for dinfo max(|exact dinfo|, |exact info|), because logit dinfo crosses 0 at l = 0, and
for d1 max(|exact d1|, |exact info|) for the same reason: d1 crosses 0 at the sample's own mode, which the grid
holds exactly (Poisson and gamma y = 1 at l = +-0, the Gaussian y = l = 0.37), and no bound can be below 1e-3 of an
exact 0; the information is the scale a Newton step divides d1 by. The derived bounds meet the criterion on the whole
grid, probit dinfo at |l| = 36 included (largest bound / scale 2.3e-7 there), so no quantity's grid is narrowed.

Float64 stand-in (math / numpy, this machine's libm), largest error / bound on the main grid, printed by
tests/test_lik_reference.py: see that module's docstring.
"""
import ctypes
import functools
import math
import os
import sys

import mpmath
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from latent_ops_cases import LD, HookError, _dp, _ip, assert_longdouble  # noqa: E402,F401

mp = mpmath.mp
mp.dps = 80
mpf = mpmath.mpf

U = mpf(2) ** -53
TINY = mpf(2) ** -1075          # half the spacing of the denormals
UF_ELEM, UF_ERFC = 2, 8          # assumed ulp budgets of exp / log / log1p and of erfc (see the docstring)
MARGIN = 2
DBL_MAX = mpf(sys.float_info.max)
DBL_MIN = mpf(sys.float_info.min)
PROBIT_SERIES_FROM = 37.0        # kProbitSeriesFrom of lik_device.h
LOG100 = 4.605170185988091       # kMaxChangeMode of vif_laplace.hip

GAUSSIAN, LOGIT, PROBIT, POISSON, GAMMA = 0, 1, 2, 3, 4
LIK_NAMES = {GAUSSIAN: "gaussian", LOGIT: "bernoulli_logit", PROBIT: "bernoulli_probit", POISSON: "poisson",
             GAMMA: "gamma"}
QUANTS = ("loglik", "d1", "info", "dinfo")


# ------------------------------------------------------------------------------------------ running error bound
class E:
    """v: the formula's value in exact arithmetic; e: bound on |float64 result - v| (first order)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v = mpf(v)
        self.e = mpf(e)

    @staticmethod
    def lift(x):
        return x if isinstance(x, E) else E(x)

    def _rounded(self, v, e, ulps=None):
        rnd = U * abs(v) if ulps is None else ulps * 2 * U * abs(v)
        return E(v, e + rnd + TINY)

    def __neg__(self):
        return E(-self.v, self.e)

    def __abs__(self):
        return E(abs(self.v), self.e)

    def __add__(self, o):
        o = E.lift(o)
        return self._rounded(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = E.lift(o)
        return self._rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return E.lift(o) - self

    def __mul__(self, o):
        o = E.lift(o)
        return self._rounded(self.v * o.v, abs(self.v) * o.e + abs(o.v) * self.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.lift(o)
        return self._rounded(self.v / o.v, self.e / abs(o.v) + abs(self.v) * o.e / (o.v * o.v))

    def __rtruediv__(self, o):
        return E.lift(o) / self

    def half(self):
        return E(self.v / 2, self.e / 2)       # exact in binary


def const(true_value):
    """a literal of the header: the double next to the real constant"""
    return E(true_value, U * abs(mpf(true_value)))


def e_exp(x):
    v = mpmath.exp(x.v)
    return x._rounded(v, v * x.e, UF_ELEM)


def e_log(x):
    return x._rounded(mpmath.log(x.v), x.e / abs(x.v), UF_ELEM)


def e_log1p(x):
    return x._rounded(mpmath.log1p(x.v), x.e / abs(1 + x.v), UF_ELEM)


def e_erfc(x):
    v = mpmath.erfc(x.v)
    return x._rounded(v, 2 / mpmath.sqrt(mpmath.pi) * mpmath.exp(-x.v * x.v) * x.e, UF_ERFC)


def e_sqrt(x):
    v = mpmath.sqrt(x.v)
    return x._rounded(v, x.e / (2 * v) if v > 0 else mpmath.sqrt(x.e))


def e_sum(terms):
    """a sum of E terms in any order: per-term bounds plus (terms - 1) U sum |term|"""
    v = mpmath.fsum(t.v for t in terms)
    e = mpmath.fsum(t.e for t in terms) + (len(terms) - 1) * U * mpmath.fsum(abs(t.v) for t in terms)
    return E(v, e)


C_SQRT1_2 = const(1 / mpmath.sqrt(2))
C_LN2 = const(mpmath.log(2))
C_LOGSQRT2PI = const(mpmath.log(2 * mpmath.pi) / 2)
SERIES_COEF = (-1, 3, -15, 105, -945, 10395)
SERIES_DROPPED = 135135


# ---- the header's formulas over E (l: E; y, aux: floats; branches decided on the float64 inputs, as on the device)
def f_sigmoid(x, xf):
    if xf >= 0.:
        return 1 / (1 + e_exp(-x))
    ex = e_exp(x)
    return ex / (1 + ex)


def f_softplus(x, xf):
    s = e_log1p(e_exp(-abs(x)))
    return s + x if xf > 0. else s + 0       # + fmax(x, 0.)


def f_log_pdf(x):
    return (-x * x).half() - C_LOGSQRT2PI


def f_log_cdf(x, xf):
    if xf < 0.:
        u = -x
        if -xf <= PROBIT_SERIES_FROM:
            return -C_LN2 + e_log(e_erfc(u * C_SQRT1_2))
        u2 = u * u
        v = 1 / u2
        s = E(SERIES_COEF[-1]) * v
        for c in SERIES_COEF[-2::-1]:
            s = v * (c + s)
        s = 1 + s
        s = E(s.v, s.e + SERIES_DROPPED / u2.v ** 7)     # truncation, relative in Phi; the series is 1 - O(1 / u^2)
        log2pi = e_log(2 * const(mpmath.pi))
        return -u2.half() - e_log(u) - log2pi.half() + e_log(s)
    q = e_erfc(x * C_SQRT1_2).half()
    if q.v < TINY:                 # the float64 erfc is 0 there and the code returns 0.: the error is Q itself
        return E(0, q.v + q.e)
    return e_log1p(-q)


def f_mills(x, xf, flip):
    """flip False: phi(x) / Phi(x); True: phi(x) / (1 - Phi(x))"""
    cdf = f_log_cdf(-x, -xf) if flip else f_log_cdf(x, xf)
    return e_exp(f_log_pdf(x) - cdf)


def formulas(lik, aux, y, l, lf):
    """the four functions of lik_device.h as E; l: E of the location, lf: the float64 location the device holds"""
    if lik == GAUSSIAN:
        r = y - l
        return dict(loglik=(-r * r).half() / aux - C_LOGSQRT2PI - e_log(E(aux)).half(), d1=r / aux,
                    info=1 / E(aux), dinfo=E(0))
    if lik == POISSON:
        ex = e_exp(l)
        return dict(loglik=y * l - ex, d1=y - ex, info=ex, dinfo=ex)
    if lik == GAMMA:
        em = e_exp(-l)
        w = aux * E(y) * em
        return dict(loglik=-aux * (l + y * em), d1=aux * (y * em - 1), info=w, dinfo=-w)
    if lik == LOGIT:
        p, q = f_sigmoid(l, lf), f_sigmoid(-l, -lf)
        if y == 1.:
            ll, d1 = -f_softplus(-l, -lf), q
        else:
            assert y == 0.
            ll, d1 = -f_softplus(l, lf), -p
        return dict(loglik=ll, d1=d1, info=p * q, dinfo=-p * q * (p - q))
    assert lik == PROBIT and y in (0., 1.)
    x2 = l * l
    if y == 0.:
        r = f_mills(l, lf, True)
        return dict(loglik=f_log_cdf(-l, -lf), d1=-r, info=-r * (l - r), dinfo=-r * (1 - x2 + r * (3 * l - 2 * r)))
    r = f_mills(l, lf, False)
    return dict(loglik=f_log_cdf(l, lf), d1=r, info=r * (l + r), dinfo=-r * (x2 - 1 + r * (3 * l + 2 * r)))


# ------------------------------------------------------------------------------------------ exact closed forms
def exact(lik, aux, y, l):
    """loglik, d1, info, dinfo at the real location l (mpf), from closed forms independent of the header's"""
    l, aux, y = mpf(l), mpf(aux), mpf(y)
    if lik == GAUSSIAN:
        return dict(loglik=-(y - l) ** 2 / (2 * aux) - mpmath.log(2 * mpmath.pi * aux) / 2, d1=(y - l) / aux,
                    info=1 / aux, dinfo=mpf(0))
    if lik == POISSON:
        ex = mpmath.exp(l)
        return dict(loglik=y * l - ex, d1=y - ex, info=ex, dinfo=ex)
    if lik == GAMMA:
        w = aux * y * mpmath.exp(-l)
        return dict(loglik=-aux * l - w, d1=w - aux, info=w, dinfo=-w)
    if lik == LOGIT:
        p, q = 1 / (1 + mpmath.exp(-l)), 1 / (1 + mpmath.exp(l))
        ll = -mpmath.log1p(mpmath.exp(-l)) if y == 1 else -mpmath.log1p(mpmath.exp(l))
        return dict(loglik=ll, d1=q if y == 1 else -p, info=p * q, dinfo=-p * q * mpmath.tanh(l / 2))
    s = 1 if y == 1 else -1          # y = 0 is y = 1 at -l
    x = s * l
    Phi = mpmath.erfc(-x / mpmath.sqrt(2)) / 2
    r = mpmath.exp(-x * x / 2) / mpmath.sqrt(2 * mpmath.pi) / Phi
    # log Phi from the small tail on either side (1 - 1e-85 is 1 at any working precision)
    logPhi = mpmath.log(Phi) if x < 0 else mpmath.log1p(-mpmath.erfc(x / mpmath.sqrt(2)) / 2)
    return dict(loglik=logPhi, d1=s * r, info=r * (x + r), dinfo=-s * r * (x * x - 1 + r * (3 * x + 2 * r)))


def to_ld(x):
    """mpf -> numpy.longdouble (two float64 pieces; exact to 2^-64 relative); beyond the double range: +-inf"""
    x = mpf(x)
    if abs(x) > DBL_MAX:
        return LD(np.inf) if x > 0 else LD(-np.inf)
    hi = float(x)
    return LD(hi) + LD(float(x - mpf(hi)))


def to_bound(e):
    """mpf bound -> float64, rounded up, MARGIN applied; a bound too large for a double is inf"""
    e = MARGIN * mpf(e)
    if e > DBL_MAX:
        return np.inf
    f = float(e)
    return float(np.nextafter(f, np.inf))


@functools.lru_cache(maxsize=None)
def point_reference(lik, aux, y, mode, offset=None):
    """exact values and bounds of the four quantities at the real location mode (+ offset): two dicts of mpf"""
    if offset is None:
        l, lf = E(mode), mode
    else:
        l, lf = E(mode) + E(offset), mode + offset
    ex = exact(lik, aux, y, mpf(mode) + (0 if offset is None else mpf(offset)))
    fm = formulas(lik, aux, y, l, lf)
    return ex, {q: fm[q].e for q in QUANTS}, fm


# ------------------------------------------------------------------------------------------ float64 stand-in
def _sigmoid64(x):
    if x >= 0.:
        return 1. / (1. + math.exp(-x))
    e = math.exp(x)
    return e / (1. + e)


def _softplus64(x):
    return math.log1p(math.exp(-abs(x))) + max(x, 0.)


def _exp64(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


class StandIn:
    """the header's formulas in float64 (math); defect: one of DEFECTS planted, original: the header before the
    fixes this suite forced (erfc until it returns 0, three series terms, p (1 - p), y l - softplus(l))"""

    def __init__(self, defect=None, original=False):
        self.defect, self.original = defect, original

    def log_pdf(self, x):
        return -x * x / 2. - 0.91893853320467274178

    def log_cdf(self, x):
        if x < 0.:
            u = -x
            if self.original:
                e = math.erfc(u * 0.70710678118654752440)
                if e > 0.:
                    return -0.69314718055994530942 + math.log(e)
                u2 = u * u
                series = 1. - 1. / u2 + 3. / (u2 * u2)
                return -0.5 * u2 - math.log(u) - 0.5 * math.log(2. * 3.14159265358979323846) + math.log(series)
            if u <= PROBIT_SERIES_FROM:
                return -0.69314718055994530942 + math.log(math.erfc(u * 0.70710678118654752440))
            u2 = u * u
            if math.isinf(u2):
                return -math.inf
            v = 1. / u2
            c1 = 1. if self.defect == "series-sign" else -1.
            series = 1. + v * (c1 + v * (3. + v * (-15. + v * (105. + v * (-945. + v * 10395.)))))
            return -0.5 * u2 - math.log(u) - 0.5 * math.log(2. * 3.14159265358979323846) + math.log(series)
        q = 0.5 * math.erfc(x * 0.70710678118654752440)
        if q == 0.:
            return 0.
        return math.log1p(-q)

    def mills_phi(self, x):
        return _exp64(self.log_pdf(x) - self.log_cdf(x))

    def mills_omp(self, x):
        if self.defect == "mills":
            return self.mills_phi(x)
        return _exp64(self.log_pdf(x) - self.log_cdf(-x))

    def point(self, lik, aux, y, l):
        """(loglik, d1, info, dinfo) as the device functions compute them"""
        d = self.defect
        if lik == GAUSSIAN:
            r = y - l
            return (-r * r / 2. / aux - 0.91893853320467274178 - 0.5 * math.log(aux), r / aux, 1. / aux, 0.)
        if lik == POISSON:
            ex = _exp64(l)
            return (y * l - ex, y - ex, ex, -ex if d == "poisson-dinfo-sign" else ex)
        if lik == GAMMA:
            em = _exp64(-l)
            return (-aux * (l + y * em), aux * (y * em - 1.), aux * y * em, -y * em if d == "gamma-aux" else -aux * y * em)
        if lik == LOGIT:
            p, q = _sigmoid64(l), _sigmoid64(-l)
            if self.original:
                return (y * l - _softplus64(l), y - p, p * (1. - p), -p * (1. - p) * (2. * p - 1.))
            ll = -_softplus64(-l) if y == 1. else -_softplus64(l)
            d1 = q if y == 1. else y - p
            return (ll, d1, p * q, -p * q * ((q - p) if d == "2p-1" else (p - q)))
        y0 = (y == 0.) != (d == "probit-branches")
        x2 = l * l
        if y0:
            r = self.mills_omp(l)
            return (self.log_cdf(-l), -r, -r * (l - r), -r * (1. - x2 + r * (3. * l - 2. * r)))
        r = self.mills_phi(l)
        return (self.log_cdf(l), r, r * (l + r), -r * (x2 - 1. + r * (3. * l + 2. * r)))

    def points(self, lik, aux, y, loc):
        out = np.array([self.point(lik, aux, float(a), float(b)) for a, b in zip(y, loc)])
        return {q: out[:, k] for k, q in enumerate(QUANTS)}


POINT_DEFECTS = ("probit-branches", "mills", "2p-1", "series-sign", "gamma-aux", "poisson-dinfo-sign")


# ------------------------------------------------------------------------------------------ grids
def _main_l():
    """about 300 locations in [-36, 36]: a regular step, irrational offsets, +-0 and values within 1e-10 of 0"""
    reg = np.arange(-36., 36.25, 0.5)                                  # 145
    irr = np.concatenate([np.arange(-35., 36., 1.) + math.sqrt(2.) / 3., -np.arange(-35., 36., 1.) - math.pi / 7.])
    irr = irr[np.abs(irr) <= 36.]
    near0 = np.array([0., -0., 1e-10, -1e-10, 3.3e-11, -7.1e-12, 1e-300, -1e-300])
    frac = np.array([0.1, -0.1, 0.37, -0.37, 2.2250738585072014e-308])
    return np.concatenate([reg, irr, near0, frac])


MAIN_L = _main_l()
BERNOULLI_TAIL_L = np.concatenate([s * np.concatenate([np.arange(37.5, 39.0001, 0.05), [40., 100., 700., 1000.]])
                                   for s in (1., -1.)])
COUNT_TAIL_L = np.array([700., -700., 745., -745.])


def lik_settings(lik):
    """the (aux, y) pairs of a likelihood on the grids"""
    if lik in (LOGIT, PROBIT):
        return [(1., 0.), (1., 1.)]
    if lik == POISSON:
        return [(1., y) for y in (0., 1., 7., 1000.)]
    if lik == GAMMA:
        return [(a, y) for a in (0.3, 1., 7.) for y in (1e-3, 1., 50.)]
    return [(a, y) for a in (1e-3, 1., 40.) for y in (0.37,)]


def grid(lik, which="main"):
    """(aux, y array, l array) blocks of a grid: main, or tail (Bernoulli: +-37.5 .. +-1000; counts: +-700, +-745)"""
    if which == "main":
        ls = MAIN_L
    elif lik in (LOGIT, PROBIT):
        ls = BERNOULLI_TAIL_L
    elif lik in (POISSON, GAMMA):
        ls = COUNT_TAIL_L
    else:
        return []
    return [(aux, np.full(ls.size, y), ls.copy()) for aux, y in lik_settings(lik)]


class Ref:
    """exact values (longdouble; +-inf beyond the double range), bounds (float64) and scales of a block of points"""

    def __init__(self, lik, aux, y, mode, offset=None):
        n = len(y)
        self.exact = {q: np.zeros(n, LD) for q in QUANTS}
        self.bound = {q: np.zeros(n) for q in QUANTS}
        self.exact_mp = {q: [None] * n for q in QUANTS}
        for i in range(n):
            ex, bd, _ = point_reference(lik, float(aux), float(y[i]), float(mode[i]),
                                        None if offset is None else float(offset[i]))
            for q in QUANTS:
                self.exact[q][i] = to_ld(ex[q])
                self.bound[q][i] = to_bound(bd[q])
                self.exact_mp[q][i] = ex[q]

    def representable(self, q):
        """where the exact value is a finite double"""
        return np.array([abs(v) <= DBL_MAX for v in self.exact_mp[q]])

    def ratios(self, q, got):
        """|got - exact| / bound where the exact value is finite (0 / 0 = 0); elsewhere got must be that infinity"""
        fin = self.representable(q)
        r = np.zeros(len(got))
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs(np.asarray(got, LD) - self.exact[q])
        b = self.bound[q].astype(LD)
        with np.errstate(divide="ignore", invalid="ignore"):
            rr = np.where(err == 0, LD(0), err / b)
        r[fin] = rr[fin].astype(float)
        r[fin & ~np.isfinite(np.asarray(got, float))] = np.inf
        bad_inf = ~fin & (np.asarray(got, LD) != self.exact[q])
        r[bad_inf] = np.inf
        return r

    def scale(self, q):
        s = np.array([float(abs(v)) for v in self.exact_mp[q]])
        if q in ("dinfo", "d1"):
            s = np.maximum(s, np.array([float(abs(v)) for v in self.exact_mp["info"]]))
        return s


@functools.lru_cache(maxsize=None)
def grid_reference(lik, which):
    return [(aux, y, l, Ref(lik, aux, y, l)) for aux, y, l in grid(lik, which)]


# ------------------------------------------------------------------------------------------ path cases
PATH_NS = (1, 63, 64, 65, 255, 256, 257, 1000)
WRAP_N = 1024 * 256 + 257        # every path caps its grid at 1024 blocks of 256: the grid-stride loop wraps
POOL = 48                        # distinct samples of a path case; larger n repeat them in a fixed shuffled order
GROUPED, VIF, FITC, DENSE, VECCHIA = 0, 1, 2, 3, 4
PREP, TRIAL, FINAL = 0, 1, 2
PATH_NAMES = {GROUPED: "grouped", VIF: "vif", FITC: "fitc", DENSE: "dense", VECCHIA: "vecchia"}
PATH_AUX = {GAUSSIAN: 0.7, LOGIT: 1., PROBIT: 1., POISSON: 1., GAMMA: 2.5}
GROUP_LEVELS = {1: (5,), 2: (5, 3), 3: (5, 3, 7)}        # uneven level counts


def _rng(*key):
    return np.random.default_rng([abs(hash(str(k))) % (2 ** 31) if isinstance(k, str) else int(k) for k in key])


def _stable_seed(*key):
    s = 0
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=None)
def pool(lik, with_offset):
    """POOL samples: y, mode, offset and the further per-sample inputs of the paths, moderate locations (|mode +
    offset| <= 7; for the Bernoulli likelihoods a few at +-12 .. +-20, where boosting's offset takes them)"""
    r = np.random.default_rng(_stable_seed("pool", lik, with_offset))
    mode = r.uniform(-3., 3., POOL)
    off = r.uniform(-4., 4., POOL) if with_offset else None
    if lik in (LOGIT, PROBIT) and with_offset:
        off[:6] = np.array([12., -12., 16.5, -16.5, 20., -20.]) - mode[:6] + r.uniform(-.1, .1, 6)
    if lik in (LOGIT, PROBIT):
        y = (r.random(POOL) < 0.5).astype(float)
    elif lik == POISSON:
        y = r.poisson(3., POOL).astype(float)
    elif lik == GAMMA:
        y = r.gamma(2., 1., POOL) + 1e-3
    else:
        y = r.normal(0., 1.5, POOL)
    d = dict(y=y, mode=mode, off=off, dvec=r.uniform(0.05, 2., POOL), Dinv=r.uniform(0.3, 5., POOL),
             wst=r.uniform(0.05, 3., POOL), upd=mode + r.uniform(-8., 8., POOL), a=r.normal(0., 1., POOL),
             mupd=mode + r.uniform(-2., 2., POOL), aupd=r.normal(0., 1., POOL), F=r.uniform(-2., 2., POOL),
             yrow=r.uniform(5., 9., POOL))
    # the capped step of vl_trial_kernel must not sit on its threshold (the branch is decided in float64)
    c = np.abs(d["upd"] - mode)
    d["upd"] = np.where(np.abs(c - LOG100) < 1e-3, d["upd"] + 0.01, d["upd"])
    return d


def sample_index(n, key):
    """which pool sample each of the n entries repeats: every pool sample when n >= POOL, in a fixed shuffled order"""
    r = np.random.default_rng(_stable_seed("index", n, key))
    idx = np.concatenate([r.permutation(POOL) for _ in range(n // POOL + 1)])[:n]
    return idx


def gather(pl, idx):
    return {k: (None if v is None else np.ascontiguousarray(v[idx])) for k, v in pl.items()}


def _lds(vals):
    return np.array([to_ld(v) for v in vals], dtype=LD)


def _bds(errs):
    return np.array([to_bound(e) for e in errs])


def _loc(pl, k, trial=None):
    """E and float64 of the location of pool sample k (trial: (E, float) replacing the mode)"""
    m, mf = (E(pl["mode"][k]), float(pl["mode"][k])) if trial is None else trial
    if pl["off"] is None:
        return m, mf
    return m + E(pl["off"][k]), mf + float(pl["off"][k])


class PoolRef:
    """per pool sample: exact value (longdouble), bound (float64) and the mpf pair of named outputs; sums over an
    index list come from the pool's terms and the counts"""

    def __init__(self):
        self.v, self.e, self._arr = {}, {}, {}

    def put(self, name, k, ex, err):
        self.v.setdefault(name, [None] * POOL)[k] = mpf(ex)
        self.e.setdefault(name, [None] * POOL)[k] = mpf(err)

    def arrays(self, name, idx):
        if name not in self._arr:
            self._arr[name] = (_lds(self.v[name]), _bds(self.e[name]))
        ref, bnd = self._arr[name]
        return ref[idx], bnd[idx]

    def total(self, name, idx):
        """exact sum over the entries idx of the per-sample term `name` and its bound (any summation order)"""
        cnt = np.bincount(idx, minlength=POOL)
        v = mpmath.fsum(int(c) * t for c, t in zip(cnt, self.v[name]))
        e = mpmath.fsum(int(c) * t for c, t in zip(cnt, self.e[name]))
        e += (len(idx) - 1) * U * mpmath.fsum(int(c) * abs(t) for c, t in zip(cnt, self.v[name]))
        return to_ld(v), to_bound(e)


def _exact_loc(pl, k, mode=None):
    m = mpf(float(pl["mode"][k])) if mode is None else mode
    return m if pl["off"] is None else m + mpf(float(pl["off"][k]))


@functools.lru_cache(maxsize=None)
def prep_reference(lik, with_offset, stored_w):
    """d1, W, dW and the derived arrays of every path's prep / final kernel per pool sample. stored_w: the derived
    arrays from the stored W (w_update = W_update = 0) instead of the information."""
    pl, aux, R = pool(lik, with_offset), PATH_AUX[lik], PoolRef()
    for k in range(POOL):
        y = float(pl["y"][k])
        l, lf = _loc(pl, k)
        ex = exact(lik, aux, y, _exact_loc(pl, k))
        fm = formulas(lik, aux, y, l, lf)
        for q in QUANTS:
            R.put(q, k, ex[q], fm[q].e)
        mode, dvec, dinv = (mpf(float(pl[key][k])) for key in ("mode", "dvec", "Dinv"))
        if stored_w:
            wx, w = mpf(float(pl["wst"][k])), E(float(pl["wst"][k]))
        else:
            wx, w = ex["info"], fm["info"]
        d1x, d1 = ex["d1"], fm["d1"]
        # rhs = W mode + d1 (every path); vecchia: dw = Dinv + W, sdw = sqrt(dw)
        R.put("rhs", k, wx * mode + d1x, (w * E(mode) + d1).e)
        dw = E(dinv) + w
        R.put("dw", k, dinv + wx, dw.e)
        R.put("sdw", k, mpmath.sqrt(dinv + wx), e_sqrt(dw).e)
        # fitc: DW = 1 / (W d + 1), wdw = sqrt(W)^2 DW, dpwi = 1 / (d + 1 / W) and the logarithms of the final sums
        DW = 1 / (w * E(dvec) + 1)
        R.put("DW", k, 1 / (wx * dvec + 1), DW.e)
        ws = e_sqrt(w)
        R.put("ws", k, mpmath.sqrt(wx), ws.e)
        R.put("wdw", k, wx / (wx * dvec + 1), (ws * ws * DW).e)
        p = 1 / (E(dvec) + 1 / w)
        R.put("dpwi", k, 1 / (dvec + 1 / wx), p.e)
        R.put("log_dpwi", k, mpmath.log(1 / (dvec + 1 / wx)), e_log(p).e)
        R.put("log_w", k, mpmath.log(wx), e_log(w).e)
    return R


@functools.lru_cache(maxsize=None)
def trial_reference(lik, with_offset, kind, lam, first, cap):
    """the trial mode and its log-likelihood term per pool sample. kind "vif": vl_trial_kernel (first, cap at
    log 100); kind "mix": laplace_trial_kernel (mnew, anew and the term a m of the quadratic form)"""
    pl, aux, R = pool(lik, with_offset), PATH_AUX[lik], PoolRef()
    for k in range(POOL):
        y = float(pl["y"][k])
        mf = float(pl["mode"][k])
        m, mx = E(mf), mpf(mf)
        if kind == "vif":
            uf = float(pl["upd"][k])
            if first:
                t, tx, tf = E(uf), mpf(uf), uf
            else:
                t, tx = (1 - E(lam)) * m + E(lam) * E(uf), (1 - mpf(lam)) * mx + mpf(lam) * mpf(uf)
                tf = (1. - lam) * mf + lam * uf
            if cap:
                c = abs(tf - mf)
                assert abs(c - LOG100) > 1e-4, "a trial step on the cap's threshold"
                if c > LOG100:
                    ce = abs(t - m)
                    t = m + (t - m) / ce * E(LOG100)
                    tx = mx + (tx - mx) / abs(tx - mx) * mpf(LOG100)
                    tf = mf + (tf - mf) / c * LOG100
            R.put("trial", k, tx, t.e)
        else:
            af, muf, auf = (float(pl[key][k]) for key in ("a", "mupd", "aupd"))
            if lam == 1.:
                t, tx, tf, an, anx = E(muf), mpf(muf), muf, E(auf), mpf(auf)
            else:
                an = (1 - E(lam)) * E(af) + E(lam) * E(auf)
                anx = (1 - mpf(lam)) * mpf(af) + mpf(lam) * mpf(auf)
                t, tx = (1 - E(lam)) * m + E(lam) * E(muf), (1 - mpf(lam)) * mx + mpf(lam) * mpf(muf)
                tf = (1. - lam) * mf + lam * muf
            R.put("mnew", k, tx, t.e)
            R.put("anew", k, anx, an.e)
            R.put("am", k, anx * tx, (an * t).e)
        l, lf = _loc(pl, k, (t, tf))
        ex = exact(lik, aux, y, _exact_loc(pl, k, tx))
        R.put("loglik", k, ex["loglik"], formulas(lik, aux, y, l, lf)["loglik"].e)
    return R


def grouped_case(lik, with_offset, K, n):
    """glev (K x n, global level indices), b and the index list of a grouped case: sample k sits at level
    (k * (j + 2) + j) mod M_j of effect j"""
    idx = sample_index(n, ("grouped", lik, K))
    counts = GROUP_LEVELS[K]
    cum = np.concatenate([[0], np.cumsum(counts)])
    lev = np.array([[cum[j] + (k * (j + 2) + j) % counts[j] for k in range(POOL)] for j in range(K)], dtype=np.int32)
    b = np.random.default_rng(_stable_seed("b", K)).uniform(-1.5, 1.5, int(cum[-1]))
    return idx, np.ascontiguousarray(lev[:, idx]), b, lev


@functools.lru_cache(maxsize=None)
def grouped_reference(lik, with_offset, K):
    """eta = F + sum_k b[level_k] (F: the pool's offset; 0 without), then the four quantities per pool sample"""
    pl, aux, R = pool(lik, with_offset), PATH_AUX[lik], PoolRef()
    _, _, b, lev = grouped_case(lik, with_offset, K, POOL)
    for k in range(POOL):
        y = float(pl["y"][k])
        f0 = float(pl["off"][k]) if with_offset else 0.
        eta, etaf, etax = E(f0), f0, mpf(f0)
        for j in range(K):
            bj = float(b[lev[j, k]])
            eta, etaf, etax = eta + E(bj), etaf + bj, etax + mpf(bj)
        ex = exact(lik, aux, y, etax)
        fm = formulas(lik, aux, y, eta, etaf)
        for q in QUANTS:
            R.put(q, k, ex[q], fm[q].e)
    return R


OBS_COUNTS = (1, 2, 7)


def obs_case(lik, n, with_obs_offset):
    """an ObsMap over n rows holding 1, 2 and 7 observations in turn: row i's mode is pool sample idx[i]'s, its
    observations are the pool samples idx[i], idx[i] + 1, ... (y and offset of their own)"""
    idx = sample_index(n, ("obs", lik))
    cnt = np.array([OBS_COUNTS[i % 3] for i in range(n)])
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    row = np.repeat(np.arange(n), cnt)
    within = np.arange(ptr[-1]) - ptr[row]
    obs_idx = (idx[row] + within) % POOL
    return idx, cnt, ptr, obs_idx


@functools.lru_cache(maxsize=None)
def obs_reference(lik, with_obs_offset, stored_w):
    """per (pool sample k, count c): sums over the observations k .. k + c - 1 of d1 and the information at
    mode_k + offset_e, then rhs / dw / sdw. Keys "<name><c>"."""
    pl, aux, R = pool(lik, True), PATH_AUX[lik], PoolRef()
    for k in range(POOL):
        mf = float(pl["mode"][k])
        for c in OBS_COUNTS:
            t1, tw, x1, xw = [], [], mpf(0), mpf(0)
            for j in range(c):
                e = (k + j) % POOL
                y, of = float(pl["y"][e]), float(pl["off"][e])
                if with_obs_offset:
                    l, lf, lx = E(mf) + E(of), mf + of, mpf(mf) + mpf(of)
                else:
                    l, lf, lx = E(mf), mf, mpf(mf)
                fm, ex = formulas(lik, aux, y, l, lf), exact(lik, aux, y, lx)
                t1.append(fm["d1"])
                tw.append(fm["info"])
                x1 += ex["d1"]
                xw += ex["info"]
            d1, w = e_sum(t1), e_sum(tw)
            R.put(f"d1{c}", k, x1, d1.e)
            R.put(f"info{c}", k, xw, w.e)
            if stored_w:
                xw, w = mpf(float(pl["wst"][k])), E(float(pl["wst"][k]))
            dinv = mpf(float(pl["Dinv"][k]))
            R.put(f"rhs{c}", k, xw * mpf(mf) + x1, (w * E(mf) + d1).e)
            dw = E(dinv) + w
            R.put(f"dw{c}", k, dinv + xw, dw.e)
            R.put(f"sdw{c}", k, mpmath.sqrt(dinv + xw), e_sqrt(dw).e)
    return R


def by_count(R, name, idx, cnt):
    """exact values and bounds of an ObsMap output for rows with pool samples idx and observation counts cnt"""
    v, b = np.zeros(len(idx), LD), np.zeros(len(idx))
    for c in OBS_COUNTS:
        vc, bc = R.arrays(f"{name}{c}", idx)
        v[cnt == c], b[cnt == c] = vc[cnt == c], bc[cnt == c]
    return v, b


def max_ratio(got, ref, bound):
    """largest |got - ref| / bound (0 / 0 = 0); inf when an entry is not finite"""
    got = np.asarray(got)
    if not np.isfinite(got).all():
        return np.inf
    err = np.abs(got.astype(LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / np.asarray(bound, LD))
    return float(r.max()) if r.size else 0.


# ------------------------------------------------------------------------------------------ the hooks
def _lib():
    c = ctypes
    from gpboost_amd import basic
    lib = basic.lib()
    if not getattr(lib, "_lik_ops_typed", False):
        Dp, I, L, F = c.POINTER(c.c_double), c.c_int, c.c_int64, c.c_double
        PI, PG = c.POINTER(c.c_int32), c.POINTER(c.c_int)
        lib.GPB_TestLikPoint.argtypes = [I, F, I, Dp, Dp, Dp, Dp, Dp, Dp, Dp, PG]
        lib.GPB_TestLikPath.argtypes = [I, I, I, I, F, Dp, Dp, Dp, c.POINTER(Dp), I, PI, L, Dp, Dp, L, Dp, L, F, PI, I,
                                        c.POINTER(Dp), I, Dp, I, PG]
        lib.LGBM_GetLastError.restype = c.c_char_p
        lib._lik_ops_typed = True
    return lib


def last_error():
    return _lib().LGBM_GetLastError().decode("utf-8")


def _check(ret):
    if ret != 0:
        msg = last_error()
        if "HIP error" in msg:          # the device context is gone: nothing more may run on it
            import pytest
            pytest.exit(f"HIP error, session ended: {msg}", returncode=3)
        raise HookError(msg)


SENTINEL = 7.25   # host outputs start as this; the hook overwrites them with what the device holds


def point_hook(lik, aux, y, loc):
    """GPB_TestLikPoint: dict of the four quantities and dinfo_lowrank (launch_lik_dinfo)"""
    y, loc = np.ascontiguousarray(y, dtype=np.float64), np.ascontiguousarray(loc, dtype=np.float64)
    n = y.size
    out = {q: np.full(n, SENTINEL) for q in QUANTS + ("dinfo_lowrank",)}
    g = ctypes.c_int(-1)
    _check(_lib().GPB_TestLikPoint(lik, aux, n, _dp(y), _dp(loc), *[_dp(out[q]) for q in QUANTS + ("dinfo_lowrank",)],
                                   ctypes.byref(g)))
    assert g.value == 0, "a guard word of the point outputs changed"
    return out


def path_raw(path, kernel, n, lik, aux, y, mode, offset, vecs=(), idx=None, arr0=None, arr1=None, mats=None, lam=1.,
             opts=(), want=(), n_scalars=0, idx_len=None):
    """GPB_TestLikPath; want: one flag per output of the kernel. Returns (return code, outputs (None where not
    asked for), scalars, guard)"""
    Dp = ctypes.POINTER(ctypes.c_double)
    keep = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in
            (y, mode, offset, arr0, arr1, mats)]
    y, mode, offset, arr0, arr1, mats = keep
    vecs = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in vecs]
    varr = (Dp * max(len(vecs), 1))(*[_dp(v) if v is not None else None for v in vecs])
    idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    o = np.asarray(opts, dtype=np.int32)
    outs = [np.full(n, SENTINEL) if w else None for w in want]
    oarr = (Dp * max(len(outs), 1))(*[_dp(v) if v is not None else None for v in outs])
    sc = np.full(max(n_scalars, 1), SENTINEL)
    g = ctypes.c_int(-1)
    ret = _lib().GPB_TestLikPath(path, kernel, n, lik, aux, _dp(y), None if mode is None else _dp(mode),
                                 None if offset is None else _dp(offset), varr, len(vecs),
                                 None if idx is None else _ip(idx), (0 if idx is None else idx.size) if idx_len is None else idx_len,
                                 None if arr0 is None else _dp(arr0), None if arr1 is None else _dp(arr1),
                                 0 if arr0 is None else arr0.size, None if mats is None else _dp(mats),
                                 0 if mats is None else mats.size, lam, _ip(o) if o.size else None, o.size, oarr,
                                 len(outs), _dp(sc) if n_scalars else None, n_scalars, ctypes.byref(g))
    return ret, outs, sc[:n_scalars], g.value


def path_hook(*a, **kw):
    ret, outs, sc, g = path_raw(*a, **kw)
    _check(ret)
    assert g == 0, "a guard word changed or a scalar nobody asked for was written"
    return outs, sc


# ------------------------------------------------------------------------------------------ float64 path stand-ins
def standin_prep(lik, g, stored_w=False, offset="ok", si=None):
    """the prep / final kernels' per-sample outputs in float64 on gathered inputs g. offset: "ok", "dropped" or
    "twice" (planted defects)."""
    si = si or StandIn()
    aux, mode = PATH_AUX[lik], g["mode"]
    loc = mode.copy()
    if g["off"] is not None and offset != "dropped":
        loc = loc + g["off"]
        if offset == "twice":
            loc = loc + g["off"]
    out = si.points(lik, aux, g["y"], loc)
    w = g["wst"] if stored_w else out["info"]
    d = dict(out)
    d["rhs"] = w * mode + out["d1"]
    d["dw"] = g["Dinv"] + w
    d["sdw"] = np.sqrt(d["dw"])
    d["DW"] = 1. / (w * g["dvec"] + 1.)
    d["ws"] = np.sqrt(w)
    d["wdw"] = d["ws"] * d["ws"] * d["DW"]
    with np.errstate(divide="ignore"):       # an information of 0 (a planted defect can reach one)
        d["dpwi"] = 1. / (g["dvec"] + 1. / w)
        d["log_dpwi"] = np.log(d["dpwi"])
        d["log_w"] = np.log(w)
    return d


def standin_trial(lik, g, kind, lam, first, cap, si=None):
    si = si or StandIn()
    aux, mode = PATH_AUX[lik], g["mode"]
    d = {}
    if kind == "vif":
        t = g["upd"].copy() if first else (1. - lam) * mode + lam * g["upd"]
        if cap:
            c = np.abs(t - mode)
            with np.errstate(invalid="ignore", divide="ignore"):
                t = np.where(c > LOG100, mode + (t - mode) / c * LOG100, t)
        d["trial"] = t
    else:
        if lam == 1.:
            t, an = g["mupd"].copy(), g["aupd"].copy()
        else:
            an = (1. - lam) * g["a"] + lam * g["aupd"]
            t = (1. - lam) * mode + lam * g["mupd"]
        d["mnew"], d["anew"], d["am"] = t, an, an * t
    loc = t if g["off"] is None else t + g["off"]
    d["loglik"] = si.points(lik, aux, g["y"], loc)["loglik"]
    return d


def standin_grouped(lik, with_offset, K, n, si=None):
    si = si or StandIn()
    pl = pool(lik, with_offset)
    idx, glev, b, _ = grouped_case(lik, with_offset, K, n)
    eta = pl["off"][idx].copy() if with_offset else np.zeros(n)
    for j in range(K):
        eta = eta + b[glev[j]]
    return si.points(lik, PATH_AUX[lik], pl["y"][idx], eta)


def standin_obs(lik, n, with_obs_offset, defect=None, si=None):
    """newton_prep_kernel's row sums over an ObsMap in float64. defect: "row-y" (y[i] read for obs.y[e]) or
    "drop-last" (the last observation of a row dropped)"""
    si = si or StandIn()
    pl, aux = pool(lik, True), PATH_AUX[lik]
    idx, cnt, ptr, obs_idx = obs_case(lik, n, with_obs_offset)
    d1, w = np.zeros(n), np.zeros(n)
    for i in range(n):
        hi = ptr[i + 1] - (1 if defect == "drop-last" and cnt[i] > 1 else 0)
        for e in range(ptr[i], hi):
            m = pl["mode"][idx[i]]
            l = m + pl["off"][obs_idx[e]] if with_obs_offset else m
            y = pl["y"][idx[i]] if defect == "row-y" else pl["y"][obs_idx[e]]
            p = si.point(lik, aux, float(y), float(l))
            d1[i] += p[1]
            w[i] += p[2]
    return d1, w
