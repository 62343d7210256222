"""References for models with several clusters (cluster_ids): independent realisations of one GP.

Nothing here needs a GPU except batch_hook (the GPB_TestDenseBatch call of tests/test_gpu_cluster_ops.py).

R values (R-package/tests/testthat/test_GPModel_gaussian_process.R:599-641 dense, :1208-1243 Vecchia): data
synthetic.rtest_gaussian_y(100), cluster_ids = 40 ones then 60 twos, covariance 'exponential'.
  * predictions at R_PARS = (0.1, 1, 0.15): R_PRED_* (dense) and R_VPRED_* (Vecchia, m = 30, ordering none,
    order_obs_first_cond_all, num_neighbors_pred = 30); tolerance 1e-6 on each sum of absolute differences, the R
    test's own.
  * gradient descent (lr 0.1, Nesterov, acc_rate 0.5, delta 1e-6, relative change in the parameters): 247 iterations
    to R_GD_PARS, summed absolute difference < 1e-6. oracle/internal_optim_oracle.internal_optimize on ClusterSum, the
    two-cluster model object below, gives 247 iterations and a summed difference of 5.7e-7, most of it the R file's
    rounding of its second value. The nll of that loop at its end is R_GD_NLL_ORACLE.

Batched kernel (csrc/dense_batch.hip): batch_compute is a numpy stand-in with the kernel's algebra (right-looking
Cholesky by columns, column sweeps for z and u, W = L^-1 by rows, P = W'W, traces and quadratic forms as sums over
P o C and (u u') o C); run in float64 it is measured against the same algebra in np.longdouble, and each output may
err 8 times the stand-in's own error (max norm per output over the clusters of a case), the convention of
tests/fitc_ops_cases.py: the kernel adds in another order, contracts multiply-adds and has its own exp and log.
"""
from __future__ import annotations

import ctypes
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.fitc_laplace_oracle import _dist, cov_dcov  # noqa: E402
from oracle.internal_optim_oracle import DenseModel  # noqa: E402

LD = np.longdouble

# ------------------------------------------------------------------------------------------------ R values
R_PARS = (0.1, 1., 0.15)
R_PRED_X = np.array([[0.1, 0.9], [0.2, 0.4], [0.7, 0.55]])
R_PRED_IDS = (1, 3, 1)
R_PRED_MEAN = np.array([-0.01437506, 0., 0.93112902])
R_PRED_COV = np.array([[0.743055189, 0., -0.000140644],
                       [0., 1.1, 0.],
                       [-0.000140644, 0., 0.565243468]])
R_VPRED_X = np.array([[0.1, 0.9], [0.2, 0.4], [0.1001, 0.9001]])
R_VPRED_MEAN = np.array([-0.01438585, 0., -0.01500132])
R_VPRED_COV = np.array([[0.7430552, 0., 0.6423148],
                        [0., 1.1, 0.],
                        [0.6423148, 0., 0.7434589]])
R_GD_PARS = np.array([0.05414149, 1.05789166, 0.12702368])
R_GD_ITERS = 247
R_GD_NLL_ORACLE = 129.36951485   # the oracle loop's nll at the R test's estimates
R_VGD_NLL = 129.3761486          # the Vecchia gradient-descent fit's nll, within the R test's 1e-2


def r_data():
    """(coords, y, ids) of the R cluster tests"""
    from gpboost_amd import synthetic
    X, y = synthetic.rtest_gaussian_y(100)
    return X, y, np.array([1] * 40 + [2] * 60)


def split(ids):
    """clusters in order of first appearance: [(id, row indices in their order)]"""
    ids = np.asarray(ids)
    seen = {}
    for i, v in enumerate(ids.tolist()):
        seen.setdefault(v, []).append(i)
    return [(k, np.array(v)) for k, v in seen.items()]


def range_trafo(cov_type, rho):
    return {0: 1. / rho, 1: np.sqrt(3.) / rho, 2: np.sqrt(5.) / rho, 3: 1. / (rho * rho)}[cov_type]


def range_back(cov_type, phi):
    return {0: 1. / phi, 1: np.sqrt(3.) / phi, 2: np.sqrt(5.) / phi, 3: 1. / np.sqrt(phi)}[cov_type]


def dense_predict(X, y, ids, pars, Xp, ids_pred, cov_type=0, predict_response=True):
    """mean and covariance (original scale), one Cholesky per cluster; an unseen id gets the prior"""
    s2, s1, rho = pars
    phi = range_trafo(cov_type, rho)
    ids_pred = np.asarray(ids_pred)
    npred = Xp.shape[0]
    mean, cov = np.zeros(npred), np.zeros((npred, npred))
    train = dict(split(ids))
    for cid, pidx in split(ids_pred):
        xp = Xp[pidx]
        Kpp = cov_dcov(_dist(xp, xp), s1, phi, cov_type)[0]
        np.fill_diagonal(Kpp, s1)
        if cid in train:
            rows = train[cid]
            xo = X[rows]
            Koo = cov_dcov(_dist(xo, xo), s1, phi, cov_type)[0]
            np.fill_diagonal(Koo, s1)
            L = np.linalg.cholesky(Koo + s2 * np.eye(rows.size))
            Kpo = cov_dcov(_dist(xp, xo), s1, phi, cov_type)[0]
            A = np.linalg.solve(L, Kpo.T)
            mean[pidx] = A.T @ np.linalg.solve(L, y[rows])
            Kpp = Kpp - A.T @ A
        if predict_response:
            Kpp = Kpp + s2 * np.eye(pidx.size)
        cov[np.ix_(pidx, pidx)] = Kpp
    return mean, cov


class ClusterSum:
    """duck-types oracle.internal_optim_oracle.DenseModel for several clusters: q, log|Psi|, the quadratic forms and
    the traces are sums over the clusters; sigma^2 is profiled over all n"""

    def __init__(self, X, y, ids, cov_type):
        self.parts = [DenseModel(X[r], None, y[r], cov_type) for _, r in split(ids)]
        self.n = int(sum(p.n for p in self.parts))

    def sums(self, pars, want_grad=True):
        """[log|Psi|, q, s1_var, s1_range, s2_var, s2_range], the layout of DenseSolver::Eval"""
        s = np.zeros(6)
        for p in self.parts:
            Psi, derivs = p._parts(pars)
            L = np.linalg.cholesky(Psi)
            a = np.linalg.solve(Psi, p.y)
            s[0] += 2. * float(np.sum(np.log(np.diag(L))))
            s[1] += float(p.y @ a)
            if want_grad:
                Pinv = np.linalg.inv(Psi)
                for k, D in enumerate(derivs):
                    s[2 + k] += -0.5 * float(a @ D @ a)
                    s[4 + k] += float(np.sum(Pinv * D))
        return s

    def nll(self, pars):
        s = self.sums(pars, False)
        return s[1] / 2. / pars[0] + s[0] / 2. + self.n / 2. * (np.log(pars[0]) + np.log(2. * np.pi))

    def grad(self, pars, profile):
        s = self.sums(pars)
        s2 = s[1] / self.n if profile else pars[0]
        g = [] if profile else [-s[1] / s2 / 2. + self.n / 2.]
        g += [s[2] / s2 + 0.5 * s[4], s[3] / s2 + 0.5 * s[5]]
        return np.array(g), s2


def combine(sums, n, sigma2, profile):
    """combine_partials (csrc/re_model.cpp): nll, gradient, sigma^2"""
    s2 = sums[1] / n if profile else sigma2
    nll = sums[1] / 2. / s2 + sums[0] / 2. + n / 2. * (np.log(s2) + np.log(2. * np.pi))
    g = [] if profile else [-sums[1] / s2 / 2. + n / 2.]
    g += [sums[2] / s2 + 0.5 * sums[4], sums[3] / s2 + 0.5 * sums[5]]
    return nll, np.array(g), s2


def init_pars(X, y, ids, cov_type=0):
    """FindInitCovPar (re_model_template.h:4388-4504) on the transformed scale: var(y) / 2 over all y, 1, and the range
    from the median distance of the first cluster"""
    rows = split(ids)[0][1]
    D = _dist(X[rows], X[rows])
    med = float(np.median(D[np.triu_indices(rows.size, 1)]))
    phi = {0: 6. / med, 1: 9.4 / med, 2: 11.8 / med, 3: 3. / (med / 2.) ** 2}[cov_type]
    return np.array([np.var(y, ddof=1) / 2., 1., phi])


# ------------------------------------------------------------------------------------------------ batched kernel
OUTPUTS = ("logdet", "q", "s1_var", "s1_range", "s2_var", "s2_range", "u")


def _cov_T(R, var, phi, cov_type):
    return cov_dcov(R, var, phi, cov_type)


def batch_compute(X, y, var, phi, cov_type, want_grad, T):
    """one cluster in the kernel's algebra and the arithmetic T; returns None when a pivot is not positive and finite,
    else (sums (6), u)"""
    X = np.asarray(X).astype(T)
    yv = np.asarray(y).astype(T).copy()
    n, d = X.shape
    var, phi = T(var), T(phi)
    S = np.zeros((n, n), dtype=T)
    for q in range(d):
        df = X[:, None, q] - X[None, :, q]
        S = S + df * df
    R = np.sqrt(S)
    C, dC = _cov_T(R, var, phi, cov_type)
    L = np.tril(C)
    L[np.diag_indices(n)] = np.diag(C) + T(1)
    logsum = T(0)
    for k in range(n):
        p = L[k, k]
        if not (p > 0 and np.isfinite(p)):
            return None
        l = np.sqrt(p)
        logsum = logsum + np.log(l)
        col = L[k + 1:, k] / l
        L[k + 1:, k] = col
        L[k, k] = l
        L[k + 1:, k + 1:] -= np.tril(np.outer(col, col))
    qq = T(0)
    for k in range(n):
        zk = yv[k] / L[k, k]
        qq = qq + zk * zk
        yv[k] = zk
        yv[k + 1:] -= L[k + 1:, k] * zk
    for k in range(n - 1, -1, -1):
        uk = yv[k] / L[k, k]
        yv[k] = uk
        yv[:k] -= L[k, :k] * uk
    sums = np.zeros(6, dtype=T)
    sums[0] = T(2) * logsum
    sums[1] = qq
    if want_grad:
        W = np.zeros((n, n), dtype=T)
        W[np.diag_indices(n)] = T(1) / np.diag(L)
        for i in range(1, n):
            W[i, :i] = -(L[i, :i] @ W[:i, :i]) / L[i, i]
        P = W.T @ W
        uu = np.outer(yv, yv)
        sums[4] = np.sum(np.sum(P * C, axis=1))
        sums[5] = np.sum(np.sum(P * dC, axis=1))
        sums[2] = T(-0.5) * np.sum(np.sum(uu * C, axis=1))
        sums[3] = T(-0.5) * np.sum(np.sum(uu * dC, axis=1))
    return sums, yv


def _points(rng, n, d, spread=1.):
    return rng.uniform(0., spread, size=(n, d))


def _case(name, cov, d, sizes, var=1.7, rho=0.3, want_grad=1, seed=0, special=None):
    return dict(name=name, cov=cov, d=d, sizes=tuple(sizes), var=var, rho=rho, want_grad=want_grad, seed=seed,
                special=special)


def op_cases():
    edge = (33, 1, 64, 2, 31, 63, 3, 32)   # 1, 2, 3, 31, 32, 33, 63, 64, shuffled
    cases = []
    for cov in range(4):
        for d in (1, 2, 3):
            cases.append(_case(f"edge_cov{cov}_d{d}", cov, d, edge, seed=10 * cov + d))
    cases.append(_case("edge_nograd", 0, 2, edge, want_grad=0, seed=5))
    cases.append(_case("single", 1, 2, (17,), seed=6))
    cases.append(_case("single_nograd", 2, 3, (64,), want_grad=0, seed=7))
    many = tuple(int(v) for v in np.random.default_rng(99).integers(5, 21, size=1500))
    cases.append(_case("many", 0, 2, many, seed=8))            # more clusters than compute units
    cases.append(_case("many_gauss", 3, 2, many[:300], rho=0.05, seed=9))
    cases.append(_case("duplicate", 1, 2, (9, 12), seed=11, special="duplicate"))   # r = 0, derivative 0
    cases.append(_case("far", 0, 2, (6, 11), rho=0.02, seed=12, special="far"))     # 50 ranges apart
    return cases


def not_pd_case():
    """var = 1e18 with two identical coordinates: Psi = [[v + 1, v], [v, v + 1]] rounds to v everywhere, sqrt(v) = 1e9
    and v / 1e9 = 1e9 are exact, so the second pivot is v - 1e9 * 1e9 = 0 in every IEEE arithmetic (also fused). The
    other clusters (points 50 ranges apart, single points) stay well conditioned at that variance."""
    return _case("not_pd", 0, 2, (5, 2, 1, 7), var=1e18, rho=0.02, seed=13, special="not_pd")


@functools.lru_cache(maxsize=None)
def _case_by_name(name):
    for c in op_cases() + [not_pd_case()]:
        if c["name"] == name:
            return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(ptr, X, y) of a case"""
    c = _case_by_name(name)
    rng = np.random.default_rng(1000 + c["seed"])
    ptr = np.concatenate([[0], np.cumsum(c["sizes"])]).astype(np.int32)
    Xs = []
    for k, n in enumerate(c["sizes"]):
        if c["special"] in ("far", "not_pd") and not (c["special"] == "not_pd" and k == 1):
            # a lattice with spacing 1 = 50 ranges (rho = 0.02), jittered by a hundredth of the spacing
            g = np.stack(np.unravel_index(np.arange(n), (8,) * c["d"]), axis=1).astype(float)
            x = g + rng.uniform(0., 0.01, size=g.shape)
        else:
            x = _points(rng, n, c["d"])
        if c["special"] == "duplicate":
            x[n - 1] = x[0]
        if c["special"] == "not_pd" and k == 1:
            x[1] = x[0]
        Xs.append(x)
    X = np.ascontiguousarray(np.concatenate(Xs))
    y = rng.standard_normal(X.shape[0])
    return ptr, X, y


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(ref sums C x 6, ref u, info C, allowance per output, stand-in error per output): longdouble reference, the
    float64 stand-in's error against it (max norm per output over the clusters that factor), 8 times that allowed"""
    c = _case_by_name(name)
    ptr, X, y = case_data(name)
    C = len(c["sizes"])
    phi = range_trafo(c["cov"], c["rho"])
    ref = np.full((C, 6), np.nan, dtype=LD)
    uref = np.full(X.shape[0], np.nan, dtype=LD)
    info = np.zeros(C, dtype=np.int32)
    err = {k: 0. for k in OUTPUTS}
    for k in range(C):
        a, b = ptr[k], ptr[k + 1]
        std = batch_compute(X[a:b], y[a:b], c["var"], phi, c["cov"], c["want_grad"], np.float64)
        if std is None:
            info[k] = 1
            continue
        r = batch_compute(X[a:b], y[a:b], c["var"], phi, c["cov"], c["want_grad"], LD)
        ref[k], uref[a:b] = r
        e = np.abs(std[0].astype(LD) - r[0])
        for j in range(6):
            err[OUTPUTS[j]] = max(err[OUTPUTS[j]], float(e[j]))
        err["u"] = max(err["u"], float(np.max(np.abs(std[1].astype(LD) - r[1]))))
    return ref, uref, info, {k: 8. * v for k, v in err.items()}, err


def ratios(name, sums, u):
    """error / allowance per output of a run (sums C x 6, u N) over the clusters that factor; 0 / 0 counts as 0"""
    ref, uref, info, allow, _ = case_reference(name)
    ok = info == 0
    ptr = case_data(name)[0]
    okrow = np.repeat(ok, np.diff(ptr))
    out = {}
    for j, k in enumerate(OUTPUTS[:6]):
        e = float(np.max(np.abs(sums[ok, j].astype(LD) - ref[ok, j])))
        out[k] = 0. if e == 0. else (np.inf if allow[k] == 0. else e / allow[k])
    e = float(np.max(np.abs(u[okrow].astype(LD) - uref[okrow])))
    out["u"] = 0. if e == 0. else (np.inf if allow["u"] == 0. else e / allow["u"])
    return out


def batch_raw(name, want_u=True, **over):
    """GPB_TestDenseBatch on a case; returns (return code, sums C x 6, u, info)"""
    from gpboost_amd.basic import lib
    c = dict(_case_by_name(name), **over)
    ptr, X, y = case_data(name)
    C, N = len(c["sizes"]), X.shape[0]
    sums = np.full((C, 6), -7.)
    u = np.full(N, -7.)
    info = np.full(C, -7, dtype=np.int32)
    Dp, Ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    I, L, F = ctypes.c_int, ctypes.c_int64, ctypes.c_double
    fn = lib().GPB_TestDenseBatch
    fn.argtypes = [I, I, I, Ip, L, Dp, L, Dp, L, F, F, I, Dp, L, Dp, L, Ip, L]
    ret = fn(c["cov"], C, c["d"], ptr.ctypes.data_as(Ip), ptr.size, X.ctypes.data_as(Dp), X.size,
             y.ctypes.data_as(Dp), y.size, c["var"], float(range_trafo(c["cov"], c["rho"])), c["want_grad"],
             sums.ctypes.data_as(Dp), sums.size, u.ctypes.data_as(Dp) if want_u else None, u.size if want_u else 0,
             info.ctypes.data_as(Ip), info.size)
    return ret, sums, u, info


def batch_hook(name, **over):
    from gpboost_amd.basic import GPBoostError, lib
    ret, sums, u, info = batch_raw(name, **over)
    if ret != 0:
        raise GPBoostError(lib().LGBM_GetLastError().decode())
    return sums, u, info
