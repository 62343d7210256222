"""Data, dense oracles and kernel references for grouped random slopes (group_rand_coef_data), shared by
tests/test_grouped_slope_reference.py (CPU), tests/test_gpu_grouped_slope.py and tests/test_gpu_grouped_slope_ops.py.

The model: K grouping variables, R slope covariates x_r on grouping variable ind[r] (counted from 1). Components in the
reference's order (re_model_template.h:6833-6872): the K intercepts, the R slopes, minus a dropped intercept. Component
c has the levels of its grouping variable, the value z_c[i] of Z (1 or x_r[i]) and one variance; Z is n x M with
Z[i, off_c + lev_c(i)] = z_c[i].

Data: the reference's R tests. test_GPModel_grouped_random_effects.R:16-43 (Gaussian; its generator is the LCG with
modulus 134456, multiplier 8121, increment 28411, unlike gpboost_amd.synthetic's 2^32 one) and
test_GPModel_non_Gaussian_data.R:44-58, 818-819 (probit; the 2^32 LCG of synthetic.sim_rand_unif).

Oracles, all dense numpy, written from the formulas:
  Gaussian   Cov(y) = sigma^2 Psi, Psi = Z T Z^T + I, T = diag(tau_c), tau_c = sigma_c^2 / sigma^2;
             nll = y^T Psi^-1 y / (2 sigma^2) + log|Psi| / 2 + n log(2 pi sigma^2) / 2;
             d/dlog sigma^2 (tau fixed) = -q / (2 sigma^2) + n / 2, q = y^T Psi^-1 y;
             d/dlog tau_c = -tau_c |Z_c^T Psi^-1 y|^2 / (2 sigma^2) + tau_c tr(Z_c^T Psi^-1 Z_c) / 2;
             computed twice, from an n x n Cholesky factor of Psi and from the M x M Woodbury form
             (A = T^-1 + Z^T Z; Psi^-1 = I - Z A^-1 Z^T; log|Psi| = log|A| + sum m_c log tau_c);
             predictions: mean = Z_p T Z^T Psi^-1 y, cov = sigma^2 (Z_p T Z_p^T - Z_p T Z^T Psi^-1 Z T Z_p^T [+ I]),
             Z_p over the seen and the new labels; random effects: b = T Z^T Psi^-1 y, var = sigma^2 diag(T - T Z^T Psi^-1 Z T).
  Laplace    tests/golden/grouped_laplace_restatement.py's Newton iteration on a weighted Z, and the gradient
             -b_c^T b_c / (2 s_c) + (m_c - tr(A^-1_cc) / s_c) / 2 + g^T A^-1 (b_c / s_c), g = Z^T (dW/deta . diag(Z A^-1 Z^T)) / 2,
             grad_F = -d1 + dW diag(Z A^-1 Z^T) / 2 - W Z A^-1 g, A = S^-1 + Z^T W Z at the mode.
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np
from scipy.stats import norm

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.insert(0, os.path.join(HERE, "golden"))

from gpboost_amd import synthetic  # noqa: E402


# ------------------------------------------------------------------------------------------------ data
def sim_rand_unif_r0(n, init_c):
    """test_GPModel_grouped_random_effects.R:16-22"""
    mod = 134456.0
    out = np.empty(n)
    s = float(np.floor(init_c * mod))
    out[0] = s
    for k in range(1, n):
        s = (8121.0 * s + 28411.0) % mod
        out[k] = s
    return out / mod


def gaussian_data():
    """group (100 blocks of 10), group2 (1..50 repeated), x, and the parts of y (:24-43)"""
    n, m = 1000, 100
    i = np.arange(1, n + 1)
    group = (i - 1) // (n // m) + 1
    group2 = (i - 1) % 50 + 1
    x = np.cos((i - n / 2) ** 2 * 5.5 * np.pi / n)
    b1 = norm.ppf(sim_rand_unif_r0(m, 0.546))
    b2 = norm.ppf(sim_rand_unif_r0(50, 0.46))
    b3 = norm.ppf(sim_rand_unif_r0(m, 0.69))
    xi = np.sqrt(0.5) * norm.ppf(sim_rand_unif_r0(n, 0.1))
    z1b1, z2b2, z3b3 = b1[group - 1], b2[group2 - 1], x * b3[group - 1]
    return {"n": n, "group": group, "group2": group2, "x": x, "xi": xi,
            "y_slope": z1b1 + z2b2 + z3b3 + xi,    # :497
            "y_drop": z2b2 + z3b3 + xi,            # :598
            "y_single": z1b1 + xi}                 # :57


def probit_data():
    """test_GPModel_non_Gaussian_data.R:44-58: 10 x 10 levels, x, and the three responses with a slope"""
    n, m = 100, 10
    i = np.arange(1, n + 1)
    group = (i - 1) // (n // m) + 1
    group2 = (i - 1) % (n // m) + 1
    x = np.cos((i - n / 2) ** 2 * 5.5 * np.pi / n)
    b1 = norm.ppf(synthetic.sim_rand_unif(m, 0.565))
    b2 = norm.ppf(synthetic.sim_rand_unif(n // m, 0.36))
    b3 = norm.ppf(synthetic.sim_rand_unif(m, 0.5678))
    e1, e2, e3 = b1[group - 1], b2[group2 - 1], x * b3[group - 1]

    def draw(eta, c):
        return (synthetic.sim_rand_unif(n, c) < norm.cdf(eta)).astype(np.float64)
    return {"n": n, "group": group, "group2": group2, "x": x,
            "y_slope": draw(e1 + e2 + e3, 0.57341),      # :818-819
            "y_one": draw(e1 + e3, 0.957341),            # :938-939
            "y_drop": draw(e2 + e3, 0.8341)}             # :951-952


def laplace_response(lik, pd_):
    """responses of the three likelihoods on the probit test's linear predictor pattern (inputs only)"""
    u = synthetic.sim_rand_unif(100, 0.31)
    if lik == "bernoulli_logit":
        return pd_["y_slope"]
    if lik == "poisson":
        return np.floor(4.0 * u * (1.0 + pd_["y_slope"]))
    return 0.2 + 3.0 * u * (1.0 + pd_["y_drop"])


# ------------------------------------------------------------------------------------------------ components and Z
def first_appearance_levels(col):
    _, first, inv = np.unique(col, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv]


def components(groups, slopes=None, ind=None, drop=None):
    """[(levels (n,), weight (n,) or None)] in the reference's order"""
    groups = np.asarray(groups)
    if groups.ndim == 1:
        groups = groups.reshape(-1, 1)
    K = groups.shape[1]
    lev = [first_appearance_levels(groups[:, k]) for k in range(K)]
    comps = [(lev[k], None) for k in range(K)]
    if slopes is not None:
        slopes = np.asarray(slopes, dtype=np.float64)
        if slopes.ndim == 1:
            slopes = slopes.reshape(-1, 1)
        for r in range(slopes.shape[1]):
            comps.append((lev[ind[r] - 1], slopes[:, r]))
    if drop is not None:
        comps = [c for k, c in enumerate(comps) if not (k < K and drop[k])]
    return comps


def design(comps):
    """dense Z (n x M) and the level counts m_c"""
    n = comps[0][0].size
    cols, m = [], []
    for lev, w in comps:
        Zc = np.zeros((n, lev.max() + 1))
        Zc[np.arange(n), lev] = 1.0 if w is None else w
        cols.append(Zc)
        m.append(Zc.shape[1])
    return np.hstack(cols), m


# ------------------------------------------------------------------------------------------------ Gaussian oracle
def _blocks(m):
    off = np.concatenate([[0], np.cumsum(m)])
    return [slice(off[c], off[c + 1]) for c in range(len(m))]


def gaussian_nll_grad(Z, m, y, cov_pars, form, profile=False):
    """(nll, grad, sigma2); grad wrt log [sigma^2, tau_1 .. tau_C] (profile: sigma^2 = q / n, grad wrt log tau).
    form "chol": n x n Cholesky of Psi; "woodbury": the M x M form."""
    n = y.size
    s2 = cov_pars[0]
    tau = np.asarray(cov_pars[1:], dtype=np.float64) / s2
    bl = _blocks(m)
    tvec = np.concatenate([np.full(mc, t) for mc, t in zip(m, tau)])
    if form == "chol":
        Psi = (Z * tvec) @ Z.T + np.eye(n)
        L = np.linalg.cholesky(Psi)
        a = np.linalg.solve(L.T, np.linalg.solve(L, y))            # Psi^-1 y
        logdet = 2.0 * np.log(np.diag(L)).sum()
        LiZ = np.linalg.solve(L, Z)
        tr = [np.sum(LiZ[:, b] ** 2) for b in bl]                  # tr(Z_c^T Psi^-1 Z_c)
    else:
        A = np.diag(1.0 / tvec) + Z.T @ Z
        La = np.linalg.cholesky(A)
        u = np.linalg.solve(La.T, np.linalg.solve(La, Z.T @ y))
        a = y - Z @ u
        logdet = 2.0 * np.log(np.diag(La)).sum() + np.sum(np.asarray(m) * np.log(tau))
        Ainv = np.linalg.inv(A)
        # Z^T Psi^-1 Z = S - S A^-1 S, S = T^-1
        tr = [mc / t - np.trace(Ainv[b, b]) / t ** 2 for mc, t, b in zip(m, tau, bl)]
    q = float(y @ a)
    if profile:
        s2 = q / n
    nll = q / (2 * s2) + logdet / 2 + n / 2 * np.log(2 * np.pi * s2)
    zta = Z.T @ a
    gt = [-t * np.sum(zta[b] ** 2) / (2 * s2) + t * trc / 2 for t, trc, b in zip(tau, tr, bl)]
    grad = np.array(gt if profile else [-q / (2 * s2) + n / 2] + gt)
    return float(nll), grad, float(s2)


def gaussian_predict(comps, y, cov_pars, pred_comps, same_new, predict_response=True):
    """pred_comps: per component (level or -1 for a new label, z value) arrays over the np points; same_new[c]: np x np
    boolean, the points that share a NEW label of component c. Returns (mean, cov)."""
    Z, m = design(comps)
    n = y.size
    s2 = cov_pars[0]
    tau = np.asarray(cov_pars[1:], dtype=np.float64) / s2
    tvec = np.concatenate([np.full(mc, t) for mc, t in zip(m, tau)])
    npred = pred_comps[0][0].size
    Zp = np.zeros((npred, Z.shape[1]))
    off = 0
    U = np.zeros((npred, npred))
    for c, (lev, z) in enumerate(pred_comps):
        seen = lev >= 0
        Zp[np.nonzero(seen)[0], off + lev[seen]] = z[seen]
        U += tau[c] * np.outer(z, z) * same_new[c]
        off += m[c]
    Psi = (Z * tvec) @ Z.T + np.eye(n)
    C = (Zp * tvec) @ Z.T
    mean = C @ np.linalg.solve(Psi, y)
    cov = (Zp * tvec) @ Zp.T + U - C @ np.linalg.solve(Psi, C.T)
    if predict_response:
        cov = cov + np.eye(npred)
    return mean, s2 * cov


def gaussian_random_effects(comps, y, cov_pars):
    """posterior means and variances of all M random effects (component-major)"""
    Z, m = design(comps)
    n = y.size
    s2 = cov_pars[0]
    tau = np.asarray(cov_pars[1:], dtype=np.float64) / s2
    tvec = np.concatenate([np.full(mc, t) for mc, t in zip(m, tau)])
    Psi = (Z * tvec) @ Z.T + np.eye(n)
    TZt = (Z * tvec).T
    b = TZt @ np.linalg.solve(Psi, y)
    var = s2 * (tvec - np.einsum("ij,ji->i", TZt, np.linalg.solve(Psi, TZt.T)))
    return b, var, m


def gaussian_std_dev(comps, cov_pars):
    """sqrt(diag(FI^-1)) of the original-scale parameters [sigma^2, sigma_1^2 .. sigma_C^2] from the dense n x n
    covariance V = sigma^2 I + sum_c sigma_c^2 Z_c Z_c^T: FI_jk = tr(V^-1 dV_j V^-1 dV_k) / 2 with dV_0 = I,
    dV_c = Z_c Z_c^T, i.e. |V^-1|_F^2, |V^-1 Z_c|_F^2 and |Z_a^T V^-1 Z_b|_F^2 (no Woodbury form, no n - M term)."""
    Z, m = design(comps)
    n = Z.shape[0]
    bl = _blocks(m)
    svec = np.concatenate([np.full(mc, s) for mc, s in zip(m, cov_pars[1:])])
    Vi = np.linalg.inv(cov_pars[0] * np.eye(n) + (Z * svec) @ Z.T)
    C = len(m)
    FI = np.zeros((C + 1, C + 1))
    FI[0, 0] = np.sum(Vi * Vi)
    ViZ = Vi @ Z
    ZViZ = Z.T @ ViZ
    for a in range(C):
        FI[0, a + 1] = FI[a + 1, 0] = np.sum(ViZ[:, bl[a]] ** 2)
        for b in range(C):
            FI[a + 1, b + 1] = np.sum(ZViZ[bl[a], bl[b]] ** 2)
    return np.sqrt(np.diag(np.linalg.inv(FI / 2)))


def pred_points(groups_train, groups_pred, slopes_pred=None, ind=None, drop=None):
    """The prediction points per component for gaussian_predict (the order of components()): labels of groups_pred
    (np x K) looked up in the training labels."""
    groups_train = np.asarray(groups_train)
    groups_pred = np.asarray(groups_pred)
    if groups_train.ndim == 1:
        groups_train, groups_pred = groups_train.reshape(-1, 1), groups_pred.reshape(-1, 1)
    K = groups_train.shape[1]
    npred = groups_pred.shape[0]
    lev, new = [], []
    for k in range(K):
        labels = groups_train[:, k]
        order = {}
        for v in labels:
            order.setdefault(v, len(order))
        lk = np.array([order.get(v, -1) for v in groups_pred[:, k]])
        lev.append(lk)
        same = (groups_pred[:, k][:, None] == groups_pred[:, k][None, :]) & (lk[:, None] < 0)
        new.append(same)
    out = [(lev[k], np.ones(npred)) for k in range(K)]
    same_new = list(new)
    if slopes_pred is not None:
        sp = np.asarray(slopes_pred, dtype=np.float64)
        if sp.ndim == 1:
            sp = sp.reshape(-1, 1)
        for r in range(sp.shape[1]):
            out.append((lev[ind[r] - 1], sp[:, r]))
            same_new.append(new[ind[r] - 1])
    if drop is not None:
        keep = [k for k in range(len(out)) if not (k < K and drop[k])]
        out, same_new = [out[k] for k in keep], [same_new[k] for k in keep]
    return out, same_new


# ------------------------------------------------------------------------------------------------ Laplace oracle
def _third(likelihood, y, eta, aux):
    """dW / deta"""
    if likelihood == "bernoulli_logit":
        p = 1.0 / (1.0 + np.exp(-eta))
        return p * (1.0 - p) * (1.0 - 2.0 * p)
    if likelihood == "poisson":
        return np.exp(eta)
    if likelihood == "gamma":
        return -aux * y * np.exp(-eta)
    raise ValueError(likelihood)


def laplace(comps, y, sigma2, likelihood, aux=1.0, offset=None, delta=1e-8, want_grad=False):
    """The Newton iteration of grouped_laplace_restatement.laplace_nll on the weighted Z. Returns a dict with nll, its,
    mode and (want_grad; logit, poisson, gamma) grad wrt log sigma_c^2 and grad_F."""
    import grouped_laplace_restatement as R

    lik = R.LIKELIHOODS[likelihood]
    Z, m = design(comps)
    n, M = Z.shape
    F = np.zeros(n) if offset is None else np.asarray(offset, dtype=np.float64)
    sigi = np.concatenate([np.full(mk, 1.0 / s) for mk, s in zip(m, sigma2)])
    b = np.zeros(M)

    def psi(bb):
        return lik(y, F + Z @ bb, aux)[0] - 0.5 * np.dot(bb * sigi, bb)

    obj = psi(b)
    its = 0
    for it in range(R.MAXIT):
        _, d1, W = lik(y, F + Z @ b, aux)
        grad = Z.T @ d1 - sigi * b
        A = np.diag(sigi) + Z.T @ (W[:, None] * Z)
        step = np.linalg.solve(A, grad)
        slope = float(step @ grad)
        lr = 1.0
        for _ in range(20):
            new = psi(b + lr * step)
            if new < obj + 1e-4 * lr * slope or not np.isfinite(new):
                lr *= 0.5
            else:
                break
        b = b + lr * step
        its = it + 1
        done = abs(new - obj) < delta * abs(obj) if it == 0 else (new - obj) < delta * abs(obj)
        obj = new
        if done:
            break
    _, d1, W = lik(y, F + Z @ b, aux)
    A = np.diag(sigi) + Z.T @ (W[:, None] * Z)
    L = np.linalg.cholesky(A)
    nll = -(obj - np.sum(np.log(np.diag(L))) + 0.5 * np.sum(np.log(sigi)))
    out = {"nll": float(nll), "its": its, "mode": b, "W": W, "Z": Z, "m": m}
    if want_grad:
        Ainv = np.linalg.inv(A)
        dW = _third(likelihood, y, F + Z @ b, aux)
        qd = np.einsum("ij,jk,ik->i", Z, Ainv, Z)          # diag(Z A^-1 Z^T)
        g = 0.5 * Z.T @ (dW * qd)
        v = Ainv @ g
        gr = []
        for bl, s in zip(_blocks(m), sigma2):
            e = np.zeros(M)
            e[bl] = b[bl] / s
            gr.append(-0.5 * np.sum(b[bl] ** 2) / s + 0.5 * ((bl.stop - bl.start) - np.trace(Ainv[bl, bl]) / s) + v @ e)
        out["grad"] = np.array(gr)
        out["grad_f"] = -d1 + 0.5 * dW * qd - W * (Z @ v)
    return out


# ------------------------------------------------------------------------------------------------ kernel tests
# Designs of tests/test_gpu_grouped_slope_ops.py: (levels (C x n), weights (C x n), has_weight (C)). The references
# below are numpy.longdouble; the bounds are those of tests/grouped_ops_cases.py with one more rounding per factor
# of Z on a term's way (the product z w, or z_a z_b w with the precomputed z_a z_b: 2 roundings).
def _decades(gen, n, lo=-3.0, hi=3.0):
    """mixed sign, magnitudes 10^lo .. 10^hi"""
    return gen.choice([-1.0, 1.0], n) * 10.0 ** gen.uniform(lo, hi, n)


def ops_design(name):
    gen = np.random.default_rng(abs(hash_name(name)))
    if name == "chunked":
        # n = 1500, groups (2 levels, 40 levels), slope on the first: a level of 750 observations takes the 512-chunk
        # path with a partial second chunk, the pair destinations (intercept x slope of one level: 750; first x second
        # group: 750 / 40 < 32 per pair) cover both the chunked and the one-thread path
        n = 1500
        g1 = np.arange(n) % 2
        g2 = (np.arange(n) // 2) % 40
        x = _decades(gen, n)
        lev = np.stack([g1, g2, g1])
        w = np.stack([np.ones(n), np.ones(n), x])
        return lev.astype(np.int32), w, np.array([0, 0, 1], np.int32)
    if name == "edge32":
        # n = 64: a level of exactly 32 observations (one thread) and one of 33 (chunked), two effects + slope on the second
        n = 64
        g1 = np.arange(n) % 7
        lv2 = np.concatenate([np.zeros(32, int), np.ones(32, int)])   # level 0: exactly 32
        lv3 = np.concatenate([np.zeros(31, int), np.ones(33, int)])   # level 1: exactly 33
        x = _decades(gen, n)
        lev = np.stack([g1, lv2, lv3, lv3])
        w = np.stack([np.ones(n), np.ones(n), np.ones(n), x])
        return lev.astype(np.int32), w, np.array([0, 0, 0, 1], np.int32)
    if name == "zero_level":
        # a slope whose covariate is 0 on a whole level: structural entries of value 0, a diagonal of Z^T Z equal to 0
        n = 120
        g1 = np.arange(n) % 5
        g2 = (np.arange(n) // 5) % 8
        x = _decades(gen, n, -1.0, 1.0)
        x[g1 == 3] = 0.0
        lev = np.stack([g1, g2, g1])
        w = np.stack([np.ones(n), np.ones(n), x])
        return lev.astype(np.int32), w, np.array([0, 0, 1], np.int32)
    raise KeyError(name)


OPS_DESIGNS = ("chunked", "edge32", "zero_level")


def hash_name(name):
    h = 1469598103934665603
    for ch in name.encode():
        h = ((h ^ ch) * 1099511628211) % (1 << 61)
    return h


def ld(a):
    return np.asarray(a, dtype=np.longdouble)


def ops_structure(name):
    """cum, per-level observation lists and the CSR of Z^T Z (pairs of different components), with the observation
    lists of every pair destination, as the engine builds them"""
    lev, w, _ = ops_design(name)
    C, n = lev.shape
    m = [int(lev[c].max()) + 1 for c in range(C)]
    cum = np.concatenate([[0], np.cumsum(m)]).astype(int)
    glev = lev + cum[:-1, None]
    M = int(cum[-1])
    lists = [[] for _ in range(M)]
    for c in range(C):
        for i in range(n):
            lists[glev[c, i]].append((i, c))
    pairs = {}
    for i in range(n):
        for a in range(C):
            for b in range(C):
                if a != b:
                    pairs.setdefault((int(glev[a, i]), int(glev[b, i])), []).append((i, a, b))
    keys = sorted(pairs)
    return {"C": C, "n": n, "M": M, "cum": cum, "glev": glev, "w": w, "lists": lists, "keys": keys, "pairs": pairs,
            "m": m}


def ref_zty(s, y):
    """(reference, sum of absolute terms, list lengths)"""
    w, yl = ld(s["w"]), ld(y)
    ref, ab, k = np.zeros(s["M"], np.longdouble), np.zeros(s["M"], np.longdouble), np.zeros(s["M"])
    for r, lst in enumerate(s["lists"]):
        for i, c in lst:
            t = w[c, i] * yl[i]
            ref[r] += t
            ab[r] += abs(t)
        k[r] = len(lst)
    return ref, ab, k


def ref_assemble(s, wv, diag_only):
    """diag_only: sum z_c[i] wv[i] per level; else sum z_c[i]^2 wv[i] per level, then sum z_a[i] z_b[i] wv[i] per pair"""
    w, wl = ld(s["w"]), ld(wv)
    M = s["M"]
    nd = M if diag_only else M + len(s["keys"])
    ref, ab, k = np.zeros(nd, np.longdouble), np.zeros(nd, np.longdouble), np.zeros(nd)
    for r, lst in enumerate(s["lists"]):
        for i, c in lst:
            t = (w[c, i] if diag_only else w[c, i] * w[c, i]) * wl[i]
            ref[r] += t
            ab[r] += abs(t)
        k[r] = len(lst)
    if not diag_only:
        for e, key in enumerate(s["keys"]):
            for i, a, b in s["pairs"][key]:
                t = w[a, i] * w[b, i] * wl[i]
                ref[M + e] += t
                ab[M + e] += abs(t)
            k[M + e] = len(s["pairs"][key])
    return ref, ab, k


def ref_ztz(s):
    """diagonal and CSR values of Z^T Z"""
    ones = np.ones(s["n"])
    ref, ab, k = ref_assemble(s, ones, False)
    return ref, ab, k


def ref_q(s, Ainv, W, dW):
    """dwq_i = dW_i q_i / 2, q_i = sum_jk z_j z_k Ainv[g_j, g_k]; sums_j = sum_i W_i z_j sum_k z_k Ainv[g_k, g_j];
    with the absolute sums"""
    w, A, Wl, dWl = ld(s["w"]), ld(Ainv), ld(W), ld(dW)
    C, n = s["C"], s["n"]
    dwq, dwq_ab = np.zeros(n, np.longdouble), np.zeros(n, np.longdouble)
    sums, sums_ab = np.zeros(C, np.longdouble), np.zeros(C, np.longdouble)
    for i in range(n):
        gi = s["glev"][:, i]
        qi, qab = np.longdouble(0), np.longdouble(0)
        for j in range(C):
            qj, qjab = np.longdouble(0), np.longdouble(0)
            for k in range(C):
                t = w[j, i] * w[k, i] * A[gi[k], gi[j]]
                qj += t
                qjab += abs(t)
            qi += qj
            qab += qjab
            sums[j] += Wl[i] * qj
            sums_ab[j] += abs(Wl[i]) * qjab
        dwq[i] = dWl[i] * qi / 2
        dwq_ab[i] = abs(dWl[i]) * qab / 2
    return dwq, dwq_ab, sums, sums_ab


def ref_row_trace(s, t, U, V, dW):
    w, Ul, Vl, dWl = ld(s["w"]), ld(U).reshape(s["M"], t), ld(V).reshape(s["M"], t), ld(dW)
    n = s["n"]
    out, ab = np.zeros(n, np.longdouble), np.zeros(n, np.longdouble)
    for i in range(n):
        gi = s["glev"][:, i]
        zi = w[:, i][:, None]
        a, p = (zi * Ul[gi]).sum(0), (zi * Vl[gi]).sum(0)
        aa, pa = np.abs(zi * Ul[gi]).sum(0), np.abs(zi * Vl[gi]).sum(0)
        out[i] = dWl[i] * (a * p).sum() / t / 2
        ab[i] = abs(dWl[i]) * (aa * pa).sum() / t / 2
    return out, ab


def ref_grad_f(s, d1, dwq, W, v):
    w, vl = ld(s["w"]), ld(v)
    zv = (w * vl[s["glev"]]).sum(0)
    zva = np.abs(w * vl[s["glev"]]).sum(0)
    return -ld(d1) + ld(dwq) - ld(W) * zv, np.abs(ld(d1)) + np.abs(ld(dwq)) + np.abs(ld(W)) * zva


def ref_pred(s, Li, idx, wt):
    """E[r, p] = sum_k wt[p, k] Li[r, idx[p, k]] for r >= idx[p, k], and var = sum_r E^2; with the absolute sums"""
    L, wl = ld(Li), ld(wt)
    M = s["M"]
    npred = idx.shape[0]
    E, Ea = np.zeros((M, npred), np.longdouble), np.zeros((M, npred), np.longdouble)
    for p in range(npred):
        for k in range(idx.shape[1]):
            a = idx[p, k]
            if a >= 0:
                E[a:, p] += wl[p, k] * L[a:, a]
                Ea[a:, p] += np.abs(wl[p, k] * L[a:, a])
    return E, Ea, (E ** 2).sum(0), (Ea ** 2).sum(0)


# ---- the weighted creation hook; the op hooks are tests/grouped_ops_cases.py's, on handles registered under the design's name
def weighted_handle(name):
    import grouped_ops_cases as O

    key = "slope:" + name
    if key not in O._handles:
        lib = O._lib()
        c = ctypes
        lib.GPB_TestGroupedCreateWeighted.argtypes = [c.c_int, c.c_int, c.POINTER(c.c_int32), c.c_int64,
                                                      c.POINTER(c.c_double), c.c_int64, c.POINTER(c.c_int32),
                                                      c.POINTER(c.c_void_p)]
        lev, w, has = ops_design(name)
        lev = np.ascontiguousarray(lev, dtype=np.int32)
        w = np.ascontiguousarray(w, dtype=np.float64)
        has = np.ascontiguousarray(has, dtype=np.int32)
        h = c.c_void_p()
        O._check(lib.GPB_TestGroupedCreateWeighted(lev.shape[1], lev.shape[0], O._ip(lev), lev.size, O._dp(w), w.size,
                                                   O._ip(has), c.byref(h)))
        O._handles[key] = h
    return key
