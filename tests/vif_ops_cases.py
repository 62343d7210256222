"""Cases, references and error bounds of the full-scale Vecchia ("VIF") kernel tests, shared by
tests/test_gpu_vif_ops.py (the HIP kernels of csrc/vif_kernels.hip through the GPB_TestVif* hooks) and
tests/test_vif_ops_reference.py (CPU: every case is valid, well conditioned and reaches the path it is named for,
float64 numpy stand-ins meet the very bounds the kernels are held to, single-entry defects exceed them, and the
longdouble row reference agrees with oracle/vif_oracle.py).

Inputs are float64, references numpy.longdouble (64-bit significand; assert_longdouble() checks that and both
test files call it). The row reference restates the row kernels' docstring on the hook's own inputs (the points,
the neighbour lists, V, P_0, P_1, nugget, cjit); for row i with neighbours N (k = min(i, nn) of them):
  C = k(N, N) - V_N^T V_N, its diagonal (nugget + var - |V_a|^2) cjit;  c = k(N, i) - V_N^T V_i
  d0 = nugget + var - |V_i|^2;  A = C^-1 c;  Bv = -A;  D = d0 - A . c
  dC_k = base_k(N, N) - (G_k + G_k^T), G_k = V_N^T P_k,N, base_0 = k (diagonal var), base_1 = dk / dlog phi (diagonal 0)
  dc_k = base_k(N, i) - (V_N^T P_k,i + P_k,N^T V_i);  dd0_k = [k = 0] var - 2 V_i . P_k,i
  dA_k = C^-1 (dc_k - dC_k A);  dBv_k = -dA_k;  dD_k = dd0_k - (dA_k . c + A . dc_k)

Bounds, first order in u = 2^-53 (UB = u + 2^-62 carries the longdouble reference's own rounding), gamma_j =
j UB / (1 - j UB); none of them tuned to what a kernel gives.
  Gram entries   a sum of m products in ANY order, fma or not (MFMA k-slots, LDS tiles): gamma_m |V_a| . |V_b|
                 (Higham, Accuracy and Stability, eq. 3.5); gamma_{m+2} leaves room for the subtraction from the
                 covariance and the cjit product, gamma_{m+3} for the G + G^T sum of the derivative blocks.
  covariances    cov.h: r = sqrt(sum of d squares) has relative error <= (d / 2 + 2) u, the exponent's argument
                 x = phi r (phi r^2 for the Gaussian kernel) <= (d + 6) u, exp(-x) turns that into |x| (d + 6) u
                 plus its own 2 ulp, the polynomial factor and the product with var are at most 6 roundings of
                 positive terms: |dk| <= c_cov u |k| with c_cov = 8 + (d + 6) |x|, and c_cov + 4 for dk / dlog phi.
  inputs         E_C = gamma_{m+2} |V_N|^T |V_N| + c_cov u |k(N, N) + nugget I| + 2 u |C|; E_c, E_d0, E_dC, E_dc, E_dd0
                 the same way (gamma_{m+3} (|G| + |G|^T) for the two Gram terms of a derivative).
  A              |A^ - A| <= |C^-1| ((4 gamma_{3k+1} |L||L|^T + E_C) |A| + E_c): Higham Theorem 10.4 for a Cholesky
                 solve plus the perturbed inputs; the factor 4 is the one dense_ops_cases.chol_ratios uses for a
                 pivot formed as p y with y = rsq(p) refined by two Newton steps and a column scaled by y.
  dA_k           the same solve bound with right-hand side r = dc - dC A,
                 |dr| <= E_dc + E_dC |A| + |dC| |A^ - A| + gamma_{k+1} (|dc| + |dC||A|).
  D, dD_k        |dD| <= E_d0 + |A^ - A| . |c| + |A| . E_c + gamma_{k+2} (|d0| + |A| . |c|); dD_k with the four
                 perturbed factors and gamma_{2k+3} on the absolute sum.
  products       row / column with k terms and the own entry, S = |self in_i| + sum |coef||in|:
                 (k + 4) u |1 / D| S + (k + 4) 2^-64 S, the operator bound of latent_ops_cases.py.
  sums, gemv,    gamma_{N+8} on the absolute sum of N terms (the 8: the roundings inside one term of vif_sum_kernel
  column dots    and the library logarithm); z = (e - dD u) / D: 4 u (|e| + |dD u|) / |D|.
Conditions every case meets (asserted by tests/test_vif_ops_reference.py, which prints them): cond_2(C) <= 1e4 in
every row, and in every row the largest bound of Bv is at most 1e-8 times the row's largest |Bv| and the bound of D
at most 1e-8 |D|. The derivatives are differences that can cancel, dA_0 identically so in the latent form (without
a nugget A does not depend on var), so their scale is that of their terms: the largest bound of dBv_k in a row is
at most 1e-8 times max(|dA_k|, |C^-1| (|dc_k| + |dC_k||A|)) over the row, the bound of dD_k at most 1e-8 times
max(|dD_k|, |dd0_k|, |dA_k| . |c| + |A| . |dc_k|).

Float64 stand-in (numpy Cholesky solves and @ products), largest error / bound over all cases, measured by
tests/test_vif_ops_reference.py: rows 0.15 (Bv), 0.42 (D), 0.12 (dBv), 0.26 (dD); products 0.41; vector ops 0.13;
the float64 oracle (vif_oracle.vif_factor on the pin case, both nugget values) 0.06 (Bv), 0.05 (D), 0.06 (dBv), 0.11 (dD).
The kernels on an MI355X (tests/test_gpu_vif_ops.py -s): vif_rows_mfma_kernel 0.17 / 0.42 / 0.12 / 0.26, vif_rows_kernel
0.09 / 0.40 / 0.09 / 0.26 (Bv / D / dBv / dD), the two forms against each other 0.08 of the sum of their bounds,
vif_brow_kernel 0.55, vif_bcol_kernel 0.36, vif_bvec_kernel 0.32, vif_btvec_kernel 0.27, gemv 0.11, column dots 0.11,
vif_zvec_kernel 0.45, vif_sum_kernel 0.13, vif_dkmn_kernel 0.41.
"""
import ctypes
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from latent_ops_cases import LD, U, assert_longdouble, max_ratio, HookError, _dp, _ip  # noqa: E402,F401
from sparse_chol_cases import longdouble_cholesky  # noqa: E402

UREF = 2.0 ** -64
UB = U + 2.0 ** -62
COV_NAMES = ("exponential", "matern15", "matern25", "gaussian")
FORM_PROD, FORM_MFMA, FORM_LDS = 0, 1, 2
K_CH, K_T = 32, 256          # vif_rows_kernel: m-rows per staging chunk, threads
MAX_NN, MAX_NN_GRAD, MAX_NN_MFMA = 64, 48, 31
VAR = 3.7


def gamma(j):
    return j * UB / (1.0 - j * UB)


def ldm_of(m):
    return (m + 63) // 64 * 64


def phi_of(cov, rng):
    return {0: 1. / rng, 1: np.sqrt(3.) / rng, 2: np.sqrt(5.) / rng, 3: 1. / (rng * rng)}[cov]


# ------------------------------------------------------------------------------------------------ covariances
def cov_dcov(r, var, phi, cov):
    """(k, dk / dlog phi, |exponent argument|) of cov.h's cov_dcov in r's dtype"""
    T = r.dtype.type
    var, phi = T(var), T(phi)
    if cov == 0:
        x = phi * r
        c = var * np.exp(-x)
        return c, -x * c, x
    if cov == 1:
        x = phi * r
        e = np.exp(-x)
        return var * (1 + x) * e, -var * x * x * e, x
    if cov == 2:
        x = phi * r
        e = np.exp(-x)
        return var * (1 + x + x * x / T(3)) * e, -var * x * x / T(3) * (1 + x) * e, x
    x = phi * r * r
    c = var * np.exp(-x)
    return c, -x * c, x


def dist(A, B):
    return np.sqrt(((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2))


def nearest_earlier(X, nn, i0=0):
    """rows i0 .. n - 1: the min(i, nn) nearest earlier points (brute force), -1 after them"""
    n = X.shape[0]
    nbr = np.full((n - i0, nn), -1, dtype=np.int32)
    for i in range(max(i0, 1), n):
        k = min(i, nn)
        d2 = ((X[:i] - X[i]) ** 2).sum(axis=1)
        nbr[i - i0, :k] = np.argsort(d2, kind="stable")[:k]
    return nbr


def grown_points(g, n, d, lo, hi):
    """n points grown one by one: each lies within hi of a random earlier point and no closer than lo to any, so
    every row has correlated earlier neighbours and no two points nearly coincide"""
    X = np.zeros((n, d))
    i = 1
    while i < n:
        v = g.standard_normal(d)
        cand = X[g.integers(i)] + v / np.sqrt(v @ v) * g.uniform(lo, hi)
        if ((X[:i] - cand) ** 2).sum(axis=1).min() >= lo * lo:
            X[i] = cand
            i += 1
    return X


# ------------------------------------------------------------------------------------------------ row cases
def _rows_spec(form, nn, m, cov=0, d=2, grad=True, nugget=1., kind="rand", n_total=None, i0=0, rng=0.15, seed=0,
               zgrow=False):
    return dict(form=form, nn=nn, m=m, cov=cov, d=d, grad=grad, nugget=nugget, kind=kind,
                n_total=nn + 40 if n_total is None else n_total, i0=i0, rng=rng, seed=seed, zgrow=zgrow)


# krig cases: the points' spacing (closest pair, distance to the parent point) in units of the range 0.15; the
# smoother the kernel, the wider, so that cond(C) <= 1e4 holds in the latent form (nugget 0) as well
SPACING = {0: (0.3, 0.7), 1: (0.5, 1.0), 2: (0.8, 1.4), 3: (1.2, 1.8)}
SPACING_1D = dict(SPACING)        # collinear neighbours condition C worse
SPACING_1D[2] = (1.5, 2.4)

ROW_CASES = {}
for _nn in (1, 15, 16, 17, 30, 31):
    for _m in (1, 7, 8, 9, 16, 17, 24, 25, 64, 65):
        ROW_CASES[f"mfma-rand-nn{_nn}-m{_m}"] = _rows_spec(FORM_MFMA, _nn, _m, seed=_nn * 100 + _m)
for _m in (2, 3, 4, 5, 6):      # the remaining tails of the first 8-chunk
    ROW_CASES[f"mfma-rand-nn17-m{_m}"] = _rows_spec(FORM_MFMA, 17, _m, seed=1700 + _m)
for _cov in range(4):
    for _grad in (True, False):
        for _d in (1, 2, 3):
            for _lat in (False, True):
                for _nn, _m in ((31, 25), (17, 9)):
                    ROW_CASES[f"mfma-krig-{COV_NAMES[_cov]}-{'grad' if _grad else 'nograd'}-d{_d}-"
                              f"{'latent' if _lat else 'gauss'}-nn{_nn}-m{_m}"] = _rows_spec(
                        FORM_MFMA, _nn, _m, cov=_cov, d=_d, grad=_grad, nugget=0. if _lat else 1., kind="krig",
                        seed=_cov * 7 + _d)
for _nn in (32, 33, 47, 48):
    for _m in (1, 31, 32, 33, 65):
        ROW_CASES[f"lds-rand-nn{_nn}-m{_m}"] = _rows_spec(FORM_LDS, _nn, _m, seed=_nn * 100 + _m)
for _nn in (1, 3, 4, 5, 31):
    for _m in (1, 33, 65):
        ROW_CASES[f"lds-forced-nn{_nn}-m{_m}"] = _rows_spec(FORM_LDS, _nn, _m, seed=_nn * 100 + _m + 1)
ROW_CASES["lds-krig-matern15-latent-nn33-m25"] = _rows_spec(FORM_LDS, 33, 25, cov=1, nugget=0., kind="krig", seed=5)
ROW_CASES["lds-krig-gaussian-nograd-nn64-m25"] = _rows_spec(FORM_LDS, 64, 25, cov=3, grad=False, kind="krig", seed=6)
ROW_CASES["lds-rand-nograd-nn49-m33"] = _rows_spec(FORM_LDS, 49, 33, grad=False, seed=7)
# prediction rows: i0 = n observed points, no derivatives, the production dispatch; lists over the observed and the
# earlier prediction points (cond_all); n < mp: the first prediction rows hold k = i < mp entries
for _mp in (1, 31, 32, 63, 64):
    ROW_CASES[f"pred-mp{_mp}"] = _rows_spec(FORM_PROD, _mp, 20, grad=False, n_total=_mp + 30, i0=_mp + 10, seed=_mp)
ROW_CASES["pred-mp32-n10"] = _rows_spec(FORM_PROD, 32, 20, grad=False, n_total=50, i0=10, seed=3)
ROW_CASES["pred-mp12-n5-krig"] = _rows_spec(FORM_PROD, 12, 9, cov=1, grad=False, kind="krig", n_total=30, i0=5, seed=4)
# processing order: n_total around the 8 XCD chunks (both forms run them with the order on and off)
ORDER_N = (1, 2, 7, 8, 9, 71)
for _n in ORDER_N:
    ROW_CASES[f"order-n{_n}"] = _rows_spec(FORM_PROD, 5, 9, n_total=_n, seed=_n)

# the case on which the longdouble reference is pinned to oracle/vif_oracle.py: inducing points 1.5 to 2.5 ranges
# apart, so that K_mm,s is well conditioned and the float64 oracle's detour through A = K_mm,s^-1 K_mn costs it
# no more than the roundings the bounds allow the kernels
PIN_CASE = "pin-krig-matern15-nn17-m9"
ROW_CASES[PIN_CASE] = _rows_spec(FORM_MFMA, 17, 9, cov=1, kind="krig", seed=11, zgrow=True)


@functools.lru_cache(maxsize=None)
def row_inputs(name):
    """the hook's inputs of a row case: X, nbr, V, P0, P1 (None without derivatives), Z (krig) and the scalars"""
    s = ROW_CASES[name]
    g = np.random.default_rng(1000 + s["seed"])
    n, d, m, nn = s["n_total"], s["d"], s["m"], s["nn"]
    if s["kind"] == "krig":
        lo, hi = (SPACING_1D if d == 1 else SPACING)[s["cov"]]
        X = grown_points(g, n, d, lo * s["rng"], hi * s["rng"])
    else:
        X = g.uniform(size=(n, d))
    nbr = nearest_earlier(X, nn, s["i0"])
    phi = phi_of(s["cov"], s["rng"])
    out = dict(s, X=X, nbr=nbr, var=VAR, phi=phi, cjit=1. if s["nugget"] else 1. + 1e-10, Z=None)
    if s["kind"] == "rand":
        # k max_a |V_a|^2 = 0.5: C stays positive definite with the nugget; P independent of V
        mats = []
        for _ in range(3):
            M = g.standard_normal((n, m))
            mats.append(M * np.sqrt(0.5 / (nn + 1)) / np.sqrt((M * M).sum(axis=1).max()))
        V, P0, P1 = mats
    else:
        lo_, hi_ = X.min(axis=0), X.max(axis=0)
        Z = g.uniform(lo_, hi_, size=(m, d))
        if s["zgrow"]:
            Z = grown_points(g, m, d, 1.5 * s["rng"], 2.5 * s["rng"])
            Z += 0.5 * (lo_ + hi_) - Z.mean(axis=0)
        if d == 1 and s["cov"] == 0:
            # the exponential kernel on a line is Markov: an inducing point between two points makes their residual
            # covariance exactly zero, and rows whose neighbours all lie beyond one get A = 0. Inducing points on
            # either side of the data keep every row's weights away from zero.
            Z = np.where(g.uniform(size=(m, 1)) < 0.5, lo_ - g.uniform(0.02, 0.3, size=(m, 1)),
                         hi_ + g.uniform(0.02, 0.3, size=(m, 1)))
        V, P0, P1 = krig_matrices(X, Z, s["cov"], VAR, phi)
        out["Z"] = Z
    out.update(V=np.ascontiguousarray(V), P0=np.ascontiguousarray(P0) if s["grad"] else None,
               P1=np.ascontiguousarray(P1) if s["grad"] else None)
    return out


def krig_matrices(X, Z, cov, var, phi):
    """float64 V = L^-1 K_mn and P_k = L^-1 (dK_k - 1/2 dK_mm,k A) (n x m each) for the inducing points Z"""
    from scipy.linalg import cho_solve, solve_triangular
    K, dK, _ = cov_dcov(dist(Z, X), var, phi, cov)
    Kmm, dKmm, _ = cov_dcov(dist(Z, Z), var, phi, cov)
    np.fill_diagonal(Kmm, var)
    np.fill_diagonal(dKmm, 0.)
    Ks = Kmm.copy()
    Ks[np.diag_indices_from(Ks)] *= 1. + 1e-6
    L = np.linalg.cholesky(Ks)
    V = solve_triangular(L, K, lower=True)
    A = cho_solve((L, True), K)
    P0 = solve_triangular(L, K - 0.5 * Kmm @ A, lower=True)
    P1 = solve_triangular(L, dK - 0.5 * dKmm @ A, lower=True)
    return V.T.copy(), P0.T.copy(), P1.T.copy()


def row_path(s):
    """what a case reaches, from its shapes alone: the form the production dispatch would take, the form run, the
    MFMA ping-pong loop's chunk counts, the LDS form's tiles and staging chunks, the order's padding slots"""
    nn, m, G = s["nn"], s["m"], 3 if s["grad"] else 1
    rows = s["n_total"] - s["i0"]
    prod = FORM_MFMA if nn <= MAX_NN_MFMA else FORM_LDS
    run = prod if s["form"] == FORM_PROD else s["form"]
    S = nn + 1
    Sp, T4 = ((S + 3) & ~3) + 2, (S + 3) >> 2
    chunk = (rows + 7) // 8
    return dict(production=prod, run=run, nfull=m >> 3, nch=(m + 7) >> 3, tail=m % 8, parity=(m >> 3) & 1,
                sets=S, tiles=G * T4 * T4, second_tile_pass=G * T4 * T4 > K_T, staging_chunks=(m + K_CH - 1) // K_CH,
                staging_tail=m % K_CH, Sp=Sp, pad_slots=8 * chunk - rows if rows > 1 else 0,
                short_rows=max(0, min(nn, s["n_total"]) - s["i0"]), ldm_pad=ldm_of(m) - m)


# ------------------------------------------------------------------------------------------------ row reference
def _solve(C, B, T):
    """(C^-1 B, L) by Cholesky: longdouble substitution, or numpy / scipy in float64"""
    if T is LD:
        L = longdouble_cholesky(C)
        k = C.shape[0]
        Y = np.zeros(B.shape, dtype=LD)
        for i in range(k):
            Y[i] = (B[i] - np.dot(L[i, :i], Y[:i])) / L[i, i]
        Xs = np.zeros(B.shape, dtype=LD)
        for i in range(k - 1, -1, -1):
            Xs[i] = (Y[i] - np.dot(L[i + 1:, i], Xs[i + 1:])) / L[i, i]
        return Xs, L
    from scipy.linalg import solve_triangular
    L = np.linalg.cholesky(C)
    return solve_triangular(L, solve_triangular(L, B, lower=True), lower=True, trans=1), L


def rows_compute(inp, T=LD, bounds=False):
    """D (rows), Bv (rows x nn), dD (2 x rows), dBv (2 x rows x nn) of the row factor in the dtype T; with bounds
    (T longdouble) also their float64 error bounds "e*", cond_2(C) per row and the scales of the dD condition"""
    X, V, nbr = inp["X"].astype(T), inp["V"].astype(T), inp["nbr"]
    grad, nn, m, i0, d, cov = inp["grad"], inp["nn"], inp["m"], inp["i0"], inp["d"], inp["cov"]
    P = [inp["P0"].astype(T), inp["P1"].astype(T)] if grad else []
    var, nug, cj = T(inp["var"]), T(inp["nugget"]), T(inp["cjit"])
    rows = X.shape[0] - i0
    f64 = lambda a: np.abs(np.asarray(a, dtype=np.float64))  # noqa: E731
    out = dict(D=np.zeros(rows, T), Bv=np.zeros((rows, nn), T), dD=np.zeros((2, rows), T), dBv=np.zeros((2, rows, nn), T))
    if bounds:
        out.update(eD=np.zeros(rows), eBv=np.zeros((rows, nn)), edD=np.zeros((2, rows)), edBv=np.zeros((2, rows, nn)),
                   cond=np.ones(rows), sdD=np.zeros((2, rows)), sdBv=np.zeros((2, rows)))
    gm2, gm3 = gamma(m + 2), gamma(m + 3)
    for ir in range(rows):
        i = i0 + ir
        k = min(i, nn)
        N = nbr[ir, :k]
        Vi = V[i]
        d0 = nug + var - Vi @ Vi
        dd = [var - 2 * (Vi @ P[0][i]), -2 * (Vi @ P[1][i])] if grad else []
        if bounds:
            aVi = f64(Vi)
            E_d0 = gm2 * (aVi @ aVi) + UB * float(nug + var) + UB * f64(d0)
            E_dd = [2 * gm2 * (aVi @ f64(P[p][i])) + UB * float(var) * (p == 0) + UB * f64(dd[p]) for p in range(2)] \
                if grad else []
        if k == 0:
            out["D"][ir] = d0
            for p in range(2 if grad else 0):
                out["dD"][p, ir] = dd[p]
            if bounds:
                out["eD"][ir] = E_d0
                for p in range(2 if grad else 0):
                    out["edD"][p, ir] = E_dd[p]
                    out["sdD"][p, ir] = f64(dd[p])
            continue
        VN, xs = V[N], X[N]
        knn, dknn, xnn = cov_dcov(dist(xs, xs), var, inp["phi"], cov)
        np.fill_diagonal(knn, var)
        np.fill_diagonal(dknn, 0)
        np.fill_diagonal(xnn, 0)
        kni, dkni, xni = cov_dcov(dist(xs, X[i:i + 1])[:, 0], var, inp["phi"], cov)
        C = knn - VN @ VN.T
        C[np.diag_indices(k)] = (nug + var - (VN * VN).sum(axis=1)) * cj
        c = kni - VN @ Vi
        sol, L = _solve(C, c[:, None], T)
        A = sol[:, 0]
        D = d0 - A @ c
        out["D"][ir] = D
        out["Bv"][ir, :k] = -A
        if bounds:
            aV, aA, ac = f64(VN), f64(A), f64(c)
            cc_nn, cc_ni = 8 + (d + 6) * f64(xnn), 8 + (d + 6) * f64(xni)
            E_C = gm2 * (aV @ aV.T) + cc_nn * UB * (f64(knn) + float(nug) * np.eye(k)) + 2 * UB * f64(C)
            E_c = gm2 * (aV @ aVi) + cc_ni * UB * f64(kni) + UB * ac
            Cinv = f64(_solve(C, np.eye(k, dtype=T), T)[0])
            LL = f64(L) @ f64(L).T
            M = 4 * gamma(3 * k + 1) * LL + E_C
            eA = Cinv @ (M @ aA + E_c)
            out["eBv"][ir, :k] = eA
            out["eD"][ir] = E_d0 + eA @ ac + aA @ E_c + gamma(k + 2) * (f64(d0) + aA @ ac)
            out["cond"][ir] = np.linalg.cond(np.asarray(C, dtype=np.float64))
        for p in range(2 if grad else 0):
            PN, Pi = P[p][N], P[p][i]
            base_nn, base_ni = (knn, kni) if p == 0 else (dknn, dkni)
            Gp = VN @ PN.T
            dC = base_nn - (Gp + Gp.T)
            dc = base_ni - (VN @ Pi + PN @ Vi)
            dA = _solve(C, (dc - dC @ A)[:, None], T)[0][:, 0]
            dDp = dd[p] - (dA @ c + A @ dc)
            out["dD"][p, ir] = dDp
            out["dBv"][p, ir, :k] = -dA
            if bounds:
                aP, aPi, adA, adc, adC = f64(PN), f64(Pi), f64(dA), f64(dc), f64(dC)
                absG = aV @ aP.T
                extra = 4 * (p == 1)
                E_dC = gm3 * (absG + absG.T) + (cc_nn + extra) * UB * f64(base_nn) + UB * adC
                E_dc = gm3 * (aV @ aPi + aP @ aVi) + (cc_ni + extra) * UB * f64(base_ni) + UB * adc
                E_r = E_dc + E_dC @ aA + adC @ eA + gamma(k + 1) * (adc + adC @ aA)
                edA = Cinv @ (M @ adA + E_r)
                out["edBv"][p, ir, :k] = edA
                terms = adA @ ac + aA @ adc
                out["edD"][p, ir] = (E_dd[p] + edA @ ac + adA @ E_c + eA @ adc + aA @ E_dc
                                     + gamma(2 * k + 3) * (f64(dd[p]) + terms))
                out["sdD"][p, ir] = max(f64(dDp), f64(dd[p]), terms)
                out["sdBv"][p, ir] = max(adA.max(), (Cinv @ (adc + adC @ aA)).max())
    return out


@functools.lru_cache(maxsize=None)
def row_reference(name):
    return rows_compute(row_inputs(name), LD, bounds=True)


def row_ratios(name, got):
    """largest error / bound of D, Bv and (with derivatives) dD, dBv of a result dict against the reference"""
    ref = row_reference(name)
    keys = ("D", "Bv", "dD", "dBv") if ROW_CASES[name]["grad"] else ("D", "Bv")
    return {q: max_ratio(np.abs(np.asarray(got[q]).astype(LD) - ref[q]), ref["e" + q]) for q in keys}


# ------------------------------------------------------------------------------------------------ product cases
PROD_N, PROD_M = 150, (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260)
LIST_COUNTS = (15, 16, 17, 33)


def _lists_graph(n=PROD_N, nn=4):
    """a chain whose columns 5, 30, 60, 90 receive LIST_COUNTS entries in all (the 16-lane strides of
    vif_btvec_kernel: one short of, exactly, one past a stride, and two strides plus one)"""
    nbr = np.full((n, nn), -1, dtype=np.int32)
    for i in range(1, n):
        k = min(i, nn)
        nbr[i, :k] = i - 1 - np.arange(k)
    cols = (5, 30, 60, 90)
    for c, cnt in zip(cols, LIST_COUNTS):
        # column c is named by its nn successors already: the rows c + nn + 1 ... take it in their last slot
        for i in range(c + nn + 1, c + cnt + 1):
            nbr[i, nn - 1] = c
    return nbr, cols


@functools.lru_cache(maxsize=None)
def prod_graph(kind):
    g = np.random.default_rng(77)
    X = g.uniform(size=(PROD_N, 2))
    if kind == "knn":
        return X, nearest_earlier(X, 30)
    if kind == "star":
        nbr = np.full((PROD_N, 2), -1, dtype=np.int32)
        nbr[1, 0] = 0
        for i in range(2, PROD_N):
            nbr[i] = (0, i - 1)
        return X, nbr
    if kind == "chain":
        nbr = np.full((PROD_N, 1), -1, dtype=np.int32)
        nbr[1:, 0] = np.arange(PROD_N - 1)
        return X, nbr
    return X, _lists_graph()[0]


PROD_GRAPHS = ("knn", "star", "chain", "lists")


def column_counts(nbr):
    n, nn = nbr.shape
    cnt = np.zeros(n, dtype=np.int64)
    for i in range(n):
        for r in range(min(i, nn)):
            cnt[nbr[i, r]] += 1
    return cnt


@functools.lru_cache(maxsize=None)
def prod_values(kind, m):
    """coef (n x nn, 0 past a row's entries), D (n, three decades), the m x n input (n x m) and an n-vector"""
    _, nbr = prod_graph(kind)
    n, nn = nbr.shape
    g = np.random.default_rng(500 + m)
    coef = g.standard_normal((n, nn))
    coef[nbr < 0] = 0.
    D = 10. ** g.uniform(-1.5, 1.5, size=n)
    return coef, D, g.standard_normal((n, m)), g.standard_normal(n)


def dense_b(nbr, coef, self_):
    n, nn = nbr.shape
    B = np.zeros((n, n), dtype=LD)
    for i in range(n):
        B[i, i] = self_
        for r in range(min(i, nn)):
            B[i, nbr[i, r]] += LD(coef[i, r])
    return B


def prod_reference(nbr, coef, self_, inp, transpose, inv_d=None):
    """(reference, bound) of out = (self I + N) in (rows of `inp` are the m-vectors, or an n-vector), N^T with
    transpose; inv_d: then times 1 / D_i"""
    B = dense_b(nbr, coef, self_)
    if transpose:
        B = B.T
    x = inp.astype(LD)
    ref = B @ x
    S = np.asarray(np.abs(B) @ np.abs(x), dtype=np.float64)
    k = (B != 0).sum(axis=1).astype(np.float64)
    k = k[:, None] if x.ndim == 2 else k
    scale = np.ones(B.shape[0])
    if inv_d is not None:
        ref = ref / (inv_d.astype(LD)[:, None] if x.ndim == 2 else inv_d.astype(LD))
        scale = 1. / np.abs(inv_d)
    scale = scale[:, None] if x.ndim == 2 else scale
    return ref, (k + 4) * U * scale * S + (k + 4) * UREF * scale * S


# ------------------------------------------------------------------------------------------------ vector cases
VEC_N, VEC_M = (1, 63, 64, 65, 257, 4100), (1, 64, 65)
SUM_OPS = (0, 1, 2, 3, 4)


def sum_terms(n, nt, seed):
    """nt terms (a, b, c, op) of vif_sum_kernel: every op, nullable factors; a > 0 where the logarithm is taken"""
    g = np.random.default_rng(seed)
    terms = []
    for t in range(nt):
        op = SUM_OPS[(t + seed) % 5]
        a = g.uniform(0.2, 3., size=n) if op == 1 else g.standard_normal(n)
        b = g.standard_normal(n) if (op in (3, 4) or (op in (0, 2) and t % 2 == 0)) else None
        c = g.uniform(0.3, 2., size=n) * g.choice([-1., 1.], size=n) if (op in (2, 3, 4) or (op == 0 and t % 3 == 0)) \
            else None
        terms.append((a, b, c, op))
    return terms


def sum_term(op, a, b, c):
    """the elementwise term of vif_sum_kernel's op"""
    if op == 1:
        return np.log(a)
    return {0: a * b * c, 2: a * b / c, 3: a * b * b / (c * c), 4: a * b / (c * c)}[op]


def sum_reference(terms):
    refs, bnds = [], []
    for a, b, c, op in terms:
        n = a.shape[0]
        al = a.astype(LD)
        bl = b.astype(LD) if b is not None else np.ones(n, LD)
        cl = c.astype(LD) if c is not None else np.ones(n, LD)
        v = sum_term(op, al, bl, cl)
        refs.append(v.sum())
        bnds.append(gamma(n + 8) * float(np.abs(v).sum()))
    return np.array(refs), np.array(bnds)


# ------------------------------------------------------------------------------------------------ the hooks
def _lib():
    c = ctypes
    from gpboost_amd import basic
    lib = basic.lib()
    if not getattr(lib, "_vif_ops_typed", False):
        Dp, I, L, F = c.POINTER(c.c_double), c.c_int, c.c_int64, c.c_double
        PI, PL, PG = c.POINTER(c.c_int32), c.POINTER(c.c_int64), c.POINTER(c.c_int)
        lib.GPB_TestVifRows.argtypes = [I, I, I, I, I, Dp, L, PI, L, Dp, Dp, Dp, L, I, F, F, F, F, I, I, I, F,
                                        Dp, Dp, Dp, Dp, Dp, Dp, L, PG]
        lib.GPB_TestVifApply.argtypes = [I, I, I, I, PI, L, Dp, L, Dp, Dp, L, F, I, I, Dp, I, I, F, Dp, Dp, L, PG]
        lib.GPB_TestVifVector.argtypes = [I, I, I, I, I, F, F, F, c.POINTER(Dp), PL, I, PI, I, Dp, L, PG]
        lib.LGBM_GetLastError.restype = c.c_char_p
        lib._vif_ops_typed = True
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


def rows_raw(inp, form=None, order=0, grad=None, pad_fill=np.nan, **over):
    """GPB_TestVifRows on the inputs of a case (over: replaced entries); returns (return code, outputs, guard)"""
    q = dict(inp, **over)
    grad = q["grad"] if grad is None else grad
    form = q["form"] if form is None else form
    n, nn = q["X"].shape[0], q["nn"]
    rows = n - q["i0"]
    D, Bv = np.full(rows, SENTINEL), np.full((rows, nn), SENTINEL)
    dD, dBv = np.full((2, rows), SENTINEL), np.full((2, rows, nn), SENTINEL)
    g = ctypes.c_int(-1)
    X, nbr, V = (np.ascontiguousarray(q[key]) for key in ("X", "nbr", "V"))
    P0 = np.ascontiguousarray(q["P0"]) if grad else None
    P1 = np.ascontiguousarray(q["P1"]) if grad else None
    ret = _lib().GPB_TestVifRows(n, q["d"], q["i0"], nn, q["m"], _dp(X), X.size, _ip(nbr), nbr.size, _dp(V), _dp(P0),
                                 _dp(P1), V.size, q["cov"], q["var"], q["phi"], q["nugget"], q["cjit"], int(grad), form,
                                 order, pad_fill, _dp(D), _dp(Bv), _dp(dD[0]) if grad else None,
                                 _dp(dD[1]) if grad else None, _dp(dBv[0]) if grad else None,
                                 _dp(dBv[1]) if grad else None, rows, ctypes.byref(g))
    return ret, dict(D=D, Bv=Bv, dD=dD, dBv=dBv), g.value


def rows_hook(inp, **kw):
    ret, out, g = rows_raw(inp, **kw)
    _check(ret)
    assert g == 0, "a guard word of the row outputs changed"
    return out


PROD_OPS = {"brow": 0, "bcol": 1, "bvec": 2, "btvec": 3}


def apply_raw(op, nbr, coef, inp, m, self_=1., D=None, div=0, want_div=0, X=None, order=0, pad_fill=np.nan,
              nbr_len=None):
    n, nn = nbr.shape
    mat = op in (0, 1)
    olen = n * ldm_of(m) if mat else n
    out, out2 = np.full(olen, SENTINEL), np.full(olen, SENTINEL)
    g = ctypes.c_int(-1)
    ret = _lib().GPB_TestVifApply(op, n, nn, m, _ip(nbr), nbr.size if nbr_len is None else nbr_len, _dp(coef), coef.size,
                                  _dp(D), _dp(inp), inp.size, self_, div, want_div, _dp(X), 0 if X is None else X.shape[1],
                                  order, pad_fill, _dp(out), _dp(out2) if want_div else None, olen, ctypes.byref(g))
    shape = (n, ldm_of(m)) if mat else (n,)
    return ret, out.reshape(shape), out2.reshape(shape), g.value


def apply_hook(op, *a, **kw):
    ret, out, out2, g = apply_raw(PROD_OPS[op], *a, **kw)
    _check(ret)
    assert g == 0, f"{op}: a guard word changed, or the gathered column-order values differ from the row values"
    return out, out2


VEC_OPS = {"gemv": 0, "coldot_w": 1, "coldot_m": 2, "zvec": 3, "sum": 4, "dkmn": 5}


def vector_raw(op, n, m, arrays, out_len, d=2, cov=0, var=1., phi=1., pad_fill=np.nan, sum_ops=None, lens=None):
    Dp = ctypes.POINTER(ctypes.c_double)
    arrs = (Dp * max(len(arrays), 1))(*[_dp(a) for a in arrays])
    ln = np.array([0 if a is None else a.size for a in arrays] if lens is None else lens, dtype=np.int64)
    so = None if sum_ops is None else np.asarray(sum_ops, dtype=np.int32)
    out = np.full(out_len, SENTINEL)
    g = ctypes.c_int(-1)
    ret = _lib().GPB_TestVifVector(op, n, m, d, cov, var, phi, pad_fill, arrs, _ip(ln, ctypes.c_int64), len(arrays),
                                   _ip(so), 0 if so is None else so.size, _dp(out), out_len, ctypes.byref(g))
    return ret, out, g.value


def vector_hook(op, *a, **kw):
    ret, out, g = vector_raw(VEC_OPS[op], *a, **kw)
    _check(ret)
    assert g == 0, f"{op}: a guard word changed"
    return out
