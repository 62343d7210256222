"""Cases, references and error bounds of the FITC kernel tests, shared by tests/test_gpu_fitc_ops.py (the HIP kernels
of csrc/fitc_kernels.hip and csrc/fitc_fisher.hip through the GPB_TestFitcVector / GPB_TestFitcKmeans hooks, which
call the launch functions of csrc/fitc.h that FitcSolver and fitc_inducing_points call, and the buffers of a
FitcSolver stage by stage through GPB_TestFitcStages) and
tests/test_fitc_ops_reference.py (CPU: every case reaches the path it is named for, float64 numpy stand-ins meet the
very bounds the kernels are held to, single-entry defects exceed them, the k-means reference is deterministic).

Inputs are float64, references numpy.longdouble (64-bit significand; assert_longdouble()) that restate each kernel's
comment; compute(op, case, LD) is the reference and compute(op, case, np.float64) the float64 stand-in (numpy's own
summation order). Bounds are first order in u = 2^-53 (UB = u + 2^-62 carries the reference's own rounding), gamma_j =
j UB / (1 - j UB), for a sum in ANY order, fma or not; none is tuned to what a kernel gives. N terms of c roundings
each are bounded by gamma_{N+c} times the sum of absolute values (Higham, Accuracy and Stability, eq. 3.5).

  kernel (op)            bound                                                                        c
  fitc_kmn/kmm_kernel    c_cov UB |k| + floor, c_cov = 8 + (d + 6) |x| (x: the exponent's argument;    -
  ff_dkmn_kernel         vif_ops_cases), c_cov + 4 for dk / dlog phi; floor = 2^-1022 var (1 + x + x^2):
  (kmn, kmm, dkmn)       below the smallest normal number a result is subnormal or flushed to 0. Exact:
                         kmm's diagonal (var, var (1 + 1e-6), 0) and K_mm,s = K_mm off it.
  fitc_diag_kernel       d_i = dvar - |V_i|^2 is a difference: e_d = gamma_{m+2} (dvar + |V_i|^2) absolute;   1
  (diag)                 K_d = K_mn (1 / d): |K_mn / d| (3 UB + e_d / |d|); sum log d: sum_i (e_d / |d_i| +
                         2 UB |log d_i|) + gamma_n sum |log d_i| (the library logarithm within 2 ulp).
  fitc_dy_kernel (dy)    (1 / d) y: 2 UB |y / d|                                                       2
  fitc_wsum_kernel       gamma_{chunks+1} (sum_z |P_z| + |K_mm,s|)                                     0
  fitc_gemv_part/reduce  gamma_{n+1} |M| |x|                                                           1
  fitc_symv_kernel       gamma_{m+1} |S| |x|                                                           1
  fitc_lower_t_kernel    exact: the transpose of the lower triangle, zeros above; the upper triangle of L
                         (NaN in the cases) is never read.
  symv + trmv_lower_t    t = L x: e_t = gamma_{m+1} |L| |x|; out = L^T t: gamma_{m+1} |L|^T |t| + |L|^T e_t    1
  (chol_solve)
  fitc_yaux_kernel       t = K_i . w, y_aux = Dy - t / d: gamma_{m+2} |K_i| . |w| / |d| + UB (|Dy| + |t / d|);  1
  (yaux)                 y^T y_aux: sum |y_i| e_i + gamma_{n+1} sum |y_i y_aux,i|
  fitc_grad_kernel       the eight wave sums: gamma_{m+1} on the absolute sum, plus |factor| e_dk for the   1
  (grad)                 four with dk recomputed from the coordinates (e_dk: the dkmn bound). Closing
                         expressions with absolute values: ddv = var - 2 c1v + (c1v - delta sa2): 3 e_c1v +
                         delta e_sa2 + 4 UB (var + 3 |c1v| + delta sa2); ddr = -2 c1r + c2r: 2 e_c1r + e_c2r +
                         UB (2 |c1r| + |c2r|); every product / quotient of s2*, s1* carries its factors'
                         errors and one UB per rounding (1 / d included). Block partials: sum of the up to
                         4 terms' bounds + gamma_3 sum |term|; the sums over all n: + gamma_n sum |term|.
  fitc_mm_kernel         gamma_{m^2+1} on the absolute sum for the four traces, gamma_{m^2+2} for a^T K a   1, 2
  (mm_terms)
  fitc_coldot_kernel     gamma_{m+1} |M_i| . |v| (|M_i|^2 for the squared form)                        1
  fitc_pred_corr_kernel  corr = sii - P_pi . K_oj: e_c = gamma_{m+1} |P_pi| . |K_oj| + UB (|sii| + |s|);  1
  (pred_corr)            f = corr / d: e_f = e_c / |d| + UB |f|; Maux -= K f: |K| e_f + 3 UB |K f| + UB |Maux|
  ff_diag_grad_kernel    base - (2 s1 - s2): 2 gamma_{m+1} |A_i| . |dK_i| + gamma_{m+1} |A_i| . |M_i| +       1
                         2 UB (|base| + 2 |s1| + |s2|)
  ff_recip_kernel        2 UB |1 / x|: a correctly rounded quotient is within u, a reciprocal refined by Newton
                         steps within 1 ulp = 2 u of the exact one
  ff_rowscale_kernel     v = alpha s X in any association: 3 UB |v| (two products and, unfused, the sum's share);
                         with Yin: + UB (|Yin| + |v|)
  ff_dot_kernel          gamma_{count+1} sum |a b|                                                     1
Conditions (asserted by tests/test_fitc_ops_reference.py): every bound is at most 1e-8 of its array's scale: the
largest magnitude of the array, or the scale of its terms where it is a difference that cancels (ddv by design:
the scale of s1*, s2* is the sum of the absolute values of their terms).

Bit-exact claims (np.array_equal against float64 numpy in the documented order; numpy does not contract and its sqrt
is correctly rounded): the k-means assignment (first strictly smaller rounded sqrt wins), the means (members added
in increasing index order, separately rounded, divided by the count; an empty cluster keeps its mean), the
partition arrays cnt / off / tot / base / list, the whole Lloyd loop, scanning path == member-list path.

Measured, largest error / bound over all cases. Float64 stand-in (tests/test_fitc_ops_reference.py): kmn 0.37,
kmm 0.38, dkmn 0.32, diag 0.27, dy 0.49, wsum 0.57, gemv 0.48, symv 0.34, lower_t 0, chol_solve 0.10, yaux 0.48,
grad 0.18, mm_terms 0.31, coldot 0.44, pred_corr 0.45, ff_diag_grad 0.26, ff_recip 0.49, ff_rowscale 0.98 (with Yin
and |v| << |Yin| the error is the final sum's own rounding, which reaches u |Y| in every evaluation order), ff_dot 0.29.
The kernels on an MI355X (tests/test_gpu_fitc_ops.py -s): fitc_kmn_kernel 0.37, fitc_kmm_kernel 0.35 (Kmm, Ks) /
0.33 (dK), ff_dkmn_kernel 0.31, fitc_diag_kernel 0.27 (d) / 0.21 (Kd) / 0.08 (sum log d), fitc_dy_kernel 0.87,
fitc_wsum_kernel 0.58, gemv 0.48, fitc_symv_kernel 0.34, fitc_lower_t_kernel 0, chol_solve 0.10, fitc_yaux_kernel
0.48 (y_aux) / 0.18 (y^T y_aux), fitc_grad_kernel 0.18 (sums) / 0.14 (block partials), fitc_mm_kernel 0.31,
fitc_coldot_kernel 0.44, fitc_pred_corr_kernel 0.45 (Maux) / 0.02 (corr), ff_diag_grad_kernel 0.26, ff_recip_kernel
0.49, ff_rowscale_kernel 0.99, ff_dot_kernel 0.29. Every bit-exact k-means claim held on every case, the Lloyd loops
(4, 3 (2-cycle), 2 (cap) and 9 iterations) included.

Stages (GPB_TestFitcStages: a FitcSolver on X, Z, y runs Factor, Eval with the gradient, Gram then Eval at the same
or at other parameters, or Predict, and its buffers are copied out). Cases (n, m, d, covariance) = (37, 5, 1,
exponential), (130, 65, 3, matern15), (300, 70, 2, gaussian), (4100, 130, 2, matern25); Z is a farthest-point subset
of X and the range half the smallest distance between inducing points: cond_2(K_mm,s) = 1.5, 1.7, 1.05, 1.8 and
cond_2(W) = 3.5, 2.6, 1.8, 10.6 (asserted <= 1e4 and <= 1e6). Array by array:
  Kmn, Kmm, Ks, dKmm            the covariance bound above, and the exact diagonals
  LiT, WiT                      exactly lower_t of Li, Wi
  d, Kd, Dy, u, w, y_aux, a     each kernel's own bound above on the buffers the GPU handed it (V, Kmn, d, Dy, Wi, WiT,
                                u, w, A): composition step by step, where a clobbered scratch or partial buffer shows
  the six sums                  the grad and mm_terms bounds on the GPU's own Kmn, A, G^T (in Kd_), M (in V_), a, d,
                                y_aux, Kinv, Winv, Kmm, dKmm; and 1e-9 (logdet, quadratic form) / 1e-7 (gradient
                                sums) relative to the longdouble chain, the project's scalar tolerances
  Li, Kinv, V, W (= L_W), Wi,   the chain Cholesky -> TRTRI -> MFMA GEMM is not closed to first order: the float64
  A, Winv, G^T, M; Predict's    numpy stand-in of the same algebra is measured against the longdouble chain and the
  mean, var, cov                kernels may err 8 times that (max norm per array). Stand-in errors, largest over the
                                four cases (the allowance is 8 times the case's own figure): Li 2.0e-16, Kinv 7.6e-16,
                                V 4.8e-16, W 2.0e-15, Wi 2.9e-16, A 1.1e-15, Winv 3.9e-16, G^T 5.4e-16, M 7.3e-16,
                                mean 7.8e-16, var 7.4e-16, cov 7.4e-16. On the GPU, error / allowance: Li 0.29, Kinv 0.19, V 0.19, W 0.23,
                                Wi 0.17, A 0.15, Winv 0.15, G^T 0.20, M 0.19, mean 0.22, var 0.16, cov 0.13.
  (measured on the GPU)         covariance bound: Kmn 0.49, Kmm / Ks 0.40, dKmm 0.40; kernel bounds on the GPU's own
                                buffers: d 0.11, Kd 0.17, Dy 0.87, u 0.03, w 0.10, y_aux 0.49, a 0.05, sums 0.01;
                                sums against the longdouble chain: at most 5.2e-16 relative
  every array                   within 1e-8 of its largest magnitude of the longdouble chain
Bitwise: Gram -> Eval at the same parameters (the kept_ hand-over) and Gram at other parameters -> Eval both give
the bits of a fresh Eval in every buffer and sum. Predict runs with several prediction points matched to one
training point, in no order, against the dense corr D^-1 corr^T.
"""
import ctypes
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vif_ops_cases import (LD, U, UB, COV_NAMES, HookError, assert_longdouble, cov_dcov, dist, gamma,  # noqa: E402,F401
                           ldm_of, max_ratio, phi_of)
from sparse_chol_cases import longdouble_cholesky  # noqa: E402


def _dp(a):
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a, ty=ctypes.c_int32):
    if a is None:
        return None
    assert a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.POINTER(ty))


VAR = 3.7
RANGE = 0.3
JIT = 1. + 1e-6
TINY = 2.0 ** -1022
N_COL = (1, 3, 4, 5, 9)                       # one wave per observation, 4 per block
M_COL = (1, 3, 63, 64, 65, 130)               # lane stride 64; ldm != m
N_GEMV = N_COL + (63, 64, 65, 4097)           # chunks of 64 observations; 4097: nb = 65, the reduce's second stride
M_GEMV = M_COL + (257,)                       # thread stride 256
M_SQ = (1, 4, 5, 64, 65, 130)
WSUM = tuple((c, m) for c in (1, 2, 5) for m in (3, 65))

VEC_OPS = {"kmn": 0, "kmm": 1, "dkmn": 2, "diag": 3, "dy": 4, "wsum": 5, "gemv": 6, "symv": 7, "lower_t": 8,
           "chol_solve": 9, "yaux": 10, "grad": 11, "mm_terms": 12, "coldot": 13, "pred_corr": 14, "ff_diag_grad": 15,
           "ff_recip": 16, "ff_rowscale": 17, "ff_dot": 18}


def f64(a):
    return np.asarray(a, dtype=np.float64)


def af(a):
    return np.abs(f64(a))


# ------------------------------------------------------------------------------------------------ cases
def cov_points(n, m, d, seed):
    """X (n x d), Z (m x d) in the unit cube; X[n - 1] = Z[0] (a coincident pair: r = 0 exactly) and, with n >= 3,
    X[1] 1000 units away (the exponential underflows to 0 for every inducing point)"""
    g = np.random.default_rng(seed)
    X, Z = g.uniform(size=(n, d)), g.uniform(size=(m, d))
    X[n - 1] = Z[0]
    if n >= 3:
        X[1] += 1000.
    return X, Z


def kmm_points(m, d, seed):
    """Z with Z[1] = Z[0] (m >= 4: an off-diagonal r = 0) and Z[m - 1] far from the rest (m >= 3)"""
    Z = np.random.default_rng(seed).uniform(size=(m, d))
    if m >= 4:
        Z[1] = Z[0]
    if m >= 3:
        Z[m - 1] += 1000.
    return Z


def _case(op, **kw):
    return dict(dict(op=op, d=2, cov=0, var=VAR, phi=1., extra=0., ints=None), **kw)


@functools.lru_cache(maxsize=None)
def vec_cases(op):
    """name -> case (the hook's arrays under 'arrays', shapes n, m and the scalars) of one op"""
    out = {}
    g = np.random.default_rng(1000 + VEC_OPS[op])
    nrm, uni = g.standard_normal, g.uniform
    if op in ("kmn", "dkmn", "kmm", "grad"):
        # every covariance x d at (9, 65), then the column shapes (kmm: m alone) with cov and d cycling
        shapes = [(9, 65)] * 12 + ([(1, m) for m in M_COL] if op == "kmm" else [(n, m) for n in N_COL for m in M_COL])
        for q, (n, m) in enumerate(shapes):
            cov, d = q % 4, 1 + (q // 4) % 3
            c = _case(op, n=n, m=m)
            c.update(cov=cov, d=d, phi=phi_of(cov, RANGE))
            if op == "kmm":
                c["arrays"] = [kmm_points(m, d, q)]
                c["n"] = 1
            else:
                c["arrays"] = list(cov_points(n, m, d, 50 + q))
            if op == "grad":
                sc = 1. / np.sqrt(m)
                c["arrays"] += [nrm((n, m)), nrm((n, m)) * sc, nrm((n, m)) * sc, nrm((n, m)) * sc, nrm(m),
                                uni(0.5, 2., size=n), nrm(n)]
                c["extra"] = VAR * JIT - VAR
            out[f"{op}-{q}-{COV_NAMES[cov]}-d{d}-n{n}-m{m}"] = c
        return out
    if op in ("diag", "yaux", "coldot", "ff_diag_grad"):
        for n in N_COL:
            for m in M_COL:
                c = _case(op, n=n, m=m)
                if op == "diag":
                    V = nrm((n, m))
                    c["extra"] = 1. + VAR * JIT
                    V *= np.sqrt(0.5 * c["extra"] / (V * V).sum(axis=1).max())   # d >= dvar / 2
                    c["arrays"] = [V, nrm((n, m))]
                elif op == "yaux":
                    c["arrays"] = [nrm((n, m)), nrm(m) / np.sqrt(m), nrm(n), nrm(n), uni(0.5, 2., size=n)]
                elif op == "coldot":
                    c["arrays"] = [nrm((n, m)), nrm(m)]
                    out[f"coldot-sq-n{n}-m{m}"] = dict(c, arrays=[c["arrays"][0], None])
                else:
                    c["arrays"] = [nrm((n, m)), nrm((n, m)), nrm((n, m))]
                    c["extra"] = VAR if (n + m) % 2 else 0.
                out[f"{op}-n{n}-m{m}"] = c
        return out
    if op == "gemv":
        for n in N_GEMV:
            for m in M_GEMV:
                out[f"gemv-n{n}-m{m}"] = _case(op, n=n, m=m, arrays=[nrm((n, m)), nrm(n)])
        return out
    if op in ("dy", "ff_recip"):
        for n in (1, 255, 256, 257):
            d_ = uni(0.5, 2., size=n) * g.choice([-1., 1.], size=n)
            out[f"{op}-n{n}"] = _case(op, n=n, m=1, arrays=[d_, nrm(n)] if op == "dy" else [d_])
        return out
    if op == "wsum":
        for ch, m in WSUM:
            out[f"wsum-c{ch}-m{m}"] = _case(op, n=1, m=m, arrays=[nrm((ch, m, m)), nrm((m, m))], ints=[ch])
        return out
    if op in ("symv", "lower_t", "chol_solve", "mm_terms"):
        for m in M_SQ:
            c = _case(op, n=1, m=m)
            if op == "symv":
                c["arrays"] = [nrm((m, m)), nrm(m)]
            elif op == "mm_terms":
                c["arrays"] = [nrm((m, m)), nrm((m, m)), nrm((m, m)), nrm((m, m)), nrm(m)]
            else:
                # the hook's row k is the device's column k: host[k, j] = L[j, k], so the lower triangle of L is the
                # host array's upper triangle (k <= j) and L's unread upper triangle its strict lower one: NaN
                Lh = nrm((m, m))
                Lh[np.tril_indices(m, -1)] = np.nan
                c["arrays"] = [Lh] if op == "lower_t" else [Lh, lower_t_ref(Lh), nrm(m)]
            out[f"{op}-m{m}"] = c
        return out
    if op == "pred_corr":
        n, npred = 40, 12
        pair_sets = {"none": [], "one": [(5, 17)], "same-train": [(0, 7), (3, 7), (11, 7), (4, 2)],
                     "unsorted": [(9, 30), (1, 4), (6, 39), (0, 4), (11, 0), (2, 30)]}
        for m in (50, 65):
            for pname, pairs in pair_sets.items():
                c = _case(op, n=n, m=m, np=npred, pairs=pairs, extra=VAR,
                          arrays=[nrm((npred, m)) / np.sqrt(m), nrm((n, m)), uni(0.5, 2., size=n), nrm((npred, m))],
                          ints=[npred] + [v for p in pairs for v in p])
                out[f"pred_corr-m{m}-{pname}"] = c
        return out
    if op == "ff_rowscale":
        for n, t in ((1, 1), (5, 3), (300, 7), (4100, 257)):      # 4100 x 257 > 4096 x 256: the grid-stride loop
            for yin in (False, True):
                c = _case(op, n=n, m=t, extra=-1.25, ints=[0],
                          arrays=[nrm(n), nrm((t, n)), nrm((t, n)) if yin else None])
                out[f"ff_rowscale-n{n}-t{t}-{'yin' if yin else 'noyin'}"] = c
                if yin:
                    out[f"ff_rowscale-n{n}-t{t}-alias"] = dict(c, ints=[1])
        return out
    if op == "ff_dot":
        for n in (1, 255, 131072 + 5):                          # 512 blocks x 256 threads = 131072: the stride loop
            out[f"ff_dot-n{n}"] = _case(op, n=n, m=1, arrays=[nrm(n), nrm(n)])
        return out
    raise KeyError(op)


def lower_t_ref(Lh):
    """the hook's LT (host rows = device columns) of the hook's L: LT[k, j] = L[j, k] for k <= j, exact zeros above.
    Host row j of the output is device column j of LT: out[j, k] = LT[k, j] = L[j, k] = Lh[k, j] for k <= j, else 0."""
    m = Lh.shape[0]
    out = np.zeros((m, m))
    iu = np.triu_indices(m)            # (k, j), k <= j
    out[iu[1], iu[0]] = Lh[iu]
    return out


# ------------------------------------------------------------------------------------------------ compute
def _cov(X, Z, c, T):
    """(k, dk, |x|) n x m in the dtype T"""
    k, dk, x = cov_dcov(dist(X.astype(T), Z.astype(T)), c["var"], c["phi"], c["cov"])
    return k, dk, x


def grad_pieces(c, T):
    X, Z, K, A, Gt, Mr, a, dv, ya = (v.astype(T) for v in c["arrays"])
    var, delta = T(c["var"]), T(c["extra"])
    _, dk, _ = _cov(c["arrays"][0], c["arrays"][1], c, T)
    w = dict(c1v=(A * K).sum(1), sa2=(A * A).sum(1), gv=K @ a, f=(Gt * K).sum(1), c1r=(A * dk).sum(1),
             c2r=(A * Mr).sum(1), er=(Gt * dk).sum(1), gr=dk @ a)
    inv = 1 / dv
    ddv = var - 2 * w["c1v"] + (w["c1v"] - delta * w["sa2"])
    ddr = -2 * w["c1r"] + w["c2r"]
    w.update(inv=inv, ddv=ddv, ddr=ddr, ya=ya, dk=dk)
    w["s2v"] = ddv * inv + 2 * w["f"] * inv - ddv * w["f"] * inv * inv
    w["s2r"] = ddr * inv + 2 * w["er"] * inv - ddr * w["f"] * inv * inv
    w["s1v"] = -ya * w["gv"] - ddv * ya * ya / 2
    w["s1r"] = -ya * w["gr"] - ddr * ya * ya / 2
    return w


def block4(v):
    """sums over the blocks of 4 observations"""
    n = v.shape[0]
    p = np.zeros((n + 3) // 4 * 4, dtype=v.dtype)
    p[:n] = v
    return p.reshape(-1, 4).sum(axis=1)


def compute(c, T):
    """the outputs of a case's kernel (dict name -> array) in the dtype T, restating the kernel's comment"""
    op = c["op"]
    a = [None if v is None else v.astype(T) for v in c["arrays"]]
    if op in ("kmn", "dkmn"):
        k, dk, _ = _cov(c["arrays"][0], c["arrays"][1], c, T)
        return {"K": k if op == "kmn" else dk}
    if op == "kmm":
        k, dk, _ = _cov(c["arrays"][0], c["arrays"][0], c, T)
        m = k.shape[0]
        k[np.diag_indices(m)] = T(c["var"])
        dk[np.diag_indices(m)] = 0
        ks = k.copy()
        ks[np.diag_indices(m)] = T(c["var"]) * T(JIT)
        return {"Kmm": k, "Ks": ks, "dK": dk}
    if op == "diag":
        dv = T(c["extra"]) - (a[0] * a[0]).sum(1)
        return {"d": dv, "Kd": a[1] / dv[:, None], "logd": np.log(dv).sum(keepdims=True)}
    if op == "dy":
        return {"Dy": a[1] / a[0]}
    if op == "wsum":
        return {"W": a[0].sum(axis=0) + a[1]}
    if op == "gemv":
        return {"out": a[0].T @ a[1]}
    if op == "symv":
        return {"out": a[0] @ a[1]}                 # host row j = device column j: out_j = sum_k S[k, j] x_k
    if op == "lower_t":
        return {"LT": lower_t_ref(c["arrays"][0]).astype(T)}
    if op == "chol_solve":
        L = np.triu(np.nan_to_num(a[0])).T          # L[j, k] = host[k, j], k <= j
        return {"out": L.T @ (L @ a[2])}
    if op == "yaux":
        t = a[0] @ a[1]
        ya = a[3] - t / a[4]
        return {"yaux": ya, "q": (a[2] * ya).sum(keepdims=True)}
    if op == "grad":
        w = grad_pieces(c, T)
        terms = np.stack([w["s1v"], w["s1r"], w["s2v"], w["s2r"]], axis=1)
        return {"sums": terms.sum(axis=0), "parts": np.stack([block4(terms[:, q]) for q in range(4)], axis=1)}
    if op == "mm_terms":
        ki, wi, km, dk, av = a
        return {"sums": np.array([(ki * km).sum(), (wi * km).sum(), (ki * dk).sum(), (wi * dk).sum(),
                                  av @ km @ av, av @ dk @ av], dtype=T)}
    if op == "coldot":
        return {"out": a[0] @ a[1] if a[1] is not None else (a[0] * a[0]).sum(1)}
    if op == "pred_corr":
        P, K, dv, Maux = a
        Maux = Maux.copy()
        corr = np.zeros(max(len(c["pairs"]), 1), dtype=T)
        for q, (pi, oj) in enumerate(c["pairs"]):
            corr[q] = T(c["extra"]) - P[pi] @ K[oj]
            Maux[pi] -= K[oj] * (corr[q] / dv[oj])
        return {"Maux": Maux, "corr": corr}
    if op == "ff_diag_grad":
        return {"dd": T(c["extra"]) - (2 * (a[0] * a[1]).sum(1) - (a[0] * a[2]).sum(1))}
    if op == "ff_recip":
        return {"y": 1 / a[0]}
    if op == "ff_rowscale":
        v = T(c["extra"]) * a[0][None, :] * a[1]
        return {"Y": v + a[2] if a[2] is not None else v}
    if op == "ff_dot":
        return {"sum": (a[0] * a[1]).sum(keepdims=True)}
    raise KeyError(op)


# ------------------------------------------------------------------------------------------------ bounds
def cov_bound(c, X, Z, deriv):
    k, dk, x = _cov(X, Z, c, LD)
    x = af(x)
    floor = TINY * c["var"] * (1. + x + x * x)
    return ((12. if deriv else 8.) + (c["d"] + 6) * x) * UB * af(dk if deriv else k) + floor


def bounds(c):
    """(bound, scale) dicts over compute(c, LD)'s outputs: float64 error bounds and the scale the 1e-8 condition is
    taken against (None: the array's largest magnitude)"""
    op = c["op"]
    A = c["arrays"]
    n, m = c["n"], c["m"]
    ref = compute(c, LD)
    sc = {k: None for k in ref}
    if op in ("kmn", "dkmn"):
        return {"K": cov_bound(c, A[0], A[1], op == "dkmn")}, sc
    if op == "kmm":
        b, bd = cov_bound(c, A[0], A[0], False), cov_bound(c, A[0], A[0], True)
        for e in (b, bd):
            e[np.diag_indices(m)] = 0.
        bs = b.copy()
        bs[np.diag_indices(m)] = UB * c["var"] * JIT          # the one product of the diagonal (exact in the tests)
        return {"Kmm": b, "Ks": bs, "dK": bd}, sc
    if op == "diag":
        s = (A[0] * A[0]).sum(1)
        ed = gamma(m + 2) * (c["extra"] + s)
        dv, lg = af(ref["d"]), af(np.log(ref["d"]))
        return {"d": ed, "Kd": np.abs(A[1]) / dv[:, None] * (3 * UB + ed / dv)[:, None],
                "logd": np.array([(ed / dv + 2 * UB * lg).sum() + gamma(n) * lg.sum()])}, \
            dict(sc, logd=max(lg.sum(), 1.))
    if op == "dy":
        return {"Dy": 2 * UB * af(ref["Dy"])}, sc
    if op == "wsum":
        return {"W": gamma(c["ints"][0] + 1) * (np.abs(A[0]).sum(axis=0) + np.abs(A[1]))}, sc
    if op == "gemv":
        return {"out": gamma(n + 1) * (np.abs(A[0]).T @ np.abs(A[1]))}, sc
    if op == "symv":
        return {"out": gamma(m + 1) * (np.abs(A[0]) @ np.abs(A[1]))}, sc
    if op == "lower_t":
        return {"LT": np.zeros((m, m))}, sc
    if op == "chol_solve":
        L = np.abs(np.triu(np.nan_to_num(A[0])).T)
        Ll = np.triu(np.nan_to_num(A[0])).T.astype(LD)
        t = af(Ll @ A[2].astype(LD))
        et = gamma(m + 1) * (L @ np.abs(A[2]))
        return {"out": gamma(m + 1) * (L.T @ t) + L.T @ et}, sc
    if op == "yaux":
        K, w, y, Dy, dv = A
        S = np.abs(K) @ np.abs(w)
        t = af(K.astype(LD) @ w.astype(LD))
        e = gamma(m + 2) * S / np.abs(dv) + UB * (np.abs(Dy) + t / np.abs(dv))
        ya = af(ref["yaux"])
        return {"yaux": e, "q": np.array([(np.abs(y) * e).sum() + gamma(n + 1) * (np.abs(y) * ya).sum()])}, \
            dict(sc, q=max((np.abs(y) * ya).sum(), 1e-300))
    if op == "grad":
        return grad_bounds(c)
    if op == "mm_terms":
        ki, wi, km, dk, av = (np.abs(v) for v in A)
        g1, g2 = gamma(m * m + 1), gamma(m * m + 2)
        ab = np.array([g1 * (ki * km).sum(), g1 * (wi * km).sum(), g1 * (ki * dk).sum(), g1 * (wi * dk).sum(),
                       g2 * (av @ km @ av), g2 * (av @ dk @ av)])
        scale = np.array([(ki * km).sum(), (wi * km).sum(), (ki * dk).sum(), (wi * dk).sum(), av @ km @ av, av @ dk @ av])
        return {"sums": ab}, {"sums": scale}
    if op == "coldot":
        M = np.abs(A[0])
        return {"out": gamma(m + 1) * (M @ np.abs(A[1]) if A[1] is not None else (M * M).sum(1))}, sc
    if op == "pred_corr":
        P, K, dv, Maux = A
        eM = np.zeros(Maux.shape)
        ec = np.zeros(max(len(c["pairs"]), 1))
        for q, (pi, oj) in enumerate(c["pairs"]):
            s = float(abs(P[pi].astype(LD) @ K[oj].astype(LD)))
            ec[q] = gamma(m + 1) * (np.abs(P[pi]) @ np.abs(K[oj])) + UB * (abs(c["extra"]) + s)
            f = abs(float(ref["corr"][q])) / abs(dv[oj])
            ef = ec[q] / abs(dv[oj]) + UB * f
            eM[pi] = np.abs(K[oj]) * ef + 3 * UB * np.abs(K[oj]) * f + UB * np.abs(Maux[pi])
        return {"Maux": eM, "corr": ec}, dict(sc, corr=max(abs(c["extra"]), 1.))
    if op == "ff_diag_grad":
        s1a, s2a = (np.abs(A[0]) * np.abs(A[1])).sum(1), (np.abs(A[0]) * np.abs(A[2])).sum(1)
        s1, s2 = af((A[0].astype(LD) * A[1]).sum(1)), af((A[0].astype(LD) * A[2]).sum(1))
        return {"dd": 2 * gamma(m + 1) * s1a + gamma(m + 1) * s2a + 2 * UB * (abs(c["extra"]) + 2 * s1 + s2)}, \
            {"dd": np.maximum(af(ref["dd"]), abs(c["extra"]) + 2 * s1a + s2a)}
    if op == "ff_recip":
        return {"y": 2 * UB * af(ref["y"])}, sc
    if op == "ff_rowscale":
        v = np.abs(c["extra"] * A[0][None, :] * A[1])
        return {"Y": 3 * UB * v + (UB * (np.abs(A[2]) + v) if A[2] is not None else 0.)}, \
            {"Y": float(v.max() + (np.abs(A[2]).max() if A[2] is not None else 0.))}
    if op == "ff_dot":
        S = float((np.abs(A[0]) * np.abs(A[1])).sum())
        return {"sum": np.array([gamma(n + 1) * S])}, {"sum": S}
    raise KeyError(op)


def grad_bounds(c):
    X, Z, K, A, Gt, Mr, a, dv, ya = c["arrays"]
    n, m = c["n"], c["m"]
    w = {k: f64(v) for k, v in grad_pieces(c, LD).items()}
    edk = cov_bound(c, X, Z, True)
    adk = np.abs(w["dk"])
    g = gamma(m + 1)
    aK, aA, aG, aa = np.abs(K), np.abs(A), np.abs(Gt), np.abs(a)
    e = dict(c1v=g * (aA * aK).sum(1), sa2=g * (aA * aA).sum(1), gv=g * (aK @ aa), f=g * (aG * aK).sum(1),
             c1r=g * (aA * adk).sum(1) + (aA * edk).sum(1), c2r=g * (aA * np.abs(Mr)).sum(1),
             er=g * (aG * adk).sum(1) + (aG * edk).sum(1), gr=g * (adk @ aa) + edk @ aa)
    var, delta = c["var"], c["extra"]
    ab = {k: np.abs(w[k]) for k in w}
    inv, f, yaa = ab["inv"], ab["f"], np.abs(ya)
    # ddv cancels by design: its scale is that of its terms
    sddv = var + 3 * ab["c1v"] + delta * ab["sa2"]
    eddv = 3 * e["c1v"] + delta * e["sa2"] + 4 * UB * sddv
    sddr = 2 * ab["c1r"] + ab["c2r"]
    eddr = 2 * e["c1r"] + e["c2r"] + UB * sddr

    def s2(dd, edd, sdd, x, ex):
        # dd inv + 2 x inv - dd f inv inv: (terms' bounds, terms' scale)
        t1, t2, t3 = np.abs(dd) * inv, 2 * np.abs(x) * inv, np.abs(dd) * f * inv * inv
        e1 = edd * inv + 2 * UB * t1
        e2 = 2 * ex * inv + 2 * UB * t2
        e3 = (edd * f + np.abs(dd) * e["f"]) * inv * inv + 5 * UB * t3
        return e1 + e2 + e3 + 2 * UB * (t1 + t2 + t3), sdd * inv + t2 + sdd * f * inv * inv

    def s1(dd, edd, sdd, x, ex):
        # -ya x - dd ya ya / 2
        t1, t2 = yaa * np.abs(x), 0.5 * np.abs(dd) * yaa * yaa
        return yaa * ex + 0.5 * yaa * yaa * edd + UB * (2 * t1 + 4 * t2), t1 + 0.5 * sdd * yaa * yaa

    per = [s1(w["ddv"], eddv, sddv, w["gv"], e["gv"]), s1(w["ddr"], eddr, sddr, w["gr"], e["gr"]),
           s2(w["ddv"], eddv, sddv, w["f"], e["f"]), s2(w["ddr"], eddr, sddr, w["er"], e["er"])]
    terms = [np.abs(w[k]) for k in ("s1v", "s1r", "s2v", "s2r")]
    eparts = np.stack([block4(per[q][0]) + gamma(3) * block4(terms[q]) for q in range(4)], axis=1)
    esums = np.array([per[q][0].sum() + gamma(n) * terms[q].sum() for q in range(4)])
    sparts = np.stack([block4(per[q][1]) for q in range(4)], axis=1)
    ssums = np.array([per[q][1].sum() for q in range(4)])
    return {"sums": esums, "parts": eparts}, {"sums": ssums, "parts": sparts}


def condition(c):
    """largest bound / (1e-8 scale) over a case's outputs: at most 1 (the bounds are at least ten times tighter than
    the 1e-7 of the scalar checks)"""
    ref = compute(c, LD)
    bnd, sc = bounds(c)
    worst = 0.
    for k, b in bnd.items():
        s = sc[k]
        if s is None:
            s = float(np.nanmax(af(ref[k]))) if ref[k].size else 1.
            if s == 0.:
                assert np.all(f64(b) <= TINY * 1e9), (c["op"], k)
                continue
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(f64(b) == 0., 0., f64(b) / (1e-8 * f64(s)))
        worst = max(worst, float(np.max(r)))
    return worst


def ratios(c, out):
    """name -> largest |out - reference| / bound"""
    ref = compute(c, LD)
    bnd, _ = bounds(c)
    return {k: max_ratio(np.abs(np.asarray(out[k]).reshape(ref[k].shape).astype(LD) - ref[k]),
                         np.broadcast_to(bnd[k], ref[k].shape)) for k in ref}


# ------------------------------------------------------------------------------------------------ k-means
def km_dist(X, mu):
    """float64 distances n x k with the reference's operations: squares summed in coordinate order, separately
    rounded (numpy does not contract), then a correctly rounded sqrt"""
    t = X[:, None, 0] - mu[None, :, 0]
    s = t * t
    for q in range(1, X.shape[1]):
        t = X[:, None, q] - mu[None, :, q]
        s = s + t * t
    return np.sqrt(s)


def km_assign(X, mu):
    """the first centre with the smallest rounded distance (argmin keeps the first of equal values: a later centre
    wins only with a strictly smaller one)"""
    return np.argmin(km_dist(X, mu), axis=1).astype(np.int32)


def km_means(X, cl, mu_old):
    """members added in increasing index order, divided by the count; an empty cluster keeps its mean"""
    k, d = mu_old.shape
    s = np.zeros((k, d))
    cnt = np.zeros(k, dtype=np.int64)
    for i in range(X.shape[0]):
        s[cl[i]] = s[cl[i]] + X[i]
        cnt[cl[i]] += 1
    mu = mu_old.copy()
    nz = cnt > 0
    mu[nz] = s[nz] / cnt[nz, None].astype(np.float64)
    return mu


def km_partition(cl, k):
    """cnt, off (nbk x k), tot (k), base (k + 1), list (n) of the stable partition by cluster in blocks of 256"""
    n = cl.shape[0]
    nbk = (n + 255) // 256
    cnt = np.zeros((nbk, k), dtype=np.int32)
    for b in range(nbk):
        cnt[b] = np.bincount(cl[b * 256:(b + 1) * 256], minlength=k)
    off = (np.cumsum(cnt, axis=0) - cnt).astype(np.int32)
    tot = cnt.sum(axis=0).astype(np.int32)
    base = np.concatenate([[0], np.cumsum(tot)]).astype(np.int32)
    return cnt, off, tot, base, np.argsort(cl, kind="stable").astype(np.int32)


def km_lloyd(X, seeds, max_it):
    """(final means, iterations): until the means repeat the previous or the one-before-previous iterate"""
    mu, old, old_old = seeds.copy(), np.zeros(seeds.shape), np.zeros(seeds.shape)
    count = 0
    while True:
        old_old, old = old, mu
        mu = km_means(X, km_assign(X, old), old)
        count += 1
        if np.array_equal(mu, old) or np.array_equal(mu, old_old) or count == max_it:
            return mu, count


KM_N = (1, 64, 255, 256, 257, 2305)           # 2305: nbk = 10, the 8-batched offsets loop plus its tail
KM_K = (1, 7, 8, 9, 64, 65, 257)
KM_SIZES = (0, 1, 7, 8, 9, 70)                # members per cluster around the 8-batched loads of the means


@functools.lru_cache(maxsize=None)
def km_cases():
    """name -> (X, mu): point clouds for every (n, k <= n) with d cycling, designed member counts, all points in one
    cluster, exact ties on an integer lattice"""
    out = {}
    q = 0
    for n in KM_N:
        for k in KM_K:
            if k > n:
                continue
            d = 1 + q % 3
            q += 1
            g = np.random.default_rng(7000 + q)
            X = g.uniform(size=(n, d))
            out[f"cloud-n{n}-k{k}-d{d}"] = (X, X[g.choice(n, size=k, replace=False)].copy())
    for d in (1, 2, 3):
        # cluster c has KM_SIZES[c % 6] members near centre c (centres 10 apart on the first axis); k = 12
        g = np.random.default_rng(7100 + d)
        k = 12
        mu = np.zeros((k, d))
        mu[:, 0] = 10. * np.arange(k)
        pts = [mu[c] + g.uniform(-1., 1., size=(KM_SIZES[c % 6], d)) for c in range(k)]
        X = np.concatenate(pts)
        out[f"sizes-d{d}"] = (X[g.permutation(X.shape[0])].copy(), mu)
        # every point in cluster 2 of 9
        mu1 = 100. + 10. * g.uniform(size=(9, d))
        mu1[2] = 0.5
        out[f"one-cluster-d{d}"] = (g.uniform(size=(300, d)), mu1)
    # exact ties: the lattice {0, 1, 2}^d with centres on its corners {0, 2}^d: the centre of the lattice is equally
    # far from all of them, the edge midpoints from two or four
    for d in (1, 2, 3):
        ax = np.arange(3.)
        X = np.stack(np.meshgrid(*([ax] * d), indexing="ij"), axis=-1).reshape(-1, d)
        mu = np.stack(np.meshgrid(*([np.array([0., 2.])] * d), indexing="ij"), axis=-1).reshape(-1, d)
        out[f"lattice-d{d}"] = (X, mu)
    return out


def sqrt_tie_cases():
    """(X, mu) with n = 1, k = 2, d = 2: squared distances s0 < s1 = nextafter(s0) whose square roots round to the
    same float64, in both orders of the centres (the earlier centre must win either way).
    x = 0, centres (p, 0) and (p, 2^-26) with p = i 2^-26, 2^26 < i < 2^26.5: s0 = i^2 2^-52 in [1, 2) exactly,
    s1 = s0 + 2^-52, sqrt(s1) = p (1 + 1 / (2 i^2) - ...) lies less than half an ulp above p."""
    out = []
    g = np.random.default_rng(99)
    for i in g.integers(2 ** 26 + 1, int(2 ** 26.5) - 1, size=8):
        p = float(i) * 2.0 ** -26
        a, b = np.array([p, 0.]), np.array([p, 2.0 ** -26])
        for mu in (np.stack([a, b]), np.stack([b, a])):
            out.append((np.zeros((1, 2)), mu))
    return out


def lloyd_cases():
    """name -> (X, seeds, max_it)"""
    g = np.random.default_rng(4242)
    cen = np.array([[0., 0.], [5., 0.], [0., 5.], [5., 5.], [2.5, 9.]])
    X = np.concatenate([c + 0.4 * g.standard_normal((60, 2)) for c in cen])
    X = X[g.permutation(X.shape[0])]
    out = {"blobs": (X, X[[0, 1, 2, 3, 4]].copy(), 1000)}
    Y = g.uniform(size=(2305, 3))
    out["uniform-cap2"] = (Y, Y[:9].copy(), 2)
    out["uniform-d1"] = (g.uniform(size=(257, 1)), g.uniform(size=(65, 1)), 1000)
    # the 2-cycle stop (mu == old_old != old). In exact arithmetic Lloyd's iteration cannot cycle; with integers next to
    # 2^52 the sum of a cluster's members and its mean round at the points' own spacing, and a boundary point flips
    # back and forth (found by a random search over such configurations with km_lloyd)
    b = 2.0 ** 52
    out["two-cycle"] = (b + np.array([[26.], [36.], [24.], [25.], [32.], [20.], [27.], [30.], [22.]]),
                        b + np.array([[24.], [25.], [36.]]), 1000)
    return out


# ------------------------------------------------------------------------------------------------ the hooks
def _lib():
    c = ctypes
    from gpboost_amd import basic
    lib = basic.lib()
    if not getattr(lib, "_fitc_ops_typed", False):
        Dp, I, L, F = c.POINTER(c.c_double), c.c_int, c.c_int64, c.c_double
        PI, PL, PG = c.POINTER(c.c_int32), c.POINTER(c.c_int64), c.POINTER(c.c_int)
        lib.GPB_TestFitcVector.argtypes = [I, I, I, I, I, F, F, F, F, c.POINTER(Dp), PL, I, PI, L, c.POINTER(Dp), PL, I, PG]
        lib.GPB_TestFitcKmeans.argtypes = [I, I, I, I, Dp, L, Dp, Dp, Dp, L, PI, L, I, I, Dp, PI, L, PG, PG]
        lib.LGBM_GetLastError.restype = c.c_char_p
        lib._fitc_ops_typed = True
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


def out_shapes(c):
    """name -> (rows, cols, padded): the hook's outputs in compute()'s order; padded ones come back rows x ldm"""
    op, n, m = c["op"], c["n"], c["m"]
    nb4 = (n + 3) // 4
    return {"kmn": {"K": (n, m, True)}, "dkmn": {"K": (n, m, True)},
            "kmm": {"Kmm": (m, m, True), "Ks": (m, m, True), "dK": (m, m, True)},
            "diag": {"d": (n, 1, False), "Kd": (n, m, True), "logd": (1, 1, False)},
            "dy": {"Dy": (n, 1, False)}, "wsum": {"W": (m, m, True)}, "gemv": {"out": (m, 1, False)},
            "symv": {"out": (m, 1, False)}, "lower_t": {"LT": (m, m, True)}, "chol_solve": {"out": (m, 1, False)},
            "yaux": {"yaux": (n, 1, False), "q": (1, 1, False)},
            "grad": {"sums": (4, 1, False), "parts": (nb4, 4, False)}, "mm_terms": {"sums": (6, 1, False)},
            "coldot": {"out": (n, 1, False)},
            "pred_corr": {"Maux": (c.get("np", 1), m, True), "corr": (max(len(c.get("pairs", ())), 1), 1, False)},
            "ff_diag_grad": {"dd": (n, 1, False)}, "ff_recip": {"y": (n, 1, False)},
            "ff_rowscale": {"Y": (m, n, False)}, "ff_dot": {"sum": (1, 1, False)}}[op]


def vector_raw(c, pad_fill=np.nan, **over):
    """GPB_TestFitcVector on a case (over: replaced entries, e.g. n, m, d, arrays, ints, out_lens); returns (return
    code, outputs name -> array without padding, paddings name -> array, guard)"""
    q = dict(c, **over)
    Dp = ctypes.POINTER(ctypes.c_double)
    arrays = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in q["arrays"]]
    arrs = (Dp * max(len(arrays), 1))(*[_dp(a) for a in arrays])
    ln = np.array([0 if a is None else a.size for a in arrays], dtype=np.int64)
    ints = None if q["ints"] is None else np.asarray(q["ints"], dtype=np.int32)
    shapes = out_shapes(c)
    ldm = ldm_of(c["m"])
    lens = [r * (ldm if p else cc) for r, cc, p in shapes.values()]
    lens = q.get("out_lens", lens)
    outs = [np.full(max(v, 1), SENTINEL) for v in lens]
    op_ = (Dp * len(outs))(*[_dp(o) for o in outs])
    ol = np.array(lens, dtype=np.int64)
    g = ctypes.c_int(-1)
    ret = _lib().GPB_TestFitcVector(VEC_OPS[q["op"]], q["n"], q["m"], q["d"], q["cov"], q["var"], q["phi"], q["extra"],
                                    pad_fill, arrs, _ip(ln, ctypes.c_int64), len(arrays), _ip(ints),
                                    0 if ints is None else ints.size, op_, _ip(ol, ctypes.c_int64), len(outs),
                                    ctypes.byref(g))
    res, pads = {}, {}
    if "out_lens" not in q:
        for (name, (r, cc, p)), o in zip(shapes.items(), outs):
            if p:
                o = o.reshape(r, ldm)
                res[name], pads[name] = o[:, :cc].copy(), o[:, cc:].copy()
            else:
                res[name] = o.reshape(r, cc)[:, 0].copy() if cc == 1 else o.reshape(r, cc).copy()
    return ret, res, pads, g.value, outs


def vector_hook(c, pad_fill=np.nan, **over):
    ret, res, pads, g, _ = vector_raw(c, pad_fill=pad_fill, **over)
    _check(ret)
    assert g == 0, f"{c['op']}: a guard word changed"
    return res, pads


KM_OPS = {"assign": 0, "means": 1, "cmp": 2, "lloyd": 3}
INT_SENTINEL = -77


def kmeans_raw(op, X, mu, mu_a=None, mu_b=None, cluster=None, scan=0, max_it=1000, n=None, k=None, d=None,
               ints_len=None):
    mu = np.ascontiguousarray(mu, dtype=np.float64)
    k_, d_ = mu.shape
    n_ = X.shape[0] if X is not None else k_
    n, k, d = n_ if n is None else n, k_ if k is None else k, d_ if d is None else d
    nbk = (n + 255) // 256
    want = {0: n, 1: 0 if scan else 2 * nbk * k + 2 * k + 1 + n, 2: 2, 3: 0}[KM_OPS[op]]
    want = max(want, 0) if ints_len is None else ints_len
    ints = np.full(max(want, 1), INT_SENTINEL, dtype=np.int32)
    mu_out = np.full(mu.shape, SENTINEL)
    its, g = ctypes.c_int(-1), ctypes.c_int(-1)
    Xc = None if X is None else np.ascontiguousarray(X, dtype=np.float64)
    cl = None if cluster is None else np.ascontiguousarray(cluster, dtype=np.int32)
    ret = _lib().GPB_TestFitcKmeans(KM_OPS[op], n, k, d, _dp(Xc), 0 if Xc is None else Xc.size, _dp(mu), _dp(mu_a),
                                    _dp(mu_b), mu.size, _ip(cl), 0 if cl is None else cl.size, scan, max_it,
                                    _dp(mu_out), _ip(ints), want, ctypes.byref(its), ctypes.byref(g))
    return ret, mu_out, ints[:want], its.value, g.value


def kmeans_hook(op, *a, **kw):
    ret, mu_out, ints, its, g = kmeans_raw(op, *a, **kw)
    _check(ret)
    assert g == 0, f"{op}: a guard word changed"
    return mu_out, ints, its


def split_partition(ints, n, k):
    nbk = (n + 255) // 256
    e = np.cumsum([nbk * k, nbk * k, k, k + 1, n])
    return (ints[:e[0]].reshape(nbk, k), ints[e[0]:e[1]].reshape(nbk, k), ints[e[1]:e[2]], ints[e[2]:e[3]],
            ints[e[3]:e[4]])


# ------------------------------------------------------------------------------------------------ stages
STAGE_CASES = {"n37-m5-d1-exponential": (37, 5, 1, 0), "n130-m65-d3-matern15": (130, 65, 3, 1),
               "n300-m70-d2-gaussian": (300, 70, 2, 3), "n4100-m130-d2-matern25": (4100, 130, 2, 2)}
STAGES = {"factor": 0, "eval": 1, "gram_eval": 2, "gram_other_eval": 3, "predict": 4}
STAGE_OUTS = ("Kmn", "Kmm", "Ks", "dKmm", "Li", "LiT", "Kinv", "V", "d", "Kd", "W", "Wi", "WiT", "Dy", "u", "w", "yaux",
              "A", "a", "Winv", "sums", "mean", "var", "cov")
STAGE_NM = ("Kmn", "V", "Kd", "A")                      # n x m (device: m x n, ld ldm)
STAGE_MM = ("Kmm", "Ks", "dKmm", "Li", "LiT", "Kinv", "W", "Wi", "WiT", "Winv")
STAGE_LOWER = ("Li", "W", "Wi")                         # factors: the device's lower triangle alone is defined
FACTOR_OUTS = STAGE_OUTS[:17]
STAGE_VAR = 1.3
NP_PRED = 12


@functools.lru_cache(maxsize=None)
def stage_inputs(name):
    """X, Z (a well-separated subset of X: farthest-point selection), y and the parameters; the range is half the
    smallest distance between inducing points, so that K_mm,s and the Woodbury matrix stay well conditioned"""
    n, m, d, cov = STAGE_CASES[name]
    g = np.random.default_rng(300 + n)
    X = g.uniform(size=(n, d))
    idx = [0]
    dmin = ((X - X[0]) ** 2).sum(1)
    for _ in range(m - 1):
        idx.append(int(np.argmax(dmin)))
        dmin = np.minimum(dmin, ((X - X[idx[-1]]) ** 2).sum(1))
    Z = X[idx].copy()
    dz = dist(Z, Z) + 10. * np.eye(m)
    rng = 0.5 * dz.min()
    y = g.standard_normal(n)
    # prediction points: some training points (so that the pairs exist), several of them twice, in no order
    tr = [30, 4, 30, 17, 4, 30]
    Xp = np.concatenate([X[tr], g.uniform(size=(NP_PRED - len(tr), d))])
    match = np.array(tr + [-1] * (NP_PRED - len(tr)), dtype=np.int32)
    return dict(n=n, m=m, d=d, cov=cov, X=X, Z=Z, y=y, var=STAGE_VAR, phi=phi_of(cov, rng), Xp=Xp, match=match,
                var2=STAGE_VAR * 1.25, phi2=phi_of(cov, rng * 1.1))


def _tri_inv(L, T):
    """L^-1 of a lower triangular L by forward substitution (longdouble), or LAPACK's (float64)"""
    if T is not LD:
        from scipy.linalg import solve_triangular
        return solve_triangular(L, np.eye(L.shape[0]), lower=True)
    m = L.shape[0]
    Li = np.zeros((m, m), dtype=LD)
    for i in range(m):
        r = -(L[i, :i] @ Li[:i])
        r[i] = 1
        Li[i] = r / L[i, i]
    return Li


def stage_compute(name, T):
    """every buffer of an evaluation with gradient and of a prediction in the dtype T, in the hook's layout (n x m;
    m x m arrays as host[k, j] = the device's (j, k), which matters for the triangular ones), restating fitc.h"""
    q = stage_inputs(name)
    X, Z, y = q["X"].astype(T), q["Z"].astype(T), q["y"].astype(T)
    n, m, cov = q["n"], q["m"], q["cov"]
    var, jit = T(q["var"]), T(JIT)
    c = dict(var=q["var"], phi=q["phi"], cov=cov)
    K, dKn, _ = _cov(q["X"], q["Z"], c, T)
    Kmm, dK, _ = _cov(q["Z"], q["Z"], c, T)
    Kmm[np.diag_indices(m)] = var
    dK[np.diag_indices(m)] = 0
    Ks = Kmm.copy()
    Ks[np.diag_indices(m)] = var * jit
    chol = longdouble_cholesky if T is LD else np.linalg.cholesky
    L = chol(Ks)
    Li = _tri_inv(L, T)
    V = K @ Li.T
    Kinv = Li.T @ Li
    dv = (1 + var * jit) - (V * V).sum(1)
    Kd = K / dv[:, None]
    W = K.T @ Kd + Ks
    Lw = chol(W)
    Wi = _tri_inv(Lw, T)
    Dy = y / dv
    u = K.T @ Dy
    w = Wi.T @ (Wi @ u)
    yaux = Dy - (K @ w) / dv
    o = dict(Kmn=K, Kmm=Kmm, Ks=Ks, dKmm=dK, Li=Li.T, LiT=Li, Kinv=Kinv, V=V, d=dv, Kd=Kd, W=Lw.T, Wi=Wi.T, WiT=Wi, Dy=Dy,
             u=u, w=w, yaux=yaux)
    logdet = -2 * np.log(np.diag(L)).sum() + 2 * np.log(np.diag(Lw)).sum() + np.log(dv).sum()
    # gradient: A = K_mm,s^-1 K_mn, G^T = W^-1 K_mn (left in K_d's buffer), M = dK_mm A (left in V's), a = A y_aux
    A = V @ Li
    Winv = Wi.T @ Wi
    Gt = K @ Winv
    M = A @ dK
    a = A.T @ yaux
    delta = var * jit - var
    inv = 1 / dv
    c1v, sa2, f = (A * K).sum(1), (A * A).sum(1), (Gt * K).sum(1)
    ddv = var - 2 * c1v + (c1v - delta * sa2)
    ddr = -2 * (A * dKn).sum(1) + (A * M).sum(1)
    s2v = ddv * inv + 2 * f * inv - ddv * f * inv * inv
    s2r = ddr * inv + 2 * (Gt * dKn).sum(1) * inv - ddr * f * inv * inv
    s1v = -yaux * (K @ a) - ddv * yaux * yaux / 2
    s1r = -yaux * (dKn @ a) - ddr * yaux * yaux / 2
    sums = np.array([logdet, y @ yaux, s1v.sum() + (a @ Kmm @ a) / 2, s1r.sum() + (a @ dK @ a) / 2,
                     s2v.sum() - (Kinv * Kmm).sum() + (Winv * Kmm).sum(),
                     s2r.sum() - (Kinv * dK).sum() + (Winv * dK).sum()], dtype=T)
    o.update(A=A, a=a, Winv=Winv, Gt=Gt, M=M, sums=sums)
    # prediction (transformed scale, latent: no nugget): mean, and the covariance through the dense correction
    Kp, _, _ = _cov(q["Xp"], q["Z"], c, T)
    npred = Kp.shape[0]
    mean = Kp @ w
    P = Kp @ Kinv
    C = np.zeros((npred, q["n"]), dtype=T)              # corr as a dense np x n matrix
    for i, oj in enumerate(q["match"]):
        if oj >= 0:
            C[i, oj] = var - P[i] @ K[oj]
    mean = mean + C @ yaux
    Maux = Kp - (C / dv[None, :]) @ K
    Um = Maux @ Wi.T
    resid = var - ((Kp @ Li.T) ** 2).sum(1)
    covp = Um @ Um.T + np.diag(resid) - (C / dv[None, :]) @ C.T
    o.update(mean=mean, var=np.diag(covp).copy(), cov=covp)
    return o


@functools.lru_cache(maxsize=None)
def stage_reference(name):
    """(longdouble reference, allowance per array, stand-in error per array): the float64 numpy stand-in that follows
    the same algebra is measured against the reference; a kernel chain may err 8 times that (max norm per array): a
    different summation order and the inverse by TRTRI against LAPACK's solve"""
    ref, std = stage_compute(name, LD), stage_compute(name, np.float64)
    err = {k: float(np.max(af(std[k].astype(LD) - ref[k]))) for k in ref}
    return ref, {k: 8. * v for k, v in err.items()}, err


def stage_conditions(name):
    """cond_2(K_mm,s), cond_2(W)"""
    ref = stage_compute(name, np.float64)
    Lw = ref["W"].T
    return float(np.linalg.cond(ref["Ks"])), float(np.linalg.cond(Lw @ Lw.T))


def stage_raw(name, stage, want, **over):
    """GPB_TestFitcStages; returns (return code, name -> array without padding)"""
    q = dict(stage_inputs(name), **over)
    n, m, d = q["n"], q["m"], q["d"]
    ldm = ldm_of(m)
    pred = stage == "predict"
    npred = q["Xp"].shape[0] if pred else 0
    Dp = ctypes.POINTER(ctypes.c_double)
    bufs = []
    for k in STAGE_OUTS:
        if k not in want:
            bufs.append(None)
            continue
        ln = {"sums": 6, "mean": npred, "var": npred, "cov": npred * npred}.get(k)
        if ln is None:
            ln = n * ldm if k in STAGE_NM else m * ldm if k in STAGE_MM else n if k in ("d", "Dy", "yaux") else m
        bufs.append(np.full(ln, SENTINEL))
    outs = (Dp * len(bufs))(*[_dp(b) for b in bufs])
    lens = np.array([0 if b is None else b.size for b in bufs], dtype=np.int64)
    X, Z, y, Xp = (np.ascontiguousarray(q[k], dtype=np.float64) for k in ("X", "Z", "y", "Xp"))
    match = np.ascontiguousarray(q["match"], dtype=np.int32)
    lib = _lib()
    I, F = ctypes.c_int, ctypes.c_double
    lib.GPB_TestFitcStages.argtypes = [I, I, I, I, I, F, F, F, F, Dp, Dp, Dp, I, Dp, ctypes.POINTER(ctypes.c_int32),
                                       ctypes.POINTER(Dp), ctypes.POINTER(ctypes.c_int64), I]
    ret = lib.GPB_TestFitcStages(STAGES[stage], n, m, d, q["cov"], q["var"], q["phi"], q["var2"], q["phi2"], _dp(X),
                                 _dp(Z), _dp(y), npred, _dp(Xp) if pred else None, _ip(match) if pred else None, outs,
                                 _ip(lens, ctypes.c_int64), len(bufs))
    res = {}
    for k, b in zip(STAGE_OUTS, bufs):
        if b is None:
            continue
        if k in STAGE_NM:
            res[k] = b.reshape(n, ldm)[:, :m].copy()
        elif k in STAGE_MM:
            res[k] = b.reshape(m, ldm)[:, :m].copy()
        elif k == "cov":
            res[k] = b.reshape(npred, npred).T.copy()
        else:
            res[k] = b
    return ret, res


def stage_hook(name, stage, want, **over):
    ret, res = stage_raw(name, stage, want, **over)
    _check(ret)
    return res


def defined(k, a):
    """the entries of a stage array that are defined: the device's lower triangle of a factor (the host layout's upper)"""
    return np.triu(a) if k in STAGE_LOWER else a
