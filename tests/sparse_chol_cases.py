"""Cases, generators, references and error bounds of the sparse multifrontal Cholesky tests, shared by
tests/test_gpu_sparse_chol.py (the HIP kernels through the GPB_TestSparseChol* hooks) and
tests/test_sparse_chol_reference.py (CPU: plan invariants through the host-only plan hook, and a float64
numpy / scipy stand-in of every operation meets the very bounds the kernels are held to).

The matrix is A = B^T D^-1 B + diag(W) of a Vecchia factor: row i of B holds 1 on the diagonal and Bv[i][r] at
column nbr[i][r]. Graphs are built here in numpy (brute-force nearest earlier points, stable sort; banded for
case g), the values are the workload's own kind (exponential covariance, variance 1, range 0.15, 1 + 1e-10 jitter).

References are numpy.longdouble (64-bit significand here, checked by the CPU tests) in the device's own
elimination order (perm from the plan hook): A_p = P A P^T summed in longdouble from the float64 inputs, its
Cholesky factor L column by column, L^-1 by forward substitution, A^-1 = L^-T L^-1. For a fixed order the factor
is unique, so the device's L and L^-1 P b are compared with them directly.

Bounds, first order in u = 2^-53 with gamma_k = k u / (1 - k u); none of them tuned to what a kernel gives. Let
E = |L||L|^T + P |B|^T D^-1 |B| P^T (the second term: the rounding of the clique sums that form A).
  factor    |A_p - L^ L^^T| <= 4 gamma_{n+1} E^ on the lower triangle, E^ = E with the computed |L^| in place of |L|,
            as the theorem states it (Higham, Accuracy and Stability, Theorem 10.3,
            with the constant of dense_ops_cases.chol_ratios: a Newton-refined reciprocal square root within an
            ulp at most doubles a term, the other 2 is margin at n = 1, 2); L^ exactly 0 outside the structure
  forward   |y^ - L^-1 b| <= gamma_{n+1} |L^-1| (|L||y^| + E |L^-T y^|). Derivation: forward substitution gives
            (L^ + dT) y^ = b with |dT| <= gamma_n |L^| (Theorem 8.5), and L^ = L + dL with
            dL L^T + L dL^T = dA, |dA| <= gamma_{n+1} E, whose leading part is dL ~ dA L^-T. So
            y^ - y = -L^-1 (dT + dL) y^ and |dL y^| <~ gamma_{n+1} E |L^-T y^|.
  solve     |x^ - A^-1 b| <= gamma_{3n+1} |A^-1| E |x^| (Theorem 10.4: (A + dA) x^ = b, |dA| <= gamma_{3n+1}
            |L^||L^^T|, plus the clique sums), for Solve, SolveMulti and BackwardCols(ForwardCols(b))
  inverse   |S^ - A^-1| <= gamma_{3n+1} |A^-1| E |A^-1| on the pattern and for diagS (each column of the inverse
            is a solve with a unit vector)
  logdet    |ld^ - 2 sum log L_ii| <= gamma_{n+1} sum_ij |A^-1|_ij E_ij + 2 n u (1 + max |log L_ii|)
            (d logdet = tr(A^-1 dA), plus the rounding of the n logarithms and their sum)
  traces    |tr^ - sum S_ij M_ij| <= sum dS_ij |M_ij| + gamma_N sum |S_ij M_ij| with dS the inverse's bound and N
            the number of terms (A's lower pattern; off-diagonal entries count twice, as chol_trace_kernel does)
These are first-order models, not theorems about the Takahashi recursion; float64 LAPACK stays under them (ratios
up to 0.26 at n <= 3, where a bound is a few u, and below 0.03 from n = 63 on;
tests/test_sparse_chol_reference.py prints them).
"""
import ctypes
import functools

import numpy as np

from gpboost_amd import synthetic

U = 2.0 ** -53
LD = np.longdouble
RANGE = 0.15
JITTER = 1.0 + 1e-10
RHS_COUNTS = (1, 3, 4, 5, 64, 65)

# CholOpType (gpboost_amd/csrc/sparse_chol.h)
OPS = ("AsmTile", "AsmEntries", "Reduce", "Diag", "Gemm", "GatherS", "Mirror", "AsmV", "GatherX", "ScatterX",
       "FSolve1", "BSolve1", "LoadV", "FwdVec", "CopyXS", "BwdVecPart", "BwdVecFin")
NSTATS = 6 + 3 * (len(OPS) + 2)
OPT_KEYS = ("leaf", "small_panel", "fuse_vec", "k64", "poison")


def gamma(k):
    return k * U / (1.0 - k * U)


def max_ratio(err, bound):
    """largest err / bound over the entries (0 / 0 counts as 0, err > 0 = bound as inf, NaN as inf)"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0., 0., err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(np.max(r))


# ------------------------------------------------------------------------------------------------ graphs
def knn_graph(X, m):
    """nbr[i] = the min(i, m) nearest earlier points of i (brute force, stable sort), -1 beyond"""
    n = X.shape[0]
    nbr = np.full((n, m), -1, dtype=np.int32)
    for i in range(1, n):
        d2 = ((X[:i] - X[i]) ** 2).sum(axis=1)
        k = min(i, m)
        nbr[i, :k] = np.argsort(d2, kind="stable")[:k]
    return nbr


def banded_graph(n, m):
    nbr = np.full((n, m), -1, dtype=np.int32)
    for i in range(1, n):
        k = min(i, m)
        nbr[i, :k] = i - 1 - np.arange(k)
    return nbr


# name: (n, m, graph kind): the smallest shapes at which each path can go wrong;
# tests/test_sparse_chol_reference.py::test_case_reaches_its_path asserts the plan statistics that prove each path.
# h: on bench_coords (1500, 30) has at most 445 rows below a block (one split-K slice); (1000, 50) is the smallest
# of the shapes tried (n in steps of 100, m in steps of 10) with more than 512: 518 rows, so a second slice of K = 6.
CASES = {
    "a1": (1, 1, "knn"), "a2": (2, 1, "knn"), "a3": (3, 5, "knn"),
    "b63": (63, 62, "knn"), "b64": (64, 63, "knn"), "b65": (65, 64, "knn"), "b128": (128, 127, "knn"),
    "b130": (130, 129, "knn"), "b192": (192, 191, "knn"), "b254": (254, 253, "knn"),
    "c": (260, 254, "knn"),
    "d": (400, 1, "knn"),
    "e1": (400, 10, "holes7"),      # every seventh row without neighbours: several roots
    "e2": (400, 10, "holes2"),      # every other neighbour slot -1
    "f": (700, 20, "knn"),
    "g": (900, 254, "banded"),
    "h": (1000, 50, "knn"),
}
# option sets per case (the default first)
CASE_OPTIONS = {
    "c": ({}, {"fuse_vec": 0}, {"small_panel": 1 << 20}),
    "f": ({"leaf": 64}, {"leaf": 8}, {"leaf": 64, "small_panel": 0}),
}
W_KINDS = ("bern", "pois", "none")


def case_options(name):
    return CASE_OPTIONS.get(name, ({},))


def opt_id(opt):
    return "-".join(f"{k}{v}" for k, v in sorted(opt.items())) or "default"


@functools.lru_cache(maxsize=None)
def graph(name):
    """(X, nbr): coordinates n x d and the neighbour table n x m (int32), read-only"""
    n, m, kind = CASES[name]
    if kind == "banded":
        # 1-D, increasing: x_i = (i + u_i / 2) / n, so the band is also the set of nearest earlier points
        X = ((np.arange(n) + 0.5 * synthetic.lcg_unif(n, 0.29)) / n).reshape(n, 1)
        nbr = banded_graph(n, m)
    else:
        X = synthetic.bench_coords(n)
        nbr = knn_graph(X, m)
        if kind == "holes7":
            nbr[::7] = -1
        elif kind == "holes2":
            nbr[:, 1::2] = -1
    X.setflags(write=False)
    nbr.setflags(write=False)
    return X, nbr


def _neighbours(nbr, i):
    m = nbr.shape[1]
    slots = np.flatnonzero(nbr[i, :min(i, m)] >= 0)
    return slots, nbr[i, slots]


@functools.lru_cache(maxsize=None)
def values(name):
    """Bv, Dinv, dBv, dD (float64, read-only): the Vecchia factor of the exponential covariance on the case's graph
    and its derivative with respect to the log range"""
    X, nbr = graph(name)
    n, m = nbr.shape
    Bv, dBv = np.zeros((n, m)), np.zeros((n, m))
    D, dD = np.full(n, JITTER), np.zeros(n)
    for i in range(1, n):
        slots, N = _neighbours(nbr, i)
        if N.size == 0:
            continue
        P = np.vstack([X[N], X[i:i + 1]])
        dist = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2))
        K = np.exp(-dist / RANGE)
        dK = K * dist / RANGE                       # d K / d log(range)
        KN = K[:-1, :-1] + (JITTER - 1.) * np.eye(N.size)
        k, dk = K[:-1, -1], dK[:-1, -1]
        a = np.linalg.solve(KN, k)
        da = np.linalg.solve(KN, dk - dK[:-1, :-1] @ a)
        Bv[i, slots], dBv[i, slots] = -a, -da
        D[i] = JITTER - k @ a
        dD[i] = -(dk @ a) - k @ da
    out = (Bv, 1. / D, dBv, dD)
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def w_vector(name, kind):
    n = CASES[name][0]
    if kind == "none":
        return None
    u = synthetic.lcg_unif(n, 0.43)
    w = 0.05 + 0.2 * u if kind == "bern" else np.exp(-7. + 12. * u)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def rhs(name, t):
    """n x t right-hand sides in [-0.5, 0.5), column-major flat (the hooks' layout), read-only"""
    n = CASES[name][0]
    b = synthetic.lcg_unif(n * t, 0.53) - 0.5
    b.setflags(write=False)
    return b


# ------------------------------------------------------------------------------------------------ dense forms
def _clique_sum(name, dtype, absolute=False, deriv=False):
    """sum over the rows r of D^-1_r b_r b_r^T (or of its absolute values, or of its derivative) in dtype"""
    _, nbr = graph(name)
    Bv, Dinv, dBv, dD = values(name)
    n = nbr.shape[0]
    A = np.zeros((n, n), dtype=dtype)
    for r in range(n):
        slots, N = _neighbours(nbr, r)
        idx = np.concatenate([[r], N])
        b = np.concatenate([[1.], Bv[r, slots]]).astype(dtype)
        di = dtype(Dinv[r])
        if deriv:
            db = np.concatenate([[0.], dBv[r, slots]]).astype(dtype)
            blk = di * (np.outer(db, b) + np.outer(b, db)) - di * di * dtype(dD[r]) * np.outer(b, b)
        elif absolute:
            blk = di * np.outer(np.abs(b), np.abs(b))
        else:
            blk = di * np.outer(b, b)
        A[np.ix_(idx, idx)] += blk
    return A


@functools.lru_cache(maxsize=None)
def pattern(name):
    """boolean n x n: the structural non-zeros of A (union of the cliques), matrix labels"""
    _, nbr = graph(name)
    n = nbr.shape[0]
    S = np.zeros((n, n), dtype=bool)
    for r in range(n):
        idx = np.concatenate([[r], _neighbours(nbr, r)[1]])
        S[np.ix_(idx, idx)] = True
    return S


def longdouble_lower_inverse(L):
    """L^-1 by forward substitution in longdouble, row by row"""
    n = L.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        r = np.zeros(i + 1, dtype=LD)
        if i:
            r[:i] = -np.dot(L[i, :i], X[:i, :i])
        r[i] += 1
        X[i, :i + 1] = r / L[i, i]
    return X


def longdouble_cholesky(A):
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - np.dot(L[j, :j], L[j, :j]))
        L[j + 1:, j] = (A[j + 1:, j] - np.dot(L[j + 1:, :j], L[j, :j])) / L[j, j]
    return L


@functools.lru_cache(maxsize=None)
def clique_sums(name):
    """(A0, |B|^T D^-1 |B|, dA) in matrix labels: longdouble, float64, longdouble"""
    return _clique_sum(name, LD), _clique_sum(name, np.float64, absolute=True), _clique_sum(name, LD, deriv=True)


class Reference:
    """The longdouble reference of one (case, W kind, elimination order)"""

    def __init__(self, name, wkind, perm):
        self.name, self.perm = name, np.asarray(perm)
        n = self.n = CASES[name][0]
        p = self.perm
        A0, absA0, dA = clique_sums(name)
        self.A0 = A0[np.ix_(p, p)]
        self.dA = dA[np.ix_(p, p)]
        self.pattern = pattern(name)[np.ix_(p, p)]
        w = w_vector(name, wkind)
        self.A = self.A0.copy()
        if w is not None:
            self.A[np.arange(n), np.arange(n)] += w[p].astype(LD)
        self.L = longdouble_cholesky(self.A)
        self.Linv = longdouble_lower_inverse(self.L)
        self.Ainv = np.dot(self.Linv.T, self.Linv)
        absL = np.abs(self.L.astype(np.float64))
        self.absL = absL
        self.absA0 = absA0[np.ix_(p, p)]
        self.E = absL @ absL.T + self.absA0
        self.absLinv = np.abs(self.Linv.astype(np.float64))
        self.absAinv = np.abs(self.Ainv.astype(np.float64))
        self.dS = gamma(3 * n + 1) * (self.absAinv @ self.E @ self.absAinv)      # the inverse's bound
        self.logs = np.log(np.diag(self.L))
        self.logdet = 2 * self.logs.sum()

    def cond_inf(self):
        return float(np.abs(self.A.astype(np.float64)).sum(axis=1).max() * self.absAinv.sum(axis=1).max())

    # ---- error / bound ratios of computed float64 results (all in elimination positions)
    def factor_ratio(self, Lc):
        low = np.tril(np.ones((self.n, self.n), dtype=bool))
        Ll = Lc.astype(LD)
        res = np.abs(self.A - np.dot(Ll, Ll.T))
        # the theorem's own form: the computed factor on the bound side (as dense_ops_cases.chol_ratios). Where an
        # entry of L is a sum that cancels to ~1e-25 (products of B entries near 1e-13), the computed entry is
        # relatively far from the exact one, and a bound built from the exact |L| there is missed by float64 LAPACK too
        E = np.abs(Lc) @ np.abs(Lc).T + self.absA0
        return max_ratio(res[low], (4. * gamma(self.n + 1) * E)[low])

    def forward_ratio(self, Y, b):
        """Y, b: n x t, Y = computed L^-1 P b in elimination positions, b in matrix labels"""
        ref = np.dot(self.Linv, b[self.perm].astype(LD))
        z = np.abs(np.asarray(np.dot(self.Linv.T, Y.astype(LD)), dtype=np.float64))          # |L^-T y^|
        bound = gamma(self.n + 1) * (self.absLinv @ (self.absL @ np.abs(Y) + self.E @ z))
        return max_ratio(np.abs(Y.astype(LD) - ref), bound)

    def solve_ratio(self, Xc, b):
        """Xc, b: n x t in matrix labels"""
        p = self.perm
        ref = np.dot(self.Ainv, b[p].astype(LD))
        bound = gamma(3 * self.n + 1) * (self.absAinv @ (self.E @ np.abs(Xc[p])))
        return max_ratio(np.abs(Xc[p].astype(LD) - ref), bound)

    def inverse_ratio(self, S, mask):
        """S: n x n float64 in elimination positions, compared where mask is True"""
        return max_ratio(np.abs(S.astype(LD) - self.Ainv)[mask], self.dS[mask])

    def diag_ratio(self, diagS):
        """diagS: n in matrix labels"""
        d = diagS[self.perm]
        return max_ratio(np.abs(d.astype(LD) - np.diag(self.Ainv)), np.diag(self.dS))

    def logdet_ratio(self, logdet):
        bound = gamma(self.n + 1) * float((self.absAinv * self.E).sum()) + \
            2. * self.n * U * (1. + float(np.max(np.abs(self.logs))))
        return float(abs(LD(logdet) - self.logdet)) / bound

    def trace_ratio(self, tr, deriv):
        M = self.dA if deriv else self.A0
        ref = (M * self.Ainv)[self.pattern].sum()
        absM = np.abs(M.astype(np.float64))
        nterms = int(np.tril(self.pattern).sum())
        bound = float((self.dS * absM)[self.pattern].sum()) + gamma(nterms) * float((self.absAinv * absM)[self.pattern].sum())
        return max_ratio(float(abs(LD(tr) - ref)), bound)       # n = 1: dA = 0, so 0 / 0 = 0


@functools.lru_cache(maxsize=3)
def _reference(name, wkind, perm_bytes):
    return Reference(name, wkind, np.frombuffer(perm_bytes, dtype=np.int32))


def reference(name, wkind, opt=None):
    """The reference of the case in the elimination order its plan gives under opt; the last three are kept (tests
    that share one run next to each other), and none is ever written to."""
    return _reference(name, wkind, plan_of(name, opt)["perm"].tobytes())


# ------------------------------------------------------------------------------------------------ plan
def structure(plan):
    """boolean n x n: the lower structure of L in elimination positions (the supernodes' dense panels)"""
    n = plan["n"]
    S = np.zeros((n, n), dtype=bool)
    for s in range(plan["nsup"]):
        f, l = plan["sfirst"][s], plan["sfirst"][s + 1]
        R = plan["rows"][plan["rptr"][s]:plan["rptr"][s + 1]]
        for j in range(f, l):
            S[j:l, j] = True
            S[R, j] = True
    return S


def sup_stats(plan):
    """per supernode: ns, nr, fs"""
    ns = np.diff(plan["sfirst"])
    nr = np.diff(plan["rptr"])
    return ns, nr, ns + nr


def fr_max(plan):
    """largest number of front rows below a 64-column block"""
    ns, _, fs = sup_stats(plan)
    out = 0
    for a, f in zip(ns, fs):
        for k in range((a + 63) // 64):
            out = max(out, int(f - min(64 * (k + 1), a)))
    return out


# ------------------------------------------------------------------------------ results and their ratios
def float64_results(name, wkind, plan, ts):
    """Every operation in plain float64 numpy / scipy (LAPACK) in the plan's elimination order, in the layouts the
    hooks return: L, S (NaN outside the structure), diagS, logdet, the traces, and per t in ts the forward,
    full and backward-of-forward solves (n x t, matrix labels; the forward result at label perm[k])."""
    import scipy.linalg as sl
    p = plan["perm"]
    n = plan["n"]
    A0 = _clique_sum(name, np.float64)[np.ix_(p, p)]
    dA = _clique_sum(name, np.float64, deriv=True)[np.ix_(p, p)]
    A = A0.copy()
    w = w_vector(name, wkind)
    if w is not None:
        A[np.arange(n), np.arange(n)] += w[p]
    L = np.linalg.cholesky(A)
    Linv = sl.solve_triangular(L, np.eye(n), lower=True)
    Sfull = Linv.T @ Linv
    struct = structure(plan)
    low = np.tril(pattern(name)[np.ix_(p, p)])
    wgt = np.where(np.eye(n, dtype=bool), 1., 2.)
    res = dict(L=L, S=np.where(struct, Sfull, np.nan), logdet=float(2. * np.log(np.diag(L)).sum()),
               tr_bdb=float((wgt * A0 * Sfull)[low].sum()), tr_da=float((wgt * dA * Sfull)[low].sum()),
               fwd={}, solve={}, bwd={})
    res["diagS"] = np.empty(n)
    res["diagS"][p] = np.diag(Sfull)
    for t in ts:
        b = rhs(name, t).reshape(t, n).T
        y = sl.solve_triangular(L, b[p], lower=True)
        x = sl.solve_triangular(L.T, y, lower=False)
        out = np.empty((n, t))
        out[p] = y
        res["fwd"][t] = out
        out = np.empty((n, t))
        out[p] = x
        res["bwd"][t] = out
        out = np.empty((n, t))
        out[p] = sl.cho_solve((L, True), b[p])
        res["solve"][t] = out
    return res


def result_ratios(ref, plan, res):
    """error / bound ratio of every quantity present in res (the layout of float64_results); also asserts the
    structural facts: L exactly zero outside the structure and finite inside"""
    struct = structure(plan)
    p, n = plan["perm"], plan["n"]
    out = {}
    if "L" in res:
        assert not np.any(res["L"][~struct]), "L is not exactly zero outside its structure"
        assert np.all(np.isfinite(res["L"]))
        out["factor"] = ref.factor_ratio(res["L"])
    if "S" in res:
        assert np.all(np.isnan(res["S"][~struct])) and np.all(np.isfinite(res["S"][struct]))
        out["inverse"] = ref.inverse_ratio(res["S"], struct)
    if "diagS" in res:
        out["diagS"] = ref.diag_ratio(res["diagS"])
    if "logdet" in res:
        out["logdet"] = ref.logdet_ratio(res["logdet"])
    if "tr_bdb" in res:
        out["tr_bdb"] = ref.trace_ratio(res["tr_bdb"], False)
    if res.get("tr_da") is not None:
        out["tr_da"] = ref.trace_ratio(res["tr_da"], True)
    for t, Y in res.get("fwd", {}).items():
        b = rhs(ref.name, t).reshape(t, n).T
        out[f"fwd{t}"] = ref.forward_ratio(Y[p], b)
    for key in ("solve", "bwd"):
        for t, X in res.get(key, {}).items():
            b = rhs(ref.name, t).reshape(t, n).T
            out[f"{key}{t}"] = ref.solve_ratio(X, b)
    return out


def report(label, ratios):
    print(f"{label}: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


# ------------------------------------------------------------------------------------ the library's test hooks
def _lib():
    c = ctypes
    from gpboost_amd import basic
    lib = basic.lib()
    if not getattr(lib, "_sparse_chol_typed", False):
        D, I, L, V = c.POINTER(c.c_double), c.c_int, c.c_int64, c.c_void_p
        PI, PL = c.POINTER(c.c_int32), c.POINTER(c.c_int64)
        lib.GPB_TestSparseCholPlan.argtypes = [I, I, PI, L, I, D, L, PL, I, I, PI, PI, PI, PL, PI, L, PI, PI, PL, L]
        lib.GPB_TestSparseCholCreate.argtypes = [I, I, PI, L, I, D, L, PL, c.POINTER(V)]
        lib.GPB_TestSparseCholFree.argtypes = [V]
        lib.GPB_TestSparseCholSetB.argtypes = [V, D, L, D, L, D, L, D, L]
        lib.GPB_TestSparseCholFactor.argtypes = [V, D, L, c.POINTER(I), D]
        lib.GPB_TestSparseCholSolve.argtypes = [V, I, I, I, D, L, D, L]
        lib.GPB_TestSparseCholSelectedInverse.argtypes = [V, D, D, D, L]
        lib.GPB_TestSparseCholDense.argtypes = [V, I, D, L]
        lib._sparse_chol_typed = True
    return lib


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


def _size(a):
    return 0 if a is None else a.size


def _opts(opt):
    assert set(opt) <= set(OPT_KEYS), opt
    return np.array([opt.get(k, -1) for k in OPT_KEYS], dtype=np.int64)


def last_error():
    return _lib().LGBM_GetLastError().decode("utf-8")


class HookError(RuntimeError):
    pass


def _check(ret):
    if ret != 0:
        msg = last_error()
        if "HIP error" in msg:          # the device context is gone: nothing more may run on it
            import pytest
            pytest.exit(f"HIP error, session ended: {msg}", returncode=3)
        raise HookError(msg)


def hook_plan(X, nbr, opt=None, t=1, mode=0, n=None, m=None, nbr_len=None, x_len=None):
    """GPB_TestSparseCholPlan (no device call). Returns a dict: n, nsup, levels, max_fs, max_ns, nnz_l, perm,
    sfirst, sparent, rptr, rows, lvl_ptr, lvl_sup, and per schedule ('factor', 'selinv', 'solve') a dict of op
    counts by name plus 'nslices' and 'fin_chunks'. n, m and the lengths can be overridden to test the checks."""
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = nbr.shape[0] if n is None else n
    m = nbr.shape[1] if m is None else m
    d = X.shape[1]
    o = _opts(opt or {})
    na = max(n, 1)
    perm, sfirst, sparent = (np.zeros(na + 1, dtype=np.int32) for _ in range(3))
    lvl_ptr, lvl_sup = (np.zeros(na + 1, dtype=np.int32) for _ in range(2))
    rptr = np.zeros(na + 1, dtype=np.int64)
    stats = np.zeros(NSTATS, dtype=np.int64)
    rows = None
    for _ in range(2):          # the first call sizes rows
        _check(_lib().GPB_TestSparseCholPlan(n, m, _ip(nbr), nbr.size if nbr_len is None else nbr_len, d, _dp(X),
                                             X.size if x_len is None else x_len, _ip(o, ctypes.c_int64), t, mode,
                                             _ip(perm), _ip(sfirst), _ip(sparent), _ip(rptr, ctypes.c_int64),
                                             _ip(rows), _size(rows), _ip(lvl_ptr), _ip(lvl_sup),
                                             _ip(stats, ctypes.c_int64), stats.size))
        if rows is not None:
            break
        rows = np.zeros(max(int(stats[5]), 1), dtype=np.int32)
    nsup, nlev = int(stats[0]), int(stats[1])
    out = dict(n=n, nsup=nsup, levels=nlev, max_fs=int(stats[2]), max_ns=int(stats[3]), nnz_l=int(stats[4]),
               perm=perm[:n].copy(), sfirst=sfirst[:nsup + 1].copy(), sparent=sparent[:nsup].copy(),
               rptr=rptr[:nsup + 1].copy(), rows=rows[:int(stats[5])].copy(), lvl_ptr=lvl_ptr[:nlev + 1].copy(),
               lvl_sup=lvl_sup[:nsup].copy())
    for q, key in enumerate(("factor", "selinv", "solve")):
        blk = stats[6 + q * (len(OPS) + 2):6 + (q + 1) * (len(OPS) + 2)]
        sch = {name: int(blk[i]) for i, name in enumerate(OPS)}
        sch["nslices"], sch["fin_chunks"] = int(blk[len(OPS)]), int(blk[len(OPS) + 1])
        out[key] = sch
    return out


@functools.lru_cache(maxsize=None)
def case_plan(name, opt_items=(), t=1, mode=0):
    X, nbr = graph(name)
    return hook_plan(X, nbr, dict(opt_items), t, mode)


def plan_of(name, opt=None, t=1, mode=0):
    return case_plan(name, tuple(sorted((opt or {}).items())), t, mode)


class Chol:
    """A GPB_TestSparseChol* handle of one case (values set, not yet factored)"""
    SOLVE, SOLVE_MULTI, FORWARD, BACKWARD = 0, 1, 2, 3

    def __init__(self, name, opt=None, deriv=True):
        X, nbr = graph(name)
        self.name, self.n, self.m = name, nbr.shape[0], nbr.shape[1]
        self.h = ctypes.c_void_p()
        o = _opts(opt or {})
        _check(_lib().GPB_TestSparseCholCreate(self.n, self.m, _ip(nbr), nbr.size, X.shape[1], _dp(X), X.size,
                                               _ip(o, ctypes.c_int64), ctypes.byref(self.h)))
        Bv, Dinv, dBv, dD = values(name)
        self.set_b(Bv.reshape(-1), Dinv, dBv.reshape(-1) if deriv else None, dD if deriv else None)

    def close(self):
        if self.h:
            _lib().GPB_TestSparseCholFree(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        self.close()

    def set_b(self, Bv, Dinv, dBv, dD):
        _check(_lib().GPB_TestSparseCholSetB(self.h, _dp(Bv), Bv.size, _dp(Dinv), Dinv.size, _dp(dBv), _size(dBv),
                                             _dp(dD), _size(dD)))

    def factor(self, W, want_logdet=True):
        """returns (info, logdet or None)"""
        info = ctypes.c_int(-1)
        ld = np.full(1, np.nan)
        _check(_lib().GPB_TestSparseCholFactor(self.h, _dp(W), _size(W), ctypes.byref(info),
                                               _dp(ld) if want_logdet else None))
        return info.value, (float(ld[0]) if want_logdet else None)

    def solve(self, op, b, t, inplace=0):
        """b: flat n t (column-major); returns x as an n x t array"""
        x = np.full(self.n * t, np.nan)
        _check(_lib().GPB_TestSparseCholSolve(self.h, op, t, inplace, _dp(b), b.size, _dp(x), x.size))
        return x.reshape(t, self.n).T.copy()

    def selected_inverse(self, want=(True, True, True)):
        """returns (tr_bdb, tr_da, diagS), None where not wanted"""
        tr = np.full(2, np.nan)
        diag = np.full(self.n, np.nan) if want[2] else None
        pd = ctypes.POINTER(ctypes.c_double)
        p0 = ctypes.cast(tr.ctypes.data, pd) if want[0] else None
        p1 = ctypes.cast(tr.ctypes.data + 8, pd) if want[1] else None
        _check(_lib().GPB_TestSparseCholSelectedInverse(self.h, p0, p1, _dp(diag), _size(diag)))
        return (float(tr[0]) if want[0] else None, float(tr[1]) if want[1] else None, diag)

    def dense(self, which):
        """0: L, 1: S (lower structure), 2: S's mirrored upper entries at their transposed places; n x n"""
        out = np.full(self.n * self.n, np.nan)
        _check(_lib().GPB_TestSparseCholDense(self.h, which, _dp(out), out.size))
        return out.reshape(self.n, self.n).T.copy()


def bits(a):
    """the bit patterns, for bitwise comparisons that treat NaN as equal to itself"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
