"""Cases, references and error bounds of the grouped random-effects kernel tests, shared by
tests/test_gpu_grouped_ops.py (the launchers of csrc/grouped_kernels.hip, GroupedRE::Precond / SolveVec and the
segmented sums and gradient kernels of csrc/grouped_laplace.hip through the GPB_TestGrouped* hooks) and
tests/test_grouped_ops_reference.py (CPU: every design is valid and reaches the path it is named for, the CSR
restatement equals a dense Z^T Z, float64 numpy stand-ins meet the very bounds the kernels are held to, and
single-entry defects exceed them).

Inputs are float64, references numpy.longdouble (64-bit significand; assert_longdouble() checks that on import of
either test file). structure() restates GroupedRE's constructor in numpy: the off-diagonal part of Z^T Z in CSR
over the M = sum m_k rows (columns ascending, split = the first entry of a higher effect), its diagonal cnt and the
observation lists; chunk_plan() restates GroupedRE::Plan, seg_plan() the destinations of GroupedLaplace.

Bounds. U = 2^-53, gamma_j = j U / (1 - j U); a sum of k terms in ANY order (chunks, LDS trees, shuffles, fma or
not) satisfies |fl(sum) - sum| <= gamma_{k-1} sum |terms| (Higham, Accuracy and Stability, section 4.2), and every
further rounding on a term's way adds 1 to the index. g(j) = gamma_j + the same expression at 2^-64 for the
longdouble reference's own rounding. With k = the entry count of the row (its full, lower or upper range) the
index is k + c, c counted from the formula:
  apply, apply_lower   Y = s + dg X             product, k - 1 sums, the sum with the diagonal term       c = 1
  lds_mult             Y = s + (D dis) R        val dis, its product, k sums (diagonal term: 3 roundings) c = 2
  upper                Y = (1 / D)(D X + s)     product, k sums, 1 / D, the last product                  c = 3
  forward sweep        X = (R - s) / (D dis)    val dis, product, k - 1 sums | difference, D dis, quotient c = 3
  backward sweep       Z = (X - dis s)/(D dis)  product, k - 1 sums, dis s | difference, D dis, quotient  c = 3
  The sweeps are checked twice: the componentwise residual of the device's own X (and of its Z given its X) in
  longdouble, |R_r - s_r - D_r dis_r X_r| <= g(k + 3) (sum |coef_e X_col| + |D_r dis_r X_r|), and the forward
  error against the longdouble substitution, bounded by the same substitution on absolute values (the comparison
  matrix: e_r = (g(k + 3) (sum |coef| |X_col| + |D dis X_r|) + sum |coef| e_col) / |D dis|).
  gre_zty              a list of k observations: g(k) sum |y|; an empty list gives exactly 0
  gre_diag             D = 1 / tau + cnt: g(2) |D|; dis = sqrt(1 / D): g(4) |dis|; sum log D over m rows: the
                       argument's 2 U, the logarithm's UF_ELEM ulp (tests/lik_cases.py, 2^-52 |z| each, 2 UF_ELEM
                       roundings) and m - 1 sums: g(m + 2 UF_ELEM) sum |log D| + g(3) m; sum 1 / D: g(m + 3) sum 1 / D
  gre_single           u = zty / D: g(1) |u|; sum cnt: g(m) sum |cnt|; sum cnt^2 / D: g(m + 2) of the sum
  gre_inv_diag         sum of k = M - i squares: g(k + 1) of the sum
  gre_pred_cols        E_r = the sum of the j <= K columns that reach row r: g(j - 1) sum |Li| (one column: the bits);
                       var = sum_r E_r^2: g(M + 2 K) sum_r (sum |Li|)^2
  gre_fisher_cols      b = Ainv sc_r sc_c squared and summed over the m_k rows: g(m_k + 5) sum b^2; diag: g(2)
  segmented sums       a destination of k observations: g(k) sum |w|
  glp_q                dwq_i = dW_i q_i / 2, q_i a sum of K^2 entries: g(K^2 + 1) |dW_i| sum |Ainv| / 2 (K = 1:
                       1 / D); sum_i W_i q_ij: n K terms, g(n K + 1) of the absolute sum; AUX: g(n K^2 + 1)
  glp_row_trace        (sum_k U)(sum_k V) per column, t columns, / t, dW / 2: g(2 K + t + 2) of the absolute sum
  glp_grad_f           -d1 + dwq - W (sum_k v): g(K + 2) (|d1| + |dwq| + |W| sum |v|)
  glp_effect_dots      m rows: g(m + 1) of the absolute sum; mode 1: g(m + 2 UF_ELEM) sum |log x| (the logarithm's ulp)
  SolveVec             ||rhs - A u|| <= delta + (its + 1) g(k_max + 5) || |A| |u| ||: the recursive residual that
                       stops the iteration (< delta) differs from the true one by the rounding of A h (k_max + 1),
                       a v and the update of r, a h and the update of u (5 roundings past the row sum) in each of
                       the its steps and once in the warm start's rhs - A u
Exact claims (bitwise): gre_dense_build, gre_residual, the five glp_vec forms (one or two correctly rounded
operations; x - s y and x + alpha y are one expression, which C++ lets a compiler contract to one fused
multiply-add, so every entry must carry the bits of the two-rounding result or every entry those of the fused one,
computed exactly in rational arithmetic), equal bits from two runs, a column of a block independent of the others.

Largest error / bound over all cases. Float64 stand-ins (tests/test_grouped_ops_reference.py -s): apply 0.95,
apply_lower 0.99, lds_mult 0.93, upper 0.67, sweeps 0.64 / 0.63 (residual) and 0.64 / 0.63 (forward error), gre_zty
0.48, gre_diag 0.78 / 0.39 / 0.15 (D / dis / sums), gre_single 0.99 / 0.11, gre_inv_diag 0.39, gre_pred_cols 1.00 /
0.07 (E / var), gre_fisher_cols 0.53 / 0.79, segmented sums 0.54, glp_q 0.90 / 0.70 (dwq / sums), glp_row_trace 0.31,
glp_grad_f 0.67, effect dots 0.34 / 0.11 / 0.26 / 0.22. The kernels on an MI355X (tests/test_gpu_grouped_ops.py -s):
apply 0.95, apply_lower 0.99, lds_mult 0.93, upper 0.67, gre_ssor 0.64 / 0.63 and 0.64 / 0.63, gre_zty 0.42, gre_diag
0.78 / 0.39 / 0.14, gre_single 0.99 / 0.38, gre_inv_diag 0.39, gre_pred_cols 1.00 / 0.02, gre_fisher_cols 0.53 /
0.79, glp_seg kernels 0.48, glp_q_kernel 0.90 / 0.70, glp_row_trace_kernel 0.31, glp_grad_f_kernel 0.57, effect dots
0.34 / 0.10 / 0.25 / 0.28, SolveVec's true residual 0.98 of delta + drift. The ratios near 1 belong to results of a
single rounding (one product plus one sum in a row of one entry, one quotient, one sum of two columns), whose
half-ulp error sits just under gamma_1 of the result.
"""
import ctypes
import fractions
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from latent_ops_cases import LD, U, assert_longdouble, max_ratio, HookError, _dp, _ip  # noqa: E402,F401
from lik_cases import UF_ELEM  # noqa: E402

UREF = 2.0 ** -64
K_ENTRIES_PER_LANE, K_SHORT_LEN, K_CHUNK_LEN, K_GLP_MAX_K, K_MAX_BLOCKS = 8, 32, 512, 8, 1024
TS = (1, 2, 3, 5, 9, 17, 33, 50, 64, 65, 100)        # every lane split, the production pair, two column blocks
TS_OTHER = (1, 3, 50, 65)
FULL, LOWER, UPPER = 0, 1, 2
KINDS = ("full", "lower", "upper")


def g(j):
    """gamma_j at U plus gamma_j at the longdouble reference's 2^-64, elementwise"""
    j = np.asarray(j, dtype=np.float64)
    return j * U / (1.0 - j * U) + j * UREF / (1.0 - j * UREF)


def gre_tc(t):
    tc = 1
    while tc < t and tc < 64:
        tc *= 2
    return tc


def chunk_len(tc):
    return (256 // tc) * K_ENTRIES_PER_LANE


def obs_blocks(n):
    return max(1, min((n + 255) // 256, K_MAX_BLOCKS))


# ------------------------------------------------------------------------------------------------ designs
def _cover(gen, m, n):
    """n level indices in 0..m-1 that use every index (n >= m)"""
    assert n >= m
    lv = np.concatenate([gen.permutation(m), gen.integers(0, m, n - m)])
    return lv[gen.permutation(n)]


def hub_lengths(t):
    L = chunk_len(gre_tc(t))
    return (1, L - 1, L, L + 1, 2 * L, 2 * L + 1)


@functools.lru_cache(maxsize=None)
def hubs(t):
    """K = 2. Hub level j of effect 1 is observed with the levels 0 .. len_j - 1 of effect 0, hub level W + j of
    effect 0 with the ordinary levels nh .. nh + len_j - 1 of effect 1, len = hub_lengths(t): rows of exactly that
    many lower / upper entries. Every 5th pair is observed twice, every 15th three times."""
    lens = hub_lengths(t)
    nh, W = len(lens), lens[-1]
    a, b = [], []
    for j, ln in enumerate(lens):
        a += list(range(ln))
        b += [j] * ln
        a += [W + j] * ln
        b += list(range(nh, nh + ln))
    a, b = np.array(a), np.array(b)
    rep = 1 + (np.arange(a.size) % 5 == 0) + (np.arange(a.size) % 15 == 0)
    lv = np.stack([np.repeat(a, rep), np.repeat(b, rep)])
    return np.ascontiguousarray(lv[:, np.random.default_rng(100 + t).permutation(lv.shape[1])], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _named(name):
    gen = np.random.default_rng(hash_name(name))
    if name == "three":
        # (40, 7, 300) levels: a row of the middle effect has up to 40 lower and 300 upper entries around split,
        # several chunks each at the chunk length 32 of t >= 33; level 0 of the middle effect crosses them all
        n = 1500
        lv = np.stack([_cover(gen, 40, n), _cover(gen, 7, n), _cover(gen, 300, n)])
        hub = np.stack([np.arange(300) % 40, np.zeros(300, int), np.arange(300)])
        lv = np.concatenate([lv, hub], axis=1)
    elif name == "nested":
        l1 = _cover(gen, 60, 300)
        lv = np.stack([l1 // 4, l1])
    elif name == "tiny11":
        lv = np.zeros((2, 1), int)
    elif name == "tiny15":
        lv = np.stack([np.zeros(5, int), np.arange(5)])
    elif name == "gap":
        l0 = _cover(gen, 5, 40)
        lv = np.stack([l0 + (l0 >= 3), _cover(gen, 5, 40)])          # index 3 of effect 0 is never used
    elif name == "eight":
        lv = np.stack([_cover(gen, m, 200) for m in (3, 5, 20, 4, 7, 11, 16, 9)])
    elif name == "sizes":
        lv = np.stack([np.arange(1000) % m for m in (1, 255, 256, 257, 1000)])
    elif name == "zlists":
        # observation lists of 1, 63, 64, 0 (an unused index), 65 and 129 in effect 0
        l0 = np.repeat([0, 1, 2, 4, 5], [1, 63, 64, 65, 129])
        lv = np.stack([l0, np.arange(l0.size) % 7])
    elif name == "seg":
        # pair (j, j) observed c_j times: a level of each effect and a CSR slot of each triangle with c_j
        # observations; then levels of 40 observations whose slots are short
        cs = (1, 32, 33, 512, 513, 1024, 1025)
        l0 = np.repeat(np.arange(len(cs)), cs)
        extra0 = np.repeat([7, 8], 40)
        extra1 = 7 + np.arange(80) % 40
        lv = np.stack([np.concatenate([l0, extra0]), np.concatenate([l0, extra1])])
    elif name.startswith("dense"):
        ms = {"dense1": (1,), "dense63": (3, 60), "dense64": (4, 60), "dense65": (5, 60), "dense130": (2, 128),
              "dense193": (1, 63, 64, 65)}[name]
        lv = np.stack([_cover(gen, m, 300) for m in ms])
    elif name.startswith("q-"):
        _, K, n = name.split("-")
        K, n = int(K), int(n)
        lv = np.stack([gen.integers(0, min(n, 4 + 3 * k), n) for k in range(K)])
        lv[:, 0] = [min(n, 4 + 3 * k) - 1 for k in range(K)]         # m_k does not depend on the draw
    elif name == "qbig":
        n = 256 * K_MAX_BLOCKS + 1
        lv = np.stack([_cover(gen, 50, n), _cover(gen, 70, n)])
    else:
        raise KeyError(name)
    return np.ascontiguousarray(lv, dtype=np.int32)


def hash_name(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


Q_KS, Q_NS = (1, 2, 3, 8), (1, 255, 256, 257)
NAMED = ("three", "nested", "tiny11", "tiny15", "gap", "eight", "sizes", "zlists", "seg", "dense1", "dense63",
         "dense64", "dense65", "dense130", "dense193", "qbig") + tuple(f"q-{K}-{n}" for K in Q_KS for n in Q_NS)
BLOCK_DESIGNS = ("three", "nested", "tiny11", "tiny15", "gap", "eight")
DESIGNS = tuple(f"hubs{t}" for t in TS) + NAMED


def design(name):
    return hubs(int(name[4:])) if name.startswith("hubs") else _named(name)


# every (design, t) of the block operators
BLOCK_CASES = tuple((f"hubs{t}", t) for t in TS) + tuple((d, t) for d in BLOCK_DESIGNS for t in TS_OTHER)


# ------------------------------------------------------------------------------------------------ structure
class Struct:
    pass


@functools.lru_cache(maxsize=None)
def structure(name):
    """GroupedRE's constructor in numpy"""
    lv = design(name).astype(np.int64)
    K, n = lv.shape
    s = Struct()
    s.name, s.K, s.n = name, K, n
    s.m = lv.max(axis=1) + 1
    s.cum = np.concatenate([[0], np.cumsum(s.m)]).astype(np.int64)
    M = s.M = int(s.cum[-1])
    s.glev = lv + s.cum[:-1, None]
    s.blk = np.repeat(np.arange(K), s.m)
    s.cnt = np.bincount(s.glev.ravel(), minlength=M).astype(np.float64)
    order = np.argsort(s.glev.ravel(), kind="stable")               # effect-major, observations ascending
    s.obs = (order % n).astype(np.int64)
    s.obs_ptr = np.concatenate([[0], np.cumsum(s.cnt)]).astype(np.int64)
    keys, okeys = [], []
    for k in range(K):
        for l in range(K):
            if k != l:
                keys.append(s.glev[k] * M + s.glev[l])
                okeys.append(np.arange(n))
    if keys:
        keys, okeys = np.concatenate(keys), np.concatenate(okeys)
        uq, inv, cts = np.unique(keys, return_inverse=True, return_counts=True)
    else:
        keys = okeys = inv = np.zeros(0, np.int64)
        uq, cts = np.zeros(0, np.int64), np.zeros(0, np.int64)
    s.nnz = uq.size
    s.row, s.col = uq // M, uq % M
    s.val = cts.astype(np.float64)
    s.rowptr = np.concatenate([[0], np.cumsum(np.bincount(s.row, minlength=M))]).astype(np.int64)
    lower = s.col < s.cum[s.blk[s.row]] if s.nnz else np.zeros(0, bool)
    s.split = s.rowptr[:-1] + np.bincount(s.row[lower], minlength=M)
    # the observations of every CSR slot, ascending (GroupedLaplace's inverted index)
    so = np.lexsort((okeys, inv)) if s.nnz else np.zeros(0, np.int64)
    s.slot_obs = okeys[so]
    s.slot_ptr = np.concatenate([[0], np.cumsum(cts)]).astype(np.int64)
    return s


def entry_range(s, kind):
    a = s.split if kind == UPPER else s.rowptr[:-1]
    b = s.split if kind == LOWER else s.rowptr[1:]
    return a, b


def chunk_plan(s, t):
    """GroupedRE::Plan for the lane split of t: per kind (e0, e1, ptr), and lower_q / upper_q"""
    L = chunk_len(gre_tc(t))
    plans = []
    for kind in (FULL, LOWER, UPPER):
        a, b = entry_range(s, kind)
        nch = -(-(b - a) // L)
        ptr = np.concatenate([[0], np.cumsum(nch)]).astype(np.int64)
        row = np.repeat(np.arange(s.M), nch)
        j = np.arange(ptr[-1]) - ptr[row]
        e0 = a[row] + j * L
        e1 = np.minimum(e0 + L, b[row])
        plans.append((e0, e1, ptr))
    return plans, plans[LOWER][2][s.cum], plans[UPPER][2][s.cum]


def seg_plan(s):
    """destination lengths (levels, then CSR slots) and GroupedLaplace's counts: long levels, their chunks, all long
    destinations, all chunks"""
    ln = np.concatenate([s.cnt.astype(np.int64), np.diff(s.slot_ptr)])
    long_ = ln > K_SHORT_LEN
    nch = np.where(long_, -(-ln // K_CHUNK_LEN), 0)
    M = s.M
    return ln, (int(long_[:M].sum()), int(nch[:M].sum()), int(long_.sum()), int(nch.sum()))


def dense_ztz(s):
    """Z^T Z from the incidence matrix"""
    Z = np.zeros((s.n, s.M))
    for k in range(s.K):
        Z[np.arange(s.n), s.glev[k]] = 1.
    return Z.T @ Z


# ------------------------------------------------------------------------------------------------ values
def signed_decades(gen, shape, lo=-3., hi=3.):
    return gen.choice([-1., 1.], shape) * 10. ** gen.uniform(lo, hi, shape)


def positive_decades(gen, shape, lo=-1.5, hi=1.5):
    return 10. ** gen.uniform(lo, hi, shape)


@functools.lru_cache(maxsize=None)
def block_inputs(name, t, model):
    """X (M x t, mixed signs, six decades) and the operator: model = the counts with dis = sqrt(1 / D), else positive
    val over three decades, a random positive D and a random positive dis unrelated to it"""
    s = structure(name)
    gen = np.random.default_rng(hash_name(name) + 7919 * t + model)
    X = signed_decades(gen, (s.M, t))
    if model:
        val = s.val.copy()
        D = 1. / np.array([0.7, 1.9, 0.3, 1.1, 0.5, 2.3, 0.9, 1.3])[s.blk] + s.cnt
        dis = np.sqrt(1. / D)
    else:
        val = positive_decades(gen, s.nnz)
        D = positive_decades(gen, s.M)
        dis = positive_decades(gen, s.M)
    return dict(X=X, val=val, D=D, dis=dis)


MODEL_CASES = tuple(c for c in BLOCK_CASES if c[1] in (1, 50))      # the model's own counts, dis = sqrt(1 / D)
DENSE_DESIGNS = ("dense1", "dense63", "dense64", "dense65", "dense130", "dense193")
NPS = (1, 3, 4, 5)
SMALL_DESIGNS = ("sizes", "zlists", "gap", "eight", "tiny15")
Q_DESIGNS = tuple(f"q-{K}-{n}" for K in Q_KS for n in Q_NS)
TRACE_CASES = tuple((f"q-{K}-257", t) for K in (1, 2, 8) for t in (1, 3, 50))
SOLVE_DESIGNS = ("three", "hubs50")
DELTA = 1e-6


def _gen(name, salt):
    return np.random.default_rng(hash_name(name) * 31 + salt)


def dense_ld(name, padded):
    M = structure(name).M
    return M + (7 if padded else 0)


@functools.lru_cache(maxsize=None)
def dense_inputs(name):
    """Li lower triangular with NaN strictly above the diagonal, a full symmetric Ainv, sc > 0, idx of 5 points"""
    s = structure(name)
    gen = _gen(name, 1)
    M, K = s.M, s.K
    Li = np.tril(signed_decades(gen, (M, M), -2., 1.))
    Li[np.triu_indices(M, 1)] = np.nan
    A = signed_decades(gen, (M, M), -2., 1.)
    A = np.tril(A) + np.tril(A, -1).T
    idx = np.stack([s.cum[:-1] + gen.integers(0, s.m) for _ in range(5)]).astype(np.int32)
    idx[1] = -1                                                      # a point none of whose levels was seen
    idx[2, ::2] = -1
    return dict(Li=Li, Ainv=A, sc=positive_decades(gen, M), idx=idx, val=positive_decades(gen, s.nnz),
                D=positive_decades(gen, M))


@functools.lru_cache(maxsize=None)
def small_inputs(name):
    s = structure(name)
    gen = _gen(name, 2)
    return dict(y=signed_decades(gen, s.n), cnt=positive_decades(gen, s.M), tau=positive_decades(gen, s.K, -1., 1.),
                zty=signed_decades(gen, s.M), D=positive_decades(gen, s.M), x=positive_decades(gen, s.M, -3., 3.),
                ysgn=signed_decades(gen, s.M), sigma2=positive_decades(gen, s.K, -1., 1.), alpha=-0.37,
                w=signed_decades(gen, s.n))


@functools.lru_cache(maxsize=None)
def q_inputs(name):
    s = structure(name)
    gen = _gen(name, 3)
    A = signed_decades(gen, (s.M, s.M), -2., 1.)
    return dict(Ainv=np.tril(A) + np.tril(A, -1).T if s.K > 1 else None, D=positive_decades(gen, s.M),
                W=positive_decades(gen, s.n), dW=signed_decades(gen, s.n, -2., 2.), Wa=signed_decades(gen, s.n, -2., 2.),
                d1=signed_decades(gen, s.n), dwq=signed_decades(gen, s.n), v=signed_decades(gen, s.M))


@functools.lru_cache(maxsize=None)
def trace_inputs(name, t):
    s = structure(name)
    gen = _gen(name, 4 + t)
    return dict(U=signed_decades(gen, (s.M, t)), V=signed_decades(gen, (s.M, t)), dW=signed_decades(gen, s.n, -2., 2.))


# ------------------------------------------------------------------------------------------------ references
def seg_sum(terms, a, b):
    """out[r] = sum of terms[a[r]:b[r]] along axis 0 (empty ranges give 0), in terms' dtype"""
    out = np.zeros((len(a),) + terms.shape[1:], terms.dtype)
    nz = b > a
    if nz.any():
        idx = np.stack([a[nz], b[nz]], axis=1).ravel()
        pad = np.concatenate([terms, np.zeros((1,) + terms.shape[1:], terms.dtype)])
        out[nz] = np.add.reduceat(pad, idx, axis=0)[::2]
    return out


def _ld(x):
    return np.asarray(x, dtype=LD)


OP_KIND = {"apply": FULL, "apply_lower": LOWER, "lds_mult": LOWER, "upper": UPPER}
OP_C = {"apply": 1, "apply_lower": 1, "lds_mult": 2, "upper": 3}


def product_reference(s, op, val, D, dis, X):
    """(reference, bound) of one of the four products, longdouble"""
    a, b = entry_range(s, OP_KIND[op])
    k = b - a
    val, D, X = _ld(val), _ld(D)[:, None], _ld(X)
    coef = val * _ld(dis)[s.col] if op == "lds_mult" else val
    terms = coef[:, None] * X[s.col]
    sm, sa = seg_sum(terms, a, b), seg_sum(np.abs(terms), a, b)
    if op == "lds_mult":
        dgx = D * _ld(dis)[:, None] * X
        ref, ab = sm + dgx, sa + np.abs(dgx)
    elif op == "upper":
        ref, ab = (D * X + sm) / D, (np.abs(D * X) + sa) / np.abs(D)
    else:
        ref, ab = sm + D * X, sa + np.abs(D * X)
    return ref, g(k + OP_C[op])[:, None] * ab


def _sweep(s, kind, coef, dd, rhs, scale, absolute=None):
    """the substitution of one sweep, effects ascending (kind LOWER) or descending (UPPER): out_r = (rhs_r - scale_r
    sum_e coef_e out_col) / dd_r; absolute = (gk, xhat): the same substitution on absolute values, e_r = (gk_r
    (|scale_r| sum |coef| |xhat_col| + |dd_r xhat_r|) + |scale_r| sum |coef| e_col) / |dd_r|"""
    a, b = entry_range(s, kind)
    out = np.zeros_like(rhs)
    order = range(s.K) if kind == LOWER else range(s.K - 1, -1, -1)
    for k in order:
        r0, r1 = s.cum[k], s.cum[k + 1]
        e0, e1 = s.rowptr[r0], s.rowptr[r1]
        cols = s.col[e0:e1]
        ar, br = a[r0:r1] - e0, b[r0:r1] - e0
        if absolute is None:
            sm = seg_sum(coef[e0:e1, None] * out[cols], ar, br)
            out[r0:r1] = (rhs[r0:r1] - scale[r0:r1] * sm) / dd[r0:r1]
        else:
            gk, xh = absolute
            ac = np.abs(coef[e0:e1, None])
            sx = seg_sum(ac * np.abs(xh[cols]), ar, br)
            se = seg_sum(ac * out[cols], ar, br)
            sc = np.abs(scale[r0:r1])
            out[r0:r1] = (gk[r0:r1] * (sc * sx + np.abs(dd[r0:r1] * xh[r0:r1])) + sc * se) / np.abs(dd[r0:r1])
    return out


def ssor_ratios(s, val, D, dis, R, Xh, Zh):
    """the two checks of both sweeps on the device's X and Z: (residual ratio fwd, bwd, forward-error ratio fwd, bwd)"""
    val, D, dis, R, Xh, Zh = _ld(val), _ld(D), _ld(dis), _ld(R), _ld(Xh), _ld(Zh)
    dd = (D * dis)[:, None]
    one = np.ones((s.M, 1), LD)
    out = []
    for kind, coef, scale, rhs, sol in ((LOWER, val * dis[s.col], one, R, Xh), (UPPER, val, dis[:, None], Xh, Zh)):
        a, b = entry_range(s, kind)
        gk = g(b - a + 3)[:, None]
        terms = coef[:, None] * sol[s.col]
        res = rhs - scale * seg_sum(terms, a, b) - dd * sol
        rb = gk * (np.abs(scale) * seg_sum(np.abs(terms), a, b) + np.abs(dd * sol))
        ref = _sweep(s, kind, coef, dd, rhs, scale)
        eb = _sweep(s, kind, coef, dd, rhs, scale, absolute=(gk, sol))
        out.append((max_ratio(np.abs(res), rb), max_ratio(np.abs(sol - ref), eb)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def ssor_reference(s, val, D, dis, R):
    """longdouble X and Z of the two sweeps"""
    val, D, dis, R = _ld(val), _ld(D), _ld(dis), _ld(R)
    dd = (D * dis)[:, None]
    X = _sweep(s, LOWER, val * dis[s.col], dd, R, np.ones((s.M, 1), LD))
    return X, _sweep(s, UPPER, val, dd, X, dis[:, None])


def list_sums(ptr, obs, w):
    """(sum, bound) of w over every list"""
    w = _ld(w)
    a, b = ptr[:-1], ptr[1:]
    t = w[obs]
    return seg_sum(t, a, b), g(b - a) * seg_sum(np.abs(t), a, b)


def assemble_reference(s, w, diag_only):
    ref, bnd = list_sums(s.obs_ptr, s.obs, w)
    if not diag_only:
        r2, b2 = list_sums(s.slot_ptr, s.slot_obs, w)
        ref, bnd = np.concatenate([ref, r2]), np.concatenate([bnd, b2])
    return ref, bnd


def diag_reference(s, cnt, tau):
    D = 1 / _ld(tau)[s.blk] + _ld(cnt)
    dis = np.sqrt(1 / D)
    m = s.m.astype(np.float64)
    a, b = s.cum[:-1], s.cum[1:]
    lg = np.log(D)
    sl, sal = seg_sum(lg, a, b), seg_sum(np.abs(lg), a, b)
    si = seg_sum(1 / D, a, b)
    return dict(D=(D, g(2) * np.abs(D)), dis=(dis, g(4) * dis),
                sums=(np.concatenate([sl, si]), np.concatenate([g(m + 2 * UF_ELEM) * sal + g(3) * m, g(m + 3) * si])))


def single_reference(zty, cnt, D):
    zty, cnt, D = _ld(zty), _ld(cnt), _ld(D)
    m = zty.size
    u = zty / D
    q = cnt * cnt / D
    return dict(u=(u, g(1) * np.abs(u)),
                sums=(np.array([cnt.sum(), q.sum()]), np.array([g(m) * np.abs(cnt).sum(), g(m + 2) * np.abs(q).sum()])))


def inv_diag_reference(Li):
    M = Li.shape[0]
    sq = np.tril(_ld(Li)) ** 2                                      # Li[r, c]: row r of column c, r >= c
    ref = sq.sum(axis=0)
    return ref, g(M - np.arange(M) + 1) * ref


def pred_reference(s, Li, idx, greater=False):
    """E (M x np) and var (np) with their bounds; greater: the defect r > a in the place of r >= a"""
    M, K = s.M, s.K
    L = _ld(Li)
    npts = idx.shape[0]
    E, Ea, cntt = np.zeros((M, npts), LD), np.zeros((M, npts), LD), np.zeros((M, npts))
    r = np.arange(M)
    for p in range(npts):
        for k in range(K):
            a = idx[p, k]
            if a >= 0:
                reach = r > a if greater else r >= a
                E[reach, p] += L[reach, a]
                Ea[reach, p] += np.abs(L[reach, a])
                cntt[reach, p] += 1
    return (E, g(np.maximum(cntt - 1, 0)) * Ea), ((E * E).sum(axis=0), g(M + 2 * K) * (Ea * Ea).sum(axis=0))


def fisher_reference(s, sc, Ainv):
    sc, A = _ld(sc), _ld(Ainv)
    B2 = (A * sc[:, None] * sc[None, :]) ** 2                       # [r, c]
    part = np.stack([B2[s.cum[k]:s.cum[k + 1]].sum(axis=0) for k in range(s.K)], axis=1)      # [c, k]
    dg = np.diag(A) * sc * sc
    return (part, g(s.m + 5)[None, :] * part), (dg, g(2) * np.abs(dg))


def dense_build_expected(s, val, D, ld):
    A = np.zeros((s.M, ld))                                         # column c at A[c]
    A[np.arange(s.M), np.arange(s.M)] = D
    A[s.col, s.row] = val
    return A


def q_reference(s, Ainv, D, W, dW, Wa):
    """dwq with its bound, and the K (+ 1) sums with theirs"""
    K, n = s.K, s.n
    W, dW = _ld(W), _ld(dW)
    q = np.zeros((K, n), LD)
    qa = np.zeros((K, n), LD)
    if K == 1:
        q[0] = 1 / _ld(D)[s.glev[0]]
        qa[0] = np.abs(q[0])
    else:
        A = _ld(Ainv)
        for j in range(K):
            for k in range(K):
                v = A[s.glev[j], s.glev[k]]                         # symmetric; the kernel reads column g_k, row g_j
                q[j] += v
                qa[j] += np.abs(v)
    qi, qai = q.sum(axis=0), qa.sum(axis=0)
    dwq = (dW * qi / 2, g(K * K + 1) * np.abs(dW) * qai / 2)
    sums = [(W * q[j]).sum() for j in range(K)]
    bnds = [g(n * K + 1) * (np.abs(W) * qa[j]).sum() for j in range(K)]
    if Wa is not None:
        sums.append((_ld(Wa) * qi).sum())
        bnds.append(g(n * K * K + 1) * (np.abs(Wa) * qai).sum())
    return dwq, (np.array(sums), np.array(bnds))


def row_trace_reference(s, t, Ub, Vb, dW):
    Ub, Vb, dW = _ld(Ub), _ld(Vb), _ld(dW)
    a = sum(Ub[s.glev[k]] for k in range(s.K))
    p = sum(Vb[s.glev[k]] for k in range(s.K))
    aa = sum(np.abs(Ub[s.glev[k]]) for k in range(s.K))
    pa = sum(np.abs(Vb[s.glev[k]]) for k in range(s.K))
    ref = dW * (a * p).sum(axis=1) / t / 2
    return ref, g(2 * s.K + t + 2) * np.abs(dW) * (aa * pa).sum(axis=1) / t / 2


def grad_f_reference(s, d1, dwq, W, v):
    d1, dwq, W, v = _ld(d1), _ld(dwq), _ld(W), _ld(v)
    zv = sum(v[s.glev[k]] for k in range(s.K))
    za = sum(np.abs(v[s.glev[k]]) for k in range(s.K))
    return -d1 + dwq - W * zv, g(s.K + 2) * (np.abs(d1) + np.abs(dwq) + np.abs(W) * za)


def effect_dots_reference(s, mode, x, y):
    x = _ld(x)
    if mode == 0:
        v = x * _ld(y)
    elif mode == 1:
        v = np.log(x)
    elif mode == 2:
        v = 1 / x
    else:
        v = x / _ld(y)
    a, b = s.cum[:-1], s.cum[1:]
    m = s.m.astype(np.float64)
    return seg_sum(v, a, b), g(m + (2 * UF_ELEM if mode == 1 else 1)) * seg_sum(np.abs(v), a, b)


def _fused(x, s_, y, sign):
    """fl(x + sign s y) with one rounding, exactly: float(Fraction) rounds to nearest even"""
    F = fractions.Fraction
    return np.array([float(F(a) + sign * F(b) * F(c)) for a, b, c in zip(x, np.broadcast_to(s_, x.shape), y)])


def vec_expected(s, form, sigma2, alpha, x, y):
    """the float64 results that the IEEE operations of a form can give (a list of one or two arrays)"""
    sigi = (1. / np.asarray(sigma2))[s.blk]
    if form == 0:
        return [sigi + x]
    if form == 1:
        return [x - sigi * y, _fused(x, sigi, y, -1)]
    if form == 2:
        return [x / y]
    if form == 3:
        return [x + alpha * y, _fused(x, alpha, y, 1)]
    return [np.sqrt(1. / x)]


def solve_drift(s, val, D, u, its):
    """(its + 1) g(k_max + 5) || |A| |u| ||_2"""
    a, b = entry_range(s, FULL)
    au = seg_sum(np.abs(_ld(val))[:, None] * np.abs(_ld(u))[s.col][:, None], a, b)[:, 0] + np.abs(_ld(D) * _ld(u))
    return (its + 1) * float(g((b - a).max() + 5)) * float(np.sqrt((au * au).sum()))


def true_residual(s, val, D, rhs, u):
    a, b = entry_range(s, FULL)
    Au = seg_sum(_ld(val)[:, None] * _ld(u)[s.col][:, None], a, b)[:, 0] + _ld(D) * _ld(u)
    r = _ld(rhs) - Au
    return float(np.sqrt((r * r).sum()))


@functools.lru_cache(maxsize=None)
def solve_inputs(name, model):
    """an operator that is positive definite: the model's own, or weights with D above the row's absolute sum"""
    s = structure(name)
    gen = np.random.default_rng(hash_name(name) + 31 + model)
    if model:
        q = block_inputs(name, 1, 1)
        val, D, dis = q["val"], q["D"], q["dis"]
    else:
        w = positive_decades(gen, s.nnz // 2 + 1)
        # symmetric weights: entry (r, c) and entry (c, r) share one
        lo = np.minimum(s.row, s.col) * s.M + np.maximum(s.row, s.col)
        val = w[np.unique(lo, return_inverse=True)[1]]
        a, b = entry_range(s, FULL)
        D = seg_sum(val, a, b) * gen.uniform(1.05, 1.5, s.M) + 0.1
        dis = np.sqrt(1. / D)
    rhs = signed_decades(gen, s.M, -1., 1.)
    return dict(val=val, D=D, dis=dis, rhs=rhs)


# ------------------------------------------------------------------------------------------------ the hooks
def _lib():
    c = ctypes
    from gpboost_amd import basic
    lib = basic.lib()
    if not getattr(lib, "_grouped_ops_typed", False):
        Dp, I, L, F, V = c.POINTER(c.c_double), c.c_int, c.c_int64, c.c_double, c.c_void_p
        PI, PL, PG, PD = c.POINTER(c.c_int32), c.POINTER(c.c_int64), c.POINTER(c.c_int), c.POINTER(Dp)
        lib.GPB_TestGroupedCreate.argtypes = [I, I, PI, L, c.POINTER(V)]
        lib.GPB_TestGroupedFree.argtypes = [V]
        lib.GPB_TestGroupedInfo.argtypes = [V, I, PL, L, PI, L, Dp, L]
        lib.GPB_TestGroupedApply.argtypes = [V, I, I, Dp, Dp, Dp, Dp, Dp, Dp, L, PG]
        lib.GPB_TestGroupedSmall.argtypes = [V, I, PD, PL, I, PD, PL, I, PG]
        lib.GPB_TestGroupedDense.argtypes = [V, I, I, I, PI, PD, PL, I, PD, PL, I, PG]
        lib.GPB_TestGroupedSolve.argtypes = [V, Dp, Dp, Dp, Dp, Dp, I, Dp, I, F, Dp, PG, PG]
        lib.GPB_TestGroupedLaplaceOps.argtypes = [V, I, I, I, I, F, PD, PL, I, PD, PL, I, PG]
        lib.LGBM_GetLastError.restype = c.c_char_p
        lib._grouped_ops_typed = True
    return lib


def _check(ret):
    if ret != 0:
        msg = _lib().LGBM_GetLastError().decode("utf-8")
        if "HIP error" in msg:          # the device context is gone: nothing more may run on it
            import pytest
            pytest.exit(f"HIP error, session ended: {msg}", returncode=3)
        raise HookError(msg)


_handles = {}


def handle(name):
    if name not in _handles:
        lv = design(name)
        h = ctypes.c_void_p()
        _check(_lib().GPB_TestGroupedCreate(lv.shape[1], lv.shape[0], _ip(lv), lv.size, ctypes.byref(h)))
        _handles[name] = h
    return _handles[name]


def free_handles():
    for h in _handles.values():
        _check(_lib().GPB_TestGroupedFree(h))
    _handles.clear()


STATS = ("M", "nnz", "n", "K", "tc", "L", "n_full", "n_lower", "n_upper", "n_ints", "long_levels", "level_chunks",
         "long_all", "chunks_all")


def info_hook(name, t):
    """what the engine holds for the design and the lane split of t, as a dict"""
    h = handle(name)
    st = np.zeros(len(STATS), np.int64)
    _check(_lib().GPB_TestGroupedInfo(h, t, _ip(st, ctypes.c_int64), st.size, None, 0, None, 0))
    q = dict(zip(STATS, (int(v) for v in st)))
    ints, dbls = np.zeros(q["n_ints"], np.int32), np.zeros(q["nnz"] + q["M"])
    _check(_lib().GPB_TestGroupedInfo(h, t, _ip(st, ctypes.c_int64), st.size, _ip(ints), ints.size, _dp(dbls), dbls.size))
    M, K, nnz, n = q["M"], q["K"], q["nnz"], q["n"]
    pos = [0]

    def take(ln):
        pos[0] += ln
        return ints[pos[0] - ln:pos[0]].astype(np.int64)
    for key, ln in (("cum", K + 1), ("rowptr", M + 1), ("split", M), ("col", nnz), ("obs_ptr", M + 1), ("obs", n * K)):
        q[key] = take(ln)
    for kind, key in enumerate(KINDS):
        nk = q["n_" + key]
        q["plan_" + key] = (take(nk), take(nk), take(M + 1))
    q["lower_q"], q["upper_q"] = take(K + 1), take(K + 1)
    assert pos[0] == ints.size
    q["val"], q["cnt"] = dbls[:nnz], dbls[nnz:]
    return q


APPLY_OPS = {"apply": 0, "apply_lower": 1, "lds_mult": 2, "ssor": 3, "upper": 4, "precond": 5}


def apply_hook(name, op, t, val, dg, dis, X):
    """(Out0, Out1 or None) of GPB_TestGroupedApply; the guard bands of the outputs and of the chunk partials intact"""
    two = op in ("ssor", "precond")
    X = np.ascontiguousarray(X)
    o0 = np.full(X.shape, 7.25)
    o1 = np.full(X.shape, 7.25) if two else None
    gd = ctypes.c_int(-1)
    _check(_lib().GPB_TestGroupedApply(handle(name), APPLY_OPS[op], t, _dp(val), _dp(dg),
                                       _dp(dis) if op in ("lds_mult", "ssor", "precond") else None, _dp(X), _dp(o0),
                                       _dp(o1), X.size, ctypes.byref(gd)))
    assert gd.value == 0, f"{name} {op} t={t}: a guard word changed"
    return o0, o1


def _arrays(ins, out_lens):
    Dp = ctypes.POINTER(ctypes.c_double)
    ins = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in ins]
    outs = [np.full(n, 7.25) for n in out_lens]
    pin = (Dp * max(len(ins), 1))(*[_dp(a) for a in ins])
    pout = (Dp * max(len(outs), 1))(*[_dp(a) for a in outs])
    li = np.array([0 if a is None else a.size for a in ins], np.int64)
    lo = np.array(out_lens, np.int64)
    return ins, outs, pin, _ip(li, ctypes.c_int64), len(ins), pout, _ip(lo, ctypes.c_int64), len(outs), (li, lo)


SMALL_OPS = {"zty": 0, "diag": 1, "single": 2, "residual": 3}


def small_hook(name, op, ins, out_lens):
    keep = _arrays(ins, out_lens)
    gd = ctypes.c_int(-1)
    _check(_lib().GPB_TestGroupedSmall(handle(name), SMALL_OPS[op], *keep[2:8], ctypes.byref(gd)))
    assert gd.value == 0, f"{name} {op}: a guard word changed"
    return keep[1]


DENSE_OPS = {"build": 0, "inv_diag": 1, "pred_e": 2, "pred_var": 3, "fisher": 4}


def dense_hook(name, op, ld, ins, out_lens, idx=None):
    """matrices in ins are M x M arrays indexed [row, column]; they go to the hook column-major"""
    ins = [np.asfortranarray(a).ravel(order="F") if a is not None and a.ndim == 2 else a for a in ins]
    keep = _arrays(ins, out_lens)
    idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    gd = ctypes.c_int(-1)
    _check(_lib().GPB_TestGroupedDense(handle(name), DENSE_OPS[op], ld, 0 if idx is None else idx.shape[0], _ip(idx),
                                       *keep[2:8], ctypes.byref(gd)))
    assert gd.value == 0, f"{name} {op}: a guard word changed"
    return keep[1]


def solve_hook(name, val, cnt, D, dis, rhs, u0, pmax, delta):
    s = structure(name)
    u = np.full(s.M, 7.25)
    its, gd = ctypes.c_int(-1), ctypes.c_int(-1)
    _check(_lib().GPB_TestGroupedSolve(handle(name), _dp(val), _dp(cnt), _dp(D), _dp(dis), _dp(rhs), int(u0 is not None),
                                       _dp(u0), pmax, delta, _dp(u), ctypes.byref(its), ctypes.byref(gd)))
    assert gd.value == 0, f"{name} solve: a guard word changed"
    return u, its.value


LAPLACE_OPS = {"assemble": 0, "q": 1, "row_trace": 2, "grad_f": 3, "vec": 4, "effect_dots": 5}


def laplace_hook(name, op, ins, out_lens, sub=0, t=1, ld=0, alpha=0.):
    ins = [np.asfortranarray(a).ravel(order="F") if a is not None and a.ndim == 2 and op == "q" else a for a in ins]
    keep = _arrays(ins, out_lens)
    gd = ctypes.c_int(-1)
    _check(_lib().GPB_TestGroupedLaplaceOps(handle(name), LAPLACE_OPS[op], sub, t, ld, alpha, *keep[2:8],
                                            ctypes.byref(gd)))
    assert gd.value == 0, f"{name} {op}: a guard word changed"
    return keep[1]
