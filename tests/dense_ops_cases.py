"""Cases, generators, references and error bounds of the dense fp64 primitive tests, shared by
tests/test_gpu_dense_ops.py (the HIP kernels through the GPB_TestDense* hooks) and
tests/test_dense_ops_reference.py (CPU: the cases are exact where they claim to be, and a float64 numpy
stand-in of each primitive meets the very bounds the kernels are held to).

Everything is column-major like the library. Inputs come from synthetic.lcg_unif (portable, no numpy.random).
Bounds (u = 2^-53, gamma_k = k u / (1 - k u)), none of them tuned to what a kernel gives:
  gemm      |C^ - C| <= gamma_{K+2} (|alpha| |A||B| + |beta| |C0|)   (inner product of length K, the alpha
            product, the beta product and the final sum: Higham, Accuracy and Stability, 2nd ed., (3.5);
            fused multiply-adds only lower it)
  Cholesky  |A - L^ L^^T| <= 4 gamma_{n+1} |L^||L^^T|   (Theorem 10.3 has constant 1 for a correctly
            rounded square root and division; the default diagonal-block kernel scales by a Newton-refined
            reciprocal square root within an ulp (2u), which at most doubles a term; the other factor 2 is
            margin at n = 1, 2 where the bound has no slack)
  inverse   |W^ - L^^-1| <= 4 gamma_n |L^^-1||L^||L^^-1|   (forward bound of triangular inversion by any
            standard method, section 14.2; 4 for the two levels of blocked products over rounded blocks)
  logdet    |ld^ - 2 sum log L^_ii| <= 2 n u (1 + max |log L^_ii|)
  SPD       ||x^ - x||_inf <= 8 n u cond_inf(A) ||x||_inf, the same for diag(A^-1) and A^-1
The residual side of each comparison is computed in numpy.longdouble (64-bit significand here, checked by the
CPU tests), the bound side in float64 (its own rounding, ~n u relative, is far below the margins).
"""
import functools

import numpy as np

from gpboost_amd import synthetic

U = 2.0 ** -53
SENTINEL = -777.25          # never a value of an integer case, exactly representable
LD = np.longdouble


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------ generators
# draws kept per LCG seed (lcg_unif is a Python loop): the integer and real operand streams wrap around, the
# stream of A1 is as long as its largest matrix, the right-hand sides need one vector
_STREAM_SIZE = {0.61: 1 << 18, 0.23: 1 << 18, 0.37: 577 * 577, 0.53: 577}


@functools.lru_cache(maxsize=None)
def _stream(seed):
    return synthetic.lcg_unif(_STREAM_SIZE[seed], seed)


def unif(count, seed, offset=0):
    """count draws of the LCG stream of this seed from position offset (wrapping around the stream's length)."""
    s = _stream(seed)
    idx = (offset + np.arange(count)) % s.size
    return s[idx]


def ints(rows, cols, offset):
    """rows x cols integers in [-8, 8] as float64"""
    return (np.floor(unif(rows * cols, 0.61, offset) * 17.0) - 8.0).reshape(cols, rows).T.copy()


def reals(rows, cols, offset):
    """rows x cols reals in [-0.5, 0.5)"""
    return (unif(rows * cols, 0.23, offset) - 0.5).reshape(cols, rows).T.copy()


def pack(vals, ld, fill=np.nan, extra_cols=0):
    """column-major buffer of leading dimension ld holding vals, every other entry = fill"""
    rows, cols = vals.shape
    assert ld >= max(1, rows)
    buf = np.full((cols + extra_cols, ld), fill, dtype=np.float64)
    buf[:cols, :rows] = vals.T
    return buf.reshape(-1)


def unpack(buf, ld, rows, cols):
    return buf.reshape(-1, ld)[:cols, :rows].T


def a_mask(M, K, a_lower, a_upper):
    """True where op(A)[i][k] is a structural zero"""
    i, k = np.indices((M, K))
    m = np.zeros((M, K), dtype=bool)
    if a_lower:
        m |= k > i
    if a_upper:
        m |= k < i
    return m


def b_mask(K, N, b_lower):
    k, j = np.indices((K, N))
    return (k < j) if b_lower else np.zeros((K, N), dtype=bool)


# ------------------------------------------------------------------------------------------------ gemm cases
GRID_MN = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)
GRID_K = (0, 1, 3, 4, 5, 15, 16, 17, 31, 33, 64, 100)
TRANSPOSES = ((0, 0), (0, 1), (1, 0), (1, 1))
ALPHA_BETA = tuple((a, b) for a in (1., -1., 2.) for b in (0., 1., -1.))
NO_MASK = (0, 0, 0, 0)      # lower_out, a_lower, a_upper, b_lower


def _grid_cases():
    """For every transpose pair and every variant 1..3: 12 shapes in which every M, every N and every K of the
    grid occurs (the M and N lists are walked with a stride that depends on the combination, so the pairings
    differ between combinations); alpha / beta walk all nine pairs; two thirds of the cases have every leading
    dimension strictly above its row count."""
    cases = []
    for c, ((ta, tb), variant) in enumerate((t, v) for t in TRANSPOSES for v in (1, 2, 3)):
        for t in range(12):
            M = GRID_MN[(t + c) % 11]
            N = GRID_MN[(3 * t + 5 * c + 4) % 11]
            K = GRID_K[t]
            alpha, beta = ALPHA_BETA[(t + c) % 9]
            pad = 0 if t % 3 == 0 else 1 + (t + c) % 5
            cases.append(dict(variant=variant, M=M, N=N, K=K, ta=ta, tb=tb, alpha=alpha, beta=beta, pad=pad,
                              masks=NO_MASK, seed=len(cases)))
    return tuple(cases)


GEMM_GRID_CASES = _grid_cases()

# Every (masks, transA, transB) combination that a gemm / gemm_f64 call site of gpboost_amd/csrc uses with a mask
# set (found by listing the arguments of all of them), and lower_out without a transpose:
#   lower_out, transB                 the Cholesky panel and trailing updates A -= L L^T
#   b_lower                           X = L21 W11 (trtri_lower, VADU)
#   a_lower                           W21 = -W22 X, z = W b, W Z (20 sites)
#   a_lower, transB                   W Sigma_po^T products of the predictions
#   a_lower, transA                   fitc_fisher.hip
#   a_upper                           fitc_fisher.hip (U X with U = W^T stored upper)
#   a_upper, transA                   W^T X (FITC, VIF, dense-Laplace)
#   a_upper + b_lower, transA         the full W^T W (spd_solve_inverse, FITC, dense-Laplace)
#   lower_out + a_upper + b_lower, transA   P = W^T W, lower triangle (the dense gradient and Fisher traces)
MASK_CONFIGS = (
    dict(masks=(1, 0, 0, 0), ta=0, tb=0),
    dict(masks=(1, 0, 0, 0), ta=0, tb=1),
    dict(masks=(0, 0, 0, 1), ta=0, tb=0),
    dict(masks=(0, 1, 0, 0), ta=0, tb=0),
    dict(masks=(0, 1, 0, 0), ta=0, tb=1),
    dict(masks=(0, 1, 0, 0), ta=1, tb=0),
    dict(masks=(0, 0, 1, 0), ta=0, tb=0),
    dict(masks=(0, 0, 1, 0), ta=1, tb=0),
    dict(masks=(0, 0, 1, 1), ta=1, tb=0),
    dict(masks=(1, 0, 1, 1), ta=1, tb=0),
)
# the diagonal inside a tile, on a tile edge and one past it, for 64- and 128-tiles; rectangular both ways
MASK_SHAPES = ((17, 17, 17), (63, 63, 63), (64, 64, 64), (65, 65, 65), (127, 127, 127), (128, 128, 128),
               (129, 129, 129), (200, 200, 200), (129, 65, 100), (65, 129, 33), (200, 63, 64), (64, 200, 127),
               (128, 127, 17))


def _mask_cases():
    cases = []
    for c, cfg in enumerate(MASK_CONFIGS):
        for s, (M, N, K) in enumerate(MASK_SHAPES):
            for variant in (1, 2, 3):
                alpha, beta = ALPHA_BETA[(c + s + variant) % 9]
                cases.append(dict(variant=variant, M=M, N=N, K=K, ta=cfg["ta"], tb=cfg["tb"], alpha=alpha,
                                  beta=beta, pad=(s + c) % 3, masks=cfg["masks"], seed=1000 + 13 * c + s))
    return tuple(cases)


GEMM_MASK_CASES = _mask_cases()

# real-valued cases (tile-size invariance, rounding): shapes of the grid, masks, beta != 0, alpha not a power of 2
GEMM_REAL_CASES = tuple(
    dict(M=M, N=N, K=K, ta=ta, tb=tb, alpha=alpha, beta=beta, pad=pad, masks=masks, seed=2000 + i)
    for i, (M, N, K, ta, tb, alpha, beta, pad, masks) in enumerate((
        (200, 200, 100, 0, 0, 1., 1., 0, NO_MASK),
        (129, 127, 64, 0, 1, -1., 1., 3, NO_MASK),
        (65, 200, 33, 1, 0, 0.7, -0.3, 1, NO_MASK),
        (127, 129, 31, 1, 1, 1.3, 0.5, 2, NO_MASK),
        (200, 200, 64, 0, 1, -1., 1., 0, (1, 0, 0, 0)),
        (129, 129, 100, 0, 1, -0.9, 1., 5, (1, 0, 0, 0)),
        (200, 128, 128, 0, 0, 1., 0.25, 0, (0, 0, 0, 1)),
        (200, 129, 200, 0, 0, -1., -1.5, 4, (0, 1, 0, 0)),
        (200, 200, 200, 1, 0, 1., 0.1, 0, (0, 0, 1, 1)),
        (200, 200, 200, 1, 0, 1., 0.5, 3, (1, 0, 1, 1)),
        (129, 129, 129, 1, 0, -0.8, 1., 0, (1, 0, 1, 1)),
        (17, 63, 5, 0, 0, 2.5, 1., 1, NO_MASK),
        (1, 1, 100, 1, 0, 1., 3., 0, NO_MASK),
        (64, 65, 17, 1, 1, -0.6, 0., 2, NO_MASK),
        (128, 16, 15, 0, 1, 1., 0., 0, NO_MASK),
    )))


def gemm_operands(case, real=False):
    """The case's operands. Returns a dict with the device buffers (A, B, C with NaN in the parts the masks
    declare zero, in the padding rows of A and B, and in C where beta == 0; SENTINEL in C's padding rows, its two
    guard columns and, under lower_out, above the diagonal), their leading dimensions, and the reference operands
    opA (M x K), opB (K x N), C0 (M x N) with the masked parts zero."""
    M, N, K, ta, tb = case["M"], case["N"], case["K"], case["ta"], case["tb"]
    lower_out, a_lower, a_upper, b_lower = case["masks"]
    gen = reals if real else ints
    off = 7919 * case["seed"]
    opA = gen(M, K, off)
    opB = gen(K, N, off + M * K + 11)
    C0 = gen(M, N, off + M * K + K * N + 29)
    am, bm = a_mask(M, K, a_lower, a_upper), b_mask(K, N, b_lower)
    devA, devB = np.where(am, np.nan, opA), np.where(bm, np.nan, opB)
    opA, opB = np.where(am, 0., opA), np.where(bm, 0., opB)
    stA, stB = (devA.T if ta else devA), (devB.T if tb else devB)
    pad = case["pad"]
    lda, ldb, ldc = max(1, stA.shape[0]) + pad, max(1, stB.shape[0]) + pad, max(1, M) + pad
    i, j = np.indices((M, N))
    keep = (j > i) if lower_out else np.zeros((M, N), dtype=bool)     # elements the call must not write
    devC = np.where(keep, SENTINEL, C0 if case["beta"] != 0. else np.nan)
    return dict(A=pack(stA, lda), B=pack(stB, ldb), C=pack(devC, ldc, SENTINEL, extra_cols=2), lda=lda, ldb=ldb,
                ldc=ldc, opA=opA, opB=opB, C0=C0, keep=keep)


def gemm_expected_buffer(case, ops, value):
    """C's whole buffer after the call, given the M x N result value: untouched entries keep their SENTINEL"""
    return pack(np.where(ops["keep"], SENTINEL, value), ops["ldc"], SENTINEL, extra_cols=2)


def gemm_exact(case, ops):
    """alpha opA opB + beta C0 for integer-valued operands (exact in float64: see the CPU tests)"""
    out = case["alpha"] * (ops["opA"] @ ops["opB"])
    if case["beta"] != 0.:
        out = out + case["beta"] * ops["C0"]
    return out


def gemm_magnitude(case):
    """upper limit of any partial result of an integer case"""
    return abs(case["alpha"]) * 64. * case["K"] + abs(case["beta"]) * 8.


def gemm_longdouble(case, ops):
    """(reference, bound) of a real-valued case"""
    ref = LD(case["alpha"]) * np.dot(ops["opA"].astype(LD), ops["opB"].astype(LD))
    mag = abs(case["alpha"]) * (np.abs(ops["opA"]) @ np.abs(ops["opB"]))
    if case["beta"] != 0.:
        ref = ref + LD(case["beta"]) * ops["C0"].astype(LD)
        mag = mag + abs(case["beta"]) * np.abs(ops["C0"])
    return ref, gamma(case["K"] + 2) * mag


def max_ratio(err, bound):
    """largest err / bound over the entries (0 / 0 counts as 0, err > 0 = bound as inf)"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0., 0., err / bound)
    return float(np.max(r))


# --------------------------------------------------------------------------------------- production dispatch
# (M, N, K, transA, transB, alpha, beta, lower_out): 23 x 24 = 552 128-tiles (>= 512: the 128-tile kernel), ragged
# in both dimensions; a lower_out update with beta = 1; 22 x 23 = 506 128-tiles (the 64-tile kernel)
DISPATCH_CASES = (
    dict(M=2897, N=2945, K=40, ta=0, tb=1, alpha=1., beta=0., lower_out=0),
    dict(M=2945, N=2945, K=24, ta=0, tb=1, alpha=-1., beta=1., lower_out=1),
    dict(M=2700, N=2900, K=40, ta=0, tb=1, alpha=1., beta=0., lower_out=0),
)


def tiles128(M, N):
    return ((M + 127) // 128) * ((N + 127) // 128)


# ------------------------------------------------------------------------------------------------ split-K cases
SPLITK_MN = (1, 40, 64, 127, 128, 130, 200)
SPLITK_K = (1, 15, 16, 17, 255, 256, 257, 1000, 4099)
SPLITK_TARGET = (1, 256, 1024)
SPLITK_MAXCHUNKS = (1, 3, 64)


def _splitk_cases():
    """Per transpose pair 18 cases: every M, N, K, target_blocks, max_chunks and variant (0 rule, 1 64-tile,
    2 128-tile) occurs; target_blocks x max_chunks walks all nine pairs twice, and the variant meets every
    target_blocks and every max_chunks."""
    cases = []
    for c, (ta, tb) in enumerate(TRANSPOSES):
        for t in range(18):
            cases.append(dict(M=SPLITK_MN[(t + c) % 7], N=SPLITK_MN[(3 * t + 2 * c + 1) % 7], K=SPLITK_K[(t + 2 * c) % 9],
                              ta=ta, tb=tb, target=SPLITK_TARGET[t % 3], max_chunks=SPLITK_MAXCHUNKS[(t // 3) % 3],
                              variant=(t % 3 + t // 3 + c) % 3, pad=(t + c) % 4, seed=3000 + 18 * c + t))
    return tuple(cases)


SPLITK_CASES = _splitk_cases()
SPLITK_REAL_CASES = (
    dict(M=130, N=200, K=1000, ta=0, tb=1, target=256, max_chunks=64, pad=1, seed=3500),
    dict(M=128, N=128, K=4099, ta=1, tb=0, target=1024, max_chunks=64, pad=0, seed=3501),
    dict(M=200, N=130, K=257, ta=0, tb=0, target=1024, max_chunks=3, pad=2, seed=3502),
)


def splitk_operands(case, real=False):
    M, N, K, ta, tb = case["M"], case["N"], case["K"], case["ta"], case["tb"]
    gen = reals if real else ints
    off = 7919 * case["seed"]
    opA, opB = gen(M, K, off), gen(K, N, off + M * K + 11)
    stA, stB = (opA.T if ta else opA), (opB.T if tb else opB)
    pad = case["pad"]
    lda, ldb, ldc = stA.shape[0] + pad, stB.shape[0] + pad, M + pad
    nslabs = case["max_chunks"] + 1
    cstride = ldc * N + 3 * pad
    return dict(A=pack(stA, lda), B=pack(stB, ldb), C=np.full(nslabs * cstride, SENTINEL), lda=lda, ldb=ldb, ldc=ldc,
                nslabs=nslabs, cstride=cstride, opA=opA, opB=opB)


# ------------------------------------------------------------------------------- Cholesky / inverse / logdet
CHOL_ORDERS = (1, 2, 63, 64, 65, 128, 255, 256, 257, 320, 513, 577)
SPD_ORDERS = (1, 63, 65, 257)
BAD_PIVOT_ORDER = 130


def roundup64(n):
    return (n + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def spd_matrix(kind, n):
    """A1 = G G^T / n + I, G = lcg_unif(n n, 0.37) - 0.5 (condition ~1.3); A2 = 4 exp(-d / 0.15) + I on
    synthetic.bench_coords(n), the workload's own kind (condition ~230 at n = 577). Read-only."""
    if kind == 1:
        G = (unif(n * n, 0.37) - 0.5).reshape(n, n)
        A = G @ G.T / n + np.eye(n)
    else:
        X = synthetic.bench_coords(n)
        d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
        A = 4. * np.exp(-d / 0.15) + np.eye(n)
    A = np.tril(A) + np.tril(A, -1).T       # exactly symmetric
    A.setflags(write=False)
    return A


def chol_buffers(A, ld):
    """(A, W) device inputs, ld x ld column-major: A's lower triangle, NaN everywhere else (strict upper triangle
    and the padding); W all NaN"""
    n = A.shape[0]
    buf = np.full((ld, ld), np.nan)
    buf[:n, :n] = np.where(np.tril(np.ones((n, n), dtype=bool)), A, np.nan).T
    return buf.reshape(-1), np.full(ld * ld, np.nan)


def block_structure(n):
    """boolean n x n masks: upper (j > i) inside a diagonal 64-block; strictly upper off-diagonal blocks"""
    i, j = np.indices((n, n))
    same = (i // 64) == (j // 64)
    return same & (j > i), (j // 64) > (i // 64)


def longdouble_lower_inverse(L):
    """L^-1 by forward substitution in longdouble, row by row"""
    n = L.shape[0]
    Ll = L.astype(LD)
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        r = -np.dot(Ll[i, :i], X[:i, :]) if i else np.zeros(n, dtype=LD)
        r[i] += 1
        X[i, :] = r / Ll[i, i]
    return X


def chol_ratios(A, L, W, logdet):
    """Largest error / bound ratios (Cholesky residual, inverse, logdet) of a computed lower factor L, its inverse
    W (or None) and 2 sum log L_ii (or None), all n x n float64 with exact zeros above the diagonal."""
    n = A.shape[0]
    low = np.tril(np.ones((n, n), dtype=bool))
    Ll = L.astype(LD)
    res = np.abs(A.astype(LD) - np.dot(Ll, Ll.T))
    bound = 4. * gamma(n + 1) * (np.abs(L) @ np.abs(L).T)
    out = {"chol": max_ratio(res[low], bound[low])}
    if W is not None:
        X = longdouble_lower_inverse(L)
        Xa = np.abs(X.astype(np.float64))
        bound = 4. * gamma(n) * (Xa @ np.abs(L) @ Xa)
        out["inverse"] = max_ratio(np.abs(W.astype(LD) - X)[low], bound[low])
    if logdet is not None:
        logs = np.log(np.diag(L).astype(LD))
        ref = 2 * logs.sum()
        out["logdet"] = float(abs(LD(logdet) - ref)) / (2. * n * U * (1. + float(np.max(np.abs(logs)))))
    return out


@functools.lru_cache(maxsize=None)
def spd_reference(kind, n):
    """longdouble x = A^-1 b, diag(A^-1), A^-1, b and the error bounds 8 n u cond_inf(A) ||exact||_inf"""
    A = spd_matrix(kind, n)
    Al = A.astype(LD)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):                       # longdouble Cholesky, column by column
        L[j, j] = np.sqrt(Al[j, j] - np.dot(L[j, :j], L[j, :j]))
        L[j + 1:, j] = (Al[j + 1:, j] - np.dot(L[j + 1:, :j], L[j, :j])) / L[j, j]
    Wl = longdouble_lower_inverse(L)
    inv = np.dot(Wl.T, Wl)
    b = unif(n, 0.53) - 0.5
    x = np.dot(inv, b.astype(LD))
    norm = lambda v: float(np.max(np.abs(v).sum(axis=1))) if v.ndim == 2 else float(np.max(np.abs(v)))
    cond = norm(Al) * norm(inv)
    c = 8. * n * U * cond
    return dict(A=A, b=b, x=x, diag=np.diag(inv).copy(), inv=inv, cond=cond,
                bound=dict(x=c * norm(x), diag=c * norm(np.diag(inv)), inv=c * norm(inv)), norm=norm)


def spd_ratios(ref, x, diag, inv):
    """error / bound ratios of computed x, diag, inv (each may be None), inv's asymmetry against the same bound,
    and |diag - diag(inv)| against 2 gamma_{n+1} diag: both are sums of the n - j nonnegative squares W_ij^2 (one
    rounding each) in different orders (a wave reduction and the MFMA's k-ascending chain), each within gamma_{n+1}
    of the exact sum, so no fixed few-ulp limit holds at every n; at n = 1 they must be equal"""
    norm, n, out = ref["norm"], ref["A"].shape[0], {}
    if x is not None:
        out["x"] = norm(x.astype(LD) - ref["x"]) / ref["bound"]["x"]
    if diag is not None:
        out["diag"] = norm(diag.astype(LD) - ref["diag"]) / ref["bound"]["diag"]
    if inv is not None:
        out["inv"] = norm(inv.astype(LD) - ref["inv"]) / ref["bound"]["inv"]
        out["sym"] = norm(inv - inv.T) / ref["bound"]["inv"]
    if diag is not None and inv is not None:
        few = 0. if n == 1 else 2. * gamma(n + 1)        # n = 1: one and the same product, no sum
        out["diag_vs_inv"] = max_ratio(np.abs(diag - np.diag(inv)), few * np.abs(np.diag(inv)))
    return out


# ------------------------------------------------------------------------------------ the library's test hooks
def _lib():
    import ctypes as c
    from gpboost_amd import basic
    lib = basic.lib()
    if not getattr(lib, "_dense_ops_typed", False):
        D, I, L = c.POINTER(c.c_double), c.c_int, c.c_int64
        lib.GPB_TestDenseGemm.argtypes = [I, I, I, I, c.c_double, D, L, I, I, D, L, I, I, c.c_double, D, L, I,
                                          I, I, I, I, I]
        lib.GPB_TestDenseGemmSplitK.argtypes = [I, I, I, I, D, L, I, I, D, L, I, I, D, L, I, L, I, I, I, c.POINTER(I)]
        lib.GPB_TestDenseChol.argtypes = [I, I, D, D, I, D, c.POINTER(I)]
        lib.GPB_TestDenseSpdSolveInverse.argtypes = [I, D, D, D, D, D]
        lib._dense_ops_typed = True
    return lib


def _dp(a):
    import ctypes as c
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(c.POINTER(c.c_double))


def last_error():
    return _lib().LGBM_GetLastError().decode("utf-8")


def hook_gemm(variant, M, N, K, alpha, A, lda, ta, B, ldb, tb, beta, C, ldc, masks=NO_MASK, alias=0):
    """GPB_TestDenseGemm on flat float64 buffers (C in / out); returns the C ABI's return code"""
    return _lib().GPB_TestDenseGemm(variant, M, N, K, alpha, _dp(A), A.size, lda, ta, _dp(B), B.size, ldb, tb, beta,
                                    _dp(C), C.size, ldc, masks[0], masks[1], masks[2], masks[3], alias)


def hook_splitk(variant, M, N, K, A, lda, ta, B, ldb, tb, C, ldc, cstride, nslabs, target, max_chunks):
    """GPB_TestDenseGemmSplitK; returns (return code, chunks)"""
    import ctypes as c
    chunks = c.c_int(-1)
    ret = _lib().GPB_TestDenseGemmSplitK(variant, M, N, K, _dp(A), A.size, lda, ta, _dp(B), B.size, ldb, tb, _dp(C),
                                         C.size, ldc, cstride, nslabs, target, max_chunks, c.byref(chunks))
    return ret, chunks.value


def hook_chol(n, ld, A, W, want_inverse=1, want_logdet=True):
    """GPB_TestDenseChol (A, W in / out); returns (return code, info, logdet or None)"""
    import ctypes as c
    info = c.c_int(-1)
    logdet = np.full(1, np.nan)
    ret = _lib().GPB_TestDenseChol(n, ld, _dp(A), _dp(W), want_inverse, _dp(logdet) if want_logdet else None,
                                   c.byref(info))
    return ret, info.value, (float(logdet[0]) if want_logdet else None)


def hook_spd(n, A, b, x, diag, inv):
    return _lib().GPB_TestDenseSpdSolveInverse(n, _dp(A), _dp(b), _dp(x), _dp(diag), _dp(inv))
