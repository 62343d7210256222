"""GPU: the dense fp64 MFMA primitives of dense_kernels.hip (gemm_f64 with its three tile kernels and triangle
masks, gemm_f64_splitk, chol_lower, trtri_lower, launch_logdet_chol, spd_solve_inverse), element by element
against exact or numpy.longdouble references through the GPB_TestDense* hooks.

Cases, generators, references and the derivation of every bound are in tests/dense_ops_cases.py;
tests/test_dense_ops_reference.py shows on the CPU that the integer cases are exact in float64 and that a plain
float64 numpy version of each primitive meets the same bounds. Tests that have an error bound print the largest
error / bound ratio they saw (pytest -s).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ops_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _run_gemm(case, ops, variant):
    C = ops["C"].copy()
    ret = dc.hook_gemm(variant, case["M"], case["N"], case["K"], case["alpha"], ops["A"], ops["lda"], case["ta"],
                       ops["B"], ops["ldb"], case["tb"], case["beta"], C, ops["ldc"], case["masks"])
    assert ret == 0, dc.last_error()
    return C


def _check_exact(case):
    """integer data: the whole C buffer (result, untouched elements, padding rows, guard columns) is as expected"""
    ops = dc.gemm_operands(case)
    C = _run_gemm(case, ops, case["variant"])
    want = dc.gemm_expected_buffer(case, ops, dc.gemm_exact(case, ops))
    if not np.array_equal(C, want):
        bad = np.flatnonzero(~((C == want) | (np.isnan(C) & np.isnan(want))))
        pytest.fail(f"{case}: {bad.size} wrong entries, first at flat index {bad[0]} (row {bad[0] % ops['ldc']}, "
                    f"col {bad[0] // ops['ldc']}): got {C[bad[0]]}, want {want[bad[0]]}")


# ------------------------------------------------------------------------------------------------------- a, b, c
def test_gemm_exact_indexing_over_the_shape_grid():
    """2a: every M, N, K of the grid with every transpose pair and each forced kernel; C starts as NaN where
    beta == 0; K == 0 gives beta C; padding rows and guard columns keep their sentinel."""
    assert sum(c["pad"] > 0 for c in dc.GEMM_GRID_CASES) * 2 >= len(dc.GEMM_GRID_CASES)
    for case in dc.GEMM_GRID_CASES:
        _check_exact(case)


def test_gemm_masks_never_read_structural_zeros():
    """2b: the parts the masks declare zero hold NaN on the device, the result equals the product with zeros
    there; under lower_out the elements above the diagonal keep their sentinel, inside diagonal tiles too."""
    for case in dc.GEMM_MASK_CASES:
        _check_exact(case)


def test_gemm_in_place_trsm_form():
    """2c: C aliases A (chol_lower's L21 = A21 L11^-T): the result equals the out-of-place product."""
    seed = 0
    for variant in (0, 1, 2, 3):
        for M in (1, 63, 64, 65, 200):
            for N in (1, 63, 64):
                seed += 1
                pad = seed % 3
                A, B = dc.ints(M, N, 4001 * seed), dc.ints(N, N, 4001 * seed + M * N + 7)     # B stored N x K
                lda, ldb = M + pad, N + pad
                bufA, bufB = dc.pack(A, lda, dc.SENTINEL), dc.pack(B, ldb)
                C = np.full(bufA.size, np.nan)
                ret = dc.hook_gemm(variant, M, N, N, 1., bufA, lda, 0, bufB, ldb, 1, 0., C, lda, alias=1)
                assert ret == 0, dc.last_error()
                assert np.array_equal(C, dc.pack(A @ B.T, lda, dc.SENTINEL)), (variant, M, N)


# ---------------------------------------------------------------------------------------------------------- d, e
@pytest.fixture(scope="module")
def real_results():
    """the real-valued cases run once with each forced kernel: (case, operands, {variant: C buffer})"""
    out = []
    for case in dc.GEMM_REAL_CASES:
        ops = dc.gemm_operands(case, real=True)
        out.append((case, ops, {v: _run_gemm(case, ops, v) for v in (1, 2, 3)}))
    return out


def test_gemm_tile_size_never_changes_a_bit(real_results):
    """2d: 'the tile size never changes a result bit': the three kernels agree bitwise on real-valued data."""
    for case, ops, res in real_results:
        assert np.array_equal(_bits(res[1]), _bits(res[2])), case
        assert np.array_equal(_bits(res[2]), _bits(res[3])), case


def test_gemm_rounding_within_the_inner_product_bound(real_results):
    """2e: |C^ - C| <= gamma_{K+2} (|alpha| |A||B| + |beta| |C0|) against the longdouble product."""
    worst = 0.
    for case, ops, res in real_results:
        ref, bound = dc.gemm_longdouble(case, ops)
        got = dc.unpack(res[2], ops["ldc"], case["M"], case["N"])
        w = ~ops["keep"]
        assert np.all(np.isfinite(got[w])), case
        worst = max(worst, dc.max_ratio(np.abs(got.astype(dc.LD) - ref)[w], bound[w]))
        assert np.array_equal(res[2], dc.gemm_expected_buffer(case, ops, got)), case     # sentinels untouched
    print(f"\ngemm rounding: largest error / bound = {worst:.3f}")
    assert worst <= 1.


# ------------------------------------------------------------------------------------------------------------- f
@pytest.mark.parametrize("idx", range(len(dc.DISPATCH_CASES)))
def test_gemm_production_dispatch_around_the_128_tile_threshold(idx):
    """2f: variant 0 on both sides of the 512-tile threshold, exact integer data."""
    c = dc.DISPATCH_CASES[idx]
    assert (dc.tiles128(c["M"], c["N"]) >= 512) == (idx < 2)
    M, N, K = c["M"], c["N"], c["K"]
    A = dc.ints(M, K, 17 + 1000 * idx)
    B = A[:N] if M == N else dc.ints(N, K, 5 + M * K + 1000 * idx)          # stored N x K (transB)
    ldc = M + 3
    C0 = np.resize(dc.ints(251, 257, 3), (M, N))
    keep = np.triu(np.ones((M, N), dtype=bool), 1) if c["lower_out"] else np.zeros((M, N), dtype=bool)
    dev = np.where(keep, dc.SENTINEL, C0 if c["beta"] != 0. else np.nan)
    C = dc.pack(dev, ldc, dc.SENTINEL, extra_cols=1)
    ret = dc.hook_gemm(0, M, N, K, c["alpha"], dc.pack(A, M + 1), M + 1, 0, dc.pack(B, N), N, 1, c["beta"], C, ldc,
                       (c["lower_out"], 0, 0, 0))
    assert ret == 0, dc.last_error()
    want = c["alpha"] * (A @ B.T) + (c["beta"] * C0 if c["beta"] != 0. else 0.)
    assert np.array_equal(C, dc.pack(np.where(keep, dc.SENTINEL, want), ldc, dc.SENTINEL, extra_cols=1))


# ------------------------------------------------------------------------------------------------------------- g
def _run_splitk(case, ops, variant):
    C = ops["C"].copy()
    ret, chunks = dc.hook_splitk(variant, case["M"], case["N"], case["K"], ops["A"], ops["lda"], case["ta"], ops["B"],
                                 ops["ldb"], case["tb"], C, ops["ldc"], ops["cstride"], ops["nslabs"], case["target"],
                                 case["max_chunks"])
    assert ret == 0, dc.last_error()
    return chunks, C.reshape(ops["nslabs"], ops["cstride"])


def test_splitk_chunks_cover_k_exactly_once():
    """2g: 1 <= chunks <= max_chunks; slabs >= chunks untouched; slabs < chunks fully written (and nothing else
    of them); the slabs summed in chunk order are the exact product."""
    for case in dc.SPLITK_CASES:
        ops = dc.splitk_operands(case)
        M, N, ldc = case["M"], case["N"], ops["ldc"]
        chunks, slabs = _run_splitk(case, ops, case["variant"])
        assert 1 <= chunks <= case["max_chunks"], case
        assert np.all(slabs[chunks:] == dc.SENTINEL), case
        total = np.zeros((M, N))
        for z in range(chunks):
            part = dc.unpack(slabs[z][:ldc * N], ldc, M, N)
            assert np.all(part != dc.SENTINEL) and np.all(np.isfinite(part)), (case, z)
            assert np.array_equal(slabs[z], np.append(dc.pack(part, ldc, dc.SENTINEL), slabs[z][ldc * N:])), (case, z)
            assert np.all(slabs[z][ldc * N:] == dc.SENTINEL), (case, z)
            total += part
        assert np.array_equal(total, ops["opA"] @ ops["opB"]), case


def test_splitk_same_chunks_same_bits():
    """2g: 'same chunks -> same bits': the 64-tile and 128-tile forms give bitwise-equal slabs on real data, and
    the production rule (128-tiles at M, N >= 128) is one of them."""
    for case in dc.SPLITK_REAL_CASES:
        ops = dc.splitk_operands(case, real=True)
        c1, s1 = _run_splitk(case, ops, 1)
        c2, s2 = _run_splitk(case, ops, 2)
        c0, s0 = _run_splitk(case, ops, 0)
        assert c0 == c1 == c2 and c1 >= 2, case
        assert np.array_equal(_bits(s1), _bits(s2)) and np.array_equal(_bits(s0), _bits(s2)), case
        total = sum(dc.unpack(s1[z][:ops["ldc"] * case["N"]], ops["ldc"], case["M"], case["N"]).astype(dc.LD)
                    for z in range(c1))
        ref = np.dot(ops["opA"].astype(dc.LD), ops["opB"].astype(dc.LD))
        bound = dc.gamma(case["K"]) * (np.abs(ops["opA"]) @ np.abs(ops["opB"]))
        assert dc.max_ratio(np.abs(total - ref), bound) <= 1., case


# ------------------------------------------------------------------------------------------------------------- h
_chol_worst = {}


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("n", dc.CHOL_ORDERS)
def test_cholesky_inverse_logdet(n, kind):
    """2h: structure (what is written, what is never touched) and the residual bounds, for ld = roundup64(n) and
    64 more."""
    A = dc.spd_matrix(kind, n)
    low = np.tril(np.ones((n, n), dtype=bool))
    diag_upper, off_upper = dc.block_structure(n)
    seen = None
    for ld in (dc.roundup64(n), dc.roundup64(n) + 64):
        bufA, bufW = dc.chol_buffers(A, ld)
        ret, info, logdet = dc.hook_chol(n, ld, bufA, bufW)
        assert ret == 0, dc.last_error()
        assert info == 0
        fullA, fullW = bufA.reshape(ld, ld).T, bufW.reshape(ld, ld).T
        outside = np.ones((ld, ld), dtype=bool)
        outside[:n, :n] = ~low
        assert np.all(np.isnan(fullA[outside]))            # strict upper triangle and padding: still NaN
        outside[:n, :n] = off_upper
        assert np.all(np.isnan(fullW[outside]))            # strictly-upper off-diagonal blocks and padding
        L, W = fullA[:n, :n], fullW[:n, :n]
        assert np.all(np.isfinite(L[low])) and np.all(np.isfinite(W[low]))
        assert np.all(W[diag_upper] == 0.)                 # the TRSM reads these without a mask
        L, W = np.where(low, L, 0.), np.where(low, W, 0.)
        if seen is not None and np.array_equal(L, seen[0]) and np.array_equal(W, seen[1]) and logdet == seen[2]:
            continue                                       # same bits as the first ld: same ratios
        seen = (L, W, logdet)
        r = dc.chol_ratios(A, L, W, logdet)
        print(f"\nn = {n} A{kind} ld = {ld}: error / bound: Cholesky {r['chol']:.3f}, inverse {r['inverse']:.3f}, "
              f"logdet {r['logdet']:.3f}")
        for k, v in r.items():
            _chol_worst[k] = max(_chol_worst.get(k, 0.), v)
        assert r["chol"] <= 1. and r["inverse"] <= 1. and r["logdet"] <= 1.
    print(f"largest so far: {_chol_worst}")


def test_cholesky_alone_leaves_the_rest_of_w_untouched():
    """chol_lower without trtri_lower writes only the diagonal 64-blocks of W and gives the same factor."""
    n, ld = 257, 320
    A = dc.spd_matrix(2, n)
    bufA, bufW = dc.chol_buffers(A, ld)
    ret, info, logdet = dc.hook_chol(n, ld, bufA, bufW, want_inverse=0, want_logdet=False)
    assert ret == 0 and info == 0 and logdet is None
    bufA2, bufW2 = dc.chol_buffers(A, ld)
    assert dc.hook_chol(n, ld, bufA2, bufW2)[:2] == (0, 0)
    assert np.array_equal(_bits(bufA), _bits(bufA2))
    W = bufW.reshape(ld, ld).T
    i, j = np.indices((ld, ld))
    blocks = (i // 64 == j // 64) & (i < n) & (j < n)
    assert np.all(np.isnan(W[~blocks])) and np.all(np.isfinite(W[blocks]))
    assert np.array_equal(W[blocks], bufW2.reshape(ld, ld).T[blocks])


# ------------------------------------------------------------------------------------------------------------- i
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("n", dc.SPD_ORDERS)
def test_spd_solve_inverse(n, kind):
    """2i: x, diag(A^-1), A^-1 against longdouble, with all outputs and with each of them absent."""
    ref = dc.spd_reference(kind, n)
    A = np.ascontiguousarray(ref["A"].T).reshape(-1)
    first = None
    for want in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        x = np.full(n, np.nan) if want[0] else None
        diag = np.full(n, np.nan) if want[1] else None
        inv = np.full(n * n, np.nan) if want[2] else None
        ret = dc.hook_spd(n, A, ref["b"].copy() if want[0] else None, x, diag, inv)
        assert ret == 0, dc.last_error()
        inv2 = inv.reshape(n, n).T if want[2] else None
        for v in (x, diag, inv):
            assert v is None or np.all(np.isfinite(v))
        r = dc.spd_ratios(ref, x, diag, inv2)
        print(f"\nn = {n} A{kind} cond_inf = {ref['cond']:.1f} outputs {want}: error / bound: "
              + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
        assert all(v <= 1. for v in r.values()), r
        if first is None:
            first = (x, diag, inv)
        else:                                              # an absent output changes no bit of the others
            for v, f in zip((x, diag, inv), first):
                assert v is None or np.array_equal(_bits(v), _bits(f))


# ------------------------------------------------------------------------------------------------------------- j
@pytest.mark.parametrize("pos", [0, 70, dc.BAD_PIVOT_ORDER - 1])
@pytest.mark.parametrize("value", [0., -1., float("nan"), float("inf")])
def test_bad_pivot_is_reported(value, pos):
    """2j: a pivot that is zero, negative, NaN or +inf in the first, a middle or the last (ragged) diagonal block
    gives info > 0 and a normal return."""
    n = dc.BAD_PIVOT_ORDER
    A = dc.spd_matrix(1, n).copy()
    A[pos, pos] = value
    bufA, bufW = dc.chol_buffers(A, dc.roundup64(n))
    ret, info, _ = dc.hook_chol(n, dc.roundup64(n), bufA, bufW)
    assert ret == 0, dc.last_error()
    assert info > 0


@pytest.mark.parametrize("n", [64, 128])
def test_infinite_last_pivot_of_a_full_block_is_reported(n):
    """A +inf pivot used to pass the p > 0 guard and turn into NaN through rsq(inf) = 0 and 0 * inf in the Newton
    step. At order 130 that NaN reaches a later pivot (at the last index: the identity padding of the ragged
    block), which fails the guard, so info was raised all the same; only as the very last pivot of a full block
    did it give a NaN factor with info == 0. Now it counts in info and is replaced by 1: the factor stays finite."""
    A = dc.spd_matrix(1, n).copy()
    A[n - 1, n - 1] = np.inf
    bufA, bufW = dc.chol_buffers(A, n)
    ret, info, _ = dc.hook_chol(n, n, bufA, bufW, want_inverse=0, want_logdet=False)
    assert ret == 0, dc.last_error()
    assert info > 0
    assert np.all(np.isfinite(bufA.reshape(n, n).T[np.tril(np.ones((n, n), dtype=bool))]))


def test_hooks_reject_bad_arguments():
    """a mistake in a test is an error return, never a device access"""
    A, B, C = np.zeros(12), np.zeros(12), np.zeros(12)
    assert dc.hook_gemm(4, 3, 3, 2, 1., A, 3, 0, B, 2, 0, 0., C, 3) == -1 and "variant" in dc.last_error()
    assert dc.hook_gemm(1, 3, 3, 2, 1., A, 2, 0, B, 2, 0, 0., C, 3) == -1
    assert dc.hook_gemm(1, 3, 5, 2, 1., A, 3, 0, B, 2, 0, 0., C, 3) == -1
    assert dc.hook_chol(3, 96, np.zeros(96 * 96), np.zeros(96 * 96))[0] == -1
    assert dc.hook_gemm(1, 3, 3, 2, 1., A, 3, 0, B, 2, 0, 0., C, 3) == 0
