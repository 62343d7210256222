"""CPU: the cases and bounds of tests/test_gpu_dense_ops.py (shared through tests/dense_ops_cases.py) are sound.

Two things are shown without a GPU. The integer cases stay far below 2^53 in magnitude, so every product and
partial sum is exact in float64 and 'equal to the int64 product' is the right demand on any summation order. And
a plain float64 numpy version of each primitive (matmul, numpy.linalg.cholesky, scipy's triangular solve, log,
numpy.linalg.solve / inv) stays within the very bounds the HIP kernels are held to, so none of them asks for
more than a correct fp64 implementation can give. The hooks' argument checks are exercised too: they come before
any device call, so they answer without a GPU.
"""
import os
import sys

import numpy as np
import pytest
from scipy.linalg import solve_triangular

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ops_cases as dc  # noqa: E402


def test_longdouble_is_wider_than_double():
    """the references need a significand well beyond 53 bits (x87 extended: 64)"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_case_lists_cover_the_grids():
    for ta, tb in dc.TRANSPOSES:
        for variant in (1, 2, 3):
            sel = [c for c in dc.GEMM_GRID_CASES if (c["ta"], c["tb"], c["variant"]) == (ta, tb, variant)]
            assert {c["M"] for c in sel} == set(dc.GRID_MN) and {c["N"] for c in sel} == set(dc.GRID_MN)
            assert {c["K"] for c in sel} == set(dc.GRID_K)
    assert {(c["alpha"], c["beta"]) for c in dc.GEMM_GRID_CASES} == set(dc.ALPHA_BETA)
    assert {(c["alpha"], c["beta"]) for c in dc.GEMM_GRID_CASES if c["K"] == 0} == set(dc.ALPHA_BETA)
    assert sum(c["pad"] > 0 for c in dc.GEMM_GRID_CASES) * 2 >= len(dc.GEMM_GRID_CASES)
    assert len(dc.GEMM_GRID_CASES) <= 400 and len(dc.GEMM_MASK_CASES) <= 400 and len(dc.SPLITK_CASES) <= 400
    for cfg in dc.MASK_CONFIGS:
        sel = [c for c in dc.GEMM_MASK_CASES if (c["masks"], c["ta"], c["tb"]) == (cfg["masks"], cfg["ta"], cfg["tb"])]
        assert {c["variant"] for c in sel} == {1, 2, 3}
        assert {(c["M"], c["N"], c["K"]) for c in sel} == set(dc.MASK_SHAPES)
    for ta, tb in dc.TRANSPOSES:
        sel = [c for c in dc.SPLITK_CASES if (c["ta"], c["tb"]) == (ta, tb)]
        assert {c["M"] for c in sel} == set(dc.SPLITK_MN) and {c["N"] for c in sel} == set(dc.SPLITK_MN)
        assert {c["K"] for c in sel} == set(dc.SPLITK_K) and {c["variant"] for c in sel} == {0, 1, 2}
        assert {(c["target"], c["max_chunks"]) for c in sel} == {(t, m) for t in dc.SPLITK_TARGET
                                                                 for m in dc.SPLITK_MAXCHUNKS}
        assert {(c["variant"], c["target"]) for c in sel} == {(v, t) for v in (0, 1, 2) for t in dc.SPLITK_TARGET}
        assert {(c["variant"], c["max_chunks"]) for c in sel} == {(v, m) for v in (0, 1, 2)
                                                                  for m in dc.SPLITK_MAXCHUNKS}
    # the (masks, transA, transB) combinations of the library's gemm call sites (see MASK_CONFIGS)
    used = {((1, 0, 0, 0), 0, 1), ((0, 0, 0, 1), 0, 0), ((0, 1, 0, 0), 0, 0), ((0, 1, 0, 0), 0, 1), ((0, 1, 0, 0), 1, 0),
            ((0, 0, 1, 0), 0, 0), ((0, 0, 1, 0), 1, 0), ((0, 0, 1, 1), 1, 0), ((1, 0, 1, 1), 1, 0)}
    assert used <= {(c["masks"], c["ta"], c["tb"]) for c in dc.MASK_CONFIGS}
    assert any(c["masks"] == (1, 0, 1, 1) for c in dc.GEMM_REAL_CASES)
    assert [dc.tiles128(c["M"], c["N"]) for c in dc.DISPATCH_CASES] == [552, 576, 506]


def test_integer_cases_are_exact_in_float64():
    """operands are integers in [-8, 8]; |alpha| K 64 + |beta| 8 bounds every partial result"""
    for case in dc.GEMM_GRID_CASES + dc.GEMM_MASK_CASES:
        assert dc.gemm_magnitude(case) < 2.0 ** 53
    for case in (dc.GEMM_GRID_CASES[::7] + dc.GEMM_MASK_CASES[::11]):
        ops = dc.gemm_operands(case)
        for v in (ops["opA"], ops["opB"], ops["C0"]):
            assert np.array_equal(v, np.round(v)) and (v.size == 0 or np.max(np.abs(v)) <= 8)
        want = case["alpha"] * (ops["opA"].astype(np.int64) @ ops["opB"].astype(np.int64)) \
            + case["beta"] * ops["C0"].astype(np.int64)
        assert np.array_equal(dc.gemm_exact(case, ops), want)
        assert np.max(np.abs(want), initial=0) <= dc.gemm_magnitude(case)
        # the device operands hold NaN exactly where the reference operands hold the structural zeros
        stA = dc.unpack(ops["A"], ops["lda"], *((case["K"], case["M"]) if case["ta"] else (case["M"], case["K"])))
        assert np.array_equal(np.isnan(stA.T if case["ta"] else stA), dc.a_mask(case["M"], case["K"], *case["masks"][1:3]))
    for case in dc.SPLITK_CASES + dc.SPLITK_REAL_CASES + dc.DISPATCH_CASES:
        assert 64. * case["K"] + 8. < 2.0 ** 53
    for case in dc.SPLITK_CASES[::9]:
        ops = dc.splitk_operands(case)
        assert np.array_equal(ops["opA"] @ ops["opB"], ops["opA"].astype(np.int64) @ ops["opB"].astype(np.int64))


def test_float64_matmul_meets_the_gemm_bound():
    worst = 0.
    for case in dc.GEMM_REAL_CASES:
        ops = dc.gemm_operands(case, real=True)
        ref, bound = dc.gemm_longdouble(case, ops)
        got = case["alpha"] * (ops["opA"] @ ops["opB"]) + (case["beta"] * ops["C0"] if case["beta"] != 0. else 0.)
        worst = max(worst, dc.max_ratio(np.abs(got.astype(dc.LD) - ref), bound))
    assert 0. < worst <= 1.


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("n", dc.CHOL_ORDERS)
def test_float64_cholesky_inverse_logdet_meet_their_bounds(n, kind):
    A = dc.spd_matrix(kind, n)
    L = np.linalg.cholesky(A)
    W = solve_triangular(L, np.eye(n), lower=True)
    r = dc.chol_ratios(A, L, np.tril(W), 2. * np.sum(np.log(np.diag(L))))
    # the Cholesky and inverse bounds carry a factor 4 for the kernels' reciprocal-square-root scaling and blocked
    # recursion; LAPACK's square root and division meet the constant-1 forms
    assert r["chol"] <= 0.25 and r["inverse"] <= 0.25 and r["logdet"] <= 1., r


def test_conditioning_of_the_test_matrices():
    assert np.linalg.cond(dc.spd_matrix(1, 577)) < 2.
    assert 100. < np.linalg.cond(dc.spd_matrix(2, 577)) < 500.


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("n", dc.SPD_ORDERS)
def test_float64_solve_and_inverse_meet_the_spd_bound(n, kind):
    ref = dc.spd_reference(kind, n)
    A = ref["A"]
    inv = np.linalg.inv(A)
    W = solve_triangular(np.linalg.cholesky(A), np.eye(n), lower=True)
    r = dc.spd_ratios(ref, np.linalg.solve(A, ref["b"]), (W * W).sum(axis=0), W.T @ W)
    assert all(v <= 1. for v in r.values()), r
    assert dc.spd_ratios(ref, None, None, inv)["inv"] <= 1.
    # the longdouble reference itself: A inv = I to longdouble rounding
    resid = np.dot(A.astype(dc.LD), ref["inv"]) - np.eye(n)
    assert float(np.max(np.abs(resid))) <= 64 * n * ref["cond"] * float(np.finfo(np.longdouble).eps)


def test_hooks_check_their_arguments_before_touching_the_device():
    A, B, C = np.zeros(12), np.zeros(12), np.zeros(12)
    bad = [
        dict(variant=4), dict(variant=-1), dict(M=-1), dict(lda=2), dict(ldb=1), dict(ldc=2), dict(N=5), dict(K=7),
        dict(ta=2), dict(masks=(0, 0, 3, 0)),
        dict(alias=1, ta=1), dict(alias=1, ldc=4), dict(alias=1, C=np.zeros(11)),
    ]
    for kw in bad:
        a = dict(variant=1, M=3, N=3, K=2, alpha=1., A=A, lda=3, ta=0, B=B, ldb=2, tb=0, beta=0., C=C, ldc=3,
                 masks=dc.NO_MASK, alias=0)
        a.update(kw)
        assert dc.hook_gemm(**a) == -1, kw
        assert "GPB_TestDenseGemm" in dc.last_error(), kw
    S = np.zeros(4 * 12)
    ok = dict(variant=0, M=3, N=3, K=2, A=A, lda=3, ta=0, B=B, ldb=2, tb=0, C=S, ldc=3, cstride=12, nslabs=4,
              target=1, max_chunks=4)
    for kw in (dict(variant=3), dict(nslabs=3), dict(cstride=8), dict(cstride=13), dict(ldc=2), dict(target=0),
               dict(max_chunks=0), dict(lda=2), dict(K=7)):
        a = dict(ok)
        a.update(kw)
        assert dc.hook_splitk(**a)[0] == -1, kw
        assert "GPB_TestDenseGemmSplitK" in dc.last_error(), kw
    Z = np.zeros(64 * 64)
    for n, ld in ((0, 64), (3, 96), (65, 64), (3, 0)):
        assert dc.hook_chol(n, ld, Z, Z.copy())[0] == -1
        assert "GPB_TestDenseChol" in dc.last_error()
    assert dc.hook_spd(0, Z, None, None, None, None) == -1
    assert dc.hook_spd(2, Z, np.zeros(2), None, None, None) == -1 and "together" in dc.last_error()
