"""GPU: the sparse multifrontal Cholesky (gpboost_amd/csrc/sparse_chol.hip) element by element through the
GPB_TestSparseChol* hooks, against the numpy.longdouble references and the bounds of tests/sparse_chol_cases.py
(derived there, none tuned to a kernel; tests/test_sparse_chol_reference.py holds a float64 LAPACK stand-in to the
same bounds and proves from the plan that every case reaches its path). Also: no result depends on what the
scratch buffers held before (NaN / zero poison), the bitwise identities the code claims, and pivots that are not
positive and finite. Every test prints its largest error / bound ratios under pytest -s. No test provokes a
fault: bad inputs are either rejected by the host checks or NaN / inf values in otherwise valid data.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_chol_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu


def _wkinds(name):
    return ("bern",) if name in ("g", "h") else sc.W_KINDS


def _rhs_counts(name):
    return sc.RHS_COUNTS if name in ("c", "f") else ((1, 5) if name in ("g", "h") else (1, 3))


# options that share an elimination order run next to each other, so the longdouble reference is computed once
BOUND_CASES = [(name, wk, opt) for name in sc.CASES for wk in _wkinds(name) for opt in sc.case_options(name)]


def run_all(ch, name, wkind, ts, inplace=0, want=(True, True, True)):
    """factor, log-determinant, selected inverse and every solve form of one handle, in float64_results' layout"""
    info, logdet = ch.factor(sc.w_vector(name, wkind))
    assert info == 0
    res = dict(L=ch.dense(0), logdet=logdet, fwd={}, solve={}, bwd={})
    res["tr_bdb"], res["tr_da"], res["diagS"] = ch.selected_inverse(want)
    res["S"], res["S_mirror"] = ch.dense(1), ch.dense(2)
    res["solve1"] = ch.solve(sc.Chol.SOLVE, sc.rhs(name, 1), 1, inplace)
    for t in ts:
        b = sc.rhs(name, t)
        res["solve"][t] = ch.solve(sc.Chol.SOLVE_MULTI, b, t, inplace)
        res["fwd"][t] = ch.solve(sc.Chol.FORWARD, b, t, inplace)
        res["bwd"][t] = ch.solve(sc.Chol.BACKWARD, np.ascontiguousarray(res["fwd"][t].T).reshape(-1), t, inplace)
    return res


def assert_same_bits(a, b, what=""):
    """every float64 of two results of run_all is bitwise equal (NaN outside S's structure included)"""
    for k in a:
        if isinstance(a[k], dict):
            for t in set(a[k]) & set(b[k]):
                assert np.array_equal(sc.bits(a[k][t]), sc.bits(b[k][t])), f"{what}: {k}[{t}] differs"
        elif a[k] is None or b[k] is None:
            continue
        else:
            assert np.array_equal(sc.bits(np.asarray(a[k])), sc.bits(np.asarray(b[k]))), f"{what}: {k} differs"


def assert_finite(res, plan):
    struct = sc.structure(plan)
    for k, v in res.items():
        if isinstance(v, dict):
            assert all(np.all(np.isfinite(x)) for x in v.values()), k
        elif k in ("S", "S_mirror"):
            assert np.all(np.isfinite(v[struct])) and np.all(np.isnan(v[~struct])), k
        elif v is not None:
            assert np.all(np.isfinite(v)), k


BOUND_IDS = [f"{n}-{w}-{sc.opt_id(o)}" for n, w, o in BOUND_CASES]


@pytest.mark.parametrize("name,wkind,opt", BOUND_CASES, ids=BOUND_IDS)
def test_every_bound(name, wkind, opt):
    """Every bound of sparse_chol_cases on every case, option set and W kind, with every scratch and output buffer
    holding NaN beforehand: the componentwise factor residual, L exactly zero outside its structure, the solves,
    the selected inverse, diagS, the log-determinant and the traces; S bitwise symmetric wherever both copies are
    stored; diagS = diag(S) and Solve = SolveMulti(1) bitwise.

    The factor residual is what the panel step's substitution (chol_trsm_kernel) is for: as a product with the
    explicit inverse of the diagonal block the same step missed it on e1-none (ratio 27.5), e2-none (1.26),
    f-none-leaf8 (1.8e12) and g-bern (9.71), at fill-in entries of L that cancel to ~1e-10 and less beside entries
    of order 1; with the substitution the largest ratio over all cases is 0.29 (float64 LAPACK: 0.11)."""
    plan = sc.plan_of(name, opt)
    ref = sc.reference(name, wkind, opt)
    ch = sc.Chol(name, dict(opt, poison=1))
    res = run_all(ch, name, wkind, _rhs_counts(name))
    ch.close()
    assert_finite(res, plan)
    assert np.array_equal(sc.bits(res["S"]), sc.bits(res["S_mirror"])), "S differs from its mirrored copy"
    assert np.array_equal(res["diagS"][plan["perm"]], np.diag(res["S"])), "diagS is not diag(S)"
    assert np.array_equal(res["solve1"], res["solve"][1]), "Solve differs from SolveMulti with one column"
    ratios = sc.result_ratios(ref, plan, res)
    _FACTOR_RATIO[(name, wkind, sc.opt_id(opt))] = ratios["factor"]
    sc.report(f"device {name} {sc.opt_id(opt)} {wkind}", ratios)
    assert max(ratios.values()) <= 1., ratios


_FACTOR_RATIO = {}          # left by test_every_bound, so the reference and the factor are computed once


@pytest.mark.parametrize("name,wkind,opt", BOUND_CASES, ids=BOUND_IDS)
def test_factor_residual(name, wkind, opt):
    """|A_p - L^ L^^T| <= 4 gamma_{n+1} (|L^||L^|^T + P |B|^T D^-1 |B| P^T), componentwise on the lower triangle,
    on its own: the bound that only a panel step by substitution meets (see test_every_bound)."""
    key = (name, wkind, sc.opt_id(opt))
    if key not in _FACTOR_RATIO:
        ch = sc.Chol(name, dict(opt, poison=1))
        assert ch.factor(sc.w_vector(name, wkind))[0] == 0
        _FACTOR_RATIO[key] = sc.reference(name, wkind, opt).factor_ratio(ch.dense(0))
        ch.close()
    print(f"device {name} {sc.opt_id(opt)} {wkind}: factor={_FACTOR_RATIO[key]:.3g}")
    assert _FACTOR_RATIO[key] <= 1., _FACTOR_RATIO[key]


def test_no_derivative_gives_zero_trace():
    ch = sc.Chol("e1", {"poison": 1}, deriv=False)
    assert ch.factor(sc.w_vector("e1", "bern"))[0] == 0
    tr_bdb, tr_da, _ = ch.selected_inverse()
    assert tr_da == 0. and np.isfinite(tr_bdb)
    ch.close()


POISON_CASES = [(name, opt) for name in ("b130", "c", "e1", "e2", "f") for opt in sc.case_options(name)]


@pytest.mark.parametrize("name,opt", POISON_CASES, ids=[f"{n}-{sc.opt_id(o)}" for n, o in POISON_CASES])
def test_poison(name, opt):
    """NaN in every scratch and output buffer before each phase changes no bit of any output (zeros instead),
    and every output is finite: every value a kernel reads was written first, or is masked by a select."""
    plan = sc.plan_of(name, opt)
    out = []
    for poison in (1, 0):
        ch = sc.Chol(name, dict(opt, poison=poison))
        out.append(run_all(ch, name, "pois", (1, 5, 65)))
        ch.close()
    assert_finite(out[0], plan)
    assert_same_bits(out[0], out[1], "NaN against zero poison")


@pytest.mark.parametrize("name", ["c", "f", "g"])
def test_k64_kernel_gives_the_same_bits(name):
    out = []
    for k64 in (1, 0):
        ch = sc.Chol(name, {"k64": k64, "poison": 1})
        out.append(run_all(ch, name, "bern", (3, 65)))
        ch.close()
    assert_same_bits(out[0], out[1], "k64 = 1 against 0")


@pytest.mark.parametrize("name,opt", [("c", {}), ("f", {"leaf": 8}), ("f", {"small_panel": 0}), ("e1", {})],
                         ids=["c", "f-leaf8", "f-tiled", "e1"])
def test_same_bits(name, opt):
    ts = (1, 3, 4, 5, 64, 65)
    ch = sc.Chol(name, opt)          # the buffers as production leaves them
    first = run_all(ch, name, "bern", ts)
    # a repeated Factor + solves + SelectedInverse on the same object
    assert_same_bits(first, run_all(ch, name, "bern", ts), "repeat")
    # x aliasing b on the device
    assert_same_bits(first, run_all(ch, name, "bern", ts, inplace=1), "in place")
    # an absent SelectedInverse output changes no bit of the others
    for want in ((True, False, False), (False, True, False), (False, False, True), (False, False, False)):
        assert_same_bits(first, run_all(ch, name, "bern", (1,), want=want), f"outputs {want}")
    # t = 3, then 65, then 3: the schedule cache and the scratch regrowth
    ch2 = sc.Chol(name, opt)
    assert ch2.factor(sc.w_vector(name, "bern"))[0] == 0
    seq = [ch2.solve(sc.Chol.SOLVE_MULTI, sc.rhs(name, t), t) for t in (3, 65, 3)]
    assert np.array_equal(seq[0], seq[2]) and np.array_equal(seq[0], first["solve"][3])
    assert np.array_equal(seq[1], first["solve"][65])
    # W = null against an array of zeros
    a = run_all(ch2, name, "none", (1, 3))
    info, logdet = ch2.factor(np.zeros(ch2.n))
    assert info == 0 and logdet == a["logdet"] and np.array_equal(ch2.dense(0), a["L"])
    assert np.array_equal(ch2.solve(sc.Chol.SOLVE, sc.rhs(name, 1), 1), a["solve1"])
    ch.close()
    ch2.close()


@pytest.mark.parametrize("name", ["b64", "b128", "b130", "f"])
def test_bad_pivots(name):
    """A pivot that is zero, negative, NaN or +inf: a normal return with Info() > 0, wherever it sits (the label
    eliminated first, in the middle of the root, last); +inf as the last pivot of a full 64-block leaves L finite;
    the next factorization with a good W reports 0 (the counter is reset by the first assembly launch) and
    reproduces the first factor bit for bit."""
    plan = sc.plan_of(name, sc.case_options(name)[0])
    n, perm = plan["n"], plan["perm"]
    ref = sc.reference(name, "bern", sc.case_options(name)[0])
    W = sc.w_vector(name, "bern")
    ch = sc.Chol(name, dict(sc.case_options(name)[0], poison=1))
    info, logdet = ch.factor(W)
    assert info == 0
    L0 = ch.dense(0)
    root0 = int(plan["sfirst"][plan["nsup"] - 1])
    positions = dict(first=0, middle=(root0 + n) // 2, last=n - 1)
    for where, k in positions.items():
        pivot = float(ref.L[k, k]) ** 2          # the Schur complement's diagonal at elimination position k
        for what, value in (("negative", W[perm[k]] - 2. * pivot), ("nan", np.nan), ("inf", np.inf)):
            Wb = W.copy()
            Wb[perm[k]] = value
            info, _ = ch.factor(Wb)
            assert info > 0, (where, what)
            if what == "inf" and where == "last" and n % 64 == 0:
                assert np.all(np.isfinite(ch.dense(0))), "+inf as the last pivot of a full block left a NaN column"
        info, ld = ch.factor(W)
        assert info == 0 and ld == logdet and np.array_equal(ch.dense(0), L0), where
    # zero: label n - 1 is nobody's neighbour, so its diagonal entry of A is the single product D^-1_{n-1} and
    # W = -D^-1_{n-1} makes it exactly 0: the pivot is 0 minus the squares of the row's earlier entries
    Wb = W.copy()
    Wb[n - 1] = -sc.values(name)[1][n - 1]
    assert ch.factor(Wb)[0] > 0
    info, ld = ch.factor(W)
    assert info == 0 and ld == logdet and np.array_equal(ch.dense(0), L0)
    ch.close()


def test_exactly_zero_pivot():
    ch = sc.Chol("a1", {"poison": 1})
    assert ch.factor(-sc.values("a1")[1])[0] > 0          # A = D^-1_0 + W = 0
    assert ch.factor(None)[0] == 0
    ch.close()


def test_argument_checks():
    """wrong extents and a solve before a factorization are error returns with a message, never a device access"""
    import ctypes
    lib = sc._lib()
    ch = sc.Chol("a3")
    n, m = ch.n, ch.m
    d = lambda k: np.zeros(k)
    err = lambda fn: fn in sc.last_error()
    assert lib.GPB_TestSparseCholSolve(ch.h, 0, 1, 0, sc._dp(d(n)), n, sc._dp(d(n)), n) == -1
    assert "before a factorization" in sc.last_error()
    assert lib.GPB_TestSparseCholSelectedInverse(ch.h, None, None, None, 0) == -1
    assert "before a factorization" in sc.last_error()
    assert lib.GPB_TestSparseCholDense(ch.h, 0, sc._dp(d(n * n)), n * n) == -1
    assert lib.GPB_TestSparseCholSetB(ch.h, sc._dp(d(n * m)), n * m - 1, sc._dp(d(n)), n, None, 0, None, 0) == -1
    assert err("GPB_TestSparseCholSetB")
    assert lib.GPB_TestSparseCholSetB(ch.h, sc._dp(d(n * m)), n * m, sc._dp(d(n)), n, sc._dp(d(n * m)), n * m, None, 0) == -1
    assert err("GPB_TestSparseCholSetB")
    info = ctypes.c_int(0)
    assert lib.GPB_TestSparseCholFactor(ch.h, sc._dp(d(n + 1)), n + 1, ctypes.byref(info), None) == -1
    assert err("GPB_TestSparseCholFactor")
    assert ch.factor(None)[0] == 0
    for op, t, bl, xl in ((0, 2, 2 * n, 2 * n), (1, 0, 0, 0), (4, 1, n, n), (1, 2, 2 * n, n), (2, 2, n, 2 * n)):
        assert lib.GPB_TestSparseCholSolve(ch.h, op, t, 0, sc._dp(d(2 * n)), bl, sc._dp(d(2 * n)), xl) == -1
        assert err("GPB_TestSparseCholSolve")
    assert lib.GPB_TestSparseCholSelectedInverse(ch.h, None, None, sc._dp(d(n)), n - 1) == -1
    assert err("GPB_TestSparseCholSelectedInverse")
    assert lib.GPB_TestSparseCholDense(ch.h, 1, sc._dp(d(n * n)), n * n) == -1       # no selected inverse yet
    assert lib.GPB_TestSparseCholDense(ch.h, 3, sc._dp(d(n * n)), n * n) == -1
    assert lib.GPB_TestSparseCholDense(ch.h, 0, sc._dp(d(n * n)), n * n - 1) == -1
    assert err("GPB_TestSparseCholDense")
    h = ctypes.c_void_p()
    X, nbr = sc.graph("a3")
    bad = nbr.copy()
    bad[2, 1] = 2
    o = sc._opts({})
    assert lib.GPB_TestSparseCholCreate(3, 5, sc._ip(bad), 15, 2, sc._dp(X), 6, sc._ip(o, ctypes.c_int64),
                                        ctypes.byref(h)) == -1 and err("GPB_TestSparseCholCreate")
    ch.close()
