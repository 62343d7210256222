"""CPU: the sparse Cholesky's plan and the bounds of tests/sparse_chol_cases.py, without a GPU.

* numpy.longdouble has the 64-bit significand the references rely on;
* the plan (GPB_TestSparseCholPlan, host only) is a valid supernodal elimination structure on every case and on
  three degenerate inputs, and contains the exact symbolic Cholesky;
* every case reaches the path it is meant to reach (plan statistics and op counts of the schedules);
* a plain float64 numpy / scipy implementation of every operation, in the device's elimination order, meets every
  bound the kernels are held to (run with -s for the ratios);
* the hooks' argument checks reject bad extents before any device call.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_chol_cases as sc  # noqa: E402
from gpboost_amd import synthetic  # noqa: E402

CASE_OPTS = [(name, opt) for name in sc.CASES for opt in sc.case_options(name)]
IDS = [f"{name}-{sc.opt_id(opt)}" for name, opt in CASE_OPTS]


def test_longdouble_has_64_bit_significand():
    assert np.finfo(np.longdouble).nmant >= 63
    one = np.longdouble(1)
    assert one + np.longdouble(2.0) ** -63 != one


# ------------------------------------------------------------------------------------------------ plan invariants
def symbolic_cholesky(pat):
    """lower pattern of the Cholesky factor of a symmetric boolean pattern, by dense elimination"""
    P = pat.copy()
    n = P.shape[0]
    for k in range(n):
        r = np.flatnonzero(P[k + 1:, k]) + k + 1
        P[np.ix_(r, r)] = True
    return np.tril(P)


def check_plan(plan, nbr):
    n, nsup = plan["n"], plan["nsup"]
    perm, sfirst, sparent, rptr, rows = (plan[k] for k in ("perm", "sfirst", "sparent", "rptr", "rows"))
    assert sorted(perm.tolist()) == list(range(n)), "perm is not a permutation"
    assert sfirst[0] == 0 and sfirst[nsup] == n and np.all(np.diff(sfirst) >= 1), "sfirst does not partition 0..n"
    col_sup = np.repeat(np.arange(nsup), np.diff(sfirst))
    level = np.empty(nsup, dtype=int)
    for l in range(plan["levels"]):
        level[plan["lvl_sup"][plan["lvl_ptr"][l]:plan["lvl_ptr"][l + 1]]] = l
    assert sorted(plan["lvl_sup"].tolist()) == list(range(nsup))
    for s in range(nsup):
        R = rows[rptr[s]:rptr[s + 1]]
        assert np.all(np.diff(R) > 0), f"rows of supernode {s} not ascending"
        assert R.size == 0 or (R[0] >= sfirst[s + 1] and R[-1] < n), f"rows of supernode {s} not below its columns"
        if R.size == 0:
            assert sparent[s] == -1
            continue
        p = sparent[s]
        assert p == col_sup[R[0]], f"parent of supernode {s} is not the supernode of its first row"
        own = set(range(sfirst[p], sfirst[p + 1])) | set(rows[rptr[p]:rptr[p + 1]].tolist())
        assert set(R.tolist()) <= own, f"rows of supernode {s} not contained in its parent"
        assert level[s] < level[p], f"supernode {s} is not on a lower level than its parent"
    ns, nr, fs = sc.sup_stats(plan)
    assert plan["nnz_l"] == int((ns * (ns + 1) // 2 + ns * nr).sum())
    assert plan["max_fs"] == int(fs.max()) and plan["max_ns"] == int(ns.max())
    struct = sc.structure(plan)
    assert plan["nnz_l"] == int(struct.sum())
    if n <= 400:
        pat = np.zeros((n, n), dtype=bool)
        m = nbr.shape[1]
        for r in range(n):
            idx = np.concatenate([[r], nbr[r, :min(r, m)][nbr[r, :min(r, m)] >= 0]])
            pat[np.ix_(idx, idx)] = True
        fill = symbolic_cholesky(pat[np.ix_(perm, perm)])
        assert not np.any(fill & ~struct), "the structure misses an entry of the symbolic Cholesky"


@pytest.mark.parametrize("name,opt", CASE_OPTS, ids=IDS)
def test_plan_invariants(name, opt):
    check_plan(sc.plan_of(name, opt), sc.graph(name)[1])


def _degenerate(kind):
    if kind == "identical":
        X = np.full((120, 2), 0.25)
        return X, sc.knn_graph(X, 7), {}
    if kind == "collinear":
        X = synthetic.bench_coords(150)
        X[:, 1] = 2. * X[:, 0] + 1.
        return X, sc.knn_graph(X, 7), {}
    X = synthetic.bench_coords(300)
    return X, sc.knn_graph(X, 10), {"leaf": 1}


@pytest.mark.parametrize("kind", ["identical", "collinear", "leaf1"])
def test_plan_invariants_degenerate(kind):
    X, nbr, opt = _degenerate(kind)
    for t, mode in ((1, 0), (3, 1), (65, 2)):
        check_plan(sc.hook_plan(X, nbr, opt, t, mode), nbr)


# ------------------------------------------------------------------------------------------------ paths
def test_case_reaches_its_path():
    P = sc.plan_of
    for name in ("a1", "a2", "a3"):         # single supernode, n <= m, no GEMM task in the factorization
        p = P(name)
        assert p["nsup"] == 1 and p["factor"]["Gemm"] == 0 and p["factor"]["Diag"] == 1
    for name, blocks, last in (("b63", 1, 63), ("b64", 1, 64), ("b65", 2, 1), ("b128", 2, 64), ("b130", 3, 2),
                               ("b192", 3, 64), ("b254", 4, 62)):
        p = P(name)
        n = sc.CASES[name][0]
        assert p["nsup"] == 1 and p["max_ns"] == n and p["factor"]["Diag"] == blocks == (n + 63) // 64
        assert n - 64 * (blocks - 1) == last
        assert p["solve"]["FSolve1"] == 1 and p["solve"]["BSolve1"] == 1 and p["solve"]["FwdVec"] == 0
    p = P("c")          # one supernode of 260, fs ns > 65536: the fused tiled t = 1 form, five blocks, ragged 4
    assert p["nsup"] == 1 and p["max_fs"] == 260 and 260 * 260 > 65536 and p["factor"]["Diag"] == 5
    s = p["solve"]
    assert s["FwdVec"] == 5 and s["CopyXS"] == 1 and s["BwdVecPart"] == 4 and s["BwdVecFin"] == 5 and s["FSolve1"] == 0
    s = P("c", {"fuse_vec": 0})["solve"]         # the two-launch GEMM form
    assert s["FwdVec"] == 0 and s["FSolve1"] == 0 and s["Gemm"] == 18 and s["Reduce"] == 4
    s = P("c", {"small_panel": 1 << 20})["solve"]      # the single-workgroup sweep on the same matrix
    assert s["FSolve1"] == 1 and s["BSolve1"] == 1 and s["FwdVec"] == 0 and s["Gemm"] == 0
    s = P("c", {}, 1, 2)["solve"]
    assert s["LoadV"] == 1 and s["BwdVecFin"] == 5
    p = P("d")          # many small supernodes
    assert p["nsup"] >= 70 and p["max_fs"] <= 32 and p["levels"] >= 5
    roots = lambda p: int((p["sparent"] < 0).sum())
    assert roots(P("e1")) > 1 and roots(P("e2")) >= 1
    assert np.all(sc.graph("e1")[1][::7] == -1) and np.all(sc.graph("e2")[1][:, 1::2] == -1)
    for opt, nsup in (({"leaf": 64}, 16), ({"leaf": 8}, 27)):       # the general case
        p = P("f", opt)
        ns, nr, fs = sc.sup_stats(p)
        kids = np.bincount(p["sparent"][p["sparent"] >= 0], minlength=p["nsup"])
        assert p["nsup"] == nsup and p["levels"] >= 4 and kids.max() >= 2      # extend-add over several children
        assert ns[p["sparent"] < 0].max() > 128                                  # a root of three or more blocks
        assert np.any((nr > 0) & (ns > 64)) and np.any((nr > 0) & (ns <= 64))    # update blocks with K > 64 and K <= 64
        assert p["solve"]["FSolve1"] == p["levels"] and p["solve"]["FwdVec"] == 0
    s = P("f", {"leaf": 64, "small_panel": 0})["solve"]       # every level in the tiled t = 1 form
    assert s["FSolve1"] == 0 and s["BSolve1"] == 0 and s["FwdVec"] > 0 and s["BwdVecFin"] > 0 and s["GatherX"] > 0
    p = P("g")          # banded: more than 256 rows below a block
    assert sc.fr_max(p) > 256 and p["solve"]["fin_chunks"] == 2
    assert P("g", {}, 5, 0)["solve"]["nslices"] == 2 and P("g", {}, 5, 2)["solve"]["nslices"] == 2
    assert P("g", {}, 1, 2)["solve"]["fin_chunks"] == 2
    p = P("h")          # more than 512 rows below a block: two split-K slices in the selected inverse
    assert sc.fr_max(p) > 512 and p["selinv"]["nslices"] == 2
    for name in ("c", "f"):     # more than one right-hand side: the tiled GEMM form at every count
        for t in sc.RHS_COUNTS[1:]:
            for mode in (0, 1, 2):
                s = P(name, sc.case_options(name)[0], t, mode)["solve"]
                assert s["Gemm"] > 0 and s["FSolve1"] == 0 and s["BSolve1"] == 0 and s["FwdVec"] == 0


# ------------------------------------------------------------------------------------------------ float64 stand-in
def _wkinds(name):
    return ("bern",) if name in ("g", "h") else sc.W_KINDS


FLOAT64_CASES = [(name, opt, wk) for name, opt in CASE_OPTS for wk in _wkinds(name)
                 if opt in ({}, {"leaf": 64}, {"leaf": 8})]          # the other option sets change no elimination order


@pytest.mark.parametrize("name,opt,wkind", FLOAT64_CASES,
                         ids=[f"{n}-{sc.opt_id(o)}-{w}" for n, o, w in FLOAT64_CASES])
def test_float64_meets_every_bound(name, opt, wkind):
    plan = sc.plan_of(name, opt)
    ref = sc.reference(name, wkind, opt)
    ts = (1, 5) if name in ("g", "h") else ((1, 3, 65) if name in ("c", "f") else (1, 3))
    ratios = sc.result_ratios(ref, plan, sc.float64_results(name, wkind, plan, ts))
    sc.report(f"float64 {name} {sc.opt_id(opt)} {wkind} cond_inf={ref.cond_inf():.2g}", ratios)
    assert max(ratios.values()) <= 1., ratios


def test_same_plan_across_option_sets():
    """small_panel, fuse_vec, k64 and poison change schedules and launches, never the elimination order"""
    for name, opts in sc.CASE_OPTIONS.items():
        for opt in opts:
            base = {k: v for k, v in opt.items() if k == "leaf"}
            assert np.array_equal(sc.plan_of(name, opt)["perm"], sc.plan_of(name, base)["perm"])


# ------------------------------------------------------------------------------------------------ argument checks
def test_plan_hook_rejects_bad_arguments():
    X, nbr = sc.graph("a3")
    bad = nbr.copy()
    bad[2, 0] = 2          # nbr[i][r] >= i
    low = nbr.copy()
    low[2, 1] = -2
    for kw, arr in ((dict(n=0), nbr), (dict(m=255), nbr), (dict(m=0), nbr), (dict(nbr_len=14), nbr),
                    (dict(x_len=5), nbr), ({}, bad), ({}, low)):
        with pytest.raises(sc.HookError, match="GPB_TestSparseCholPlan"):
            sc.hook_plan(X, arr, **kw)
    with pytest.raises(sc.HookError, match="GPB_TestSparseCholPlan"):
        sc.hook_plan(X, nbr, t=0)
    X255 = synthetic.bench_coords(300)
    with pytest.raises(sc.HookError, match="m = 255"):
        sc.hook_plan(X255, np.full((300, 255), -1, dtype=np.int32))


def test_create_hook_rejects_bad_arguments_before_any_device_call():
    """the checks come first, so the error names the argument even on a machine without a GPU"""
    import ctypes
    X, nbr = sc.graph("a3")
    lib = sc._lib()
    h = ctypes.c_void_p()
    bad = nbr.copy()
    bad[1, 0] = 1
    o = sc._opts({})
    for n, m, arr, nbr_len, x_len, what in ((3, 5, bad, 15, 6, "nbr"), (3, 255, nbr, 15, 6, "m = 255"),
                                            (3, 5, nbr, 14, 6, "nbr holds"), (3, 5, nbr, 15, 7, "X holds"),
                                            (0, 5, nbr, 15, 6, "n = 0")):
        ret = lib.GPB_TestSparseCholCreate(n, m, sc._ip(np.ascontiguousarray(arr)), nbr_len, 2, sc._dp(X), x_len,
                                           sc._ip(o, ctypes.c_int64), ctypes.byref(h))
        assert ret == -1 and not h.value
        assert "GPB_TestSparseCholCreate" in sc.last_error() and what in sc.last_error(), sc.last_error()
    for fn, args in ((lib.GPB_TestSparseCholSolve, (None, 0, 1, 0, None, 0, None, 0)),
                     (lib.GPB_TestSparseCholFactor, (None, None, 0, None, None)),
                     (lib.GPB_TestSparseCholDense, (None, 0, None, 0))):
        assert fn(*args) == -1 and "handle is NULL" in sc.last_error()
