"""GPU: the grouped random-effects engine element by element through the GPB_TestGrouped* hooks
(csrc/grouped_test.cpp: the production launch functions of csrc/grouped_kernels.hip on a GroupedRE's own structure
and chunk plans, GroupedRE::Precond and SolveVec, GroupedLaplace::Assemble and the gradient kernels of
csrc/grouped_laplace.hip) against the longdouble references and the derived bounds of tests/grouped_ops_cases.py
(none tuned to a kernel; tests/test_grouped_ops_reference.py holds float64 stand-ins to the same bounds and shows
that single-entry defects exceed them). Outputs, scratch and the chunk partials start as NaN between guard bands,
the ld - M padding of every dense input holds NaN. Run with -s for the largest error / bound ratio of every kernel.

Bitwise claims checked here: gre_dense_build, gre_residual and the glp_vec forms; two runs give the same bits; a
column of a block does not depend on the other columns (one input column NaN: that output column NaN, every other
bit unchanged); GroupedRE::Precond gives the bits of launch_gre_ssor; rows of E above a point's smallest level
index are exactly 0, a point without a seen level has variance exactly 0, the padding of E keeps its NaN."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grouped_ops_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
LD = gc.LD
_worst = {}


def setup_module(module):
    gc.assert_longdouble()


def teardown_module(module):
    gc.free_handles()
    for key in sorted(_worst):
        print(f"[grouped ops] largest error / bound, {key}: {_worst[key]:.3g}")


def _note(key, v):
    _worst[key] = max(_worst.get(key, 0.), float(v))
    return v


def _ratio(key, got, ref, bnd, where):
    assert np.isfinite(got).all(), (key, where, "not finite or not written")
    r = _note(key, gc.max_ratio(np.abs(got.astype(LD) - ref), bnd))
    print(f"{key} {where}: {r:.3g}")
    assert r < 1., (key, where, r)


def _same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def _twice(hook):
    """every operation runs twice and gives the same bits"""
    def run(*a, **kw):
        first, second = hook(*a, **kw), hook(*a, **kw)
        for x, y in zip(first, second):
            assert x is None or _same_bits(x, y), (hook.__name__, a[:2], "two runs differ")
        return first
    return run


apply_hook, small_hook, dense_hook, laplace_hook = (_twice(h) for h in (gc.apply_hook, gc.small_hook, gc.dense_hook,
                                                                        gc.laplace_hook))


# ------------------------------------------------------------------------------------------------ structure
INFO_CASES = gc.BLOCK_CASES + tuple((d, 1) for d in gc.NAMED if d not in gc.BLOCK_DESIGNS)


@pytest.mark.parametrize("name,t", INFO_CASES)
def test_engine_holds_the_structure_and_the_plans_of_the_design(name, t):
    s = gc.structure(name)
    q = gc.info_hook(name, t)
    assert (q["M"], q["nnz"], q["n"], q["K"]) == (s.M, s.nnz, s.n, s.K)
    assert q["tc"] == gc.gre_tc(t) and q["L"] == gc.chunk_len(q["tc"])
    for key in ("cum", "rowptr", "split", "col", "obs_ptr", "obs"):
        assert np.array_equal(q[key], getattr(s, key)), key
    assert np.array_equal(q["val"], s.val) and np.array_equal(q["cnt"], s.cnt)
    plans, lq, uq = gc.chunk_plan(s, t)
    for kind, key in enumerate(gc.KINDS):
        for got, want in zip(q["plan_" + key], plans[kind]):
            assert np.array_equal(got, want), key
    assert np.array_equal(q["lower_q"], lq) and np.array_equal(q["upper_q"], uq)
    _, counts = gc.seg_plan(s)
    assert (q["long_levels"], q["level_chunks"], q["long_all"], q["chunks_all"]) == counts


# ------------------------------------------------------------------------------------------------ products
PRODUCTS = ("apply", "apply_lower", "lds_mult", "upper")
KERNEL = {"apply": "gre_chunk/combine apply", "apply_lower": "gre_chunk/combine apply_lower",
          "lds_mult": "gre_chunk/combine lds_mult", "upper": "gre_chunk/combine upper"}


def _models(name, t):
    return (0, 1) if (name, t) in gc.MODEL_CASES else (0,)


def _run_product(name, op, t, q, X):
    # val = None for the model's own counts: the engine's values, not a copy
    val = None if q.get("model") else q["val"]
    return apply_hook(name, op, t, val, q["D"], q["dis"], X)[0]


@pytest.mark.parametrize("name,t", gc.BLOCK_CASES)
def test_products_meet_their_bounds_and_the_exact_claims(name, t):
    s = gc.structure(name)
    for model in _models(name, t):
        q = dict(gc.block_inputs(name, t, model), model=model)
        for op in PRODUCTS:
            ref, bnd = gc.product_reference(s, op, q["val"], q["D"], q["dis"], q["X"])
            got = _run_product(name, op, t, q, q["X"])
            _ratio(KERNEL[op], got, ref, bnd, f"{name} t={t} model={model}")
            if t > 1 and not model:
                c = t // 2
                Xn = q["X"].copy()
                Xn[:, c] = np.nan
                gn = _run_product(name, op, t, q, Xn)
                keep = np.arange(t) != c
                assert np.isnan(gn[:, c]).all() and _same_bits(gn[:, keep], got[:, keep]), (name, t, op, "columns mix")


@pytest.mark.parametrize("name,t", gc.BLOCK_CASES)
def test_ssor_sweeps_residual_and_forward_error_and_the_production_wiring(name, t):
    s = gc.structure(name)
    for model in _models(name, t):
        q = gc.block_inputs(name, t, model)
        val = None if model else q["val"]
        X, Z = apply_hook(name, "ssor", t, val, q["D"], q["dis"], q["X"])
        assert np.isfinite(X).all() and np.isfinite(Z).all(), (name, t, "not finite or not written")
        ratios = gc.ssor_ratios(s, q["val"], q["D"], q["dis"], q["X"], X, Z)
        for key, r in zip(("gre_ssor residual fwd", "gre_ssor residual bwd", "gre_ssor error fwd", "gre_ssor error bwd"),
                          ratios):
            print(f"{key} {name} t={t} model={model}: {r:.3g}")
            assert _note(key, r) < 1., (name, t, model, key, r)
        Xp, Zp = apply_hook(name, "precond", t, val, q["D"], q["dis"], q["X"])
        assert _same_bits(X, Xp) and _same_bits(Z, Zp), (name, t, "GroupedRE::Precond differs from launch_gre_ssor")
        if t > 1 and not model:
            c = t - 1
            Rn = q["X"].copy()
            Rn[:, c] = np.nan
            Xn, Zn = gc.apply_hook(name, "ssor", t, val, q["D"], q["dis"], Rn)
            assert np.isnan(Xn[:, c]).all() and np.isnan(Zn[:, c]).all()
            assert _same_bits(Xn[:, :c], X[:, :c]) and _same_bits(Zn[:, :c], Z[:, :c]), (name, t, "columns mix")


def test_hooks_refuse_wrong_extents_before_any_launch():
    q = gc.block_inputs("tiny15", 3, 0)
    with pytest.raises(gc.HookError):
        gc.apply_hook("tiny15", "apply", 2, q["val"], q["D"], None, q["X"])          # M x 3 block given as t = 2
    with pytest.raises(gc.HookError):
        gc.apply_hook("tiny15", "apply", 3, q["val"], q["D"], None, q["X"][:-1].copy())   # a row short
    with pytest.raises(gc.HookError):
        gc.small_hook("tiny15", "zty", [np.zeros(4)], [6])                           # y shorter than n
    with pytest.raises(gc.HookError):
        gc.dense_hook("dense63", "inv_diag", 62, [np.zeros((63, 63))], [63])         # ld < M


# ------------------------------------------------------------------------------------------------ small kernels
@pytest.mark.parametrize("name", gc.SMALL_DESIGNS)
def test_small_kernels(name):
    s = gc.structure(name)
    q = gc.small_inputs(name)
    zty, = small_hook(name, "zty", [q["y"]], [s.M])
    ref, bnd = gc.list_sums(s.obs_ptr, s.obs, q["y"])
    _ratio("gre_zty", zty, ref, bnd, name)
    assert (zty[s.cnt == 0] == 0).all()
    D, dis, sums = small_hook(name, "diag", [q["cnt"], q["tau"]], [s.M, s.M, 2 * s.K])
    ref = gc.diag_reference(s, q["cnt"], q["tau"])
    for key, got in (("D", D), ("dis", dis), ("sums", sums)):
        _ratio("gre_diag " + key, got, ref[key][0], ref[key][1], name)
    for m in sorted({1, s.M} | ({255, 256, 257, 1000} if name == "sizes" else set())):
        u, sm = small_hook(name, "single", [q["zty"][:m], q["cnt"][:m], q["D"][:m]], [m, 2])
        ref = gc.single_reference(q["zty"][:m], q["cnt"][:m], q["D"][:m])
        _ratio("gre_single u", u, ref["u"][0], ref["u"][1], f"{name} m={m}")
        _ratio("gre_single sums", sm, ref["sums"][0], ref["sums"][1], f"{name} m={m}")
        assert _same_bits(u, q["zty"][:m] / q["D"][:m])                              # one correctly rounded division
    for ln in (1, 255, 256, 257, s.M):
        a, b = np.resize(q["zty"], ln), np.resize(q["ysgn"], ln)
        r, = small_hook(name, "residual", [a, b], [ln])
        assert _same_bits(r, a - b), (name, ln)


# ------------------------------------------------------------------------------------------------ dense readers
@pytest.mark.parametrize("padded", (False, True))
@pytest.mark.parametrize("name", gc.DENSE_DESIGNS)
def test_dense_factor_readers(name, padded):
    s = gc.structure(name)
    q = gc.dense_inputs(name)
    M, K = s.M, s.K
    ld = gc.dense_ld(name, padded)
    where = f"{name} ld={ld}"
    for val in (q["val"], None):                                     # a caller's values, the model's counts
        A, = dense_hook(name, "build", ld, [val, q["D"]], [ld * M])
        want = gc.dense_build_expected(s, s.val if val is None else val, q["D"], ld)
        assert _same_bits(A.reshape(M, ld), want), (where, "dense build")
    Lz = np.tril(q["Li"])
    out, = dense_hook(name, "inv_diag", ld, [q["Li"]], [M])       # NaN above the diagonal: finite = never read
    ref, bnd = gc.inv_diag_reference(Lz)
    _ratio("gre_inv_diag", out, ref, bnd, where)
    for npts in gc.NPS:
        idx = q["idx"][:npts]
        (Er, eb), (vr, vb) = gc.pred_reference(s, Lz, idx)
        E, = dense_hook(name, "pred_e", ld, [q["Li"]], [ld * npts], idx=idx)
        E = E.reshape(npts, ld)
        assert np.isnan(E[:, M:]).all(), (where, "the padding of E was written")
        _ratio("gre_pred_cols E", E[:, :M].T, Er, eb, f"{where} np={npts}")
        var, = dense_hook(name, "pred_var", ld, [q["Li"]], [npts], idx=idx)
        _ratio("gre_pred_cols var", var, vr, vb, f"{where} np={npts}")
        lo = np.where(idx >= 0, idx, M).min(axis=1)
        for p in range(npts):
            assert (E[p, :lo[p]] == 0).all(), (where, p, "a row above the smallest level index is not 0")
            if lo[p] == M:
                assert (E[p, :M] == 0).all() and var[p] == 0, (where, p, "a point without a seen level")
    part, dg = dense_hook(name, "fisher", ld, [q["sc"], q["Ainv"]], [M * K, M])
    (pr, pb), (dr, db) = gc.fisher_reference(s, q["sc"], q["Ainv"])
    _ratio("gre_fisher_cols part", part.reshape(M, K), pr, pb, where)
    _ratio("gre_fisher_cols diag", dg, dr, db, where)


# ------------------------------------------------------------------------------------------------ Laplace kernels
@pytest.mark.parametrize("name", ("seg", "eight", "gap"))
def test_segmented_sums(name):
    s = gc.structure(name)
    w = gc.small_inputs(name)["w"]
    for diag_only in (1, 0):
        ref, bnd = gc.assemble_reference(s, w, bool(diag_only))
        out, = laplace_hook(name, "assemble", [w], [ref.size], sub=diag_only)
        _ratio("glp_seg kernels", out, ref, bnd, f"{name} diag_only={diag_only}")
        assert (out[:s.M][s.cnt == 0] == 0).all()


@pytest.mark.parametrize("name", gc.Q_DESIGNS + ("qbig",))
def test_q_kernel_and_the_fixed_effect_gradient(name):
    s = gc.structure(name)
    q = gc.q_inputs(name)
    K, n, M = s.K, s.n, s.M
    ld = M + 3
    for aux in (0, 1):
        (dr, db), (sr, sb) = gc.q_reference(s, q["Ainv"], q["D"], q["W"], q["dW"], q["Wa"] if aux else None)
        ins = [q["Ainv"], q["D"], q["W"], q["dW"], q["Wa"] if aux else None]
        dwq, sums = laplace_hook(name, "q", ins, [n, K + aux], sub=aux, ld=ld)
        _ratio("glp_q_kernel dwq", dwq, dr, db, f"{name} aux={aux}")
        _ratio("glp_q_kernel + glp_finish sums", sums, sr, sb, f"{name} aux={aux}")
    ref, bnd = gc.grad_f_reference(s, q["d1"], q["dwq"], q["W"], q["v"])
    out, = laplace_hook(name, "grad_f", [q["d1"], q["dwq"], q["W"], q["v"]], [n])
    _ratio("glp_grad_f_kernel", out, ref, bnd, name)


@pytest.mark.parametrize("name,t", gc.TRACE_CASES)
def test_row_trace_kernel(name, t):
    s = gc.structure(name)
    q = gc.trace_inputs(name, t)
    ref, bnd = gc.row_trace_reference(s, t, q["U"], q["V"], q["dW"])
    out, = laplace_hook(name, "row_trace", [q["U"], q["V"], q["dW"]], [s.n], t=t)
    _ratio("glp_row_trace_kernel", out, ref, bnd, f"{name} t={t}")


@pytest.mark.parametrize("name", gc.SMALL_DESIGNS)
def test_vector_forms_are_exact_and_effect_dots_meet_their_bounds(name):
    s = gc.structure(name)
    q = gc.small_inputs(name)
    for form in range(5):
        y = q["ysgn"] if form in (1, 2, 3) else None
        out, = laplace_hook(name, "vec", [q["sigma2"], q["x"], y], [s.M], sub=form, alpha=q["alpha"])
        exp = gc.vec_expected(s, form, q["sigma2"], q["alpha"], q["x"], y)
        assert any(_same_bits(out, e) for e in exp), (name, form, "not the bits of the IEEE operations")
    for mode in range(4):
        y = q["ysgn"] if mode in (0, 3) else None
        ref, bnd = gc.effect_dots_reference(s, mode, q["x"], y)
        out, = laplace_hook(name, "effect_dots", [q["sigma2"], q["x"], y], [s.K], sub=mode)
        _ratio(f"glp_effect_dots_kernel mode {mode}", out, ref, bnd, name)


# ------------------------------------------------------------------------------------------------ SolveVec
@pytest.mark.parametrize("model", (0, 1))
@pytest.mark.parametrize("name", gc.SOLVE_DESIGNS)
def test_solve_vec_true_residual_and_warm_start(name, model):
    s = gc.structure(name)
    q = gc.solve_inputs(name, model)
    val = None if model else q["val"]
    u, its = gc.solve_hook(name, val, None, q["D"], q["dis"], q["rhs"], None, 1000, gc.DELTA)
    assert np.isfinite(u).all() and 0 < its < 1000
    u2, its2 = gc.solve_hook(name, val, None, q["D"], q["dis"], q["rhs"], None, 1000, gc.DELTA)
    assert its2 == its and _same_bits(u, u2), (name, "two runs differ")
    res = gc.true_residual(s, q["val"], q["D"], q["rhs"], u)
    lim = gc.DELTA + gc.solve_drift(s, q["val"], q["D"], u, its)
    print(f"SolveVec {name} model={model}: cold {its} its, ||rhs - A u|| = {res:.3g}, limit {lim:.3g}")
    assert _note("SolveVec true residual / (delta + drift)", res / lim) < 1.
    u0 = u * (1. + 1e-3 * np.cos(np.arange(s.M)))
    uw, itw = gc.solve_hook(name, val, None, q["D"], q["dis"], q["rhs"], u0, 1000, gc.DELTA)
    res = gc.true_residual(s, q["val"], q["D"], q["rhs"], uw)
    lim = gc.DELTA + gc.solve_drift(s, q["val"], q["D"], uw, itw)
    print(f"SolveVec {name} model={model}: warm {itw} its, ||rhs - A u|| = {res:.3g}, limit {lim:.3g}")
    assert _note("SolveVec true residual / (delta + drift)", res / lim) < 1.
    assert itw <= its
