"""GPU: the sparse Vecchia operators (gpboost_amd/csrc/sparse_kernels.hip) in every selectable kernel form, their
production composition and the VADU preconditioner plans, element by element through the GPB_TestLatentOps*
hooks against the numpy.longdouble references and the bounds of tests/latent_ops_cases.py (derived there, none
tuned to a kernel; tests/test_latent_ops_reference.py holds float64 stand-ins to the same bounds and proves from
the neighbour tables that every case reaches its path). Outputs start as NaN between guard bands: a write out of
range or a row left unwritten fails the test without a fault. Every test prints its largest error / bound
ratios under pytest -s. Bad inputs are rejected by the host checks; no test provokes a fault.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_ops_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

FORM_CASES = ("knn-30", "star", "hubs", "chain")
PLAN_CASES = ("knn-30", "knn-64", "star", "hubs")


def setup_module(module):
    lc.assert_longdouble()


def _same(a, b):
    return np.array_equal(lc.bits(a), lc.bits(b))


def _b(h, form, t, unit, alt, with_scale):
    X, _, scale, _, _ = lc.case_inputs(h.name, t)
    return h.apply(lc.OP_B, form, t, unit, alt, X, scale=scale if with_scale else None)


def _bt(h, form, t, unit, alt, with_pre, with_wh):
    X, H, _, pre, W = lc.case_inputs(h.name, t)
    return h.apply(lc.OP_BT, form, t, unit, alt, X, pre=pre if with_pre else None, W=W if with_wh else None,
                   H=H if with_wh else None)


# ------------------------------------------------------------------------------------------------ structure
@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_info_matches_the_restatement(name):
    """with relabel = 0 the builder's counts are those of the numpy restatement, which
    tests/test_latent_ops_reference.py shows to reach the thresholds; with relabel = 1 vo is a permutation that keeps
    the first min(n, m) rows"""
    h = lc.LatentOps(name, {"relabel": 0}, set_values=False)
    st, vo = h.info()
    exp = lc.expected_stats(name)
    got = {k: st[k] for k in exp if not k.startswith("_")}
    assert got == {k: v for k, v in exp.items() if not k.startswith("_")}, (got, exp)
    assert np.array_equal(vo, np.arange(h.n))
    h.close()
    h = lc.LatentOps(name, {"relabel": 1}, set_values=False)
    st, vo = h.info()
    assert st["nnz"] == exp["nnz"] and st["max_list"] == exp["max_list"]
    assert sorted(vo.tolist()) == list(range(h.n))
    k = min(h.n, h.m)
    assert np.array_equal(vo[:k], np.arange(k))
    h.close()


# ------------------------------------------------------------------------------------------------ every bound
BOUND_PARAMS = [(name, "rand", rl) for name in sorted(lc.CASES) for rl in (0, 1)] + [("knn-30", "krig", 1)]


@pytest.mark.parametrize("name,kind,relabel", BOUND_PARAMS)
def test_operators_meet_the_bound_in_the_production_dispatch(name, kind, relabel):
    """B, B^T and their composition on every t and every argument combination: unit 0 / 1, scale, pre, W / H null or
    given, Bv's or alt_vals' values"""
    h = lc.LatentOps(name, {"relabel": relabel}, kind)
    worst = {}
    for t in lc.t_set(name):
        for alt in (0, 1):
            for unit in (0, 1):
                for sc in (0, 1):
                    r = lc.case_b_ratio(name, kind, alt, unit, sc, t, _b(h, 0, t, unit, alt, sc))
                    worst["b"] = max(worst.get("b", 0.), r)
                    assert r <= 1., ("b", name, t, alt, unit, sc, r)
                for pre in (0, 1):
                    for wh in (0, 1):
                        r = lc.case_bt_ratio(name, kind, alt, unit, pre, wh, t, _bt(h, 0, t, unit, alt, pre, wh))
                        worst["bt"] = max(worst.get("bt", 0.), r)
                        assert r <= 1., ("bt", name, t, alt, unit, pre, wh, r)
        ref, bound = lc.case_a_ref_bound(name, kind, t)
        V = h.apply(lc.OP_A, 0, t, 1, 0, lc.block(name, t, 1))
        r = lc.max_ratio(np.abs(V.astype(lc.LD) - ref), bound)
        worst["A"] = max(worst.get("A", 0.), r)
        assert r <= 1., ("A", name, t, r)
    print(f"{name}/{kind}/relabel={relabel}: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    h.close()


# ------------------------------------------------------------------------------------------------ every form
def _t1_forms_b(m):
    return [f for f in ("ell", "groups", "old") if f != "groups" or m <= 32]


@pytest.mark.parametrize("relabel", [0, 1])
@pytest.mark.parametrize("name", FORM_CASES)
def test_every_t1_form_meets_the_bound(name, relabel):
    h = lc.LatentOps(name, {"relabel": relabel})
    worst = {}
    for unit in (0, 1):
        for sc in (0, 1):
            for f in _t1_forms_b(h.m):
                alt = 0 if f == "ell" else unit        # the lane-group forms also on alt_vals
                r = lc.case_b_ratio(name, "rand", alt, unit, sc, 1, _b(h, lc.B_FORMS[f], 1, unit, alt, sc))
                worst["b:" + f] = max(worst.get("b:" + f, 0.), r)
        for pre in (0, 1):
            for wh in (0, 1):
                for f in ("paired", "e2", "e4", "s2", "shfl", "e1", "groups", "old"):
                    r = lc.case_bt_ratio(name, "rand", 0, unit, pre, wh, 1,
                                         _bt(h, lc.BT_FORMS[f], 1, unit, 0, pre, wh))
                    worst["bt:" + f] = max(worst.get("bt:" + f, 0.), r)
    print(f"{name}/relabel={relabel}: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1., worst
    h.close()


@pytest.mark.parametrize("t", [3, 65])
@pytest.mark.parametrize("name", FORM_CASES)
def test_every_block_form_meets_the_bound_and_shares_one_summation_order(name, t):
    """t >= 2: the wave forms (16 / 32 gathers in flight), b_apply_kernel / bt_apply_kernel with CH 0 / 16,
    persistent or not, and the LDS-tiled form (unit = 1) claim one summation order (unit term, then entries
    ascending): bit equality between them, and the bound on each. With alt_vals only the tslot gather kernels
    run; they share the order too."""
    h = lc.LatentOps(name, {"relabel": 1})
    worst = {}
    forms = ("wave16", "wave32", "ch0", "ch16", "ch0p", "ch16p")
    for unit in (0, 1):
        for sc in (0, 1):
            out = {f: _b(h, lc.B_FORMS[f], t, unit, 0, sc) for f in forms}
            if unit:
                out["tiled"] = _b(h, lc.B_FORMS["tiled"], t, 1, 0, sc)
            for f, Y in out.items():
                worst["b:" + f] = max(worst.get("b:" + f, 0.), lc.case_b_ratio(name, "rand", 0, unit, sc, t, Y))
                assert _same(Y, out["wave16"]), ("b", f, unit, sc)
            assert _same(out["wave16"], _b(h, 0, t, unit, 0, sc))
        for pre in (0, 1):
            for wh in (0, 1):
                out = {f: _bt(h, lc.BT_FORMS[f], t, unit, 0, pre, wh) for f in forms}
                if unit and not pre:
                    out["tiled"] = _bt(h, lc.BT_FORMS["tiled"], t, 1, 0, 0, wh)
                for f, Y in out.items():
                    worst["bt:" + f] = max(worst.get("bt:" + f, 0.),
                                           lc.case_bt_ratio(name, "rand", 0, unit, pre, wh, t, Y))
                    assert _same(Y, out["wave16"]), ("bt", f, unit, pre, wh)
                assert _same(out["wave16"], _bt(h, 0, t, unit, 0, pre, wh))
                alt = {f: _bt(h, lc.BT_FORMS[f], t, unit, 1, pre, wh) for f in ("ch0", "ch16", "ch0p", "ch16p")}
                for f, Y in alt.items():
                    worst["bt-alt:" + f] = max(worst.get("bt-alt:" + f, 0.),
                                               lc.case_bt_ratio(name, "rand", 1, unit, pre, wh, t, Y))
                    assert _same(Y, alt["ch0"]), ("bt-alt", f, unit, pre, wh)
                assert _same(alt["ch0"], _bt(h, 0, t, unit, 1, pre, wh))
    ref, bound = lc.case_a_ref_bound(name, "rand", t)
    Vt = h.apply(lc.OP_A, 1, t, 1, 0, lc.block(name, t, 1))
    worst["A:tiled"] = lc.max_ratio(np.abs(Vt.astype(lc.LD) - ref), bound)
    assert _same(Vt, h.apply(lc.OP_A, 0, t, 1, 0, lc.block(name, t, 1)))
    print(f"{name}/t={t}: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1., worst
    h.close()


def test_wide_rows_take_the_row_kernels():
    """m = 65 > 64: the production dispatch of B is b_apply_kernel<16>, bit-equal to the CH 0 and persistent forms;
    the wave forms are refused"""
    h = lc.LatentOps("knn-65", {"relabel": 1})
    for t in (2, 64, 65):
        X = lc.block("knn-65", t, 0)
        Y0 = h.apply(lc.OP_B, 0, t, 1, 0, X)
        for f in ("ch0", "ch16", "ch0p", "ch16p"):
            assert _same(Y0, h.apply(lc.OP_B, lc.B_FORMS[f], t, 1, 0, X)), (t, f)
        ret, _, _, g = h.apply_raw(lc.OP_B, lc.B_FORMS["wave16"], t, 1, 0, X)
        assert ret == -1 and "not admitted" in lc.last_error() and g == -1
    h.close()


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name", ["knn-30", "hubs"])
def test_two_calls_are_bit_equal(name):
    h = lc.LatentOps(name, {"relabel": 1})
    for t in (1, 51):
        for call in (lambda: _b(h, 0, t, 1, 0, 1), lambda: _bt(h, 0, t, 1, 0, 1, 1), lambda: _bt(h, 0, t, 1, 1, 1, 1),
                     lambda: h.apply(lc.OP_A, 0, t, 1, 0, lc.block(name, t, 1))):
            assert _same(call(), call()), t
        Z1, X1 = h.apply(lc.OP_PRECOND, 0, t, 1, 0, lc.block(name, t, 2))     # captures the graph
        Z2, X2 = h.apply(lc.OP_PRECOND, 0, t, 1, 0, lc.block(name, t, 2))     # replays it
        assert _same(Z1, Z2) and _same(X1, X2), t
    h.close()


# ------------------------------------------------------------------------------------------------ preconditioner
def _plans(n):
    return [(0, 0, 1), (0, n, 1), (1, 1, 1), (63, 200, 4), (64, 64, 16), (65, 400, 4), (130, n, 4), (n, n, 1)]


PLAN_PARAMS = [(name, i, v) for name in PLAN_CASES for i in range(8) for v in (0, 1)]


@pytest.mark.parametrize("name,plan,variant", PLAN_PARAMS)
def test_preconditioner_plans_meet_the_bound(name, plan, variant):
    """Z = P^-1 R and Xt = B^-T R (rows >= K0) of the plan (K0, K, g), the segment in block / wave form and the tail in row /
    level order (variant 0: block + row, 1: wave + level), eager launches against the captured graph's replay bit for
    bit, and P Z^ ~ R through the operator hooks (independent of the substitution reference)"""
    n = lc.structure(name)[1].shape[0]
    K0, K, g = _plans(n)[plan]
    opt = {"relabel": 1, "dense_rows": K0, "head_rows": K, "tail_merge": g, "seg_form": variant,
           "tail_order": variant, "tail_form": 0}
    kind = "krig" if (name == "knn-30" and plan % 2 == 1) else "rand"
    h = lc.LatentOps(name, dict(opt, no_graph=0), kind)
    eager = lc.LatentOps(name, dict(opt, no_graph=1), kind)
    st, _ = h.info()
    assert st["K0"] == min(K0, n) and st["K"] == max(min(K, n), st["K0"]), st
    C = lc.precond_c(h.nbr, st["ld0"])
    v = lc.values(name, kind)
    for t in (1, 51):
        R = lc.block(name, t, 2)
        z, xt, e, et = lc.case_precond_ref(name, kind, t)
        Z, Xt = h.apply(lc.OP_PRECOND, 0, t, 1, 0, R)
        Zr, Xtr = h.apply(lc.OP_PRECOND, 0, t, 1, 0, R)
        Ze, Xte = eager.apply(lc.OP_PRECOND, 0, t, 1, 0, R)
        assert _same(Z, Zr) and _same(Xt, Xtr), "the replay differs from the first launch"
        assert _same(Z, Ze) and _same(Xt, Xte), "the captured graph differs from the eager launches"
        rz = lc.max_ratio(np.abs(Z.astype(lc.LD) - z), lc.U * e)
        # Xt is the plan's scratch: B^-T R on the Vecchia rows >= K0; the dense head's rows hold what the head was
        # given (R minus the later rows' terms), its own B_00^-T being applied inside the dense products
        k0 = st["K0"]
        rx = lc.max_ratio(np.abs(Xt.astype(lc.LD) - xt)[k0:], lc.U * et[k0:])
        # P Z^ = B^T diag(dw) B Z^: the operator bound twice on Z^, plus Z^'s own error C u e carried through |P|
        ref, bound = lc.a_ref_bound(h.nbr, v["Bv"], v["dw"], None, Z, carried_in=(C * lc.U * e))
        G = h.apply(lc.OP_B, 0, t, 1, 0, Z, scale=v["dw"])
        PZ = h.apply(lc.OP_BT, 0, t, 1, 0, G)
        rp = lc.max_ratio(np.abs(PZ.astype(lc.LD) - R.astype(lc.LD)), bound)
        print(f"{name}/{kind} plan ({K0}, {K}, {g}) variant {variant} t={t}: error / (u e): z={rz:.3g} xt={rx:.3g} "
              f"(C={C}), |P z - r| / bound={rp:.3g}, launches={st['launches']}")
        assert rz <= C and rx <= C / 2 and rp <= 1., (rz, rx, rp, C)
    h.close()
    eager.close()


def test_persistent_tail_plan_meets_the_bound():
    """the persistent tail solve (one launch, grid barriers between merged levels) in the plan shape of
    test_gpu_latent.py::test_persistent_tail_agrees: no heads, g = 1, 8 workgroups per XCD group, t = 12"""
    name, t = "knn-30", 12
    opt = {"relabel": 1, "dense_rows": 0, "head_rows": 0, "tail_merge": 1, "tail_form": 1, "tail_w": 8}
    h = lc.LatentOps(name, opt)
    st, _ = h.info()
    assert st["launches"] == 2, st                      # one launch per solve
    C = lc.precond_c(h.nbr, st["ld0"])
    R = lc.block(name, t, 2)
    z, xt, e, et = lc.case_precond_ref(name, "rand", t)
    Z, Xt = h.apply(lc.OP_PRECOND, 0, t, 1, 0, R)
    Z2, Xt2 = h.apply(lc.OP_PRECOND, 0, t, 1, 0, R)
    assert _same(Z, Z2) and _same(Xt, Xt2)
    rz = lc.max_ratio(np.abs(Z.astype(lc.LD) - z), lc.U * e)
    rx = lc.max_ratio(np.abs(Xt.astype(lc.LD) - xt), lc.U * et)
    print(f"{name} persistent tail t={t}: error / (u e): z={rz:.3g} xt={rx:.3g} (C={C})")
    assert rz <= C and rx <= C / 2
    h.close()


# ------------------------------------------------------------------------------------------------ host checks
def test_host_checks_are_error_returns():
    h = lc.LatentOps("tiny-65-5", {"relabel": 1})
    n = h.n
    X1, X3 = lc.block(h.name, 1, 0), lc.block(h.name, 3, 0)
    vec = lc.vector(h.name, 0)

    def refused(what, *a, **kw):
        ret, Y, _, g = h.apply_raw(*a, **kw)
        assert ret == -1 and "GPB_TestLatentOpsApply" in lc.last_error() and what in lc.last_error(), lc.last_error()
        assert g == -1 and (Y == 7.25).all()           # nothing was written

    refused("unknown op", 4, 0, 1, 1, 0, X1)
    refused("unknown op", -1, 0, 1, 1, 0, X1)
    refused("n t", lc.OP_B, 0, 1, 1, 0, X1, block_len=n - 1)
    refused("n t", lc.OP_B, 0, 3, 1, 0, X3, block_len=n)
    refused("vectors hold", lc.OP_B, 0, 1, 1, 0, X1, scale=vec, vec_len=n + 1)
    refused("t =", lc.OP_B, 0, 0, 1, 0, X1, block_len=0)
    refused("W and H", lc.OP_BT, 0, 1, 1, 0, X1, W=vec)
    refused("no scale", lc.OP_BT, 0, 1, 1, 0, X1, scale=vec)
    refused("no pre", lc.OP_B, 0, 1, 1, 0, X1, pre=vec)
    for form in (lc.B_FORMS["wave16"], lc.B_FORMS["ch0"], lc.B_FORMS["tiled"], 11, -1):
        refused("not admitted", lc.OP_B, form, 1, 1, 0, X1)             # a t >= 2 form at t = 1
    for form in (lc.B_FORMS["ell"], lc.B_FORMS["groups"], lc.B_FORMS["old"]):
        refused("not admitted", lc.OP_B, form, 3, 1, 0, X3)             # a t = 1 form at t = 3
    refused("not admitted", lc.OP_B, lc.B_FORMS["ell"], 1, 1, 1, X1)    # the ELL copy holds Bv's values only
    refused("not admitted", lc.OP_B, lc.B_FORMS["tiled"], 3, 0, 0, X3)  # the tiled form has the unit term built in
    refused("not admitted", lc.OP_BT, lc.BT_FORMS["paired"], 1, 1, 1, X1)
    refused("not admitted", lc.OP_BT, lc.BT_FORMS["wave16"], 3, 1, 1, X3)
    refused("not admitted", lc.OP_BT, lc.BT_FORMS["tiled"], 3, 1, 0, X3, pre=vec)
    refused("not admitted", lc.OP_BT, 16, 3, 1, 0, X3)
    refused("not admitted", lc.OP_A, 2, 3, 1, 0, X3)
    refused("not admitted", lc.OP_PRECOND, 1, 3, 1, 0, X3)
    h.close()
    wide = lc.LatentOps("knn-33", {"relabel": 1})
    refused_w = wide.apply_raw(lc.OP_B, lc.B_FORMS["groups"], 1, 1, 0, lc.block("knn-33", 1, 0))
    assert refused_w[0] == -1 and "not admitted" in lc.last_error()      # b_apply1m holds two entries per lane: m <= 32
    wide.close()
    novals = lc.LatentOps("tiny-3-5", set_values=False)
    ret, _, _, _ = novals.apply_raw(lc.OP_B, 0, 1, 1, 0, lc.block("tiny-3-5", 1, 0))
    assert ret == -1 and "no values set" in lc.last_error()
    lib, v = lc._lib(), lc.values("tiny-3-5")
    assert lib.GPB_TestLatentOpsSetValues(novals.h, lc._dp(v["Bv"]), v["Bv"].size - 1, lc._dp(v["Dinv"]), lc._dp(v["W"]),
                                          lc._dp(v["dw"]), 3, None, 0) == -1 and "entries" in lc.last_error()
    assert lib.GPB_TestLatentOpsSetValues(novals.h, lc._dp(v["Bv"]), v["Bv"].size, lc._dp(v["Dinv"]), lc._dp(v["W"]),
                                          lc._dp(v["dw"]), 3, None, 0) == 0
    ret, _, _, _ = novals.apply_raw(lc.OP_BT, 0, 1, 1, 1, lc.block("tiny-3-5", 1, 0))
    assert ret == -1 and "without alt_vals" in lc.last_error()
    st = np.zeros(5, dtype=np.int64)
    import ctypes
    assert lib.GPB_TestLatentOpsInfo(novals.h, lc._ip(st, ctypes.c_int64), 5, None, 0) == -1
    novals.close()


# ------------------------------------------------------------------------------------------------ vector kernels
def _vec_inputs(n, t):
    rng = np.random.default_rng([n, t])
    blocks = [rng.standard_normal((n, t)) for _ in range(6)]
    a = rng.standard_normal(t)
    act = (rng.random(t) < 0.6).astype(np.int32)      # frozen columns among the active ones
    if t > 1:
        act[0], act[-1] = 1, 0
    return blocks, a, act


@pytest.mark.parametrize("n", lc.VEC_N)
def test_vector_kernels(n):
    """the block-CG vector kernels at n x t around the lane-group, 64-column and 512-block borders ((2500, 51) and
    (2500, 65) take the grid-stride path of the reductions): reductions within (n + 2) u sum |a b| and bit-equal on
    a second call, updates within two roundings per element, frozen columns of alpha / beta, exact copies"""
    u, LD = lc.U, lc.LD
    worst = {}
    for t in lc.VEC_T:
        B, a, act = _vec_inputs(n, t)
        for np_ in (1, 2, 3):
            _, _, out = lc.vec_op("coldots", n, t, B[:2 * np_], np_=np_)
            _, _, again = lc.vec_op("coldots", n, t, B[:2 * np_], np_=np_)
            assert np.array_equal(lc.bits(out), lc.bits(again)), (t, np_)
            for q in range(np_):
                ref, bound = lc.dots_bound(B[2 * q], B[2 * q + 1])
                r = lc.max_ratio(np.abs(out[q * t:(q + 1) * t].astype(LD) - ref), bound)
                worst["coldots"] = max(worst.get("coldots", 0.), r)
        H, V, U0, R0 = B[:4]
        Un, Rn, rr = lc.vec_op("cg_update", n, t, [H, V, U0, R0], sv0=a)
        bu = 2 * (u + lc.UREF) * (np.abs(U0) + np.abs(a) * np.abs(H))
        br = 2 * (u + lc.UREF) * (np.abs(R0) + np.abs(a) * np.abs(V))
        worst["cg_U"] = max(worst.get("cg_U", 0.), lc.max_ratio(np.abs(Un.astype(LD) - (U0.astype(LD) + a.astype(LD) * H)), bu))
        worst["cg_R"] = max(worst.get("cg_R", 0.), lc.max_ratio(np.abs(Rn.astype(LD) - (R0.astype(LD) - a.astype(LD) * V)), br))
        ref, bound = lc.dots_bound(Rn, Rn)              # of the residual the kernel itself wrote
        worst["cg_rr"] = max(worst.get("cg_rr", 0.), lc.max_ratio(np.abs(rr.astype(LD) - ref), bound))
        assert not np.isnan(Un).any() and not np.isnan(Rn).any()
        Hn, _, _ = lc.vec_op("h_update", n, t, [B[0], B[1]], sv0=a)
        bh = 2 * (u + lc.UREF) * (np.abs(B[0]) + np.abs(a) * np.abs(B[1]))
        worst["h"] = max(worst.get("h", 0.), lc.max_ratio(np.abs(Hn.astype(LD) - (B[0].astype(LD) + a.astype(LD) * B[1])), bh))
        Zn, _, _ = lc.vec_op("axpby", n, t, [B[0], B[1]], alpha=1.5, beta=-0.3)
        ba = 3 * (u + lc.UREF) * (1.5 * np.abs(B[0]) + 0.3 * np.abs(B[1]))
        worst["axpby"] = max(worst.get("axpby", 0.), lc.max_ratio(np.abs(Zn.astype(LD) - (LD(1.5) * B[0] + LD(-0.3) * B[1])), ba))
        assert not np.isnan(Zn).any()
        # alpha / beta with frozen columns
        rz, hv = np.abs(B[0][0]) + 0.1, np.abs(B[1][0]) + 0.1
        for mask in (None, act):
            on = np.ones(t, bool) if mask is None else mask.astype(bool)
            _, _, sm = lc.vec_op("alpha", n, t, sv0=rz, sv1=hv, act=mask)
            assert np.array_equal(sm[:t], np.where(on, rz / hv, 0.)) and np.array_equal(sm[t:], sm[:t])
            _, _, sm = lc.vec_op("beta", n, t, sv0=rz, sv1=hv, act=mask)
            assert np.array_equal(sm[:t], np.where(on, rz / hv, 0.))
            assert np.array_equal(sm[t:2 * t][on], (rz / hv)[on]) and np.isnan(sm[t:2 * t][~on]).all()   # hist untouched
            assert np.array_equal(sm[2 * t:], np.where(on, rz, hv))                                      # rz <- rz_new
        # the Newton step's cap: |mnew - mode| <= log(100), entries below it untouched
        mode, step = B[0], 3. * B[1]
        cap, _, _ = lc.vec_op("cap_mode", n, t, [mode, mode + step])
        big = np.abs((mode + step) - mode) > np.log(100.)
        assert np.array_equal(cap[~big], (mode + step)[~big])
        if big.any():
            want = mode.astype(LD) + np.sign(step) * LD(4.605170185988091)
            assert lc.max_ratio(np.abs(cap.astype(LD) - want)[big], (4 * u * (np.abs(mode) + np.log(100.)))[big]) <= 1.
        for (nc, ia, ib) in {(1, 0, t - 1), (t, 0, 0), (max(t // 2, 1), t - max(t // 2, 1), 0)}:
            dst, _, _ = lc.vec_op("pack", n, t, [B[0], B[1]], np_=nc, ia=ia, ib=ib)
            want = B[1].copy()
            want[:, ib:ib + nc] = B[0][:, ia:ia + nc]
            assert np.array_equal(lc.bits(dst), lc.bits(want)), (t, nc, ia, ib)
    print(f"n={n}: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1., worst


def test_vector_host_checks():
    B = [np.zeros((4, 3)) for _ in range(6)]
    v = np.ones(3)
    for what, kw in (("unknown op", dict(op=8)), ("unknown op", dict(op=-1)), ("n t", dict(op=5, block_len=11)),
                     ("np =", dict(op=0, np_=4, small_out_len=12)), ("np =", dict(op=0, np_=0, small_out_len=0)),
                     ("column vectors", dict(op=1, sv0=v, small_len=2)), ("needs", dict(op=1)),
                     ("needs", dict(op=3, sv0=v)), ("small_out holds", dict(op=0, np_=2, small_out_len=3)),
                     ("pack_columns", dict(op=7, np_=2, ia=2, ib=0)), ("pack_columns", dict(op=7, np_=0))):
        op = kw.pop("op")
        ret, o0, o1, sm, g = lc.vector_raw(op, 4, 3, B, **kw)
        assert ret == -1 and "GPB_TestLatentOpsVector" in lc.last_error() and what in lc.last_error(), lc.last_error()
        assert g == -1 and (o0 == 7.25).all() and (o1 == 7.25).all()
    ret = lc.vector_raw(5, 4, 3, B[:1])[0]                      # a missing input block
    assert ret == -1 and "needs" in lc.last_error()
    assert lc.vector_raw(5, 0, 3, B)[0] == -1 and lc.vector_raw(5, 4, 0, B, block_len=0)[0] == -1


# ------------------------------------------------------------------------------------------------ PCG
def _pcg_check(h, kind, t, n_single, delta, RHS, U, its, pmax):
    """every column that stopped by its rule: ||rhs - A u^|| in longdouble <= delta + (its + 1)(m + 4) u
    || |A||u^| + |rhs| || (the recursive residual's drift); the block by the mean"""
    v = lc.values(h.name, kind)
    ref, _ = lc.a_ref_bound(h.nbr, v["Bv"], v["Dinv"], v["W"], U)
    k1, S1 = lc.ref_b(h.nbr, v["Bv"], 1, U, None, absolute=True)
    _, AU = lc.ref_bt(h.nbr, v["Bv"], 1, S1 * v["Dinv"].astype(lc.LD)[:, None], None, v["W"], U, absolute=True)
    res = np.sqrt(((RHS.astype(lc.LD) - ref) ** 2).sum(axis=0)).astype(np.float64)
    drift = np.sqrt(((AU + np.abs(RHS)) ** 2).sum(axis=0)).astype(np.float64)
    out = {}
    if n_single > 0 and its[0] < pmax:
        tol = delta + (its[0] + 1) * (h.m + 4) * lc.U * drift[:n_single]
        out["single"] = float(np.max(res[:n_single] / tol))
    if n_single < t and its[1] < pmax:
        tol = delta + (its[1] + 1) * (h.m + 4) * lc.U * drift[n_single:].mean()
        out["block"] = float(res[n_single:].mean() / tol)
    return out


@pytest.mark.parametrize("name,kind", [("knn-30", "krig"), ("hubs", "rand")])
def test_pcg_stops_by_its_rule(name, kind):
    h = lc.LatentOps(name, {"relabel": 1}, kind)
    n, pmax = h.n, 200
    for t, n_single in ((1, 1), (13, 0), (13, 1), (13, 13)):
        RHS = lc.block(name, t, 3).copy()
        zero_col = t > 1 and n_single == 13
        if zero_col:
            RHS[:, 5] = 0.                  # a single column with a zero right-hand side
        for delta in (1e-2, 1e-8):
            ret, Uo, its, flags = h.pcg(t, n_single, delta, pmax, pmax, RHS)
            lc._check(ret)
            assert flags == (0, 0) and 0 <= its[0] <= pmax and 0 <= its[1] <= pmax, (its, flags)
            assert np.isfinite(Uo).all()
            if zero_col:
                assert (Uo[:, 5] == 0.).all() and np.array_equal(lc.bits(Uo[:, 5]), lc.bits(np.zeros(n)))
            got = _pcg_check(h, kind, t, n_single, delta, RHS, Uo, its, pmax)
            print(f"{name}/{kind} t={t} n_single={n_single} delta={delta:g}: its={its} residual / allowed: {got}")
            assert got and max(got.values()) <= 1., got
            ret2, U2, its2, _ = h.pcg(t, n_single, delta, pmax, pmax, RHS)
            assert ret2 == 0 and its2 == its and np.array_equal(lc.bits(U2), lc.bits(Uo))      # repeatable
    # pmax is a cap
    ret, Uo, its, flags = h.pcg(1, 1, 1e-300, 3, 3, lc.block(name, 1, 3))
    assert ret == 0 and its[0] == 3 and flags == (0, 0)
    # a zero right-hand side at t = 1: u = 0 without iterating
    ret, Uo, its, flags = h.pcg(1, 1, 1e-2, pmax, pmax, np.zeros((n, 1)))
    assert ret == 0 and flags == (0, 1) and (Uo == 0.).all() and its == (0, 0)
    # NaN in one right-hand side column sets the flag and returns
    for t, n_single in ((1, 1), (13, 1)):
        RHS = lc.block(name, t, 3).copy()
        RHS[n // 2, t - 1] = np.nan
        ret, Uo, its, flags = h.pcg(t, n_single, 1e-2, pmax, pmax, RHS)
        assert ret == 0 and flags[0] == 1, (t, flags)
    # host checks
    for what, args in (("n_single", (3, 4, 1e-2, 5, 5, lc.block(name, 3, 3))), ("pmax", (1, 1, 1e-2, 0, 5, lc.block(name, 1, 3))),
                       ("delta", (1, 1, 0., 5, 5, lc.block(name, 1, 3)))):
        ret, Uo, _, _ = h.pcg(*args)
        assert ret == -1 and what in lc.last_error() and (Uo == 7.25).all(), lc.last_error()
    ret, Uo, _, _ = h.pcg(1, 1, 1e-2, 5, 5, lc.block(name, 1, 3), block_len=n - 1)
    assert ret == -1 and "n t" in lc.last_error()
    h.close()
