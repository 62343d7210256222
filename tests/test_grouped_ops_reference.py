"""CPU: the cases of tests/grouped_ops_cases.py without a GPU. Every design is valid and reaches the path it is
named for (chunk counts per row and plan, the lower_q / upper_q ranges, short and long destinations, worked out
from the design alone; tests/test_gpu_grouped_ops.py compares them with what the engine holds); the CSR
restatement equals a dense Z^T Z; float64 numpy stand-ins of every operation, summing in another order than the
longdouble reference, meet the very bounds the kernels are held to; single-entry defects in a stand-in exceed the
bound in every case. Run with -s for the largest error / bound ratio of every operation."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grouped_ops_cases as gc  # noqa: E402

LD = gc.LD
_worst = {}


def setup_module(module):
    gc.assert_longdouble()


def teardown_module(module):
    for key in sorted(_worst):
        print(f"[grouped ops, float64 stand-in] largest error / bound, {key}: {_worst[key]:.3g}")


def _note(key, v):
    _worst[key] = max(_worst.get(key, 0.), float(v))
    return v


# ------------------------------------------------------------------------------------------------ designs
@pytest.mark.parametrize("name", gc.DESIGNS)
def test_design_is_valid(name):
    lv = gc.design(name)
    s = gc.structure(name)
    assert lv.dtype == np.int32 and lv.flags.c_contiguous and lv.ndim == 2 and lv.min() >= 0 and lv.max() < lv.shape[1]
    assert 1 <= s.K <= gc.K_GLP_MAX_K and s.M == s.m.sum() and s.cnt.sum() == s.K * s.n
    unused = np.flatnonzero(s.cnt == 0)
    assert list(unused) == ({"gap": [3], "zlists": [3]}.get(name, []))
    # columns ascending in every row, none in the row's own effect, split at the first column of a higher effect
    assert s.rowptr[-1] == s.nnz and (np.diff(s.rowptr) >= 0).all()
    if s.nnz:
        same_row = s.row[1:] == s.row[:-1]
        assert (s.col[1:][same_row] > s.col[:-1][same_row]).all()
        assert (s.blk[s.row] != s.blk[s.col]).all()
        e = np.arange(s.nnz)
        assert ((s.col < s.cum[s.blk[s.row]]) == (e < s.split[s.row])).all()
    assert ((s.rowptr[:-1] <= s.split) & (s.split <= s.rowptr[1:])).all()
    assert (s.val >= 1).all() and s.val.sum() == s.n * s.K * (s.K - 1)
    # observation lists: ascending, the row's own
    for r in (0, s.M // 2, s.M - 1):
        o = s.obs[s.obs_ptr[r]:s.obs_ptr[r + 1]]
        assert (np.diff(o) > 0).all() and (s.glev[s.blk[r], o] == r).all()
    for e in (0, s.nnz // 2, s.nnz - 1) if s.nnz else ():
        o = s.slot_obs[s.slot_ptr[e]:s.slot_ptr[e + 1]]
        assert o.size == s.val[e] and (np.diff(o) > 0).all()
        assert (s.glev[s.blk[s.row[e]], o] == s.row[e]).all() and (s.glev[s.blk[s.col[e]], o] == s.col[e]).all()


@pytest.mark.parametrize("name", gc.DESIGNS)
def test_csr_equals_dense_ztz(name):
    """entry by entry against the dense Z^T Z where that is small; for every design the products with integer
    vectors, exact in float64, against Z^T (Z x) taken over the observations"""
    s = gc.structure(name)
    if s.M <= 1200 and s.n <= 5000:
        A = np.zeros((s.M, s.M))
        A[s.row, s.col] = s.val
        A[np.arange(s.M), np.arange(s.M)] = s.cnt
        assert np.array_equal(A, gc.dense_ztz(s))
    gen = np.random.default_rng(5)
    for _ in range(3):
        x = gen.integers(-8, 9, s.M).astype(np.float64)
        zx = x[s.glev].sum(axis=0)
        want = np.bincount(s.glev.ravel(), weights=np.tile(zx, s.K), minlength=s.M)
        got = s.cnt * x + np.bincount(s.row, weights=s.val * x[s.col], minlength=s.M)
        assert np.array_equal(got, want)


def _chunks(s, t, kind):
    plans, lq, uq = gc.chunk_plan(s, t)
    return np.diff(plans[kind][2]), lq, uq


def test_column_counts_reach_every_lane_split_and_a_second_column_block():
    assert {gc.gre_tc(t) for t in gc.TS} == {1, 2, 4, 8, 16, 32, 64}
    assert sorted(gc.chunk_len(gc.gre_tc(t)) for t in (1, 2, 3, 5, 9, 17, 33)) == [32, 64, 128, 256, 512, 1024, 2048]
    assert {1, 50} <= set(gc.TS) and sum(t > 64 for t in gc.TS) == 2
    assert all(t in gc.TS for t in gc.TS_OTHER)


@pytest.mark.parametrize("t", gc.TS)
def test_hubs_reach_zero_one_and_several_chunks_in_every_plan(t):
    s = gc.structure(f"hubs{t}")
    lens = np.array(gc.hub_lengths(t))
    L = gc.chunk_len(gc.gre_tc(t))
    nh, W = len(lens), lens[-1]
    want = [1, 1, 1, 2, 2, 3]
    a, b = gc.entry_range(s, gc.LOWER)
    hub1 = s.cum[1] + np.arange(nh)                                  # hub rows of effect 1: lower entries only
    assert list((b - a)[hub1]) == list(lens)
    low, lq, uq = _chunks(s, t, gc.LOWER)
    assert list(low[hub1]) == want and (low[:s.cum[1]] == 0).all()
    a, b = gc.entry_range(s, gc.UPPER)
    hub0 = W + np.arange(nh)
    assert list((b - a)[hub0]) == list(lens)
    up, _, _ = _chunks(s, t, gc.UPPER)
    assert list(up[hub0]) == want and (up[s.cum[1]:] == 0).all()
    full, _, _ = _chunks(s, t, gc.FULL)
    assert list(full[hub0]) == want and list(full[hub1]) == want and full.min() >= 1
    assert lens[2] == L and s.val.max() == 3 and (s.val == 1).any()
    # effect 0 has no lower chunks, effect 1 no upper ones
    assert lq[0] == lq[1] == 0 and lq[2] == low.sum() and uq[1] == uq[2] == up.sum() and uq[0] == 0
    assert s.n < 50000 and (t < 33 or s.n < 1500)


def test_three_has_a_middle_effect_with_several_chunks_on_both_sides_of_split():
    s = gc.structure("three")
    assert s.K == 3 and list(s.m) == [40, 7, 300]
    mid = np.arange(s.cum[1], s.cum[2])
    for t in (50, 65):
        low, lq, uq = _chunks(s, t, gc.LOWER)
        up, _, _ = _chunks(s, t, gc.UPPER)
        assert low[mid].min() >= 2 and up[mid].min() >= 2
        assert low[mid[0]] == 2 and up[mid[0]] == -(-300 // 32)       # the hub level crosses all 40 and all 300
        assert lq[1] < lq[2] and uq[1] < uq[2]                        # the middle effect has chunks in both sweeps
        assert lq[0] == lq[1] == 0 and uq[2] == uq[3]
    assert ((s.split[mid] > s.rowptr[:-1][mid]) & (s.split[mid] < s.rowptr[1:][mid])).all()
    for t in (1, 3):
        assert _chunks(s, t, gc.FULL)[0].max() == 1


def test_other_designs_reach_their_paths():
    s = gc.structure("nested")
    assert (np.diff(s.rowptr)[s.cum[1]:] == 1).all() and (np.diff(s.rowptr)[:s.cum[1]] == 4).all()
    assert gc.structure("tiny11").M == 2 and gc.structure("tiny11").nnz == 2
    assert gc.structure("tiny15").M == 6 and list(gc.structure("tiny15").val) == [1.] * 10
    s = gc.structure("gap")
    assert s.cnt[3] == 0 and s.rowptr[3] == s.rowptr[4] and _chunks(s, 1, gc.FULL)[0][3] == 0
    assert gc.structure("eight").K == gc.K_GLP_MAX_K and gc.structure("eight").n == 200
    assert list(gc.structure("sizes").m) == [1, 255, 256, 257, 1000]
    s = gc.structure("zlists")
    assert list(s.cnt[:6]) == [1, 63, 64, 0, 65, 129]
    assert [gc.structure(d).M for d in gc.DENSE_DESIGNS] == [1, 63, 64, 65, 130, 193]
    assert list(gc.structure("dense193").m) == [1, 63, 64, 65]
    for K in gc.Q_KS:
        for n in gc.Q_NS:
            s = gc.structure(f"q-{K}-{n}")
            assert (s.K, s.n) == (K, n) and gc.obs_blocks(n) == (n + 255) // 256
    s = gc.structure("qbig")
    assert s.n == 256 * 1024 + 1 and gc.obs_blocks(s.n) == gc.K_MAX_BLOCKS and gc.obs_blocks(s.n - 1) * 256 == s.n - 1


def test_seg_reaches_the_short_the_one_chunk_and_the_several_chunk_form():
    s = gc.structure("seg")
    ln, counts = gc.seg_plan(s)
    want = (1, 32, 33, 512, 513, 1024, 1025)
    for part in (ln[:s.M], ln[s.M:]):                                # levels, CSR slots
        assert set(want) <= set(part)
    # per kind of destination: short (1, 32, and the slots of the 40-observation levels), one chunk (33, 512),
    # two chunks (513, 1024), three (1025)
    assert counts[0] == 2 * 5 + 2 and counts[1] == 2 * (1 + 1 + 2 + 2 + 3) + 2
    assert counts[2] - counts[0] == 2 * 5 and counts[3] - counts[1] == 2 * 9
    assert (ln[s.M:] == 1).sum() == 2 * 80 + 2                       # and the pair observed once, in both triangles


# ------------------------------------------------------------------------------------------------ stand-ins
def _rowsum64(s, terms, kind, defect=None):
    """float64, one column at a time, entries of a row in descending order (numpy.bincount adds in index order)"""
    a, b = (x.copy() for x in gc.entry_range(s, kind))
    e = np.arange(s.nnz)
    if defect == "split":                                            # one entry at split goes to the wrong triangle
        if kind == gc.LOWER:
            r = np.flatnonzero(s.split < s.rowptr[1:])[-1]
            b[r] += 1
        else:
            r = np.flatnonzero(s.split > s.rowptr[:-1])[-1]
            a[r] -= 1
    mask = (e >= a[s.row]) & (e < b[s.row])
    if defect == "drop":                                             # the first entry of the longest range
        r = np.argmax(b - a)
        mask[a[r]] = False
    rows, tm = s.row[mask][::-1], terms[mask][::-1]
    return np.stack([np.bincount(rows, weights=tm[:, c], minlength=s.M) for c in range(terms.shape[1])], axis=1)


def _standin_product(s, op, q, defect=None):
    X, val, D = q["X"], q["val"], q["D"][:, None]
    dis = np.sqrt(1. / q["D"]) if defect == "dis_sqrt" else q["dis"]
    coef = val * dis[s.col] if op == "lds_mult" else val
    sm = _rowsum64(s, coef[:, None] * X[s.col], gc.OP_KIND[op], defect)
    if op == "lds_mult":
        return sm + (D if defect == "D_for_Ddis" else D * dis[:, None]) * X
    if op == "upper":
        return (1. / D) * (D * X + sm)
    return sm + D * X


def _standin_ssor(s, q, defect=None):
    """float64 substitution, effect by effect; rows not solved yet hold NaN, as the hook's outputs do"""
    R, val, D = q["X"], q["val"], q["D"]
    dis = np.sqrt(1. / D) if defect == "dis_sqrt" else q["dis"]
    dd = (D if defect == "D_for_Ddis" else D * dis)[:, None]
    X, Z = np.full_like(R, np.nan), np.full_like(R, np.nan)
    coef = val * dis[s.col]
    for k in range(s.K):
        r0, r1 = s.cum[k], s.cum[k + 1]
        sm = _rowsum64(s, coef[:, None] * X[s.col], gc.LOWER, defect)
        X[r0:r1] = ((R - sm) / dd)[r0:r1]
    for k in range(s.K - 1, -1, -1):
        r0, r1 = s.cum[k], s.cum[k + 1]
        sm = _rowsum64(s, val[:, None] * Z[s.col], gc.UPPER, defect)
        Z[r0:r1] = ((X - dis[:, None] * sm) / dd)[r0:r1]
    return X, Z


PRODUCTS = ("apply", "apply_lower", "lds_mult", "upper")
# which defects an operation can show: a dropped entry everywhere; dis and D dis where the formula has them; the
# entry at split where the operation reads one triangle
DEFECTS = {"apply": ("drop",), "apply_lower": ("drop", "split"), "lds_mult": ("drop", "split", "dis_sqrt", "D_for_Ddis"),
           "upper": ("drop", "split"), "ssor": ("drop", "split", "dis_sqrt", "D_for_Ddis")}


def _cases(model):
    return gc.MODEL_CASES if model else gc.BLOCK_CASES


@pytest.mark.parametrize("model", (0, 1))
def test_product_standins_meet_the_bounds_and_defects_exceed_them(model):
    for name, t in _cases(model):
        s = gc.structure(name)
        q = gc.block_inputs(name, t, model)
        for op in PRODUCTS:
            ref, bnd = gc.product_reference(s, op, q["val"], q["D"], q["dis"], q["X"])
            r = _note(op, gc.max_ratio(np.abs(_standin_product(s, op, q) - ref), bnd))
            assert r < 1., (name, t, op, r)
            for defect in DEFECTS[op]:
                if model and defect == "dis_sqrt":                   # dis = sqrt(1 / D) there: no defect
                    continue
                r = gc.max_ratio(np.abs(_standin_product(s, op, q, defect) - ref), bnd)
                assert r > 1., (name, t, op, defect, r)


@pytest.mark.parametrize("model", (0, 1))
def test_ssor_standin_meets_both_checks_and_defects_exceed_them(model):
    for name, t in _cases(model):
        s = gc.structure(name)
        q = gc.block_inputs(name, t, model)
        X, Z = _standin_ssor(s, q)
        ratios = gc.ssor_ratios(s, q["val"], q["D"], q["dis"], q["X"], X, Z)
        for key, r in zip(("ssor residual fwd", "ssor residual bwd", "ssor error fwd", "ssor error bwd"), ratios):
            assert _note(key, r) < 1., (name, t, key, r)
        Xr, Zr = gc.ssor_reference(s, q["val"], q["D"], q["dis"], q["X"])
        assert np.isfinite(Xr.astype(np.float64)).all() and np.isfinite(Zr.astype(np.float64)).all()
        for defect in DEFECTS["ssor"]:
            if model and defect == "dis_sqrt":
                continue
            Xd, Zd = _standin_ssor(s, q, defect)
            rd = gc.ssor_ratios(s, q["val"], q["D"], q["dis"], q["X"], Xd, Zd)
            assert max(rd[:2]) > 1. and max(rd[2:]) > 1., (name, t, defect, rd)


def test_segmented_sum_standins_and_a_dropped_observation():
    for name in ("seg", "eight", "gap"):
        s = gc.structure(name)
        w = gc.small_inputs(name)["w"]
        for diag_only in (True, False):
            ref, bnd = gc.assemble_reference(s, w, diag_only)
            got = np.bincount(s.glev.ravel(), weights=np.tile(w, s.K), minlength=s.M)
            if not diag_only:
                slot = np.repeat(np.arange(s.nnz), np.diff(s.slot_ptr))
                got = np.concatenate([got, np.bincount(slot[::-1], weights=w[s.slot_obs][::-1], minlength=s.nnz)])
            assert _note("segmented sums", gc.max_ratio(np.abs(got - ref), bnd)) < 1.
            if name == "seg":
                ln, _ = gc.seg_plan(s)
                for d in np.flatnonzero(ln[:got.size] == 33):        # one observation of a 33-long list dropped
                    lst = s.obs[s.obs_ptr[d]:s.obs_ptr[d + 1]] if d < s.M else \
                        s.slot_obs[s.slot_ptr[d - s.M]:s.slot_ptr[d - s.M + 1]]
                    bad = got.copy()
                    bad[d] = w[lst[:-1]].sum()
                    assert gc.max_ratio(np.abs(bad - ref), bnd) > 1.
        y = gc.small_inputs(name)["y"]
        ref, bnd = gc.list_sums(s.obs_ptr, s.obs, y)
        got = np.bincount(s.glev.ravel()[::-1], weights=np.tile(y, s.K)[::-1], minlength=s.M)
        assert _note("gre_zty", gc.max_ratio(np.abs(got - ref), bnd)) < 1.


def test_small_kernel_standins():
    for name in gc.SMALL_DESIGNS:
        s = gc.structure(name)
        q = gc.small_inputs(name)
        ref = gc.diag_reference(s, q["cnt"], q["tau"])
        D = 1. / q["tau"][s.blk] + q["cnt"]
        got = dict(D=D, dis=np.sqrt(1. / D),
                   sums=np.concatenate([np.add.reduceat(np.log(D), s.cum[:-1]), np.add.reduceat(1. / D, s.cum[:-1])]))
        for key in ref:
            assert _note("gre_diag " + key, gc.max_ratio(np.abs(got[key] - ref[key][0]), ref[key][1])) < 1., (name, key)
        ref = gc.single_reference(q["zty"], q["cnt"], q["D"])
        got = dict(u=q["zty"] / q["D"], sums=np.array([q["cnt"].sum(), (q["cnt"] * q["cnt"] / q["D"]).sum()]))
        for key in ref:
            assert _note("gre_single " + key, gc.max_ratio(np.abs(got[key] - ref[key][0]), ref[key][1])) < 1., (name, key)
        for mode in range(4):
            y = q["ysgn"] if mode in (0, 3) else None
            ref, bnd = gc.effect_dots_reference(s, mode, q["x"], y)
            v = (lambda x: x * y, np.log, lambda x: 1. / x, lambda x: x / y)[mode](q["x"])
            got = np.add.reduceat(v, s.cum[:-1])
            assert _note(f"glp_effect_dots mode {mode}", gc.max_ratio(np.abs(got - ref), bnd)) < 1., (name, mode)
        for form in range(5):                                        # the exact forms: numpy's own operations
            y = q["ysgn"] if form in (1, 2, 3) else None
            exp = gc.vec_expected(s, form, q["sigma2"], q["alpha"], q["x"], y)
            assert all(np.isfinite(e).all() for e in exp)
            if len(exp) == 2:                                        # the fused form differs in at most the last bit
                assert np.abs(exp[0] - exp[1]).max() <= np.spacing(np.abs(exp[0])).max()


@pytest.mark.parametrize("name", gc.DENSE_DESIGNS)
def test_dense_standins_and_the_strict_comparison_defect(name):
    s = gc.structure(name)
    q = gc.dense_inputs(name)
    M = s.M
    Lz = np.tril(q["Li"])                                            # the NaN above the diagonal is never read
    ref, bnd = gc.inv_diag_reference(Lz)
    assert _note("gre_inv_diag", gc.max_ratio(np.abs((Lz[::-1] ** 2).sum(axis=0) - ref), bnd)) < 1.
    for npts in gc.NPS:
        idx = q["idx"][:npts]
        (E, eb), (var, vb) = gc.pred_reference(s, Lz, idx)
        got = np.zeros((M, npts))
        for p in range(npts):
            for k in range(s.K - 1, -1, -1):
                if idx[p, k] >= 0:
                    got[idx[p, k]:, p] += Lz[idx[p, k]:, idx[p, k]]
        assert _note("gre_pred_cols E", gc.max_ratio(np.abs(got - E), eb)) < 1.
        assert _note("gre_pred_cols var", gc.max_ratio(np.abs((got[::-1] ** 2).sum(axis=0) - var), vb)) < 1.
        (Eg, _), (varg, _) = gc.pred_reference(s, Lz, idx, greater=True)
        if (idx >= 0).any():                                         # r > a drops the diagonal entry of a column
            assert gc.max_ratio(np.abs(Eg.astype(np.float64) - E), eb) > 1.
            assert gc.max_ratio(np.abs(varg.astype(np.float64) - var), vb) > 1.
        lo = np.where(idx >= 0, idx, M).min(axis=1)
        for p in range(npts):
            assert (E[:lo[p], p] == 0).all()
    (part, pb), (dg, db) = gc.fisher_reference(s, q["sc"], q["Ainv"])
    B = q["Ainv"] * q["sc"][:, None] * q["sc"][None, :]
    got = np.stack([(B[s.cum[k]:s.cum[k + 1]][::-1] ** 2).sum(axis=0) for k in range(s.K)], axis=1)
    assert _note("gre_fisher_cols part", gc.max_ratio(np.abs(got - part), pb)) < 1.
    assert _note("gre_fisher_cols diag", gc.max_ratio(np.abs(np.diag(q["Ainv"]) * q["sc"] * q["sc"] - dg), db)) < 1.
    A = gc.dense_build_expected(s, q["val"], q["D"], gc.dense_ld(name, True))
    assert (A != 0).sum() == s.nnz + M and A[:, M:].sum() == 0


@pytest.mark.parametrize("name", gc.Q_DESIGNS + ("qbig",))
def test_observation_kernel_standins(name):
    s = gc.structure(name)
    q = gc.q_inputs(name)
    K = s.K
    for aux in (False, True):
        (dwq, db), (sums, sb) = gc.q_reference(s, q["Ainv"], q["D"], q["W"], q["dW"], q["Wa"] if aux else None)
        if K == 1:
            qj = (1. / q["D"][s.glev[0]])[None, :]
        else:
            qj = np.stack([sum(q["Ainv"][s.glev[k], s.glev[j]] for k in range(K - 1, -1, -1)) for j in range(K)])
        qi = qj[::-1].sum(axis=0)
        got = [float((q["W"] * qj[j])[::-1].sum()) for j in range(K)] + ([float((q["Wa"] * qi)[::-1].sum())] if aux else [])
        assert _note("glp_q dwq", gc.max_ratio(np.abs(0.5 * q["dW"] * qi - dwq), db)) < 1.
        assert _note("glp_q sums", gc.max_ratio(np.abs(np.array(got) - sums), sb)) < 1.
    ref, bnd = gc.grad_f_reference(s, q["d1"], q["dwq"], q["W"], q["v"])
    zv = sum(q["v"][s.glev[k]] for k in range(K - 1, -1, -1))
    assert _note("glp_grad_f", gc.max_ratio(np.abs(-q["d1"] + q["dwq"] - q["W"] * zv - ref), bnd)) < 1.


@pytest.mark.parametrize("name,t", gc.TRACE_CASES)
def test_row_trace_standin(name, t):
    s = gc.structure(name)
    q = gc.trace_inputs(name, t)
    ref, bnd = gc.row_trace_reference(s, t, q["U"], q["V"], q["dW"])
    a = sum(q["U"][s.glev[k]] for k in range(s.K - 1, -1, -1))
    p = sum(q["V"][s.glev[k]] for k in range(s.K - 1, -1, -1))
    got = 0.5 * q["dW"] * ((a * p)[:, ::-1].sum(axis=1) / t)
    assert _note("glp_row_trace", gc.max_ratio(np.abs(got - ref), bnd)) < 1.


@pytest.mark.parametrize("name", gc.SOLVE_DESIGNS)
@pytest.mark.parametrize("model", (0, 1))
def test_solve_operators_are_positive_definite_and_the_drift_term_is_small(name, model):
    s = gc.structure(name)
    q = gc.solve_inputs(name, model)
    A = np.zeros((s.M, s.M))
    A[s.row, s.col] = q["val"]
    assert np.array_equal(A, A.T)
    A[np.arange(s.M), np.arange(s.M)] = q["D"]
    assert np.linalg.eigvalsh(A).min() > 0
    u = np.linalg.solve(A, q["rhs"])
    # a float64 direct solve meets the residual bound that the device's iteration is held to, and the drift term
    # of a 100-step run stays far below delta, so the bound means what delta means
    assert gc.true_residual(s, q["val"], q["D"], q["rhs"], u) < gc.DELTA
    assert gc.solve_drift(s, q["val"], q["D"], u, 100) < 1e-2 * gc.DELTA
