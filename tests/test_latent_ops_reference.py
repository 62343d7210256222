"""CPU: the cases of tests/latent_ops_cases.py are valid, each reaches the dispatch path it is named for (shown from
its neighbour table alone by the numpy restatement of the structure builder), the restated packed words decode to
what the segmented kernels expect, legitimate float64 methods stay inside every bound the kernels are held to, and
the hooks refuse bad graphs before any device call."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_ops_cases as lc  # noqa: E402

LD = lc.LD


def setup_module(module):
    lc.assert_longdouble()


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_cases_are_valid(name):
    X, nbr = lc.structure(name)
    assert X.shape == (nbr.shape[0], 2) and nbr.dtype == np.int32
    lc.check_structure(nbr)
    v = lc.values(name)
    for key in ("Bv", "alt"):
        assert np.abs(v[key]).sum(axis=1).max() <= 0.9 + 1e-15
        n, m = nbr.shape
        assert (v[key][np.arange(m)[None, :] >= lc.kcount(n, m)[:, None]] == 0).all()
    assert not np.array_equal(v["Bv"], v["alt"]) or nbr.shape[0] == 1
    for key in ("Dinv", "W", "dw"):
        assert (v[key] > 0).all() and np.isfinite(v[key]).all()
    if nbr.shape[0] >= 400:
        assert v["Dinv"].max() / v["Dinv"].min() > 500.      # spread over three decades
    b = lc.block(name, 3, 0)
    assert len(np.unique(b)) == b.size


def test_kriging_values_are_the_oracle_factor():
    v = lc.values("knn-30", "krig")
    assert np.isfinite(v["Bv"]).all() and (v["Dinv"] > 0).all()
    assert np.abs(v["Bv"]).sum(axis=1).max() > 0.9        # real kriging weights are not diagonally dominant


def test_star_reaches_long_row_overlong_run_and_tile_fallback():
    s = lc.expected_stats("star")
    assert s["max_list"] == 1299 and s["nlong"] >= 1
    assert s["seg_overlong"] == 1 and s["_runlen"][0] == 1299       # column 0: a run of its own
    assert 1299 > 2 * lc.K_SEG_ENTRIES and 1299 % lc.K_SEG_ENTRIES not in (0,)   # three iterations, partial last
    assert 1299 % 128 != 0                                           # and a partial last 128-entry chunk
    assert s["fb_bt"] >= 1 and s["fb_b"] == 0
    assert lc.depth(lc.structure("star")[1]) == 1300                 # the DAG is as deep as n


def test_hubs_reach_every_threshold():
    _, nbr = lc.structure("hubs")
    _, cols = lc._hubs()
    s = lc.expected_stats("hubs")
    ln = np.diff(s["_tptr"])
    assert 2500 <= nbr.shape[0] <= 2800
    assert tuple(int(ln[c]) for c in cols) == lc.HUB_COUNTS
    other = np.delete(ln, cols)
    assert other.max() <= 16                                         # nothing else is long
    assert s["nlong"] == sum(c > lc.K_LONG_ROW for c in lc.HUB_COUNTS) == 10
    assert s["fb_bt"] == sum(c > lc.K_TILE_UNION for c in lc.HUB_COUNTS) == 4
    assert s["seg_overlong"] == 1
    seg = set(s["_seg"].tolist())
    for c, T in zip(cols, lc.HUB_COUNTS):
        if T >= 511:      # a run of its own, closed by the entry limit immediately before and after the hub
            assert c in seg and c + 1 in seg, (c, T)
    assert s["seg_by_entries"] >= 6 and s["seg_by_rows"] == 0
    assert (s["_runlen"] & 1).any() and not (s["_runlen"] & 1).all()  # odd (a pad entry) and even runs
    assert s["seg_pad"] >= 1


def test_chain_closes_runs_by_the_row_limit():
    s = lc.expected_stats("chain")
    assert s["nnz"] == 399 and s["max_list"] == 1 and s["min_list"] == 0     # the last row's list is empty
    assert s["seg_by_rows"] == 3 and s["seg_by_entries"] == 0 and s["nseg"] == 4
    assert list(np.diff(s["_seg"])) == [127, 127, 127, 19]


def test_tiny_and_knn_cover_the_borders():
    for n in (1, 2, 3, 65):
        for m in (1, 5, 70):
            s = lc.expected_stats(f"tiny-{n}-{m}")
            assert s["nnz"] == sum(min(i, m) for i in range(n))
            assert s["min_list"] == 0                              # the last row
    assert lc.expected_stats("tiny-1-1")["nnz"] == 0 and lc.expected_stats("tiny-1-1")["nseg"] == 1
    assert lc.expected_stats("tiny-65-70")["max_list"] == 64      # k_i < m everywhere
    ms = sorted(lc.CASES[k][2] for k in lc.CASES if k.startswith("knn-"))
    for border in (16, 32, 64):                                    # b_apply1m / b_apply1 / wave form borders
        assert border in ms and border + 1 in ms
    assert any(t < 64 for t in lc.T_ALL) and 64 in lc.T_ALL and 65 in lc.T_ALL
    s = lc.expected_stats("knn-30")
    assert s["nlong"] >= 1 and s["seg_by_entries"] >= 1            # early Vecchia rows are long rows


@pytest.mark.parametrize("name", ["star", "hubs", "chain", "knn-30", "tiny-65-70", "tiny-1-1"])
def test_packed_words_decode(name):
    """every entry decodes to its source row, a run-row index < 127 and its row-end flag; the last real entry of
    every run carries the flag (the kernels' padding lanes then never hold an open row)"""
    s = lc.expected_stats(name)
    tptr, trow, pk, seg = s["_tptr"], s["_trow"], s["_pk"], s["_seg"]
    n = len(tptr) - 1
    for w in range(len(seg) - 1):
        rb, re = int(seg[w]), int(seg[w + 1])
        assert 1 <= re - rb <= lc.K_SEG_ROWS
        ents = int(tptr[re] - tptr[rb])
        assert ents <= lc.K_SEG_ENTRIES or re - rb == 1
        for j in range(rb, re):
            for e in range(int(tptr[j]), int(tptr[j + 1])):
                word = int(pk[e])
                assert word & 0xFFFFFF == trow[e] and trow[e] > j
                assert (word >> 24) & 0x7F == j - rb < lc.K_SEG_ROWS
                assert (word >> 31) == (1 if e + 1 == tptr[j + 1] else 0)
        if ents:
            assert int(pk[int(tptr[re]) - 1]) >> 31 == 1
    assert seg[-1] == n


# ------------------------------------------------------------------------------- float64 stand-ins under the bounds
def _b_f64(nbr, V, unit, X, scale, order):
    n, m = nbr.shape
    k = lc.kcount(n, m)
    if order == "pairwise":
        G = np.where((np.arange(m)[None, :] < k[:, None])[:, :, None], V[:, :, None] * X[nbr], 0.)
        Y = G.sum(axis=1) + (X if unit else 0.)
    else:
        Y = X.copy() if unit else np.zeros_like(X)
        rs = range(m) if order == "forward" else range(m - 1, -1, -1)
        for r in rs:
            rows = np.nonzero(k > r)[0]
            Y[rows] += V[rows, r, None] * X[nbr[rows, r]]
    return Y * scale[:, None] if scale is not None else Y


def _bt_f64(nbr, V, unit, X, pre, W, H, order):
    n, m = nbr.shape
    k = lc.kcount(n, m)
    PX = X * pre[:, None] if pre is not None else X
    Y = np.zeros_like(X)
    rows_all = range(n) if order == "forward" else range(n - 1, -1, -1)
    if order == "pairwise":
        tptr, trow, tslot = lc.transposed(nbr)
        for j in range(n):
            e = slice(int(tptr[j]), int(tptr[j + 1]))
            Y[j] = ((V.reshape(-1)[tslot[e]] * (pre[trow[e]] if pre is not None else 1.))[:, None] * X[trow[e]]).sum(axis=0)
    else:
        for i in rows_all:
            for r in range(k[i]):
                Y[nbr[i, r]] += (V[i, r] * (pre[i] if pre is not None else 1.)) * X[i]
    if unit:
        Y = Y + PX
    if W is not None:
        Y = Y + W[:, None] * H
    return Y


@pytest.mark.parametrize("order", ["forward", "backward", "pairwise"])
@pytest.mark.parametrize("name", ["knn-30", "star", "chain", "tiny-65-70"])
def test_float64_operators_meet_the_bound(name, order):
    _, nbr = lc.structure(name)
    v = lc.values(name)
    t = 3
    X, H = lc.block(name, t, 0), lc.block(name, t, 1)
    scale, pre, W = lc.vector(name, 0), lc.vector(name, 1), lc.vector(name, 2)
    rb = lc.b_ratio(nbr, v["Bv"], 1, X, scale, _b_f64(nbr, v["Bv"], 1, X, scale, order))
    rbt = lc.bt_ratio(nbr, v["alt"], 1, X, pre, W, H, _bt_f64(nbr, v["alt"], 1, X, pre, W, H, order))
    G = _b_f64(nbr, v["Bv"], 1, H, v["Dinv"], order)
    ra = lc.a_ratio(nbr, v, H, _bt_f64(nbr, v["Bv"], 1, G, None, v["W"], H, order))
    print(f"{name} {order}: b={rb:.3g} bt={rbt:.3g} A={ra:.3g}")
    assert rb <= 1. and rbt <= 1. and ra <= 1.


def test_a_wrong_entry_breaks_the_operator_bound():
    """the bound is far below the effect of one misplaced entry"""
    _, nbr = lc.structure("knn-30")
    v = lc.values("knn-30")
    X = lc.block("knn-30", 3, 0)
    Y = lc.ref_b(nbr, v["Bv"], 1, X, None).astype(np.float64)
    bad = nbr.copy()
    bad[500, 3] = nbr[500, 4]
    bad[500, 4] = nbr[500, 3]
    assert lc.b_ratio(bad, v["Bv"], 1, X, None, Y) > 1e8


@pytest.mark.parametrize("name,kind", [("knn-30", "rand"), ("knn-30", "krig"), ("star", "rand"), ("hubs", "rand")])
def test_float64_solves_meet_the_preconditioner_bound(name, kind):
    _, nbr = lc.structure(name)
    n, m = nbr.shape
    v = lc.values(name, kind)
    R = lc.block(name, 3, 2)
    z, xt, e, et = lc.precond_ref(nbr, v, R)
    C = lc.precond_c(nbr, 0)
    xs = lc.solve_upper(nbr, v["Bv"], R)
    zs = lc.solve_lower(nbr, v["Bv"], xs / v["dw"][:, None])
    r_sub = lc.max_ratio(np.abs(zs - z), lc.U * e)
    r_subt = lc.max_ratio(np.abs(xs - xt), lc.U * et)
    B = np.eye(n)
    k = lc.kcount(n, m)
    for r in range(m):
        rows = np.nonzero(k > r)[0]
        B[rows, nbr[rows, r]] = v["Bv"][rows, r]
    Bi = np.linalg.inv(B)
    xi = Bi.T @ R
    zi = Bi @ (xi / v["dw"][:, None])
    r_inv = lc.max_ratio(np.abs(zi - z), lc.U * e)
    r_invt = lc.max_ratio(np.abs(xi - xt), lc.U * et)
    print(f"{name}/{kind}: error / (u e): substitution z={r_sub:.3g} xt={r_subt:.3g}, explicit inverse z={r_inv:.3g} "
          f"xt={r_invt:.3g}, C={C}")
    assert max(r_sub, r_inv) <= C and max(r_subt, r_invt) <= C / 2
    # one dropped entry is far outside
    bad = dict(v, Bv=v["Bv"].copy())
    bad["Bv"][n // 2, 0] = 0.
    zb = lc.precond_ref(nbr, bad, R)[0]
    assert lc.max_ratio(np.abs(zb - z), lc.U * e) > 1e4 * C


# ---------------------------------------------------------------------------------------------- host-side checks
@pytest.fixture(scope="module")
def lib():
    from gpboost_amd import basic, build
    import os
    if not os.path.exists(basic.LIB_PATH):
        build.build(verbose=False)
    return lc._lib()


def test_create_rejects_bad_graphs_before_any_device_call(lib):
    X, nbr = lc.structure("tiny-65-5")
    n, m = nbr.shape
    h = ctypes.c_void_p()

    def create(nb, n_=n, m_=m, nbr_len=None, x_len=None, X_=X, opts=None):
        o = None if opts is None else lc._ip(opts, ctypes.c_int64)
        return lib.GPB_TestLatentOpsCreate(n_, m_, lc._ip(nb), nb.size if nbr_len is None else nbr_len, 2, lc._dp(X_),
                                           X_.size if x_len is None else x_len, o, ctypes.byref(h))
    forward, dup, neg = nbr.copy(), nbr.copy(), nbr.copy()
    forward[10, 2] = 10
    dup[20, 1] = dup[20, 0]
    neg[30, 4] = -1
    for what, kw in (("earlier", dict(nb=forward)), ("twice", dict(nb=dup)), ("earlier", dict(nb=neg)),
                     ("entries", dict(nb=nbr, nbr_len=n * m - 1)), ("entries", dict(nb=nbr, x_len=2 * n + 1)),
                     ("n =", dict(nb=nbr, n_=0)), ("n =", dict(nb=nbr, m_=0))):
        assert create(**kw) == -1, what
        assert "GPB_TestLatentOpsCreate" in lc.last_error() and what in lc.last_error(), lc.last_error()
    Xn = X.copy()
    Xn[3, 1] = np.nan
    assert create(nbr, X_=Xn) == -1 and "finite" in lc.last_error()
    bad_opt = lc.opts_array({"tail_merge": 65})
    assert create(nbr, opts=bad_opt) == -1 and "tail_merge" in lc.last_error()
    assert not h.value
    for fn, args in ((lib.GPB_TestLatentOpsSetValues, (None, None, 0, None, None, None, 0, None, 0)),
                     (lib.GPB_TestLatentOpsInfo, (None, None, 0, None, 0)),
                     (lib.GPB_TestLatentOpsApply, (None, 0, 0, 1, 1, 0, None, None, None, None, 0, None, None, None, 0,
                                                   None))):
        assert fn(*args) == -1 and "handle is NULL" in lc.last_error()
    assert lib.GPB_TestLatentOpsFree(None) == 0


@pytest.mark.parametrize("delta", [1e-2, 1e-8])
def test_textbook_float64_pcg_meets_the_residual_bound(delta):
    """a plain float64 PCG with the VADU preconditioner by substitution, stopped by ||r|| < delta on its recursive
    residual, has a true residual (longdouble) within delta + (its + 1)(m + 4) u || |A||u| + |rhs| ||"""
    name = "knn-30"
    _, nbr = lc.structure(name)
    n, m = nbr.shape
    v = lc.values(name, "krig")
    Bv, Dinv, W, dw = v["Bv"], v["Dinv"], v["W"], v["dw"]
    rhs = lc.block(name, 1, 3)

    def A(h):
        return _bt_f64(nbr, Bv, 1, _b_f64(nbr, Bv, 1, h, Dinv, "forward"), None, W, h, "pairwise")

    def P(r):
        return lc.solve_lower(nbr, Bv, lc.solve_upper(nbr, Bv, r) / dw[:, None])
    u, r = np.zeros_like(rhs), rhs.copy()
    z = P(r)
    h, rz, its = z.copy(), float((r * z).sum()), 0
    while its < 400:
        vv = A(h)
        a = rz / float((h * vv).sum())
        u, r = u + a * h, r - a * vv
        its += 1
        if np.sqrt((r * r).sum()) < delta:
            break
        z = P(r)
        rz_new = float((r * z).sum())
        h, rz = z + (rz_new / rz) * h, rz_new
    assert its < 400
    ref, _ = lc.a_ref_bound(nbr, Bv, Dinv, W, u)
    _, S1 = lc.ref_b(nbr, Bv, 1, u, None, absolute=True)
    _, AU = lc.ref_bt(nbr, Bv, 1, S1 * Dinv.astype(LD)[:, None], None, W, u, absolute=True)
    res = float(np.sqrt(((rhs.astype(LD) - ref) ** 2).sum()))
    tol = delta + (its + 1) * (m + 4) * lc.U * float(np.sqrt(((AU + np.abs(rhs)) ** 2).sum()))
    print(f"textbook PCG delta={delta:g}: its={its} residual / allowed = {res / tol:.3g}")
    assert res <= tol
