"""CPU: the cases of tests/vif_ops_cases.py are valid and well conditioned, each reaches the path it is named for
(worked out from its shapes alone), float64 numpy stand-ins of every operation meet the very bounds the kernels
are held to (the largest ratios are printed), single-entry defects exceed the bounds in every case, and the
longdouble row reference agrees with oracle/vif_oracle.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vif_ops_cases as vc  # noqa: E402

LD = vc.LD
ROWS = sorted(vc.ROW_CASES)
_worst = {}


def setup_module(module):
    vc.assert_longdouble()


def teardown_module(module):
    for key in sorted(_worst):
        print(f"[vif ops reference] largest {key}: {_worst[key]:.3g}")


def _note(key, v):
    _worst[key] = max(_worst.get(key, 0.), float(v))


def _standin(name, **over):
    inp = dict(vc.row_inputs(name), **over)
    try:
        out = vc.rows_compute(inp, np.float64)
    except np.linalg.LinAlgError:        # a damaged input can leave C indefinite: no finite result at all
        return None, {"D": np.inf}
    return out, vc.row_ratios(name, out)


# ------------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("name", ROWS)
def test_row_case_is_valid_conditioned_and_the_standin_meets_the_bounds(name):
    s = vc.ROW_CASES[name]
    inp = vc.row_inputs(name)
    n, nn, i0 = s["n_total"], s["nn"], s["i0"]
    assert 1 <= s["d"] <= 3 and 1 <= nn <= (vc.MAX_NN_GRAD if s["grad"] else vc.MAX_NN)
    assert s["form"] != vc.FORM_MFMA or nn <= vc.MAX_NN_MFMA
    nbr = inp["nbr"]
    assert nbr.shape == (n - i0, nn) and nbr.dtype == np.int32
    for i in range(i0, n):
        k = min(i, nn)
        row = nbr[i - i0]
        assert (row[k:] == -1).all() and (row[:k] >= 0).all() and (row[:k] < i).all() and len(set(row[:k])) == k
    if s["kind"] == "rand":
        for key in ("V", "P0", "P1"):
            if inp[key] is not None:
                assert (nn + 1) * (inp[key] ** 2).sum(axis=1).max() <= 0.5 * (1 + 1e-12)
        if s["grad"]:
            assert not np.array_equal(inp["P0"], inp["P1"]) and not np.array_equal(inp["P0"], inp["V"])
    ref = vc.row_reference(name)
    cond = ref["cond"].max()
    print(f"{name}: largest cond_2(C) {cond:.3g}")
    assert cond <= 1e4
    assert (ref["D"] > 0).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        bm = np.abs(ref["Bv"]).max(axis=1).astype(np.float64)
        rel = {"Bv": np.where(ref["eBv"].max(axis=1) > 0, ref["eBv"].max(axis=1) / bm, 0.).max(),
               "D": (ref["eD"] / np.abs(ref["D"]).astype(np.float64)).max()}
        if s["grad"]:
            eb = ref["edBv"].max(axis=2)
            rel["dBv"] = np.where(eb > 0, eb / ref["sdBv"], 0.).max()
            rel["dD"] = (ref["edD"] / ref["sdD"]).max()
    for key, v in rel.items():
        _note("bound / scale of " + key, v)
        assert v <= 1e-8, (key, v)
    _, ratios = _standin(name)
    for key, v in ratios.items():
        _note("float64 stand-in error / bound, rows " + key, v)
        assert v < 1., (key, v)


def _paths(prefix):
    return {name: vc.row_path(vc.ROW_CASES[name]) for name in ROWS if name.startswith(prefix)}


def test_mfma_cases_reach_every_chunk_parity_and_tail():
    p = _paths("mfma-rand")
    assert all(q["run"] == vc.FORM_MFMA and q["production"] == vc.FORM_MFMA for q in p.values())
    got = {(q["nfull"], q["tail"]) for q in p.values()}
    # no full chunk with every tail 1..7; odd and even counts of full chunks, each with and without a tail
    assert {(0, t) for t in range(1, 8)} <= got
    assert {(1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1), (8, 0), (8, 1)} <= got
    assert {q["sets"] for q in p.values()} == {2, 16, 17, 18, 31, 32}      # one tile, the tile edge, exactly 32 points
    assert {q["ldm_pad"] for q in p.values()} >= {0, 63}                   # m = 64 (no padding) and 65 (ld 128)
    k = _paths("mfma-krig")
    assert len(k) == 96 and {(q["nfull"], q["tail"]) for q in k.values()} == {(3, 1), (1, 1)}


def test_lds_cases_reach_the_tile_and_staging_edges():
    p = _paths("lds-rand-nn")
    assert all(q["run"] == vc.FORM_LDS and q["production"] == vc.FORM_LDS for q in p.values())
    tiles = {name.split("-")[2]: q["tiles"] for name, q in p.items()}
    assert tiles == {"nn32": 243, "nn33": 243, "nn47": 432, "nn48": 507}   # 507 of the 512 register-tile slots
    assert {q["second_tile_pass"] for q in p.values()} == {False, True}
    assert {(q["staging_chunks"], q["staging_tail"]) for q in p.values()} == {(1, 1), (1, 31), (1, 0), (2, 1), (3, 1)}
    f = _paths("lds-forced")
    assert all(q["run"] == vc.FORM_LDS and q["production"] == vc.FORM_MFMA for q in f.values())
    assert {q["sets"] for q in f.values()} == {2, 4, 5, 6, 32}             # S % 4 in {2, 0, 1, 2, 0}
    assert vc.row_path(vc.ROW_CASES["lds-krig-gaussian-nograd-nn64-m25"])["tiles"] == 289      # S = 65 without derivatives
    assert vc.row_path(vc.ROW_CASES["lds-rand-nograd-nn49-m33"])["sets"] == 50                  # beyond the derivative limit


def test_prediction_and_order_cases():
    p = _paths("pred-")
    form = {name: q["run"] for name, q in p.items()}
    assert form["pred-mp1"] == form["pred-mp31"] == vc.FORM_MFMA
    assert form["pred-mp32"] == form["pred-mp63"] == form["pred-mp64"] == vc.FORM_LDS
    assert p["pred-mp64"]["sets"] == 65 and p["pred-mp64"]["second_tile_pass"]
    assert p["pred-mp32-n10"]["short_rows"] == 22 and p["pred-mp12-n5-krig"]["short_rows"] == 7
    for name in p:                       # lists over earlier prediction points as well (cond_all)
        s = vc.ROW_CASES[name]
        assert (vc.row_inputs(name)["nbr"] >= s["i0"]).any()
    pads = {vc.ROW_CASES[n_]["n_total"]: q["pad_slots"] for n_, q in _paths("order-").items()}
    assert pads == {1: 0, 2: 6, 7: 1, 8: 0, 9: 7, 71: 1}


def _defects(name):
    """inputs with one defect each: a Gram term removed, P_0 and P_1 swapped, one neighbour moved"""
    s, inp = vc.ROW_CASES[name], vc.row_inputs(name)
    n, nn, i0 = s["n_total"], s["nn"], s["i0"]
    out = {}
    ir = (n - i0) // 2 if n - i0 > 1 else 0
    i = i0 + ir
    k = min(i, nn)
    V = inp["V"].copy()
    used = np.zeros(n, dtype=bool)        # the points some row reads: its own and its neighbours
    used[i0:] = True
    used[inp["nbr"][inp["nbr"] >= 0]] = True
    j, q = np.unravel_index(np.argmax(np.abs(V) * used[:, None]), V.shape)
    V[j, q] = 0.                          # the term q of every Gram entry of point j (the largest term there is)
    out["gram term"] = dict(V=V)
    if s["grad"]:
        out["P0 / P1 swapped"] = dict(P0=inp["P1"], P1=inp["P0"])
    free = [c for c in range(i) if c not in set(inp["nbr"][ir, :k])]
    if k and free:
        nbr = inp["nbr"].copy()
        nbr[ir, 0] = free[-1]            # the nearest neighbour (a far one can carry no weight at all)
        out["neighbour moved"] = dict(nbr=nbr)
    return out


@pytest.mark.parametrize("name", ROWS)
def test_row_defects_exceed_the_bounds(name):
    s = vc.ROW_CASES[name]
    for what, over in _defects(name).items():
        _, ratios = _standin(name, **over)
        assert max(ratios.values()) > 1., (what, ratios)
    # one entry of each output off by 1e-7 relative
    good = vc.rows_compute(vc.row_inputs(name), np.float64)
    ref = vc.row_reference(name)
    for key in ("D", "Bv", "dD", "dBv") if s["grad"] else ("D", "Bv"):
        bad = {q: np.array(v, copy=True) for q, v in good.items()}
        at = np.unravel_index(np.argmax(np.abs(good[key])), good[key].shape)
        if good[key][at] == 0.:
            continue
        bad[key][at] *= 1. + 1e-7
        r = vc.row_ratios(name, bad)[key]
        assert r > 1., (key, at, r)
        # ... and in every row, the entry that carries the row's scale
        if key == "Bv":
            rows = np.abs(ref["Bv"]).max(axis=1).astype(np.float64)
            assert (1e-7 * rows >= 5. * ref["eBv"].max(axis=1)).all()


def test_row_reference_agrees_with_the_oracle():
    """B, D, dB, dD of oracle.vif_oracle.vif_factor (float64, on A and dK) deviate from the longdouble restatement
    (on V and P_k) by less than the bounds, for both nugget values"""
    from oracle.vif_oracle import vif_factor
    s = vc.ROW_CASES[vc.PIN_CASE]
    base = vc.row_inputs(vc.PIN_CASE)
    for nugget in (1., 0.):
        inp = dict(base, nugget=nugget, cjit=1. if nugget else 1. + 1e-10)
        ref = vc.rows_compute(inp, LD, bounds=True)
        o = vif_factor(inp["X"], inp["nbr"], inp["Z"], s["cov"], inp["var"], inp["phi"], nugget=nugget)
        n, nn = s["n_total"], s["nn"]
        got = dict(D=o["D"], Bv=np.zeros((n, nn)), dD=np.array(o["dD"]), dBv=np.zeros((2, n, nn)))
        for i in range(n):
            k = min(i, nn)
            N = inp["nbr"][i, :k]
            got["Bv"][i, :k] = o["B"][i, N]
            for p in range(2):
                got["dBv"][p, i, :k] = o["dB"][p][i, N]
        for key in ("D", "Bv", "dD", "dBv"):
            r = vc.max_ratio(np.abs(got[key].astype(LD) - ref[key]), ref["e" + key])
            _note(f"oracle deviation / bound, {key}", r)
            assert r < 1., (nugget, key, r)


# ------------------------------------------------------------------------------------------------ products
@pytest.mark.parametrize("kind", vc.PROD_GRAPHS)
def test_product_graphs_and_standins(kind):
    _, nbr = vc.prod_graph(kind)
    n, nn = nbr.shape
    cnt = vc.column_counts(nbr)
    assert cnt.sum() == sum(min(i, nn) for i in range(n))
    if kind == "star":
        assert cnt[0] == n - 1
    if kind == "chain":
        assert nn == 1 and cnt.max() == 1
    if kind == "lists":
        assert tuple(cnt[list(vc._lists_graph()[1])]) == vc.LIST_COUNTS
    if kind == "knn":
        assert nn == 30
    for i in range(n):
        k = min(i, nn)
        assert len(set(nbr[i, :k])) == k and (nbr[i, :k] < i).all() and (nbr[i, :k] >= 0).all()
    for m in (1, 5, 65, 260):
        coef, D, M, x = vc.prod_values(kind, m)
        for self_ in (0., 1.):
            for tr in (False, True):
                B = np.asarray(vc.dense_b(nbr, coef, self_), dtype=np.float64)
                B = B.T if tr else B
                for inp, inv in ((M, None), (M, D if not tr else None), (x, None), (x, D if not tr else None)):
                    ref, bnd = vc.prod_reference(nbr, coef, self_, inp, tr, inv)
                    got = B @ inp
                    if inv is not None:
                        got = got / (inv[:, None] if inp.ndim == 2 else inv)
                    r = vc.max_ratio(np.abs(got.astype(LD) - ref), bnd)
                    _note("float64 stand-in error / bound, products", r)
                    assert r < 1.
                    # one coefficient dropped, one output entry off by 1e-7
                    i = n - 1
                    c2 = coef.copy()
                    c2[i, 0] = 0.
                    B2 = np.asarray(vc.dense_b(nbr, c2, self_), dtype=np.float64)
                    bad = (B2.T if tr else B2) @ inp
                    if inv is not None:
                        bad = bad / (inv[:, None] if inp.ndim == 2 else inv)
                    assert vc.max_ratio(np.abs(bad.astype(LD) - ref), bnd) > 1.
                    at = np.unravel_index(np.argmax(np.abs(got)), got.shape)
                    bad = got.copy()
                    bad[at] *= 1. + 1e-7
                    assert vc.max_ratio(np.abs(bad.astype(LD) - ref), bnd) > 1.


def test_product_shapes_reach_the_store_tails_and_the_second_pass():
    assert {m % 4 for m in vc.PROD_M} == {0, 1, 2, 3}
    assert {m > 256 for m in vc.PROD_M} == {False, True} and 256 in vc.PROD_M
    assert {vc.ldm_of(m) - m for m in vc.PROD_M} >= {0, 63, 1}
    assert (vc.PROD_N + 3) // 4 % 8 != 0 and vc.PROD_N % 4 != 0     # padding blocks and a partial last block


# ------------------------------------------------------------------------------------------------ vector ops
def vec_data(n, m, seed=0):
    g = np.random.default_rng(9000 + 17 * n + m + seed)
    return g.standard_normal((n, m)), g.standard_normal((n, m)), g.standard_normal(n), g.standard_normal(m)


@pytest.mark.parametrize("n", vc.VEC_N)
def test_vector_standins(n):
    assert (max(vc.VEC_N) + 63) // 64 > 64            # the reduce kernel strides past its 64 lanes
    for m in vc.VEC_M:
        M, M2, x, w = vec_data(n, m)
        Ml = M.astype(LD)
        for got, ref, bnd in ((M.T @ x, Ml.T @ x.astype(LD), vc.gamma(n + 8) * (np.abs(M).T @ np.abs(x))),
                              (M @ w, Ml @ w.astype(LD), vc.gamma(m + 8) * (np.abs(M) @ np.abs(w))),
                              ((M * M2).sum(axis=1), (Ml * M2.astype(LD)).sum(axis=1),
                               vc.gamma(m + 8) * (np.abs(M) * np.abs(M2)).sum(axis=1))):
            r = vc.max_ratio(np.abs(got.astype(LD) - ref), bnd)
            _note("float64 stand-in error / bound, vector ops", r)
            assert r < 1.
    for nt in (1, 8):
        terms = vc.sum_terms(n, nt, seed=n + nt)
        assert nt == 1 or {t[3] for t in terms} == set(vc.SUM_OPS)
        ref, bnd = vc.sum_reference(terms)
        got = []
        for a, b, c, op in terms:
            b1 = np.ones(n) if b is None else b
            c1 = np.ones(n) if c is None else c
            got.append(vc.sum_term(op, a, b1, c1).sum())
        r = vc.max_ratio(np.abs(np.array(got).astype(LD) - ref), bnd)
        _note("float64 stand-in error / bound, vector ops", r)
        assert r < 1.
