"""CPU: the cases, references and bounds of tests/fitc_ops_cases.py hold what tests/test_gpu_fitc_ops.py relies on.
Every case is valid and reaches the path it is named for (lane, thread and block strides, member counts per cluster,
partition blocks, tie properties); every bound is at most 1e-8 of its array's scale; float64 numpy stand-ins meet the
very bounds the kernels are held to (largest ratio per kernel printed); single-entry defects (a dropped lane-tail
element, one observation of a block of 4 dropped, two block sums swapped, the jitter on an off-diagonal entry, d where
1 / d belongs) exceed them; the k-means reference is deterministic under ties; the stage cases are well conditioned
and their allowances (8 x the float64 stand-in's error) at most 1e-8 of each array's scale."""
import numpy as np
import pytest

import fitc_ops_cases as fc

LD = fc.LD
OPS = tuple(fc.VEC_OPS)


def setup_module(module):
    fc.assert_longdouble()


def test_cases_reach_their_paths():
    for op in ("diag", "yaux", "coldot", "ff_diag_grad", "grad"):
        cs = fc.vec_cases(op).values()
        assert {(c["n"] + 3) // 4 for c in cs} >= {1, 2, 3}                    # blocks of 4 observations
        assert {c["n"] % 4 for c in cs} >= {0, 1, 3}                           # full and partial blocks
        assert {(c["m"] + 63) // 64 for c in cs} >= {1, 2, 3}                  # lane strides
        assert {c["m"] % 64 for c in cs} >= {0, 1, 63}
        assert any(fc.ldm_of(c["m"]) != c["m"] for c in cs)
    g = fc.vec_cases("gemv").values()
    assert max((c["n"] + 63) // 64 for c in g) == 65                           # the reduce's second lane stride
    assert {c["n"] % 64 for c in g} >= {0, 1, 63} and max(c["m"] for c in g) > 256   # the part's second thread stride
    for op in ("kmn", "kmm", "dkmn", "grad"):
        cs = fc.vec_cases(op).values()
        assert {(c["cov"], c["d"]) for c in cs} == {(cv, d) for cv in range(4) for d in (1, 2, 3)}
    for c in fc.vec_cases("kmn").values():
        X, Z = c["arrays"]
        r = fc.dist(X, Z)
        k, _, _ = fc.cov_dcov(r, c["var"], c["phi"], c["cov"])
        assert r[-1, 0] == 0. and k[-1, 0] == c["var"]                         # the coincident pair
        if c["n"] >= 3:
            assert (c["phi"] * r[1] > 745.).all() and (k[1] == 0.).all()       # exp underflows
    for op in ("kmn", "dkmn"):
        cs = fc.vec_cases(op).values()
        assert {(c["n"], c["m"]) for c in cs} >= {(n, m) for n in fc.N_COL for m in fc.M_COL}
    assert {c["m"] for c in fc.vec_cases("kmm").values()} >= set(fc.M_COL)
    assert len(fc.vec_cases("grad")) == 12 + len(fc.N_COL) * len(fc.M_COL)
    for c in fc.vec_cases("kmm").values():
        r = fc.dist(c["arrays"][0], c["arrays"][0])
        if c["m"] >= 4:
            assert r[0, 1] == 0. and (c["phi"] * r[-1, :-1] > 745.).all()
    assert {c["ints"][0] for c in fc.vec_cases("wsum").values()} == {1, 2, 5}
    for op in ("symv", "lower_t", "chol_solve", "mm_terms"):
        assert tuple(c["m"] for c in fc.vec_cases(op).values()) == fc.M_SQ
    for c in fc.vec_cases("lower_t").values():
        m = c["m"]
        assert np.isnan(c["arrays"][0][np.tril_indices(m, -1)]).all() and np.isfinite(np.triu(c["arrays"][0])).all()
    pc = fc.vec_cases("pred_corr")
    assert {c["m"] for c in pc.values()} == {50, 65}
    for c in pc.values():
        pi = [p for p, _ in c["pairs"]]
        assert len(set(pi)) == len(pi)
    oj = [o for _, o in pc["pred_corr-m65-same-train"]["pairs"]]
    assert oj.count(7) == 3
    oj = [o for _, o in pc["pred_corr-m65-unsorted"]["pairs"]]
    assert oj != sorted(oj) and len(set(oj)) < len(oj)
    assert max(c["n"] * c["m"] for c in fc.vec_cases("ff_rowscale").values()) > 4096 * 256
    assert max(c["n"] for c in fc.vec_cases("ff_dot").values()) > 512 * 256


def test_kmeans_cases_reach_their_paths():
    cases = fc.km_cases()
    seen_n, seen_k, seen_d = set(), set(), set()
    for name, (X, mu) in cases.items():
        assert mu.shape[0] <= X.shape[0] and X.shape[1] == mu.shape[1]
        if name.startswith("cloud"):
            seen_n.add(X.shape[0])
            seen_k.add(mu.shape[0])
            seen_d.add(X.shape[1])
    assert seen_n == set(fc.KM_N) and seen_k == set(fc.KM_K) and seen_d == {1, 2, 3}
    assert (2305 + 255) // 256 == 10                                           # one 8-batch of blocks plus a tail of 2
    for d in (1, 2, 3):
        X, mu = cases[f"sizes-d{d}"]
        cnt = np.bincount(fc.km_assign(X, mu), minlength=mu.shape[0])
        assert tuple(cnt) == fc.KM_SIZES * 2 and cnt.max() > 64
        X, mu = cases[f"one-cluster-d{d}"]
        assert (fc.km_assign(X, mu) == 2).all()
        X, mu = cases[f"lattice-d{d}"]
        D = fc.km_dist(X, mu)
        ties = (D == D.min(axis=1, keepdims=True)).sum(axis=1)
        assert ties.max() == 2 ** d and (ties > 1).sum() >= 1
        # the earlier centre wins every tie
        cl = fc.km_assign(X, mu)
        for i in range(X.shape[0]):
            assert cl[i] == np.flatnonzero(D[i] == D[i].min())[0]
    for X, mu in fc.sqrt_tie_cases():
        t = X[0] - mu
        s = t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]
        lo, hi = s.min(), s.max()
        assert hi == np.nextafter(lo, np.inf) and lo < hi and np.sqrt(lo) == np.sqrt(hi)
        assert fc.km_assign(X, mu)[0] == 0                                     # also when centre 1 has the smaller square
    assert any((lambda t: t[1, 0] ** 2 + t[1, 1] ** 2 < t[0, 0] ** 2 + t[0, 1] ** 2)(X[0] - mu)
               for X, mu in fc.sqrt_tie_cases())


def test_kmeans_reference_is_deterministic():
    def assign_loop(X, mu):
        out = np.zeros(X.shape[0], dtype=np.int32)
        for i in range(X.shape[0]):
            best, bd = 0, None
            for j in range(mu.shape[0]):
                t = X[i] - mu[j]
                s = t[0] * t[0]
                for q in range(1, X.shape[1]):
                    s = s + t[q] * t[q]
                dj = np.sqrt(s)
                if bd is None or dj < bd:
                    best, bd = j, dj
            out[i] = best
        return out

    for name, (X, mu) in fc.km_cases().items():
        cl = fc.km_assign(X, mu)
        assert np.array_equal(cl, fc.km_assign(X.copy(), mu.copy()))
        if X.shape[0] * mu.shape[0] <= 3000:
            assert np.array_equal(cl, assign_loop(X, mu)), name
        m1, m2 = fc.km_means(X, cl, mu), fc.km_means(X, cl, mu)
        assert np.array_equal(m1, m2)
        empty = np.bincount(cl, minlength=mu.shape[0]) == 0
        assert np.array_equal(m1[empty], mu[empty])
        cnt, off, tot, base, lst = fc.km_partition(cl, mu.shape[0])
        assert base[-1] == X.shape[0] and np.array_equal(np.sort(lst), np.arange(X.shape[0]))
        for c in range(mu.shape[0]):
            mem = lst[base[c]:base[c + 1]]
            assert (cl[mem] == c).all() and (np.diff(mem) > 0).all()
    lc = fc.lloyd_cases()
    mu, its = fc.km_lloyd(*lc["blobs"])
    assert 2 <= its <= 20 and np.array_equal(mu, fc.km_lloyd(*lc["blobs"])[0])
    assert fc.km_lloyd(*lc["uniform-cap2"])[1] == 2
    assert fc.km_lloyd(lc["uniform-cap2"][0], lc["uniform-cap2"][1], 1000)[1] > 2
    assert fc.km_lloyd(*lc["uniform-d1"])[1] < 1000
    # the 2-cycle stop: the loop ends early on means that are no fixed point (mu == old would make them one)
    X, seeds, cap = lc["two-cycle"]
    mu, its = fc.km_lloyd(X, seeds, cap)
    assert 2 < its < 10 and not np.array_equal(fc.km_means(X, fc.km_assign(X, mu), mu), mu)
    assert np.array_equal(fc.km_lloyd(X, seeds, its - 2)[0], mu)               # mu == old_old


@pytest.mark.parametrize("op", OPS)
def test_bounds_are_tight_and_standins_meet_them(op):
    worst_c, worst_r = 0., 0.
    for name, c in fc.vec_cases(op).items():
        cond = fc.condition(c)
        assert cond <= 1., (name, cond)
        worst_c = max(worst_c, cond)
        out = fc.compute(c, np.float64)
        for k, r in fc.ratios(c, out).items():
            assert r < 1., (name, k, r)
            worst_r = max(worst_r, r)
    print(f"{op}: {len(fc.vec_cases(op))} cases, largest bound / (1e-8 scale) {worst_c:.2g}, "
          f"float64 stand-in error / bound {worst_r:.2f}")


def _zeroed(c, idx, where):
    arrays = [None if a is None else a.copy() for a in c["arrays"]]
    arrays[idx][where] = 0.
    return dict(c, arrays=arrays)


def _pick(op, **want):
    for name, c in fc.vec_cases(op).items():
        if all(c[k] == v for k, v in want.items()) and all(a is not None for a in c["arrays"]):
            return c
    raise KeyError((op, want))


def _defects(op):
    """(what, case, defective outputs) of one op"""
    out = []
    if op in ("kmn", "dkmn"):
        c = _pick(op)
        o = fc.compute(c, np.float64)
        o["K"][3, 64] = 0.
        out.append(("lane tail element unwritten", c, o))
    elif op == "kmm":
        c = _pick(op)
        o = fc.compute(c, np.float64)
        o["Ks"][0, 1] *= fc.JIT
        out.append(("jitter on an off-diagonal entry", c, o))
    elif op == "diag":
        c = _pick(op, n=5, m=65)
        out.append(("lane tail element dropped", c, fc.compute(_zeroed(c, 0, (2, 64)), np.float64)))
        o = fc.compute(c, np.float64)
        o["logd"] = o["logd"] - np.log(o["d"][1])
        out.append(("one observation of a block of 4 dropped", c, o))
        o = fc.compute(c, np.float64)
        o["Kd"] = c["arrays"][1] * o["d"][:, None]
        out.append(("d for 1 / d", c, o))
    elif op == "dy":
        c = _pick(op, n=257)
        out.append(("d for 1 / d", c, {"Dy": c["arrays"][1] * c["arrays"][0]}))
    elif op == "wsum":
        c = _pick(op, m=65, ints=[5])
        out.append(("last chunk dropped", c, {"W": c["arrays"][0][:4].sum(axis=0) + c["arrays"][1]}))
    elif op == "gemv":
        c = _pick(op, n=65, m=65)
        out.append(("the second chunk's observation dropped", c, fc.compute(_zeroed(c, 1, 64), np.float64)))
        c = _pick(op, n=4097, m=257)
        out.append(("partial 64 dropped", c, fc.compute(_zeroed(c, 1, slice(4096, 4097)), np.float64)))
    elif op == "symv":
        c = _pick(op, m=65)
        out.append(("lane tail element dropped", c, fc.compute(_zeroed(c, 0, (3, 64)), np.float64)))
    elif op == "lower_t":
        c = _pick(op, m=65)
        o = fc.compute(c, np.float64)
        o["LT"][0, 64] = c["arrays"][0][0, 64]
        out.append(("an entry above the diagonal kept", c, o))
    elif op == "chol_solve":
        c = _pick(op, m=65)
        out.append(("lane tail element dropped", c, fc.compute(_zeroed(c, 0, (0, 64)), np.float64)))
    elif op == "yaux":
        c = _pick(op, n=5, m=65)
        out.append(("lane tail element dropped", c, fc.compute(_zeroed(c, 0, (2, 64)), np.float64)))
        o = fc.compute(c, np.float64)
        o["q"] = o["q"] - c["arrays"][2][1] * o["yaux"][1]
        out.append(("one observation of a block of 4 dropped", c, o))
    elif op == "grad":
        c = [v for v in fc.vec_cases(op).values() if v["n"] == 5 and v["m"] == 65][0]
        for idx, what in ((2, "K"), (3, "A"), (4, "Gt"), (5, "Mr")):
            out.append((f"lane tail element of {what} dropped", c, fc.compute(_zeroed(c, idx, (2, 64)), np.float64)))
        o = fc.compute(c, np.float64)
        o["sums"] = o["sums"][[1, 0, 2, 3]]
        out.append(("s1v and s1r swapped", c, o))
        o = fc.compute(c, np.float64)
        o["sums"] = o["sums"][[0, 1, 3, 2]]
        o["parts"] = o["parts"][:, [0, 1, 3, 2]]
        out.append(("s2v and s2r swapped", c, o))
        w = fc.grad_pieces(c, np.float64)
        o = fc.compute(c, np.float64)
        o["parts"][0, 2] -= w["s2v"][1]
        o["sums"][2] -= w["s2v"][1]
        out.append(("one observation of a block of 4 dropped", c, o))
    elif op == "mm_terms":
        c = _pick(op, m=65)
        o = fc.compute(c, np.float64)
        o["sums"] = o["sums"][[1, 0, 2, 3, 4, 5]]
        out.append(("two sums swapped", c, o))
        out.append(("lane tail element dropped", c, fc.compute(_zeroed(c, 2, (3, 64)), np.float64)))
    elif op == "coldot":
        c = _pick(op, n=5, m=65)
        out.append(("lane tail element dropped", c, fc.compute(_zeroed(c, 0, (2, 64)), np.float64)))
    elif op == "pred_corr":
        c = fc.vec_cases(op)["pred_corr-m65-same-train"]
        out.append(("lane tail element dropped", c, fc.compute(_zeroed(c, 0, (3, 64)), np.float64)))
        o = fc.compute(c, np.float64)
        pi, oj = c["pairs"][0]
        o["Maux"][pi] = c["arrays"][3][pi] - c["arrays"][1][oj] * o["corr"][0] * c["arrays"][2][oj]
        out.append(("d for 1 / d", c, o))
    elif op == "ff_diag_grad":
        c = _pick(op, n=5, m=65)
        out.append(("lane tail element dropped", c, fc.compute(_zeroed(c, 1, (2, 64)), np.float64)))
    elif op == "ff_recip":
        c = _pick(op, n=257)
        out.append(("x for 1 / x", c, {"y": c["arrays"][0].copy()}))
    elif op == "ff_rowscale":
        c = fc.vec_cases(op)["ff_rowscale-n300-t7-yin"]
        out.append(("Yin ignored", c, fc.compute(dict(c, arrays=c["arrays"][:2] + [None]), np.float64)))
    elif op == "ff_dot":
        c = _pick(op, n=131072 + 5)
        out.append(("the stride loop's tail dropped", c, fc.compute(_zeroed(c, 0, slice(131072, None)), np.float64)))
    return out


@pytest.mark.parametrize("op", OPS)
def test_single_entry_defects_exceed_the_bounds(op):
    defects = _defects(op)
    assert defects
    for what, c, o in defects:
        r = max(fc.ratios(c, o).values())
        print(f"{op}: {what}: {r:.3g} bounds")
        assert r > 1., (op, what, r)


# ------------------------------------------------------------------------------------------------ stages
@pytest.mark.parametrize("name", sorted(fc.STAGE_CASES))
def test_stage_cases_are_well_conditioned_and_the_allowances_tight(name):
    ck, cw = fc.stage_conditions(name)
    print(f"{name}: cond(K_mm,s) {ck:.3g}, cond(W) {cw:.3g}")
    assert ck <= 1e4 and cw <= 1e6
    q = fc.stage_inputs(name)
    dz = fc.dist(q["Z"], q["Z"]) + 10. * np.eye(q["m"])
    assert dz.min() > 0. and all((q["Z"][j] == q["X"]).all(axis=1).any() for j in range(q["m"]))   # Z is a subset of X
    m = q["match"]
    assert (m >= 0).sum() >= 2 and len(set(m[m >= 0])) < (m >= 0).sum() and list(m[m >= 0]) != sorted(m[m >= 0])
    ref, allow, err = fc.stage_reference(name)
    worst = 0.
    for k, v in ref.items():
        if k == "sums":
            continue
        scale = float(np.max(fc.af(v)))
        assert allow[k] <= 1e-8 * scale, (k, allow[k], scale)
        worst = max(worst, allow[k] / (1e-8 * scale))
    # the far end: the stand-in meets the project's scalar tolerances (nll 1e-9, gradient 1e-7) with room for the 8x
    std = fc.stage_compute(name, np.float64)
    rel = np.abs((std["sums"].astype(LD) - ref["sums"]) / ref["sums"]).astype(np.float64)
    assert (8 * rel[:2] <= 1e-9).all() and (8 * rel[2:] <= 1e-7).all(), rel
    print(f"{name}: largest allowance / (1e-8 scale) {worst:.2g}; stand-in errors " +
          ", ".join(f"{k} {err[k]:.2g}" for k in ref if k != "sums") + f"; sums rel {rel.max():.2g}")
    # defects the allowances catch: a buffer that was not overwritten (V for M, K_d for G^T), the jittered K_mm in
    # the derivative's place, the corrections of pairs that share a training point dropped
    assert np.max(fc.af(ref["V"] - ref["M"])) > allow["M"] and np.max(fc.af(ref["Kd"] - ref["Gt"])) > allow["Gt"]
    assert np.max(fc.af(ref["Ks"] - ref["Kmm"])) > allow["Kmm"]
    C = np.zeros((fc.NP_PRED, q["n"]))
    for i, oj in enumerate(m):
        if oj >= 0:
            C[i, oj] = float(ref["var"][i] * 0 + q["var"] - (ref["Kmn"][oj] @ ref["Kinv"] @ ref["Kmn"][oj]))
    full = (C / fc.f64(ref["d"])[None, :]) @ C.T
    assert np.max(np.abs(full - np.diag(np.diag(full)))) > allow["cov"]       # the off-diagonal pair terms matter
