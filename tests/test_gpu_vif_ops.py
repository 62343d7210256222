"""GPU: the full-scale Vecchia kernels of csrc/vif_kernels.hip element by element through the GPB_TestVif* hooks
(csrc/vif_test.cpp, the launch functions VifSolver uses): the residual row factor in the MFMA and the LDS-staged
form, the sparse B / B^T products and the small vector kernels against the longdouble references and the derived
bounds of tests/vif_ops_cases.py (none tuned to a kernel; tests/test_vif_ops_reference.py holds float64 stand-ins
to the same bounds). The ld-m padding of every input holds NaN, outputs and scratch start as NaN between guard
bands. Run with -s for the largest error / bound ratio of every case.

Bitwise claims checked here: the processing order (Morton, XCD-chunked) changes no bit of the rows or the
products; rows without derivatives give the bits of D and Bv that rows with derivatives give. The two row forms
agree within the sum of their bounds. A row whose residual matrix has a pivot that is not > 0 gets D = NaN in both
forms and leaves every other row's bits alone.

Model level: GPModel.vif_factor (the GEMM chain that makes V and P_k, then the rows) against
oracle.vif_oracle.vif_factor with the project's tolerances: D rtol 1e-10, B rtol 1e-8 / atol 1e-11
(test_gpu_vecchia.py::test_vecchia_factor_matches_reference), dD_k and dB_k 1e-7 of each array's largest magnitude
(the gradient's tolerance of test_gpu_vif.py; the gradient is linear in them)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vif_ops_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu
LD = vc.LD
ROWS = sorted(vc.ROW_CASES)
_worst = {}


def setup_module(module):
    vc.assert_longdouble()


def teardown_module(module):
    for key in sorted(_worst):
        print(f"[vif ops] largest error / bound, {key}: {_worst[key]:.3g}")


def _note(key, v):
    _worst[key] = max(_worst.get(key, 0.), float(v))


def _kernel_of(name):
    p = vc.row_path(vc.ROW_CASES[name])
    return "vif_rows_mfma_kernel" if p["run"] == vc.FORM_MFMA else "vif_rows_kernel"


def _check_rows(name, out, grad):
    """finite where defined, exactly 0 past a row's k entries, every bound"""
    s = vc.ROW_CASES[name]
    n, nn, i0 = s["n_total"], s["nn"], s["i0"]
    k = np.minimum(np.arange(i0, n), nn)
    past = np.arange(nn)[None, :] >= k[:, None]
    keys = ("D", "Bv", "dD", "dBv") if grad else ("D", "Bv")
    for key in keys:
        assert np.isfinite(out[key]).all(), (name, key, "not finite or not written")
    assert (out["Bv"][past] == 0.).all()
    if grad:
        assert (out["dBv"][:, past] == 0.).all()
    ref = vc.row_reference(name)
    ratios = {q: vc.max_ratio(np.abs(out[q].astype(LD) - ref[q]), ref["e" + q]) for q in keys}
    return ratios


@pytest.mark.parametrize("name", ROWS)
def test_rows_meet_every_bound(name):
    s = vc.ROW_CASES[name]
    inp = vc.row_inputs(name)
    out = vc.rows_hook(inp, order=0 if s["i0"] else 1)        # prediction rows run in index order
    ratios = _check_rows(name, out, s["grad"])
    print(f"{name}: " + ", ".join(f"{q} {v:.3g}" for q, v in ratios.items()))
    for q, v in ratios.items():
        _note(f"{_kernel_of(name)} {q}", v)
        assert v < 1., (name, q, v)


ORDER_CASES = [n_ for n_ in ROWS if n_.startswith("order-")] + ["lds-rand-nn48-m65", "mfma-rand-nn31-m65", "pred-mp64"]


@pytest.mark.parametrize("name", ORDER_CASES)
def test_rows_order_changes_no_bit(name):
    s = vc.ROW_CASES[name]
    inp = vc.row_inputs(name)
    forms = (s["form"],) if s["nn"] > vc.MAX_NN_MFMA else (vc.FORM_MFMA, vc.FORM_LDS)
    for form in forms:
        a = vc.rows_hook(inp, form=form, order=0)
        b = vc.rows_hook(inp, form=form, order=1)
        for key in ("D", "Bv", "dD", "dBv") if s["grad"] else ("D", "Bv"):
            assert np.array_equal(a[key], b[key]), (name, form, key)
        ratios = _check_rows(name, b, s["grad"])
        assert max(ratios.values()) < 1., (name, form, ratios)


@pytest.mark.parametrize("name", ["mfma-rand-nn31-m25", "mfma-rand-nn17-m9", "mfma-rand-nn1-m1", "lds-rand-nn48-m33",
                                  "lds-rand-nn33-m65", "lds-forced-nn5-m33",
                                  "mfma-krig-matern25-grad-d3-latent-nn31-m25"])
def test_rows_without_derivatives_give_the_same_bits(name):
    inp = vc.row_inputs(name)
    a = vc.rows_hook(inp, grad=True)
    b = vc.rows_hook(inp, grad=False)
    assert np.array_equal(a["D"], b["D"]) and np.array_equal(a["Bv"], b["Bv"])
    assert (b["dD"] == vc.SENTINEL).all() and (b["dBv"] == vc.SENTINEL).all()      # not written by the hook either


@pytest.mark.parametrize("name", [n_ for n_ in ROWS if n_.startswith("lds-forced")] +
                         ["mfma-rand-nn31-m65", "mfma-rand-nn16-m8", "mfma-krig-gaussian-grad-d1-latent-nn31-m25",
                          "pred-mp31"])
def test_row_forms_agree_within_their_bounds(name):
    s = vc.ROW_CASES[name]
    inp = vc.row_inputs(name)
    a = vc.rows_hook(inp, form=vc.FORM_MFMA)
    b = vc.rows_hook(inp, form=vc.FORM_LDS)
    ref = vc.row_reference(name)
    for key in ("D", "Bv", "dD", "dBv") if s["grad"] else ("D", "Bv"):
        r = vc.max_ratio(np.abs(a[key] - b[key]), 2. * ref["e" + key])
        _note("MFMA against LDS form / sum of bounds", r)
        assert r < 1., (name, key, r)
    for out in (a, b):
        assert max(_check_rows(name, out, s["grad"]).values()) < 1.


def test_rows_not_positive_definite_contract():
    """Valid data whose residual matrix has a negative pivot in the rows that hold point j1 and an exactly zero
    first pivot in the row that lists point j2 first: D of those rows is NaN in both forms, every row that reads
    neither point keeps its bits, and the sum of log D is NaN."""
    base = dict(vc.row_inputs("mfma-rand-nn17-m9"), var=3.)       # nugget + var = 4 = 2^2
    n, nn = base["X"].shape[0], base["nn"]
    nbr = base["nbr"].copy()
    # the two points that the fewest rows hold (at least one), j2 moved to the front of one holder's list
    cnt = np.bincount(nbr[nbr >= 0], minlength=n)
    j1, j2 = (int(j) for j in np.argsort(np.where(cnt > 0, cnt, n), kind="stable")[:2])
    assert cnt[j1] >= 1 and cnt[j2] >= 1
    r2 = int(np.nonzero((nbr == j2).any(axis=1))[0][0])
    slot = int(np.nonzero(nbr[r2] == j2)[0][0])
    nbr[r2, 0], nbr[r2, slot] = nbr[r2, slot], nbr[r2, 0]
    r1 = int(np.nonzero((nbr == j1).any(axis=1))[0][0])
    base["nbr"] = nbr
    V = base["V"].copy()
    V[j1] = 0.
    V[j1, 0] = 3.            # C_jj = 1 + 3 - 9 = -5
    V[j2] = 0.
    V[j2, 0] = 2.            # C_jj = 1 + 3 - 4 = 0 exactly, in any summation order
    holds = lambda j: (nbr == j).any(axis=1)  # noqa: E731
    bad = holds(j1) | holds(j2)
    assert bad[r1] and bad[r2]
    reads = bad.copy()
    reads[[j1, j2]] = True
    assert (~reads).sum() > n // 2
    for form in (vc.FORM_MFMA, vc.FORM_LDS):
        clean = vc.rows_hook(base, form=form)
        assert np.isfinite(clean["D"]).all()
        got = vc.rows_hook(base, form=form, V=V)
        assert np.isnan(got["D"][bad]).all(), (form, got["D"][bad])
        for key in ("D", "Bv"):
            assert np.array_equal(got[key][~reads], clean[key][~reads]), (form, key)
        for key in ("dD", "dBv"):
            assert np.array_equal(got[key][:, ~reads], clean[key][:, ~reads]), (form, key)
        assert np.isfinite(got["D"][~bad & ~reads]).all()
        # the evaluation's sum of log D (vif_sum_kernel, op 1) over these D, the finite ones replaced by 1
        total = vc.vector_hook("sum", n, 1, [np.where(np.isnan(got["D"]), got["D"], 1.), None, None], 1, sum_ops=[1])
        assert np.isnan(total[0])


@pytest.mark.parametrize("v", [2., 3.])
def test_rows_zero_last_pivot_gives_nan_in_both_forms(v):
    """k = 1: the one pivot is the last one, 1 + 3 - v^2 = 0 (or -5). A square root and divisions by L_kk = 0 give
    D = -inf, the reciprocal square root gives NaN; both forms flag the pivot and return NaN."""
    base = dict(vc.row_inputs("mfma-rand-nn1-m1"), var=3.)
    nbr = base["nbr"]
    n = nbr.shape[0]
    cnt = np.bincount(nbr[nbr >= 0], minlength=n)
    j = int(np.argsort(np.where(cnt > 0, cnt, n), kind="stable")[0])
    V = base["V"].copy()
    V[j, 0] = v
    bad = (nbr == j).any(axis=1)
    reads = bad.copy()
    reads[j] = True
    for form in (vc.FORM_MFMA, vc.FORM_LDS):
        clean = vc.rows_hook(base, form=form)
        got = vc.rows_hook(base, form=form, V=V)
        assert bad.any() and np.isnan(got["D"][bad]).all(), (form, got["D"][bad])
        for key in ("D", "Bv"):
            assert np.array_equal(got[key][~reads], clean[key][~reads]), (form, key)


def test_rows_refusals():
    inp = vc.row_inputs("mfma-rand-nn17-m9")
    n, nn = inp["X"].shape[0], inp["nn"]

    def refused(what, **kw):
        ret, out, _ = vc.rows_raw(inp, **kw)
        assert ret == -1 and "GPB_TestVifRows" in vc.last_error() and what in vc.last_error(), (kw.keys(), vc.last_error())
        assert (out["D"] == vc.SENTINEL).all()

    def wide(nn2):
        nb = np.full((70, nn2), -1, dtype=np.int32)
        for i in range(70):
            nb[i, :min(i, nn2)] = np.arange(min(i, nn2))
        return nb

    big = dict(X=np.random.default_rng(0).uniform(size=(70, 2)), V=np.zeros((70, inp["m"])), P0=np.zeros((70, inp["m"])),
               P1=np.zeros((70, inp["m"])))
    refused("nn = 49", nn=49, nbr=wide(49), **big)
    refused("nn = 65", nn=65, nbr=wide(65), grad=False, **big)
    refused("MFMA form", nn=32, nbr=wide(32), form=vc.FORM_MFMA, **big)
    nb = inp["nbr"].copy()
    nb[20, 3] = 20
    refused("not an earlier point", nbr=nb)
    nb = inp["nbr"].copy()
    nb[20, 3] = nb[20, 4]
    refused("twice", nbr=nb)
    nb = inp["nbr"].copy()
    nb[3, 5] = 0
    refused("is not -1", nbr=nb)
    refused("d = 4", d=4, X=np.ones((n, 4)))
    refused("form = 3", form=3)
    refused("var and phi", var=-1.)
    refused("cov_type", cov=4)
    ret, _, _ = vc.rows_raw(inp, X=inp["X"][:-1])
    assert ret == -1 and "entries" in vc.last_error()
    bad = inp["X"].copy()
    bad[5, 1] = np.inf
    refused("not finite", X=bad)
    # and a good call still runs after the refusals
    assert np.isfinite(vc.rows_hook(inp)["D"]).all()


# ------------------------------------------------------------------------------------------------ products
def _unpad(out, m):
    """the payload of an n x ldm product output; its padding must still hold the NaN it started with"""
    assert np.isnan(out[:, m:]).all(), "padding entries of the output were written"
    assert np.isfinite(out[:, :m]).all(), "an output entry is not finite or was not written"
    return out[:, :m]


@pytest.mark.parametrize("m", vc.PROD_M)
@pytest.mark.parametrize("kind", vc.PROD_GRAPHS)
def test_products_meet_the_bounds(kind, m):
    X, nbr = vc.prod_graph(kind)
    coef, D, M, x = vc.prod_values(kind, m)
    worst = {}
    for self_ in (0., 1.):
        ref, bnd = vc.prod_reference(nbr, coef, self_, M, False)
        refd, bndd = vc.prod_reference(nbr, coef, self_, M, False, D)
        plain = {}
        for order in (0, 1):
            out, _ = vc.apply_hook("brow", nbr, coef, M, m, self_=self_, X=X, order=order)
            plain[order] = out
            worst["brow"] = max(worst.get("brow", 0.), vc.max_ratio(np.abs(_unpad(out, m).astype(LD) - ref), bnd))
        assert np.array_equal(plain[0][:, :m], plain[1][:, :m])                    # the order changes no bit
        out, out2 = vc.apply_hook("brow", nbr, coef, M, m, self_=self_, D=D, want_div=1, X=X, order=1)
        assert np.array_equal(out[:, :m], plain[1][:, :m])
        worst["brow"] = max(worst["brow"], vc.max_ratio(np.abs(_unpad(out2, m).astype(LD) - refd), bndd))
        outd, _ = vc.apply_hook("brow", nbr, coef, M, m, self_=self_, D=D, div=1, X=X, order=1)
        assert np.array_equal(outd[:, :m], out2[:, :m])
        _unpad(outd, m)
        reft, bndt = vc.prod_reference(nbr, coef, self_, M, True)
        cols = {}
        for order in (0, 1):
            out, _ = vc.apply_hook("bcol", nbr, coef, M, m, self_=self_, X=X, order=order)
            cols[order] = out
            worst["bcol"] = max(worst.get("bcol", 0.), vc.max_ratio(np.abs(_unpad(out, m).astype(LD) - reft), bndt))
        assert np.array_equal(cols[0][:, :m], cols[1][:, :m])
    for key, v in worst.items():
        _note("vif_" + key + "_kernel", v)
        assert v < 1., (kind, m, key, v)
    print(f"products {kind} m {m}: " + ", ".join(f"{q} {v:.3g}" for q, v in worst.items()))


@pytest.mark.parametrize("kind", vc.PROD_GRAPHS)
def test_vector_products_meet_the_bounds(kind):
    _, nbr = vc.prod_graph(kind)
    coef, D, _, x = vc.prod_values(kind, 1)
    n = nbr.shape[0]
    for self_ in (0., 1.):
        for dd in (None, D):
            ref, bnd = vc.prod_reference(nbr, coef, self_, x, False, dd)
            out, _ = vc.apply_hook("bvec", nbr, coef, x, 1, self_=self_, D=dd)
            assert np.isfinite(out).all()
            r = vc.max_ratio(np.abs(out.astype(LD) - ref), bnd)
            _note("vif_bvec_kernel", r)
            assert r < 1., (kind, self_, r)
        ref, bnd = vc.prod_reference(nbr, coef, self_, x, True)
        out, _ = vc.apply_hook("btvec", nbr, coef, x, 1, self_=self_)
        assert np.isfinite(out).all() and out.shape == (n,)
        r = vc.max_ratio(np.abs(out.astype(LD) - ref), bnd)
        _note("vif_btvec_kernel", r)
        assert r < 1., (kind, self_, r)


def test_products_refusals():
    X, nbr = vc.prod_graph("lists")
    coef, D, M, x = vc.prod_values("lists", 5)

    def refused(what, op, *a, **kw):
        ret, out, _, _ = vc.apply_raw(vc.PROD_OPS[op], *a, **kw)
        assert ret == -1 and "GPB_TestVifApply" in vc.last_error() and what in vc.last_error(), vc.last_error()
        assert (out == vc.SENTINEL).all()

    nb = nbr.copy()
    nb[50, 1] = 50
    refused("not an earlier point", "brow", nb, coef, M, 5)
    nb = nbr.copy()
    nb[50, 1] = nb[50, 0]
    refused("twice", "bcol", nb, coef, M, 5)
    refused("entries", "brow", nbr, coef, M, 5, nbr_len=nbr.size - 1)
    refused("need D", "brow", nbr, coef, M, 5, div=1)
    refused("takes no D", "btvec", nbr, coef, x, 1, D=D)
    refused("m = 5000", "brow", nbr, coef, np.zeros((nbr.shape[0], 5000)), 5000)


# ------------------------------------------------------------------------------------------------ vector ops
def _vec_data(n, m):
    g = np.random.default_rng(9000 + 17 * n + m)
    return g.standard_normal((n, m)), g.standard_normal((n, m)), g.standard_normal(n), g.standard_normal(m)


@pytest.mark.parametrize("n", vc.VEC_N)
def test_vector_kernels_meet_the_bounds(n):
    for m in vc.VEC_M:
        M, M2, x, w = _vec_data(n, m)
        Ml = M.astype(LD)
        for op, arrays, olen, ref, bnd in (
                ("gemv", [M, x], m, Ml.T @ x.astype(LD), vc.gamma(n + 8) * (np.abs(M).T @ np.abs(x))),
                ("coldot_w", [M, w], n, Ml @ w.astype(LD), vc.gamma(m + 8) * (np.abs(M) @ np.abs(w))),
                ("coldot_m", [M, M2], n, (Ml * M2.astype(LD)).sum(axis=1),
                 vc.gamma(m + 8) * (np.abs(M) * np.abs(M2)).sum(axis=1))):
            out = vc.vector_hook(op, n, m, arrays, olen)
            assert np.isfinite(out).all(), op
            r = vc.max_ratio(np.abs(out.astype(LD) - ref), bnd)
            _note("vif_" + op.split("_")[0] + " kernels", r)
            assert r < 1., (op, n, m, r)
        # dK_mn / dlog phi of every covariance, d in 1..3
        for cov in range(4):
            d = 1 + (cov + m) % 3
            g = np.random.default_rng(n + m + cov)
            Xp, Z = g.uniform(size=(n, d)), g.uniform(size=(m, d))
            phi = vc.phi_of(cov, 0.3)
            out = vc.vector_hook("dkmn", n, m, [Xp, Z], n * vc.ldm_of(m), d=d, cov=cov, var=vc.VAR, phi=phi)
            out = _unpad(out.reshape(n, vc.ldm_of(m)), m)
            _, dk, arg = vc.cov_dcov(vc.dist(Xp.astype(LD), Z.astype(LD)), vc.VAR, phi, cov)
            bnd = (12 + (d + 6) * np.abs(arg).astype(np.float64)) * vc.UB * np.abs(dk).astype(np.float64)
            r = vc.max_ratio(np.abs(out.astype(LD) - dk), bnd)
            _note("vif_dkmn_kernel", r)
            assert r < 1., (cov, n, m, d, r)
    g = np.random.default_rng(n)
    dD, u, e = g.standard_normal(n), g.standard_normal(n), g.standard_normal(n)
    D = 10. ** g.uniform(-1.5, 1.5, size=n)
    out = vc.vector_hook("zvec", n, 1, [dD, u, e, D], n)
    ref = (e.astype(LD) - dD.astype(LD) * u) / D
    r = vc.max_ratio(np.abs(out.astype(LD) - ref), 4. * vc.UB * (np.abs(e) + np.abs(dD * u)) / D)
    _note("vif_zvec_kernel", r)
    assert r < 1.
    for nt in (1, 8):
        terms = vc.sum_terms(n, nt, seed=n + nt)
        ref, bnd = vc.sum_reference(terms)
        arrays = [q for a, b, c, _ in terms for q in (a, b, c)]
        out = vc.vector_hook("sum", n, 1, arrays, nt, sum_ops=[t[3] for t in terms])
        assert np.isfinite(out).all()
        r = vc.max_ratio(np.abs(out.astype(LD) - ref), bnd)
        _note("vif_sum_kernel", r)
        assert r < 1., (n, nt, r)


def test_vector_refusals():
    M, M2, x, w = _vec_data(10, 3)
    for what, args, kw in (("unknown op", (9, 10, 3, [M, x], 3), {}),
                           ("holds", (0, 10, 3, [M, x[:-1]], 3), {}),
                           ("is NULL", (0, 10, 3, [M, None], 3), {}),
                           ("out holds", (0, 10, 3, [M, x], 4), {}),
                           ("sum_ops[0]", (4, 10, 1, [x, None, None], 1), dict(sum_ops=[7])),
                           ("d = 4", (5, 10, 3, [np.ones((10, 4)), np.ones((3, 4))], 640), dict(d=4))):
        ret, out, _ = vc.vector_raw(*args, **kw)
        assert ret == -1 and "GPB_TestVifVector" in vc.last_error() and what in vc.last_error(), vc.last_error()
        assert (out == vc.SENTINEL).all()


# ------------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize("cov", [0, 1])
@pytest.mark.parametrize("n,m,nn", [(300, 20, 10), (300, 65, 31), (300, 60, 40)])
def test_model_vif_factor_matches_the_oracle(n, m, nn, cov):
    from gpboost_amd import GPModel, synthetic
    from oracle import oracle as O
    from oracle.vif_oracle import vif_factor
    X = synthetic.bench_coords(n)
    kind = dict(cov_function="exponential") if cov == 0 else dict(cov_function="matern", cov_fct_shape=1.5)
    gm = GPModel(gp_coords=X, gp_approx="full_scale_vecchia", num_ind_points=m, num_neighbors=nn, seed=3, **kind)
    cp = [0.3, 1.1, 0.2]
    f = gm.vif_factor(cp)
    assert sorted(f["perm"]) == list(range(n))
    xv, Z = X[f["perm"]], gm.inducing_points()
    nbr = f["nbr"]
    assert np.array_equal(nbr, O.find_neighbors(xv, nn))
    _, var, phi = O.transform(cov, cp)
    o = vif_factor(xv, nbr, Z, cov, var, phi)
    B, dB = np.zeros((n, nn)), np.zeros((2, n, nn))
    for i in range(n):
        k = min(i, nn)
        B[i, :k] = o["B"][i, nbr[i, :k]]
        for p in range(2):
            dB[p, i, :k] = o["dB"][p][i, nbr[i, :k]]
    np.testing.assert_allclose(f["D"], o["D"], rtol=1e-10)
    np.testing.assert_allclose(f["B"], B, rtol=1e-8, atol=1e-11)
    for p in range(2):
        assert np.abs(f["dD"][p] - o["dD"][p]).max() <= 1e-7 * np.abs(o["dD"][p]).max(), (p, "dD")
        assert np.abs(f["dB"][p] - dB[p]).max() <= 1e-7 * np.abs(dB[p]).max(), (p, "dB")
    print(f"vif_factor n {n} m {m} nn {nn} cov {cov}: D {np.abs(f['D'] / o['D'] - 1).max():.2g} rel, "
          f"dD {max(np.abs(f['dD'][p] - o['dD'][p]).max() / np.abs(o['dD'][p]).max() for p in range(2)):.2g}, "
          f"dB {max(np.abs(f['dB'][p] - dB[p]).max() / np.abs(dB[p]).max() for p in range(2)):.2g} of the largest")
    # the same factor is what an evaluation uses: the nll at these parameters is finite and reproducible
    y = synthetic.bench_spatial_gaussian_y(X)
    assert np.isfinite(gm.neg_log_likelihood(cp, y))
