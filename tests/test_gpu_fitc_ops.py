"""GPU: the FITC kernels of csrc/fitc_kernels.hip and csrc/fitc_fisher.hip element by element through the
GPB_TestFitcVector / GPB_TestFitcKmeans hooks (csrc/fitc_test.cpp, the launch functions FitcSolver and
fitc_inducing_points use) against the longdouble references and the derived bounds of tests/fitc_ops_cases.py (none
tuned to a kernel; tests/test_fitc_ops_reference.py holds float64 stand-ins to the same bounds). The ld-m padding of
every input holds NaN, outputs and scratch start as NaN between guard bands. Run with -s for the largest error /
bound ratio of every kernel.

Bitwise claims checked here: results do not depend on the padding's fill (NaN against 0); fitc_lower_t_kernel is an
exact transpose with exact zeros above the diagonal and never reads L's upper triangle; K_mm's diagonal is var,
K_mm,s's var (1 + 1e-6), dK_mm's 0, and K_mm,s = K_mm off it; ff_rowscale_kernel with Y aliasing Yin gives the bits
of the separate buffers; the k-means assignment, means, partition arrays and the whole Lloyd loop equal the float64
numpy reference that performs the documented operations in the documented order, and the scanning means kernel gives
the bits of the member-list path on every case and through the loop.

Stages (GPB_TestFitcStages): the buffers of a FitcSolver after Factor, Eval with the gradient and Predict, array by
array (tests/fitc_ops_cases.py says which array is held to which bound); Gram -> Eval at the same and at other
parameters bit-identical to a fresh Eval in every buffer and sum; Predict with several prediction points matched to
one training point against the dense correction."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fitc_ops_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu
LD = fc.LD
_worst = {}
KERNEL = {"kmn": "fitc_kmn_kernel", "kmm": "fitc_kmm_kernel", "dkmn": "ff_dkmn_kernel", "diag": "fitc_diag_kernel",
          "dy": "fitc_dy_kernel", "wsum": "fitc_wsum_kernel", "gemv": "fitc_gemv_part/reduce_kernel",
          "symv": "fitc_symv_kernel", "lower_t": "fitc_lower_t_kernel", "chol_solve": "fitc_symv + trmv_lower_t_kernel",
          "yaux": "fitc_yaux_kernel", "grad": "fitc_grad_kernel", "mm_terms": "fitc_mm_kernel",
          "coldot": "fitc_coldot_kernel", "pred_corr": "fitc_pred_corr_kernel", "ff_diag_grad": "ff_diag_grad_kernel",
          "ff_recip": "ff_recip_kernel", "ff_rowscale": "ff_rowscale_kernel", "ff_dot": "ff_dot_kernel"}


def setup_module(module):
    fc.assert_longdouble()


def teardown_module(module):
    for key in sorted(_worst):
        print(f"[fitc ops] largest error / bound, {key}: {_worst[key]:.3g}")


def _note(key, v):
    _worst[key] = max(_worst.get(key, 0.), float(v))


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a) and a.keys() == b.keys()


# ------------------------------------------------------------------------------------------------ vector ops
@pytest.mark.parametrize("op", tuple(fc.VEC_OPS))
def test_vector_kernels_meet_the_bounds(op):
    for name, c in fc.vec_cases(op).items():
        res, pads = fc.vector_hook(c)
        res0, pads0 = fc.vector_hook(c, pad_fill=0.)
        assert _same(res, res0), (name, "the result depends on the padding's fill")
        for k, p in pads.items():
            # the padding of every output holds what it held: the start value NaN, Maux (in place) the fill
            assert np.isnan(p).all(), (name, k, "output padding written")
            assert (pads0[k] == 0.).all() if op == "pred_corr" else np.isnan(pads0[k]).all(), (name, k)
        if op == "pred_corr" and not c["pairs"]:
            assert np.array_equal(res["Maux"], c["arrays"][3]) and np.isnan(res["corr"]).all(), name
            continue
        for k, v in res.items():
            assert np.isfinite(v).all(), (name, k, "not finite or not written")
        for k, r in fc.ratios(c, res).items():
            _note(f"{KERNEL[op]} {k}", r)
            assert r < 1., (name, k, r)


def test_lower_t_is_an_exact_transpose():
    for name, c in fc.vec_cases("lower_t").items():
        res, _ = fc.vector_hook(c)
        ref = fc.lower_t_ref(c["arrays"][0])
        assert np.array_equal(res["LT"], ref), name
        assert not np.signbit(res["LT"][ref == 0.]).any()


def test_kmm_diagonals_are_exact():
    for name, c in fc.vec_cases("kmm").items():
        res, _ = fc.vector_hook(c)
        m = c["m"]
        off = ~np.eye(m, dtype=bool)
        assert (np.diag(res["Kmm"]) == c["var"]).all(), name
        assert (np.diag(res["Ks"]) == np.float64(c["var"]) * np.float64(fc.JIT)).all(), name
        assert (np.diag(res["dK"]) == 0.).all(), name
        assert np.array_equal(res["Ks"][off], res["Kmm"][off]), name
        assert np.array_equal(res["Kmm"], res["Kmm"].T) and np.array_equal(res["dK"], res["dK"].T), name
        if m >= 4:
            assert res["Kmm"][0, 1] == c["var"] and res["dK"][0, 1] == 0., name  # r = 0 off the diagonal


def test_kmn_special_pairs():
    for op in ("kmn", "dkmn"):
        for name, c in fc.vec_cases(op).items():
            res, _ = fc.vector_hook(c)
            assert res["K"][-1, 0] == (c["var"] if op == "kmn" else 0.), name     # the coincident pair
            if c["n"] >= 3:
                assert (res["K"][1] == 0.).all(), name                            # exp underflows to 0


def test_rowscale_alias_gives_the_same_bits():
    cs = fc.vec_cases("ff_rowscale")
    for name, c in cs.items():
        if name.endswith("-alias"):
            a, _ = fc.vector_hook(c)
            b, _ = fc.vector_hook(cs[name[:-6] + "-yin"])
            assert np.array_equal(a["Y"], b["Y"]), name


def test_vector_refusals():
    def refused(what, c, **over):
        ret, _, _, _, outs = fc.vector_raw(c, **over)
        assert ret == -1 and "GPB_TestFitcVector" in fc.last_error() and what in fc.last_error(), (what, fc.last_error())
        assert all((o == fc.SENTINEL).all() for o in outs)

    c = fc.vec_cases("gemv")["gemv-n5-m3"]
    refused("n = 0", c, n=0)
    refused("m = 5000", c, m=5000)
    refused("holds", c, m=65)                        # m > the arrays' extent
    refused("holds", c, n=6)
    refused("is NULL", c, arrays=[c["arrays"][0], None])
    refused("takes no ints", c, ints=[1])
    refused("op 6 writes", c, out_lens=[4])
    c = fc.vec_cases("kmn")["kmn-0-exponential-d1-n9-m65"]
    for d in (0, 4):
        refused(f"d = {d}", c, d=d)
    refused("cov_type = 4", c, cov=4)
    refused("var and phi", c, phi=0.)
    bad = [c["arrays"][0].copy(), c["arrays"][1]]
    bad[0][3, 0] = np.inf
    refused("not finite", c, arrays=bad)
    c = fc.vec_cases("wsum")["wsum-c2-m3"]
    refused("chunks", c, ints=[0])
    refused("holds", c, ints=[3])
    c = fc.vec_cases("pred_corr")["pred_corr-m50-one"]
    refused("out of range", c, ints=[12, 12, 3])     # prediction point = np
    refused("out of range", c, ints=[12, 3, 40])     # training point = n
    refused("out of range", c, ints=[12, -1, 3])
    refused("paired twice", c, ints=[12, 3, 1, 3, 2])
    ret = fc._lib().GPB_TestFitcVector(99, 1, 1, 1, 0, 1., 1., 0., 0., None, None, 0, None, 0, None, None, 0, None)
    assert ret == -1 and "unknown op" in fc.last_error()


# ------------------------------------------------------------------------------------------------ k-means
@pytest.mark.parametrize("name", sorted(fc.km_cases()))
def test_kmeans_step_equals_the_reference_bit_for_bit(name):
    X, mu = fc.km_cases()[name]
    n, k = X.shape[0], mu.shape[0]
    _, cl, _ = fc.kmeans_hook("assign", X, mu)
    ref_cl = fc.km_assign(X, mu)
    assert np.array_equal(cl, ref_cl)
    ref_mu = fc.km_means(X, ref_cl, mu)
    mu_list, ints, _ = fc.kmeans_hook("means", X, mu, cluster=ref_cl, scan=0)
    mu_scan, _, _ = fc.kmeans_hook("means", X, mu, cluster=ref_cl, scan=1)
    assert np.array_equal(mu_list, ref_mu), "member-list means"
    assert np.array_equal(mu_scan, ref_mu), "scanning means"
    assert np.array_equal(mu_scan.view(np.int64), mu_list.view(np.int64)), "scan path != list path"
    for got, ref, what in zip(fc.split_partition(ints, n, k), fc.km_partition(ref_cl, k),
                              ("cnt", "off", "tot", "base", "list")):
        assert np.array_equal(got, ref), what
    # an assignment that is not the nearest-centre one: every point in the last cluster but one, the rest empty
    cl2 = np.full(n, k - 1, dtype=np.int32)
    cl2[n // 2] = 0
    for scan in (0, 1):
        got, _, _ = fc.kmeans_hook("means", X, mu, cluster=cl2, scan=scan)
        assert np.array_equal(got, fc.km_means(X, cl2, mu)), scan


def test_kmeans_sqrt_ties_keep_the_earlier_centre():
    for X, mu in fc.sqrt_tie_cases():
        _, cl, _ = fc.kmeans_hook("assign", np.repeat(X, 2, axis=0), mu)      # k <= n: the point twice
        assert (cl == 0).all(), mu


def test_kmeans_cmp_flags():
    g = np.random.default_rng(5)
    for k, d in ((1, 1), (65, 3), (257, 2)):                                  # 514 entries: the second thread stride
        mu = g.uniform(size=(k, d))
        a, b = mu.copy(), mu.copy()
        assert tuple(fc.kmeans_hook("cmp", None, mu, mu_a=a, mu_b=b)[1]) == (0, 0)
        b[k - 1, d - 1] = np.nextafter(b[k - 1, d - 1], 2.)
        assert tuple(fc.kmeans_hook("cmp", None, mu, mu_a=a, mu_b=b)[1]) == (0, 1)
        a[0, 0] += 1.
        assert tuple(fc.kmeans_hook("cmp", None, mu, mu_a=a, mu_b=b)[1]) == (1, 1)
        assert tuple(fc.kmeans_hook("cmp", None, mu, mu_a=a, mu_b=mu.copy())[1]) == (1, 0)
    z = np.zeros((3, 2))
    assert tuple(fc.kmeans_hook("cmp", None, z, mu_a=-z, mu_b=z)[1]) == (0, 0)   # -0 == 0, as the reference's ==


@pytest.mark.parametrize("name", sorted(fc.lloyd_cases()))
def test_lloyd_equals_the_reference_bit_for_bit(name):
    X, seeds, cap = fc.lloyd_cases()[name]
    ref_mu, ref_its = fc.km_lloyd(X, seeds, cap)
    for scan in (0, 1):
        mu, _, its = fc.kmeans_hook("lloyd", X, seeds, scan=scan, max_it=cap)
        assert its == ref_its, (scan, its, ref_its)
        assert np.array_equal(mu, ref_mu), scan
    print(f"lloyd {name}: {ref_its} iterations")


def test_kmeans_refusals():
    X, mu = [v for key, v in fc.km_cases().items() if key.startswith("cloud-n64-k7-")][0]
    X, mu = X[:, :1].copy(), mu[:, :1].copy()

    def refused(what, op, *a, **kw):
        ret, mu_out, ints, _, _ = fc.kmeans_raw(op, *a, **kw)
        assert ret == -1 and "GPB_TestFitcKmeans" in fc.last_error() and what in fc.last_error(), (what, fc.last_error())
        assert (mu_out == fc.SENTINEL).all() and (ints == fc.INT_SENTINEL).all()

    refused("n = 0", "assign", X, mu, n=0, ints_len=0)
    refused("clusters for n", "assign", X[:5], mu)                            # cluster count > n
    refused("d = 4", "assign", X, mu, d=4)
    refused("d = 0", "assign", X, mu, d=0)
    refused("X holds", "assign", X, mu, n=65)
    refused("ints_out holds", "assign", X, mu, ints_len=63)
    cl = np.zeros(64, dtype=np.int32)
    cl[9] = 7
    refused("cluster_in[9] = 7", "means", X, mu, cluster=cl)
    cl[9] = -1
    refused("cluster_in[9] = -1", "means", X, mu, cluster=cl)
    refused("max_it = 0", "lloyd", X, mu, max_it=0)
    bad = X.copy()
    bad[3, 0] = np.nan
    refused("not finite", "assign", bad, mu)


# ------------------------------------------------------------------------------------------------ stages
STAGE_NAMES = sorted(fc.STAGE_CASES)
CHAIN = ("Li", "Kinv", "V", "W", "Wi", "A", "Winv", "Gt", "M")     # Cholesky, TRTRI and GEMM outputs: 8 x stand-in
EVAL_OUTS = tuple(k for k in fc.STAGE_OUTS if k not in ("mean", "var", "cov"))


def _kernel_check(tag, c, out):
    """the kernel's own bound for the arrays of `out`, from the inputs the GPU itself used"""
    ref = fc.compute(c, LD)
    bnd, _ = fc.bounds(c)
    for k, v in out.items():
        r = fc.max_ratio(np.abs(v.reshape(ref[k].shape).astype(LD) - ref[k]), np.broadcast_to(bnd[k], ref[k].shape))
        _note(f"stage {tag} {k}", r)
        assert r < 1., (tag, k, r)


def _stage_check(name, res, rename=None):
    """array by array: the covariances within their derived bound; the Cholesky / TRTRI / GEMM chain within 8 x the
    float64 stand-in's error; everything within 1e-8 of the array's scale of the longdouble reference; the transposed
    factors exact"""
    q = fc.stage_inputs(name)
    ref, allow, _ = fc.stage_reference(name)
    c = dict(var=q["var"], phi=q["phi"], cov=q["cov"], d=q["d"])
    cb = {"Kmn": fc.cov_bound(c, q["X"], q["Z"], False), "Kmm": fc.cov_bound(c, q["Z"], q["Z"], False),
          "dKmm": fc.cov_bound(c, q["Z"], q["Z"], True)}
    cb["Ks"] = cb["Kmm"] + fc.UB * q["var"] * fc.JIT * np.eye(q["m"])
    for k, v in res.items():
        if k == "sums":
            continue
        rk = (rename or {}).get(k, k)
        assert np.isfinite(fc.defined(k, v)).all(), (name, k)
        err = np.abs(fc.defined(k, v).astype(LD) - fc.defined(k, ref[rk])).astype(np.float64)
        scale = float(np.max(fc.af(ref[rk])))
        assert err.max() <= 1e-8 * scale, (name, rk, err.max(), scale)
        if rk in cb:
            r = fc.max_ratio(err, cb[rk])
            _note(f"stage {rk} (covariance bound)", r)
            assert r < 1., (name, rk, r)
        elif rk in CHAIN:
            _note(f"stage {rk} (8 x stand-in)", err.max() / allow[rk])
            assert err.max() <= allow[rk], (name, rk, err.max(), allow[rk])
        else:
            _note(f"stage {rk} (8 x stand-in, printed only)", err.max() / allow[rk])
    m = q["m"]
    assert (np.diag(res["Kmm"]) == q["var"]).all() and (np.diag(res["dKmm"]) == 0.).all()
    assert (np.diag(res["Ks"]) == np.float64(q["var"]) * np.float64(fc.JIT)).all()
    assert np.array_equal(res["Ks"][~np.eye(m, dtype=bool)], res["Kmm"][~np.eye(m, dtype=bool)])
    assert np.array_equal(res["LiT"], fc.lower_t_ref(res["Li"])) and np.array_equal(res["WiT"], fc.lower_t_ref(res["Wi"]))


@pytest.mark.parametrize("name", STAGE_NAMES)
def test_stage_factor_array_by_array(name):
    q = fc.stage_inputs(name)
    n, m = q["n"], q["m"]
    res = fc.stage_hook(name, "factor", fc.FACTOR_OUTS)
    _stage_check(name, res)
    # each column kernel against its own bound on the buffers the GPU handed it (the aliasing of part_ and of the
    # a slot as fitc_chol_solve's scratch shows here)
    base = dict(n=n, m=m, d=q["d"], cov=q["cov"], var=q["var"], phi=q["phi"], ints=None)
    _kernel_check("diag", dict(base, op="diag", arrays=[res["V"], res["Kmn"]], extra=1. + q["var"] * fc.JIT),
                  {"d": res["d"], "Kd": res["Kd"]})
    _kernel_check("dy", dict(base, op="dy", arrays=[res["d"], q["y"]], extra=0.), {"Dy": res["Dy"]})
    _kernel_check("gemv u", dict(base, op="gemv", arrays=[res["Kmn"], res["Dy"]], extra=0.), {"out": res["u"]})
    Wi = res["Wi"].copy()
    Wi[np.tril_indices(m, -1)] = np.nan                      # the factor's undefined triangle must not matter
    _kernel_check("chol_solve w", dict(base, op="chol_solve", arrays=[Wi, res["WiT"], res["u"]], extra=0.),
                  {"out": res["w"]})
    _kernel_check("yaux", dict(base, op="yaux", arrays=[res["Kmn"], res["w"], q["y"], res["Dy"], res["d"]], extra=0.),
                  {"yaux": res["yaux"]})


@pytest.mark.parametrize("name", STAGE_NAMES)
def test_stage_eval_array_by_array_and_the_kept_path(name):
    q = fc.stage_inputs(name)
    n, m = q["n"], q["m"]
    res = fc.stage_hook(name, "eval", EVAL_OUTS)
    _stage_check(name, res, rename={"V": "M", "Kd": "Gt"})   # the gradient leaves M = dK_mm A in V, G^T in K_d
    base = dict(n=n, m=m, d=q["d"], cov=q["cov"], var=q["var"], phi=q["phi"], ints=None)
    _kernel_check("gemv a", dict(base, op="gemv", arrays=[res["A"], res["yaux"]], extra=0.), {"out": res["a"]})
    # the sums from the GPU's own buffers: the gradient kernel's and the m x m kernel's bounds together
    cg = dict(base, op="grad", extra=q["var"] * fc.JIT - q["var"],
              arrays=[q["X"], q["Z"], res["Kmn"], res["A"], res["Kd"], res["V"], res["a"], res["d"], res["yaux"]])
    cm = dict(base, op="mm_terms", arrays=[res["Kinv"], res["Winv"], res["Kmm"], res["dKmm"], res["a"]], extra=0.)
    g, t = fc.compute(cg, LD)["sums"], fc.compute(cm, LD)["sums"]
    eg, et = fc.bounds(cg)[0]["sums"], fc.bounds(cm)[0]["sums"]
    want = np.array([g[0] + t[4] / 2, g[1] + t[5] / 2, g[2] - t[0] + t[1], g[3] - t[2] + t[3]])
    bnd = np.array([eg[0] + et[4] / 2, eg[1] + et[5] / 2, eg[2] + et[0] + et[1], eg[3] + et[2] + et[3]])
    bnd = bnd + 3 * fc.UB * (np.abs(g.astype(np.float64)) + np.abs(t.astype(np.float64))[[4, 5, 0, 2]]
                             + np.abs(t.astype(np.float64))[[4, 5, 1, 3]])
    r = fc.max_ratio(np.abs(res["sums"][2:].astype(LD) - want), bnd)
    _note("stage sums (grad + mm bounds)", r)
    assert r < 1., (name, r)
    # the far end: the project's scalar tolerances against the longdouble chain
    ref = fc.stage_reference(name)[0]["sums"]
    rel = np.abs((res["sums"].astype(LD) - ref) / ref).astype(np.float64)
    print(f"stage {name}: sums relative errors {rel}")
    assert (rel[:2] <= 1e-9).all() and (rel[2:] <= 1e-7).all(), rel
    # Gram then Eval at the same parameters takes the kept factorization, at other parameters it must not: both give
    # the bits of a fresh Eval in every buffer and sum
    for stage in ("gram_eval", "gram_other_eval"):
        other = fc.stage_hook(name, stage, EVAL_OUTS)
        for k in EVAL_OUTS:
            assert np.array_equal(fc.defined(k, other[k]).view(np.int64), fc.defined(k, res[k]).view(np.int64)), \
                (name, stage, k)


@pytest.mark.parametrize("name", STAGE_NAMES)
def test_stage_predict_groups_the_pairs(name):
    ref, allow, _ = fc.stage_reference(name)
    res = fc.stage_hook(name, "predict", ("mean", "var", "cov"))
    for k in ("mean", "var", "cov"):
        assert np.isfinite(res[k]).all()
        err = float(np.max(np.abs(res[k].astype(LD) - ref[k])))
        scale = float(np.max(fc.af(ref[k])))
        _note(f"stage predict {k} (8 x stand-in)", err / allow[k])
        assert err <= allow[k] and err <= 1e-9 * scale, (name, k, err, allow[k], scale)
    assert np.array_equal(np.diag(res["cov"]), np.diag(res["cov"].T))
    # without the covariance the mean and the variances keep their bits
    res2 = fc.stage_hook(name, "predict", ("mean", "var"))
    assert np.array_equal(res2["mean"], res["mean"])
    assert np.max(np.abs(res2["var"] - np.diag(res["cov"]))) <= allow["var"] + allow["cov"]


def test_stage_refusals():
    name = STAGE_NAMES[0]
    q = fc.stage_inputs("n37-m5-d1-exponential")

    def refused(what, stage, want, **over):
        ret, res = fc.stage_raw("n37-m5-d1-exponential", stage, want, **over)
        assert ret == -1 and "GPB_TestFitcStages" in fc.last_error() and what in fc.last_error(), (what, fc.last_error())
        assert all((np.asarray(v) == fc.SENTINEL).all() for v in res.values())

    refused("n = 0", "factor", ("d",), n=0)
    refused("m = 38", "factor", ("d",), m=38)
    refused("d = 4", "factor", ("d",), d=4)
    refused("var and phi", "gram_other_eval", ("d",), phi2=-1.)
    refused("holds 0 entries", "factor", ("mean",))
    refused("does not belong", "predict", ("sums", "mean"))
    bad = q["match"].copy()
    bad[2] = 37
    refused("match[2] = 37", "predict", ("mean",), match=bad)
    bad[2] = -2
    refused("match[2] = -2", "predict", ("mean",), match=bad)
    yb = q["y"].copy()
    yb[5] = np.inf
    refused("not finite", "factor", ("d",), y=yb)
    assert name
