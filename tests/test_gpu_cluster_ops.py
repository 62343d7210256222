"""The batched dense kernel of models with several clusters (csrc/dense_batch.hip) through GPB_TestDenseBatch:
per-cluster sums and u = Psi_c^-1 y_c, element-wise against the longdouble reference of tests/cluster_cases.py
within 8 times the float64 stand-in's own error (max norm per output over the clusters of a case)."""
import numpy as np
import pytest

import cluster_cases as cc

pytestmark = pytest.mark.gpu

CASES = [c["name"] for c in cc.op_cases()]


def _check(name, sums, u, info):
    ref, uref, rinfo, allow, _ = cc.case_reference(name)
    assert info.tolist() == rinfo.tolist()
    r = cc.ratios(name, sums, u)
    print(name, "error / allowance:", {k: round(v, 3) for k, v in r.items()})
    ok = rinfo == 0
    for j, k in enumerate(cc.OUTPUTS[:6]):
        e = np.abs(sums[ok, j].astype(cc.LD) - ref[ok, j])
        assert np.all(e <= allow[k]), (name, k, float(np.max(e)), allow[k])
    okrow = np.repeat(ok, np.diff(cc.case_data(name)[0]))
    e = np.abs(u[okrow].astype(cc.LD) - uref[okrow])
    assert np.all(e <= allow["u"]), (name, "u", float(np.max(e)), allow["u"])
    return r


@pytest.mark.parametrize("name", CASES)
def test_batch_matches_longdouble(name):
    """sizes 1, 2, 3, 31, 32, 33, 63, 64 in one launch, one cluster, 1500 clusters of 5 to 20 points, d = 1..3, the
    four covariance functions, with and without the gradient, a coincident pair (r = 0) and points 50 ranges apart"""
    sums, u, info = cc.batch_hook(name)
    _check(name, sums, u, info)
    if not cc._case_by_name(name)["want_grad"]:
        assert np.all(sums[:, 2:] == 0.)


def test_batch_without_u_gives_the_same_sums():
    a = cc.batch_hook("edge_cov1_d2")
    ret, sums, u, info = cc.batch_raw("edge_cov1_d2", want_u=False)
    assert ret == 0
    assert np.array_equal(a[0], sums) and np.array_equal(a[2], info)
    assert np.all(u == -7.)   # untouched


def test_not_positive_definite_cluster_is_flagged_alone():
    """var = 1e18 and two identical coordinates: the second pivot is exactly 0; the flag is raised for that cluster, its
    outputs are NaN, and the other clusters of the launch are as correct as ever"""
    sums, u, info = cc.batch_hook("not_pd")
    assert info.tolist() == [0, 1, 0, 0]
    ptr = cc.case_data("not_pd")[0]
    assert np.all(np.isnan(sums[1])) and np.all(np.isnan(u[ptr[1]:ptr[2]]))
    _check("not_pd", sums, u, info)


@pytest.mark.parametrize("name", ["edge_cov0_d2", "many"])
def test_batch_is_deterministic(name):
    a = cc.batch_hook(name)
    b = cc.batch_hook(name)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_batch_refuses_bad_extents():
    from gpboost_amd import GPBoostError
    with pytest.raises(GPBoostError, match="ptr"):
        ptr, X, y = cc.case_data("single")
        from gpboost_amd.basic import lib
        import ctypes
        Dp, Ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        sums, u, info = np.zeros(6), np.zeros(y.size), np.zeros(1, dtype=np.int32)
        fn = lib().GPB_TestDenseBatch
        I, L, F = ctypes.c_int, ctypes.c_int64, ctypes.c_double
        fn.argtypes = [I, I, I, Ip, L, Dp, L, Dp, L, F, F, I, Dp, L, Dp, L, Ip, L]
        ret = fn(0, 1, 2, ptr.ctypes.data_as(Ip), 1, X.ctypes.data_as(Dp), X.size, y.ctypes.data_as(Dp), y.size, 1., 1.,
                 1, sums.ctypes.data_as(Dp), 6, u.ctypes.data_as(Dp), u.size, info.ctypes.data_as(Ip), 1)
        if ret != 0:
            raise GPBoostError(lib().LGBM_GetLastError().decode())
