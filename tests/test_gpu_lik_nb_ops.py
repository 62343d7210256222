"""GPU: the negative binomial likelihood layer element by element (likelihood id 5; grouped random effects only).

GPB_TestLikPoint / GPB_TestLikAuxPoint run the nb_* device functions of csrc/lik_device.h alone: the four quantities
of every likelihood and the two shape derivatives with the per-observation term of the explicit shape gradient.
GPB_TestLikPath on the grouped path runs glp_obs_kernel<true / false> (kernels 0 / 1) and glp_nb_aux_kernel (kernel
2), each followed by glp_finish_kernel, on the production grid.

References and bounds: tests/lik_nb_cases.py (80-digit mpmath closed forms; first-order running error bounds of the
header's own formulas; tests/test_lik_nb_reference.py checks them on the CPU). Every per-observation array a kernel
writes is compared with its bound and, bit for bit, with what the point hooks give at the same (y, eta): a kernel
calls the same device functions. The block sums are compared within the bound of a sum in any order and are equal bit
for bit from call to call (fixed order). Every hook checks its guard flag (lik_cases.point_hook / path_hook and
lik_nb_cases.point_hook assert it is 0).

Sizes: PATH_NS and WRAP_N of tests/lik_cases.py (one block, the block edges, several blocks, and the size at which
the grid-stride loop of the 1024-block grid wraps), K = 1, 2, 3 with GROUP_LEVELS.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lik_cases as lc  # noqa: E402
import lik_nb_cases as nb  # noqa: E402

pytestmark = pytest.mark.gpu
NS = lc.PATH_NS + (lc.WRAP_N,)
_worst = {}


def setup_module(module):
    lc.assert_longdouble()


def teardown_module(module):
    for key in sorted(_worst):
        print(f"[lik nb ops] largest error / bound, {key}: {_worst[key]:.3g}")


def _note(key, v):
    _worst[key] = max(_worst.get(key, 0.), float(v))


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _held(key, got, ref, bnd, what):
    r = lc.max_ratio(got, ref, bnd)
    _note(key, r)
    assert r < 1., (key, what, r)


@pytest.mark.parametrize("which", ["main", "tail"])
def test_point_grids_meet_every_bound(which):
    for r, y, ls, ref in nb.grid_reference(which):
        got = nb.point_hook(r, np.full(ls.size, y), ls)
        for q in nb.NB_QUANTS:
            assert np.isfinite(got[q]).all(), (which, q, r, y, ls[~np.isfinite(got[q])])
            rr = ref.ratios(q, got[q])
            k = int(np.argmax(rr))
            _note(f"nb_{q} {which}", rr[k])
            assert rr[k] < 1., (which, q, r, y, ls[k], rr[k], got[q][k])
        assert (got["info"] >= 0.).all(), (which, r, y, ls[~(got["info"] >= 0.)])


def test_point_hooks_refuse_what_they_do_not_have():
    y, loc, out = np.zeros(4), np.zeros(4), np.zeros(4)
    g = lc.ctypes.c_int(-1)
    lib = nb._lib()
    for lik in (lc.GAMMA, 9):   # the general shape derivatives are this likelihood's
        assert lib.GPB_TestLikAuxPoint(lik, 1., 4, lc._dp(y), lc._dp(loc), lc._dp(out), lc._dp(out), lc._dp(out),
                                       lc.ctypes.byref(g)) == -1
        assert "GPB_TestLikAuxPoint" in lc.last_error() and "likelihood" in lc.last_error()
    assert lib.GPB_TestLikAuxPoint(nb.NB, -1., 4, lc._dp(y), lc._dp(loc), lc._dp(out), lc._dp(out), lc._dp(out),
                                   lc.ctypes.byref(g)) == -1
    assert "aux" in lc.last_error()
    # every path but the grouped one refuses the id before any device call, with its own name
    n = 8
    gth = lc.gather(lc.pool(lc.LOGIT, True), np.arange(n))
    for path, kw in ((lc.VIF, dict(vecs=(gth["upd"],), lam=0.5, opts=(0, 1), want=(1,), n_scalars=1)),
                     (lc.FITC, dict(vecs=(gth["a"], gth["mupd"], gth["aupd"]), want=(1, 1), n_scalars=2)),
                     (lc.DENSE, dict(vecs=(gth["a"], gth["mupd"], gth["aupd"]), want=(1, 1), n_scalars=2))):
        ret, _, _, _ = lc.path_raw(path, lc.TRIAL, n, nb.NB, 1., gth["y"], gth["mode"], gth["off"], **kw)
        assert ret == -1 and "GPB_TestLikPath" in lc.last_error() and "likelihood" in lc.last_error()
        assert lc.PATH_NAMES[path] in lc.last_error(), lc.last_error()
    # the shape pass is this likelihood's alone
    glev = np.zeros((1, n), dtype=np.int32)
    ret, _, _, _ = lc.path_raw(lc.GROUPED, lc.FINAL, n, lc.POISSON, 1., gth["y"], None, None, idx=glev,
                               arr0=np.zeros(2), opts=(1,), want=(1, 1), n_scalars=1)
    assert ret == -1 and "no kernel" in lc.last_error()


@pytest.mark.parametrize("K", [1, 2, 3])
def test_grouped_observation_pass_and_shape_pass(K):
    aux = nb.NB_PATH_AUX
    for n in NS:
        if n > 1000 and K != 3:
            continue
        for with_offset in (False, True):
            pl = nb.pool(with_offset)
            idx, glev, b, eta = nb.eta64(with_offset, K, n)
            R = nb.grouped_reference(with_offset, K)
            y, F = pl["y"][idx], (pl["off"][idx] if with_offset else None)
            what = (n, with_offset, K)
            pt = nb.point_hook(aux, y, eta)
            ll_ref, ll_bnd = R.total("loglik", idx)
            sums = []
            for want_dw in (1, 0):
                (d1, W, dW), sc = lc.path_hook(lc.GROUPED, lc.PREP, n, nb.NB, aux, y, None, F, idx=glev, arr0=b,
                                               opts=(K, want_dw), want=(1, 1, want_dw), n_scalars=1)
                assert _same_bits(d1, pt["d1"]) and _same_bits(W, pt["info"]), what
                _held("glp_obs_kernel<true> d1", d1, *R.arrays("d1", idx), what)
                _held("glp_obs_kernel<true> W", W, *R.arrays("info", idx), what)
                if want_dw:
                    assert _same_bits(dW, pt["dinfo"]), what
                    _held("glp_obs_kernel<true> dW", dW, *R.arrays("dinfo", idx), what)
                _held("glp_obs_kernel<true> + glp_finish_kernel sum loglik", sc, ll_ref, ll_bnd, what)
                sums.append(sc[0])
            for _ in range(2):
                _, sc = lc.path_hook(lc.GROUPED, lc.TRIAL, n, nb.NB, aux, y, None, F, idx=glev, arr0=b, opts=(K, 0),
                                     n_scalars=1)
                _held("glp_obs_kernel<false> + glp_finish_kernel sum loglik", sc, ll_ref, ll_bnd, what)
                sums.append(sc[0])
            assert len(set(np.array(sums).view(np.uint64).tolist())) == 1, (what, sums)   # fixed order
            # the shape pass: dd1 / dlog r, dW / dlog r and the sum of log(mu + r) + (y + r) / (mu + r)
            t_ref, t_bnd = R.total("aux_term", idx)
            terms = []
            for _ in range(2):
                (dd1a, dWa), sc = lc.path_hook(lc.GROUPED, lc.FINAL, n, nb.NB, aux, y, None, F, idx=glev, arr0=b,
                                               opts=(K,), want=(1, 1), n_scalars=1)
                assert _same_bits(dd1a, pt["dd1_aux"]) and _same_bits(dWa, pt["dinfo_aux"]), what
                _held("glp_nb_aux_kernel dd1_aux", dd1a, *R.arrays("dd1_aux", idx), what)
                _held("glp_nb_aux_kernel dW_aux", dWa, *R.arrays("dinfo_aux", idx), what)
                _held("glp_nb_aux_kernel + glp_finish_kernel sum aux_term", sc, t_ref, t_bnd, what)
                terms.append(sc[0])
            assert terms[0].tobytes() == terms[1].tobytes(), (what, terms)
