"""GPU: the likelihood layer element by element. GPB_TestLikPoint runs the four device functions of csrc/lik_device.h
alone; GPB_TestLikPath runs the per-sample kernels of the grouped, full-scale Vecchia, FITC, dense and sparse Vecchia
Laplace paths on their production grids (csrc/lik_test.cpp). Everything is compared with the 80-digit mpmath
references and the derived running error bounds of tests/lik_cases.py (none tuned to a kernel;
tests/test_lik_reference.py holds float64 stand-ins to the same bounds and shows that planted defects exceed them).
Outputs and scratch start as NaN between guard bands. Run with -s for the largest error / bound ratio of every
kernel and quantity.

Bitwise claims checked here: launch_lik_dinfo gives the bits of lik_dinfo; info(l, y = 1) == info(-l, y = 0) for logit
and probit; every path's d1, W and dW (without an ObsMap) are the bits GPB_TestLikPoint gives at the same (y,
location); with w_update = 0 / W_update = 0 the stored W is left bit-identical and the derived arrays come from it;
the first / lam == 1 trial modes are the update's bits; two runs of every reduced sum agree bit for bit.

Left out (fused with the Vecchia factor): latent_scalars_kernel and the two trace kernels that sum lik_dinfo over an
ObsMap.

Largest error / bound measured on an MI355X (-s; 38 tests in 15 s):
  device functions, main grid (loglik / d1 / info / dinfo): gaussian .32 / .44 / .25 / 0, bernoulli_logit .47 / .32 /
  .25 / .24, bernoulli_probit .37 / .30 / .30 / .27, poisson .24 / .28 / .13 / .13, gamma .38 / .29 / .18 / .18;
  tail sets: bernoulli_logit .04 / .12 / .07 / .09, bernoulli_probit .33 / .12 / .43 / .44 (the series branch),
  poisson .01 / .01 / .02 / .02, gamma .08 / .08 / .43 / .43.
  glp_obs_kernel<true> d1 .34, W .26, dW .26, sum loglik (with glp_finish_kernel, both forms) .25;
  vl_prep_kernel d1 .33, W .23, dW .22, rhs .32; vl_trial_kernel trial .24, sum loglik .13;
  fl_prep_kernel d1 .33, W .23, wdw .27, DW .30, rhs .32; laplace_trial_kernel (fitc path) mnew .20, anew .19,
  sum a m .32, sum loglik .14; fl_final_kernel d1 .33, W .23, DW .29, dpwi .27, sum log dpwi .18, sum log W .09;
  dl_prep_kernel d1 .33, W .23, sqrt W .28, rhs .32; laplace_trial_kernel (dense path) mnew .20, anew .19,
  sum a m .23, sum loglik .15;
  dl_dmll_kernel dmll .11, dg .09;
  newton_prep_kernel d1 .33, W .23, rhs .32, dw .50, sdw .46; with an ObsMap d1 .32, W .23, rhs .32, dw .50, sdw .46.
With the header as it was before (p (1 - p), y - p, y l - softplus(l); erfc until it returns 0) the same device misses
the logit information's bound by 8e13 at l = 35.5 and 5e14 at l = 37.6, the probit log-likelihood's by 8e11 at
l = 38.5, y = 0 (the denormal erfc band), and the logit information is not even.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lik_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
LD = lc.LD
LIKS = sorted(lc.LIK_NAMES)
NS = lc.PATH_NS + (lc.WRAP_N,)
_worst = {}


def setup_module(module):
    lc.assert_longdouble()


def teardown_module(module):
    for key in sorted(_worst):
        print(f"[lik ops] largest error / bound, {key}: {_worst[key]:.3g}")


def _note(key, v):
    _worst[key] = max(_worst.get(key, 0.), float(v))


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _held(key, got, ref, bnd, what):
    r = lc.max_ratio(got, ref, bnd)
    _note(key, r)
    assert r < 1., (key, what, r)


# ------------------------------------------------------------------------------------------ the device functions
@pytest.mark.parametrize("lik", LIKS)
def test_point_main_grid_meets_every_bound(lik):
    for aux, y, l, ref in lc.grid_reference(lik, "main"):
        got = lc.point_hook(lik, aux, y, l)
        for q in lc.QUANTS:
            r = ref.ratios(q, got[q])
            k = int(np.argmax(r))
            _note(f"lik_{q} {lc.LIK_NAMES[lik]} main grid", r[k])
            assert r[k] < 1., (lc.LIK_NAMES[lik], q, aux, y[k], l[k], r[k], got[q][k])
        assert _same_bits(got["dinfo"], got["dinfo_lowrank"])


@pytest.mark.parametrize("lik", [lc.LOGIT, lc.PROBIT, lc.POISSON, lc.GAMMA])
def test_point_tail_set_invariants(lik):
    """finite wherever the exact value is a finite double (the infinity of its sign, never a NaN, beyond), info >= 0
    and > 0 wherever the exact information is at least DBL_MIN, d1 with the exact value's sign (wherever that value is
    at least DBL_MIN in magnitude; below, 0 is what a double can say, the wrong sign is not), and every bound, the
    series' truncation included"""
    for aux, y, l, ref in lc.grid_reference(lik, "tail"):
        got = lc.point_hook(lik, aux, y, l)
        for q in lc.QUANTS:
            assert not np.isnan(got[q]).any(), (lc.LIK_NAMES[lik], q, l[np.isnan(got[q])])
            fin = ref.representable(q)
            assert np.isfinite(got[q][fin]).all(), (lc.LIK_NAMES[lik], q, l[fin & ~np.isfinite(got[q])])
            r = ref.ratios(q, got[q])
            k = int(np.argmax(r))
            _note(f"lik_{q} {lc.LIK_NAMES[lik]} tail set", r[k])
            assert r[k] < 1., (lc.LIK_NAMES[lik], q, aux, y[k], l[k], r[k], got[q][k])
        assert (got["info"] >= 0.).all(), l[~(got["info"] >= 0.)]
        big = np.array([v >= lc.DBL_MIN for v in ref.exact_mp["info"]])
        assert (got["info"][big] > 0.).all(), l[big & ~(got["info"] > 0.)]
        sgn = np.array([float(lc.mpmath.sign(v)) for v in ref.exact_mp["d1"]])
        assert (got["d1"] * sgn >= 0.).all(), l[~(got["d1"] * sgn >= 0.)]
        bigd = np.array([abs(v) >= lc.DBL_MIN for v in ref.exact_mp["d1"]])
        assert (np.sign(got["d1"][bigd]) == sgn[bigd]).all()
        assert _same_bits(got["dinfo"], got["dinfo_lowrank"])


@pytest.mark.parametrize("lik", [lc.LOGIT, lc.PROBIT])
def test_information_is_even_bit_for_bit(lik):
    ls = np.concatenate([lc.MAIN_L, lc.BERNOULLI_TAIL_L])
    a = lc.point_hook(lik, 1., np.ones(ls.size), ls)["info"]
    b = lc.point_hook(lik, 1., np.zeros(ls.size), -ls)["info"]
    assert _same_bits(a, b), ls[a != b]


# ------------------------------------------------------------------------------------------ the paths
def _point_bits(lik, y, loc):
    return lc.point_hook(lik, lc.PATH_AUX[lik], y, loc)


def _loc(g):
    return g["mode"] if g["off"] is None else g["mode"] + g["off"]


def _cases(lik, key):
    """(n, with_offset, pool, index, gathered inputs) of a path"""
    for n in NS:
        for with_offset in (False, True):
            pl = lc.pool(lik, with_offset)
            idx = lc.sample_index(n, (key, lik))
            yield n, with_offset, pl, idx, lc.gather(pl, idx)


def _check_point_bits(lik, g, loc, d1, W, dW, what):
    pt = _point_bits(lik, g["y"], loc)
    assert _same_bits(d1, pt["d1"]), what
    if W is not None:
        assert _same_bits(W, pt["info"]), what
    if dW is not None:
        assert _same_bits(dW, pt["dinfo"]), what


@pytest.mark.parametrize("lik", LIKS)
def test_grouped_observation_pass(lik):
    aux = lc.PATH_AUX[lik]
    for n in NS:
        for with_offset in (False, True):
            for K in (1, 2, 3):
                if n > 1000 and K != 3:
                    continue
                pl = lc.pool(lik, with_offset)
                idx, glev, b, _ = lc.grouped_case(lik, with_offset, K, n)
                R = lc.grouped_reference(lik, with_offset, K)
                y, F = pl["y"][idx], (pl["off"][idx] if with_offset else None)
                eta = F.copy() if with_offset else np.zeros(n)
                for j in range(K):
                    eta = eta + b[glev[j]]
                what = (lc.LIK_NAMES[lik], n, with_offset, K)
                ll_ref, ll_bnd = R.total("loglik", idx)
                sums = []
                for want_dw in (1, 0):
                    (d1, W, dW), sc = lc.path_hook(lc.GROUPED, lc.PREP, n, lik, aux, y, None, F, idx=glev, arr0=b,
                                                   opts=(K, want_dw), want=(1, 1, want_dw), n_scalars=1)
                    _check_point_bits(lik, dict(y=y), eta, d1, W, dW, what)
                    _held("glp_obs_kernel<true> d1", d1, *R.arrays("d1", idx), what)
                    _held("glp_obs_kernel<true> W", W, *R.arrays("info", idx), what)
                    if want_dw:
                        _held("glp_obs_kernel<true> dW", dW, *R.arrays("dinfo", idx), what)
                    _held("glp_obs_kernel<true> + glp_finish_kernel sum loglik", sc, ll_ref, ll_bnd, what)
                    sums.append(sc[0])
                for _ in range(2):
                    _, sc = lc.path_hook(lc.GROUPED, lc.TRIAL, n, lik, aux, y, None, F, idx=glev, arr0=b, opts=(K, 0),
                                         n_scalars=1)
                    _held("glp_obs_kernel<false> + glp_finish_kernel sum loglik", sc, ll_ref, ll_bnd, what)
                    sums.append(sc[0])
                assert len(set(np.array(sums).view(np.uint64).tolist())) == 1, (what, sums)   # fixed order


@pytest.mark.parametrize("lik", LIKS)
def test_vif_prep_and_trial(lik):
    aux = lc.PATH_AUX[lik]
    for n, with_offset, pl, idx, g in _cases(lik, "vif"):
        what = (lc.LIK_NAMES[lik], n, with_offset)
        R = lc.prep_reference(lik, with_offset, False)
        for want_dw, want_rhs, want_count in ((1, 1, 1), (0, 1, 0), (1, 0, 1), (0, 0, 0)):
            (d1, W, dW, rhs), sc = lc.path_hook(lc.VIF, lc.PREP, n, lik, aux, g["y"], g["mode"], g["off"],
                                                opts=(want_dw, want_rhs, want_count), want=(1, 1, want_dw, want_rhs),
                                                n_scalars=want_count)
            _check_point_bits(lik, g, _loc(g), d1, W, dW, what)
            _held("vl_prep_kernel d1", d1, *R.arrays("d1", idx), what)
            _held("vl_prep_kernel W", W, *R.arrays("info", idx), what)
            if want_dw:
                _held("vl_prep_kernel dW", dW, *R.arrays("dinfo", idx), what)
            if want_rhs:
                _held("vl_prep_kernel rhs", rhs, *R.arrays("rhs", idx), what)
            if want_count:
                assert sc[0] == float((W == 0.).sum()), (what, sc)
        for lam, first, cap in ((1., 1, 0), (1., 1, 1), (0.25, 0, 1), (0.5, 0, 0)):
            T = lc.trial_reference(lik, with_offset, "vif", lam, first, cap)
            runs = [lc.path_hook(lc.VIF, lc.TRIAL, n, lik, aux, g["y"], g["mode"], g["off"], vecs=(g["upd"],), lam=lam,
                                 opts=(first, cap), want=(1,), n_scalars=1) for _ in range(2)]
            (trial,), sc = runs[0]
            if first and not cap:
                assert _same_bits(trial, g["upd"]), what
            _held("vl_trial_kernel trial", trial, *T.arrays("trial", idx), (what, lam, first, cap))
            _held("vl_trial_kernel sum loglik", sc, *T.total("loglik", idx), (what, lam, first, cap))
            assert _same_bits(sc, runs[1][1]) and _same_bits(trial, runs[1][0][0]), what


def _mix_trial(path, kernel_name, lik, n, with_offset, idx, g, what):
    aux = lc.PATH_AUX[lik]
    for lam in (1., 0.25):
        T = lc.trial_reference(lik, with_offset, "mix", lam, 0, 0)
        runs = [lc.path_hook(path, lc.TRIAL, n, lik, aux, g["y"], g["mode"], g["off"],
                             vecs=(g["a"], g["mupd"], g["aupd"]), lam=lam, want=(1, 1), n_scalars=2) for _ in range(2)]
        (mnew, anew), sc = runs[0]
        if lam == 1.:
            assert _same_bits(mnew, g["mupd"]) and _same_bits(anew, g["aupd"]), what
        _held(f"{kernel_name} mnew", mnew, *T.arrays("mnew", idx), (what, lam))
        _held(f"{kernel_name} anew", anew, *T.arrays("anew", idx), (what, lam))
        _held(f"{kernel_name} sum a m", sc[:1], *T.total("am", idx), (what, lam))
        _held(f"{kernel_name} sum loglik", sc[1:], *T.total("loglik", idx), (what, lam))
        assert _same_bits(sc, runs[1][1]), what


@pytest.mark.parametrize("lik", LIKS)
def test_fitc_prep_trial_and_final(lik):
    aux = lc.PATH_AUX[lik]
    for n, with_offset, pl, idx, g in _cases(lik, "fitc"):
        what = (lc.LIK_NAMES[lik], n, with_offset)
        for w_update in (1, 0):
            R = lc.prep_reference(lik, with_offset, not w_update)
            for want_rhs in (1, 0):
                (d1, W, wdw, DW, rhs), _ = lc.path_hook(lc.FITC, lc.PREP, n, lik, aux, g["y"], g["mode"], g["off"],
                                                        vecs=(g["dvec"], None if w_update else g["wst"]),
                                                        opts=(w_update, want_rhs), want=(1, 1, 1, 1, want_rhs))
                if w_update:
                    _check_point_bits(lik, g, _loc(g), d1, W, None, what)
                    _held("fl_prep_kernel W", W, *R.arrays("info", idx), what)
                else:
                    _check_point_bits(lik, g, _loc(g), d1, None, None, what)
                    assert _same_bits(W, g["wst"]), what                  # the stored W, untouched
                _held("fl_prep_kernel d1", d1, *R.arrays("d1", idx), what)
                _held("fl_prep_kernel wdw", wdw, *R.arrays("wdw", idx), (what, w_update))
                _held("fl_prep_kernel DW", DW, *R.arrays("DW", idx), (what, w_update))
                if want_rhs:
                    _held("fl_prep_kernel rhs", rhs, *R.arrays("rhs", idx), (what, w_update))
        _mix_trial(lc.FITC, "laplace_trial_kernel (fitc path)", lik, n, with_offset, idx, g, what)
        R = lc.prep_reference(lik, with_offset, False)
        runs = [lc.path_hook(lc.FITC, lc.FINAL, n, lik, aux, g["y"], g["mode"], g["off"], vecs=(g["dvec"],),
                             want=(1, 1, 1, 1), n_scalars=3) for _ in range(2)]
        (d1, W, DW, dpwi), sc = runs[0]
        _check_point_bits(lik, g, _loc(g), d1, W, None, what)
        _held("fl_final_kernel d1", d1, *R.arrays("d1", idx), what)
        _held("fl_final_kernel W", W, *R.arrays("info", idx), what)
        _held("fl_final_kernel DW", DW, *R.arrays("DW", idx), what)
        _held("fl_final_kernel dpwi", dpwi, *R.arrays("dpwi", idx), what)
        _held("fl_final_kernel sum log dpwi", sc[:1], *R.total("log_dpwi", idx), what)
        _held("fl_final_kernel sum log W", sc[1:2], *R.total("log_w", idx), what)
        assert sc[2] == float((W == 0.).sum()), (what, sc)
        assert _same_bits(sc, runs[1][1]), what


@pytest.mark.parametrize("lik", LIKS)
def test_dense_prep_trial_and_dmll(lik):
    aux = lc.PATH_AUX[lik]
    for n, with_offset, pl, idx, g in _cases(lik, "dense"):
        what = (lc.LIK_NAMES[lik], n, with_offset)
        R = lc.prep_reference(lik, with_offset, False)
        for want_rhs in (1, 0):
            (d1, W, ws, rhs), _ = lc.path_hook(lc.DENSE, lc.PREP, n, lik, aux, g["y"], g["mode"], g["off"],
                                               opts=(want_rhs,), want=(1, 1, 1, want_rhs))
            _check_point_bits(lik, g, _loc(g), d1, W, None, what)
            _held("dl_prep_kernel d1", d1, *R.arrays("d1", idx), what)
            _held("dl_prep_kernel W", W, *R.arrays("info", idx), what)
            _held("dl_prep_kernel sqrt W", ws, *R.arrays("ws", idx), what)
            if want_rhs:
                _held("dl_prep_kernel rhs", rhs, *R.arrays("rhs", idx), what)
        _mix_trial(lc.DENSE, "laplace_trial_kernel (dense path)", lik, n, with_offset, idx, g, what)
        if n > 1000:
            continue
        # dmll_j = 0.5 dg_j dinfo_j, dg_j = S_jj - sum_k C_kj^2 (a sum of n squares in any order)
        ld = n + 3
        r = np.random.default_rng(lc._stable_seed("dmll", lik, n))
        C = np.zeros((n, ld))
        C[:, :n] = r.normal(0., 1. / np.sqrt(n), (n, n))         # column j: C[j, :n] (column-major n x n, ld rows)
        S = np.zeros((n, ld))
        S[np.arange(n), np.arange(n)] = r.uniform(1.5, 3., n)
        C[:, n:], S[:, n:] = np.nan, np.nan                      # the ld - n padding rows are not read
        mats = np.concatenate([C.ravel(), S.ravel()])
        sq = (C[:, :n].astype(LD) ** 2).sum(axis=1)
        dg_ref = S[np.arange(n), np.arange(n)].astype(LD) - sq
        u = float(lc.U)
        dg_bnd = lc.MARGIN * (n + 2) * u * (np.abs(S[np.arange(n), np.arange(n)]) + sq.astype(float))
        di_ref, di_bnd = R.arrays("dinfo", idx)
        dm_ref = LD(0.5) * dg_ref * di_ref
        dm_bnd = 0.5 * (np.abs(dg_ref).astype(float) * di_bnd + np.abs(di_ref).astype(float) * dg_bnd) \
            + lc.MARGIN * u * np.abs(dm_ref).astype(float) + 1e-320
        for want_dg in (1, 0):
            (dmll, dg), _ = lc.path_hook(lc.DENSE, lc.FINAL, n, lik, aux, g["y"], g["mode"], g["off"], mats=mats,
                                         opts=(ld, want_dg), want=(1, want_dg))
            _held("dl_dmll_kernel dmll", dmll, dm_ref, dm_bnd, what)
            if want_dg:
                _held("dl_dmll_kernel dg", dg, dg_ref, dg_bnd, what)


@pytest.mark.parametrize("lik", LIKS)
def test_vecchia_newton_prep(lik):
    """newton_prep_kernel in its three input forms (no ObsMap; an ObsMap of 1, 2 and 7 observations per row with
    their own y and offset; an ObsMap without offsets) and four option settings"""
    aux = lc.PATH_AUX[lik]
    settings = ((1, 1, 1, 1), (1, 0, 0, 0), (0, 1, 1, 1), (0, 0, 0, 0))      # W_update, rhs, dw, sdw
    for n, with_offset, pl, idx, g in _cases(lik, "vecchia"):
        what = (lc.LIK_NAMES[lik], n, with_offset)
        for W_update, want_rhs, want_dw, want_sdw in settings:
            R = lc.prep_reference(lik, with_offset, not W_update)
            (d1, W, rhs, dw, sdw), _ = lc.path_hook(lc.VECCHIA, lc.PREP, n, lik, aux, g["y"], g["mode"], g["off"],
                                                    vecs=(g["Dinv"], None if W_update else g["wst"]),
                                                    opts=(W_update, want_rhs, want_dw, want_sdw),
                                                    want=(1, 1, want_rhs, want_dw, want_sdw))
            if W_update:
                _check_point_bits(lik, g, _loc(g), d1, W, None, what)
                _held("newton_prep_kernel W", W, *R.arrays("info", idx), what)
            else:
                _check_point_bits(lik, g, _loc(g), d1, None, None, what)
                assert _same_bits(W, g["wst"]), what
            _held("newton_prep_kernel d1", d1, *R.arrays("d1", idx), what)
            if want_rhs:
                _held("newton_prep_kernel rhs", rhs, *R.arrays("rhs", idx), (what, W_update))
                _held("newton_prep_kernel dw", dw, *R.arrays("dw", idx), (what, W_update))
                _held("newton_prep_kernel sdw", sdw, *R.arrays("sdw", idx), (what, W_update))
    for n in NS:
        for with_obs_offset in (True, False):
            pl = lc.pool(lik, True)
            idx, cnt, ptr, obs_idx = lc.obs_case(lik, n, with_obs_offset)
            what = (lc.LIK_NAMES[lik], n, "ObsMap", with_obs_offset)
            for W_update, want_rhs, want_dw, want_sdw in settings:
                R = lc.obs_reference(lik, with_obs_offset, not W_update)
                # the rows' own y is not the observations': a kernel reading y[i] for obs.y[e] misses every bound
                (d1, W, rhs, dw, sdw), _ = lc.path_hook(
                    lc.VECCHIA, lc.PREP, n, lik, aux, pl["yrow"][idx], pl["mode"][idx], None,
                    vecs=(pl["Dinv"][idx], None if W_update else pl["wst"][idx]), idx=ptr, arr0=pl["y"][obs_idx],
                    arr1=pl["off"][obs_idx] if with_obs_offset else None, opts=(W_update, want_rhs, want_dw, want_sdw),
                    want=(1, 1, want_rhs, want_dw, want_sdw))
                _held("newton_prep_kernel ObsMap d1", d1, *lc.by_count(R, "d1", idx, cnt), what)
                if W_update:
                    _held("newton_prep_kernel ObsMap W", W, *lc.by_count(R, "info", idx, cnt), what)
                else:
                    assert _same_bits(W, pl["wst"][idx]), what
                if want_rhs:
                    _held("newton_prep_kernel ObsMap rhs", rhs, *lc.by_count(R, "rhs", idx, cnt), (what, W_update))
                    _held("newton_prep_kernel ObsMap dw", dw, *lc.by_count(R, "dw", idx, cnt), (what, W_update))
                    _held("newton_prep_kernel ObsMap sdw", sdw, *lc.by_count(R, "sdw", idx, cnt), (what, W_update))


def test_zero_information_counts():
    """the W == 0 counts of vl_prep_kernel and fl_final_kernel equal the exact zeros the kernel wrote: locations
    where the information underflows (logit at +-1000, Poisson at -800) among ordinary ones, n no multiple of 256"""
    n = 300
    for lik, extreme in ((lc.LOGIT, (1000., -1000.)), (lc.POISSON, (-800., -800.))):
        pl = lc.pool(lik, False)
        g = lc.gather(pl, lc.sample_index(n, ("zeros", lik)))
        mode = g["mode"].copy()
        mode[::17], mode[5::31] = extreme
        (d1, W, dW, rhs), sc = lc.path_hook(lc.VIF, lc.PREP, n, lik, 1., g["y"], mode, None, opts=(1, 1, 1),
                                            want=(1, 1, 1, 1), n_scalars=1)
        zeros = int((W == 0.).sum())
        assert zeros == len(set(range(0, n, 17)) | set(range(5, n, 31))) and sc[0] == zeros, (lik, zeros, sc)
        assert np.isfinite(d1).all() and np.isfinite(dW).all() and np.isfinite(rhs).all()
        (d1, W2, DW, dpwi), sc = lc.path_hook(lc.FITC, lc.FINAL, n, lik, 1., g["y"], mode, None, vecs=(g["dvec"],),
                                              want=(1, 1, 1, 1), n_scalars=3)
        assert _same_bits(W, W2) and sc[2] == zeros, (lik, zeros, sc)
        assert (dpwi[W2 == 0.] == 0.).all() and (DW[W2 == 0.] == 1.).all()


def test_refusals_come_before_any_device_call():
    lik, n = lc.LOGIT, 8
    g = lc.gather(lc.pool(lik, True), np.arange(n))
    ok = dict(vecs=(g["upd"],), lam=0.5, opts=(0, 1), want=(1,), n_scalars=1)
    base = (lc.VIF, lc.TRIAL, n, lik, 1., g["y"], g["mode"], g["off"])

    def refused(args, what, **kw):
        ret, _, _, _ = lc.path_raw(*args, **dict(ok, **kw))
        assert ret == -1 and "GPB_TestLikPath" in lc.last_error() and what in lc.last_error(), lc.last_error()

    refused(base, "lam", lam=0.)
    refused(base, "takes 1 vectors", vecs=())
    refused(base, "scalars", n_scalars=0)
    refused(base, "outs[0]", want=(0,))
    refused(base, "opts[1]", opts=(0, 2))
    refused((lc.VIF, lc.FINAL) + base[2:], "no kernel")
    refused((lc.VIF, lc.TRIAL, n, 5) + base[4:], "likelihood")
    refused((lc.VIF, lc.TRIAL, n, lik, -1.) + base[5:], "aux")
    refused(base[:6] + (None,) + base[7:], "mode")
    glev = np.zeros((1, n), dtype=np.int32)
    glev[0, 3] = 2
    grouped = (lc.GROUPED, lc.PREP, n, lik, 1., g["y"], None, None)
    refused(grouped, "glev[3]", vecs=(), idx=glev, arr0=np.zeros(2), opts=(1, 0), want=(1, 1, 0))
    refused(grouped, "K =", vecs=(), idx=glev, arr0=np.zeros(3), opts=(0, 0), want=(1, 1, 0))
    ptr = np.arange(n + 1, dtype=np.int32)
    ptr[4] = 2
    vecchia = (lc.VECCHIA, lc.PREP, n, lik, 1., g["y"], g["mode"], None)
    vk = dict(vecs=(g["Dinv"], None), opts=(1, 0, 0, 0), want=(1, 1, 0, 0, 0), n_scalars=0)
    refused(vecchia, "decreases", idx=ptr, arr0=np.zeros(n), **vk)
    refused(vecchia, "ObsMap ptr", idx=np.arange(n + 1, dtype=np.int32), arr0=np.zeros(n + 1), **vk)
    refused(vecchia, "stored W", **dict(vk, opts=(0, 0, 0, 0)))
    refused(vecchia, "sdw", **dict(vk, opts=(1, 0, 0, 1), want=(1, 1, 0, 0, 1)))
    refused((lc.DENSE, lc.FINAL, n, lik, 1., g["y"], g["mode"], None), "mats", vecs=(), mats=np.zeros(2 * n * n - 1),
            opts=(n, 0), want=(1, 0), n_scalars=0)
    y, loc, out = np.zeros(4), np.zeros(4), np.zeros(4)
    gflag = lc.ctypes.c_int(-1)
    assert lc._lib().GPB_TestLikPoint(9, 1., 4, lc._dp(y), lc._dp(loc), lc._dp(out), lc._dp(out), lc._dp(out),
                                      lc._dp(out), lc._dp(out), lc.ctypes.byref(gflag)) == -1
    assert "GPB_TestLikPoint" in lc.last_error()
