"""GPU: the weighted kernels of grouped random slopes element by element, through GPB_TestGroupedCreateWeighted and the
op hooks of tests/grouped_ops_cases.py, against numpy.longdouble references (tests/grouped_slope_cases.py).

Bounds: those of tests/grouped_ops_cases.py (g(j) = gamma_j at 2^-53 plus gamma_j at the reference's 2^-64; a sum of k
terms in any order costs k - 1, every further rounding on a term's way one more), with one more rounding per factor of
Z on a term's way:
  Z^T Z (host)       diagonal sum z^2, off-diagonal sum z_a z_b over k observations: the product and k - 1 sums, g(k)
                     (the bits of an exactly representable result: an empty product sum is exactly 0)
  weighted Z^T y     k terms w_e y: g(k + 1) sum |w y|
  assembly           diag_only: k terms z w: g(k + 1) sum |z w|; full: the stored z^2 or z_a z_b (1 rounding), its
                     product with w and k - 1 sums: g(k + 2) of the absolute sum
  glp_q              q_ij = z_j sum_k z_k Ainv: two more roundings than the unweighted g(K^2 + 1): g(K^2 + 3) of the
                     absolute sum for dwq, g(n K + 3) for the sums of W_i q_ij, g(n K^2 + 3) for the aux column
  glp_row_trace      g(2 K + t + 4) of the absolute sum (unweighted: 2 K + t + 2)
  glp_grad_f         g(K + 3) (|d1| + |dwq| + |W| sum |z v|)
  gre_pred_cols      E_r: at most K products summed: g(K) sum |wt Li|; var: g(M + 2 K + 2) sum_r (sum |wt Li|)^2
Designs (grouped_slope_cases.ops_design): "chunked" n = 1500 with a 750-observation level (the 512-chunk path with a
partial second chunk, for the level lists and for the intercept x slope pair lists) and pair lists below 32; "edge32"
n = 64 with lists of exactly 32 (one thread) and 33 (chunked) observations; "zero_level": a covariate that is 0 on a
whole level (structural entries of value 0, a zero diagonal of Z^T Z). Weights of mixed sign, 1e-3 .. 1e3.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grouped_ops_cases as gc  # noqa: E402
import grouped_slope_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu
LD = gc.LD
_worst = {}


def setup_module(module):
    gc.assert_longdouble()


def teardown_module(module):
    gc.free_handles()
    for key in sorted(_worst):
        print(f"[grouped slope ops] largest error / bound, {key}: {_worst[key]:.3g}")


def _ratio(key, got, ref, bnd, where):
    assert np.isfinite(got).all(), (key, where, "not finite or not written")
    r = gc.max_ratio(np.abs(got.astype(LD) - ref), bnd)
    _worst[key] = max(_worst.get(key, 0.), float(r))
    print(f"{key} {where}: {r:.3g}")
    assert r < 1., (key, where, r)


def _gen(name, salt):
    return np.random.default_rng(S.hash_name(name) + salt)


def _dec(gen, shape, lo, hi):
    return gen.choice([-1.0, 1.0], shape) * 10.0 ** gen.uniform(lo, hi, shape)


@pytest.mark.parametrize("name", S.OPS_DESIGNS)
def test_structure_and_values_of_ztz(name):
    s = S.ops_structure(name)
    key = S.weighted_handle(name)
    q = gc.info_hook(key, 1)
    M, C = s["M"], s["C"]
    assert q["M"] == M and q["K"] == C and q["nnz"] == len(s["keys"])
    assert q["cum"].tolist() == s["cum"].tolist()
    rows = np.repeat(np.arange(M), np.diff(q["rowptr"]))
    assert list(zip(rows.tolist(), q["col"].tolist())) == s["keys"]        # pairs of different components, ascending
    blk = np.repeat(np.arange(C), s["m"])
    assert (blk[rows] != blk[q["col"]]).all()                              # every single component's block stays diagonal
    for r in range(M):                                                     # split: the first entry of a higher component
        e0, e1, sp = q["rowptr"][r], q["rowptr"][r + 1], q["split"][r]
        assert (blk[q["col"][e0:sp]] < blk[r]).all() and (blk[q["col"][sp:e1]] > blk[r]).all()
    ref, ab, k = S.ref_ztz(s)
    got = np.concatenate([q["cnt"], q["val"]])
    _ratio("Z^T Z values", got, ref, gc.g(np.maximum(k, 1)) * ab, name)
    if name == "zero_level":
        zero_rows = np.nonzero(q["cnt"] == 0.0)[0]
        assert zero_rows.size == 1 and blk[zero_rows[0]] == 2              # the slope's level with x = 0: D = 1 / tau
        assert (q["val"] == 0.0).sum() >= 2 * 9                            # its structural entries, both triangles
    if name == "chunked":
        assert q["long_levels"] >= 4 and q["level_chunks"] >= 8            # 750-observation lists: 512 + 238
        assert q["long_all"] > q["long_levels"]                            # and chunked pair lists (intercept x slope)
        lens = np.array([len(s["pairs"][key_]) for key_ in s["keys"]])
        assert (lens <= 32).any() and (lens > 512).any()
    if name == "edge32":
        lens = np.array([len(lst) for lst in s["lists"]])
        assert (lens == 32).any() and (lens == 33).any()


@pytest.mark.parametrize("name", S.OPS_DESIGNS)
def test_weighted_zty_and_assembly(name):
    s = S.ops_structure(name)
    key = S.weighted_handle(name)
    gen = _gen(name, 1)
    y = _dec(gen, s["n"], -2.0, 2.0)
    zty, = gc.small_hook(key, "zty", [y], [s["M"]])
    ref, ab, k = S.ref_zty(s, y)
    _ratio("weighted gre_zty", zty, ref, gc.g(k + 1) * ab, name)
    for wv, tag in ((10.0 ** gen.uniform(-1.5, 1.5, s["n"]), "W"), (_dec(gen, s["n"], -2.0, 2.0), "signed")):
        for diag_only in (1, 0):
            ref, ab, k = S.ref_assemble(s, wv, bool(diag_only))
            first, = gc.laplace_hook(key, "assemble", [wv], [ref.size], sub=diag_only)
            again, = gc.laplace_hook(key, "assemble", [wv], [ref.size], sub=diag_only)
            assert np.array_equal(first.view(np.int64), again.view(np.int64))      # equal inputs give equal bits
            _ratio("weighted assembly diag_only" if diag_only else "weighted assembly full", first, ref,
                   gc.g(k + (1 if diag_only else 2)) * ab, f"{name} {tag}")


@pytest.mark.parametrize("name", S.OPS_DESIGNS)
def test_weighted_q_grad_f_and_row_trace(name):
    s = S.ops_structure(name)
    key = S.weighted_handle(name)
    gen = _gen(name, 2)
    M, C, n = s["M"], s["C"], s["n"]
    A = _dec(gen, (M, M), -2.0, 1.0)
    Ainv = np.tril(A) + np.tril(A, -1).T
    D = 10.0 ** gen.uniform(-1.5, 1.5, M)
    W = 10.0 ** gen.uniform(-1.5, 1.5, n)
    dW, Wa = _dec(gen, n, -2.0, 2.0), _dec(gen, n, -2.0, 2.0)
    dr, dab, sr, sab = S.ref_q(s, Ainv, W, dW)
    ld = M + 3
    for aux in (0, 1):
        dwq, sums = gc.laplace_hook(key, "q", [Ainv, D, W, dW, Wa if aux else None], [n, C + aux], sub=aux, ld=ld)
        _ratio("weighted glp_q dwq", dwq, dr, gc.g(C * C + 3) * dab, f"{name} aux={aux}")
        _ratio("weighted glp_q sums", sums[:C], sr, gc.g(n * C + 3) * sab, f"{name} aux={aux}")
        if aux:
            qi, qab = 2 * dr / S.ld(dW), 2 * dab / np.abs(S.ld(dW))
            _ratio("weighted glp_q aux", sums[C:], (S.ld(Wa) * qi).sum(keepdims=True),
                   gc.g(n * C * C + 3) * (np.abs(S.ld(Wa)) * qab).sum(keepdims=True), name)
    d1, dwq_in, v = _dec(gen, n, -2.0, 2.0), _dec(gen, n, -2.0, 2.0), _dec(gen, M, -2.0, 2.0)
    out, = gc.laplace_hook(key, "grad_f", [d1, dwq_in, W, v], [n])
    ref, ab = S.ref_grad_f(s, d1, dwq_in, W, v)
    _ratio("weighted glp_grad_f", out, ref, gc.g(C + 3) * ab, name)
    for t in (1, 5, 50):
        U, V = _dec(gen, (M, t), -2.0, 2.0), _dec(gen, (M, t), -2.0, 2.0)
        out, = gc.laplace_hook(key, "row_trace", [U.ravel(), V.ravel(), dW], [n], t=t)
        ref, ab = S.ref_row_trace(s, t, U, V, dW)
        _ratio("weighted glp_row_trace", out, ref, gc.g(2 * C + t + 4) * ab, f"{name} t={t}")


@pytest.mark.parametrize("name", S.OPS_DESIGNS)
def test_weighted_pred_cols(name):
    s = S.ops_structure(name)
    key = S.weighted_handle(name)
    gen = _gen(name, 3)
    M, C = s["M"], s["C"]
    Li = np.tril(_dec(gen, (M, M), -2.0, 1.0))
    npts = 9
    idx = np.stack([s["cum"][c] + gen.integers(0, s["m"][c], npts) for c in range(C)], axis=1).astype(np.int32)
    idx[1, 0] = -1               # an unseen level
    idx[2, :] = -1               # a point without a seen level: exactly 0
    wt = _dec(gen, (npts, C), -3.0, 3.0)
    wt[3, 1] = 0.0               # a covariate of exactly 0
    ld = M + 5
    E_ref, E_ab, v_ref, v_ab = S.ref_pred(s, Li, idx, wt)
    full = np.where(np.tril(np.ones((M, M), bool)), Li, np.nan)      # NaN above the diagonal: finite = never read
    E, = gc.dense_hook(key, "pred_e", ld, [full, wt.ravel()], [ld * npts], idx=idx)
    E = E.reshape(npts, ld)
    assert np.isnan(E[:, M:]).all()
    _ratio("weighted gre_pred_cols E", E[:, :M].T, E_ref, gc.g(C) * E_ab, name)
    var, = gc.dense_hook(key, "pred_var", ld, [full, wt.ravel()], [npts], idx=idx)
    _ratio("weighted gre_pred_cols var", var, v_ref, gc.g(M + 2 * C + 2) * v_ab, name)
    assert (E[2, :M] == 0).all() and var[2] == 0.0
    with pytest.raises(gc.HookError):                                # the weighted handle needs wt
        gc.dense_hook(key, "pred_var", ld, [full], [npts], idx=idx)
