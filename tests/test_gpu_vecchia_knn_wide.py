"""The wave-per-row neighbour search for 65 to 128 neighbours (knn_wide_kernel, csrc/vecchia_knn.hip) through
GPB_TestVecchiaNeighbors and through GPModel, against the CPU oracle's restatement of the reference: integers, equal."""
import ctypes as c
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (65, 96, 127, 128)


def _coords(kind, n, d):
    """bench_coords; integer lattice, shuffled (equal distances and coordinate sums); dup: every point twice"""
    from gpboost_amd import synthetic
    rng = np.random.default_rng(n + d)
    if kind == "lattice":
        g = np.indices((int(np.ceil(n ** (1. / d))),) * d).reshape(d, -1).T.astype(np.float64)
        return g[rng.permutation(len(g))[:n]].copy()
    x = synthetic.bench_coords(n, d)
    return x if kind == "bench" else np.vstack([x[:(n + 1) // 2]] * 2)[rng.permutation(2 * ((n + 1) // 2))[:n]].copy()


def _search(x, m, r0, r1, end_at, use_gpu):
    from gpboost_amd import basic
    out = np.full((r1 - r0, m), -7, dtype=np.int32)
    fn = basic.lib().GPB_TestVecchiaNeighbors
    fn.argtypes = [c.POINTER(c.c_double)] + [c.c_int] * 7 + [c.POINTER(c.c_int32), c.c_int64]
    basic._safe_call(fn(basic._dp(x), *x.shape, m, r0, r1, end_at, use_gpu, basic._ip(out), out.size))
    return out


@pytest.mark.parametrize("kind", ["bench", "lattice", "dup"])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("m", MS)
def test_whole_table_and_row_range(m, d, kind):
    """n = m + 2: one searched row, its list full only as the sweep ends; n = 700: directions that reach the array
    ends or die inside a batch, insertions at every slot; then the rows [m + 9, 650) alone (offset and range)"""
    for n in (m + 2, 700):
        x = _coords(kind, n, d)
        ref = O.find_neighbors(x, m)
        assert all(np.array_equal(_search(x, m, 0, n, -1, use_gpu), ref) for use_gpu in (1, 0))
    assert np.array_equal(_search(x, m, m + 9, 650, -1, 1), ref[m + 9:650])


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("m", MS)
def test_prediction_form(m, d):
    """the rows 520..699 among the first 520 points only (end_search_at = n_obs - 1)"""
    x = _coords("lattice", 700, d)
    ref = O.find_neighbors_pred(x[:520], x[520:], m)
    assert all(np.array_equal(_search(x, m, 520, 700, 519, use_gpu), ref) for use_gpu in (1, 0))


def _model(m):
    from gpboost_amd import GPModel, synthetic
    gm = GPModel(gp_coords=synthetic.bench_coords(700), gp_approx="vecchia", num_neighbors=m, vecchia_ordering="none")
    nll, grad, _ = gm.neg_log_likelihood_and_grad([0.3, 1.2, 0.15], synthetic.bench_gaussian_y(700))
    return gm.vecchia_structure()[1], [float(nll), *map(float, grad)]


@pytest.mark.parametrize("m", [65, 128])
def test_model_searches_on_the_gpu(m):
    """the oracle's table, and bit for bit the likelihood and gradient of a fresh process that searches on the host"""
    nbr, vals = _model(m)
    assert np.array_equal(nbr, O.find_neighbors(_coords("bench", 700, 2), m))
    child = (f"import sys, json; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\n"
             f"import test_gpu_vecchia_knn_wide as T; nbr, v = T._model({m})\n"
             "print('RESULT ' + json.dumps([nbr.tolist(), v]))")
    r = subprocess.run([sys.executable, "-c", child], env=dict(os.environ, GPBOOST_AMD_HOST_KNN="1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    host_nbr, host_vals = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert np.array_equal(nbr, np.array(host_nbr)) and vals == host_vals
