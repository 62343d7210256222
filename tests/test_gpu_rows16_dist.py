"""The stored-distance form of the 16-lane row kernel (vecchia_rows16.hip, `vecchia_rows16d_kernel`): the
pair distances of phase 1 are computed once per structure by `vecchia_rows16_dist_kernel` and read back at
every evaluation (one set ahead of their use) instead of being recomputed from the coordinates.

Shape as in test_gpu_rows16_edges.py: n = 203 leaves the last set of four rows partial (its clamped
prefetch) and rows 0..29 with k < m (padding points among the stored distances); m in {1, 15, 16, 17,
29, 30}, d in {1, 2, 3} (the distance kernel's two template forms, d = 1 and 3 through the generic one).
The 16-lane kernel serves m = 17..30 (m <= 16 runs the 16-lane-per-row bordered form of
vecchia_kernels.hip, which has no stored form), so `vecchia_rows_info()["stored"]` is 1 exactly for
those m and 0 below: the m <= 16 cases pin that nothing is stored or changed there.

Against the oracle: test_gpu_rows16_edges.py's tolerances (nll, gradient, partial sums 1e-6; D^-1 rtol
1e-10; B rtol 1e-8 / atol 1e-11; padding entries of B exactly 0). Against GPBOOST_AMD_ROWS16_DIST=0 on
the same model: bit-equal, since both kernels run the same operation sequence on the same bits (the
stored value is the on-the-fly kernel's own sqrt of its own squared distance, from shared source).
Re-partitioned model: the two row blocks' partial sums against the one-rank sums at
test_gpu_sharded.py's 1e-10.
"""
import numpy as np
import pytest

from oracle import oracle as O

RTOL = 1e-6
N = 203
PARS = [0.3, 1.2, 0.15]
COVS = {"exponential": ("exponential", 0.5, 0), "matern15": ("matern", 1.5, 1), "matern25": ("matern", 2.5, 2),
        "gaussian": ("gaussian", 0.5, 3)}
CASES = [(m, d, "exponential") for m in (1, 15, 16, 17, 29, 30) for d in (1, 2, 3)] + \
        [(30, d, c) for d in (2, 3) for c in ("matern15", "matern25", "gaussian")]
RANGES = [(7, 150), (13, N), (2, 3)]
ROW_BYTES = 15 * 16 * 2 * 8

_cache = {}


def _stored_expected(m):
    return 1 if 17 <= m <= 30 else 0


def _case(m, d, cov):
    """Model, data and the oracle's results (both modes, factor, sub-range partials), computed once per case."""
    key = (m, d, cov)
    if key not in _cache:
        from gpboost_amd import GPModel, synthetic
        X = synthetic.bench_coords(N, d)
        Y = synthetic.bench_gaussian_y(N)
        name, shape, ct = COVS[cov]
        gm = GPModel(gp_coords=X, cov_function=name, cov_fct_shape=shape, gp_approx="vecchia", num_neighbors=m,
                     vecchia_ordering="random", seed=0)
        perm, xv, nb = O.vecchia_setup(X, m, 0, True)
        tp = O.transform(ct, PARS)
        yv = np.ascontiguousarray(Y[perm])
        ref = [O.vecchia_nll_grad(xv, yv, nb, ct, tp, mode, want_factor=(mode == 0)) for mode in (0, 1)]
        parts = [O.vecchia_partials(xv, yv, nb, ct, tp, r0, r1) for r0, r1 in RANGES]
        _cache[key] = dict(gm=gm, Y=Y, ref=ref, parts=parts)
    return _cache[key]


def _close(a, b, rtol=RTOL):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1.0))


def _everything(gm, Y):
    """nll, gradient (both modes), the sub-range partials and the factor of one model, as arrays."""
    out = []
    for mode in (0, 1):
        nll, g, _ = gm.neg_log_likelihood_and_grad(PARS, Y, profile_sigma2=bool(mode))
        out += [np.array([nll]), np.asarray(g, float)]
    out += [gm.vecchia_partials(PARS, r0, r1) for r0, r1 in RANGES]
    dinv, b = gm.vecchia_factor(PARS)
    return out + [dinv, b]


@pytest.mark.gpu
@pytest.mark.parametrize("m,d,cov", CASES)
def test_stored_path_matches_oracle(m, d, cov, monkeypatch):
    monkeypatch.delenv("GPBOOST_AMD_ROWS16_DIST", raising=False)
    monkeypatch.delenv("GPBOOST_AMD_ROWS16_DIST_MB", raising=False)
    c = _case(m, d, cov)
    gm = c["gm"]
    for mode in (0, 1):
        ref = c["ref"][mode]
        nll, g, _ = gm.neg_log_likelihood_and_grad(PARS, c["Y"], profile_sigma2=bool(mode))
        print(f"m={m} d={d} {cov} mode={mode}: nll rel {abs(nll - ref['nll']) / abs(ref['nll']):.3e}, "
              f"grad abs {np.max(np.abs(np.asarray(g) - ref['grad'])):.3e}")
        assert abs(nll - ref["nll"]) <= RTOL * abs(ref["nll"])
        assert _close(g, ref["grad"]), (g, ref["grad"])
    info = gm.vecchia_rows_info()
    print(f"m={m} d={d} {cov}: {info}")
    assert info["stored"] == _stored_expected(m)
    if info["stored"]:
        assert info["rows"] == N and info["bytes"] == N * ROW_BYTES and info["build_ms"] > 0.
    for (r0, r1), ref in zip(RANGES, c["parts"]):
        got = gm.vecchia_partials(PARS, r0, r1)
        print(f"m={m} d={d} {cov} rows {r0}..{r1}: max rel {np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)):.3e}")
        assert _close(got, ref), (r0, r1, got, ref)
    dinv, b = gm.vecchia_factor(PARS)
    rd, rb = c["ref"][0]["Dinv"], c["ref"][0]["B"]
    print(f"m={m} d={d} {cov}: Dinv rel {np.max(np.abs(dinv - rd) / np.abs(rd)):.3e}, "
          f"B excess over atol {np.max((np.abs(b - rb) - 1e-11) / np.maximum(np.abs(rb), 1e-300)):.3e}")
    np.testing.assert_allclose(dinv, rd, rtol=1e-10)
    np.testing.assert_allclose(b, rb, rtol=1e-8, atol=1e-11)
    k = np.minimum(np.arange(N), m)
    pad = np.arange(m)[None, :] >= k[:, None]
    assert np.all(b[pad] == 0.0)
    assert gm.vecchia_rows_info()["stored"] == _stored_expected(m)   # the factor launch read the same buffer


@pytest.mark.gpu
@pytest.mark.parametrize("m,d,cov", CASES)
def test_stored_path_bit_equal_to_on_the_fly(m, d, cov, monkeypatch):
    monkeypatch.delenv("GPBOOST_AMD_ROWS16_DIST_MB", raising=False)
    c = _case(m, d, cov)
    gm = c["gm"]
    monkeypatch.delenv("GPBOOST_AMD_ROWS16_DIST", raising=False)
    stored = _everything(gm, c["Y"])
    assert gm.vecchia_rows_info()["stored"] == _stored_expected(m)
    monkeypatch.setenv("GPBOOST_AMD_ROWS16_DIST", "0")
    fly = _everything(gm, c["Y"])
    for k, (a, b) in enumerate(zip(stored, fly)):
        diff = np.max(np.abs(a - b))
        print(f"m={m} d={d} {cov} output {k}: max abs difference {diff:.3e}")
        assert np.array_equal(a, b), (k, diff)
    b = stored[-1]
    kk = np.minimum(np.arange(N), m)
    assert np.all(b[np.arange(m)[None, :] >= kk[:, None]] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("m,d", [(30, 2), (17, 3)])
def test_cap_below_need_keeps_on_the_fly_kernel(m, d, monkeypatch):
    """203 rows need 0.78 MB: under a 0.5 MB cap nothing is stored (a held buffer is dropped) and the
    results are the on-the-fly kernel's; 0 means never; without the cap the buffer comes back."""
    c = _case(m, d, "exponential")
    gm = c["gm"]
    monkeypatch.delenv("GPBOOST_AMD_ROWS16_DIST_MB", raising=False)
    monkeypatch.setenv("GPBOOST_AMD_ROWS16_DIST", "0")
    fly = _everything(gm, c["Y"])
    monkeypatch.delenv("GPBOOST_AMD_ROWS16_DIST", raising=False)
    for cap in ("0.5", "0"):
        monkeypatch.setenv("GPBOOST_AMD_ROWS16_DIST_MB", cap)
        capped = _everything(gm, c["Y"])
        assert gm.vecchia_rows_info() == dict(stored=0, bytes=0, rows=0, build_ms=0.0)
        for a, b in zip(capped, fly):
            assert np.array_equal(a, b)
    monkeypatch.setenv("GPBOOST_AMD_ROWS16_DIST_MB", "1")
    again = _everything(gm, c["Y"])
    assert gm.vecchia_rows_info()["stored"] == 1
    for a, b in zip(again, fly):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("m,d", [(30, 2), (17, 3)])
def test_repartition_rebuilds_the_buffer_for_the_new_row_block(m, d, monkeypatch):
    """One model moved from one rank to rank 0 of 2, then rank 1 of 2 (the host transport of
    test_gpu_sharded.py, its callback unused: partial sums are not all-reduced): each partition holds
    the distances of its own row block, and the two blocks' sums are the one-rank sums."""
    monkeypatch.delenv("GPBOOST_AMD_ROWS16_DIST", raising=False)
    monkeypatch.delenv("GPBOOST_AMD_ROWS16_DIST_MB", raising=False)
    from gpboost_amd import GPModel, synthetic
    X = synthetic.bench_coords(N, d)
    Y = synthetic.bench_gaussian_y(N)
    gm = GPModel(gp_coords=X, cov_function="exponential", gp_approx="vecchia", num_neighbors=m,
                 vecchia_ordering="random", seed=0)
    gm.neg_log_likelihood_and_grad(PARS, Y)   # sets y
    one = gm.vecchia_partials(PARS, 0, N)
    assert gm.vecchia_rows_info()["rows"] == N
    blocks = [(0, 102), (102, N)]   # n / world rows each, the remainder to the first ranks
    total = np.zeros(6)
    for rank, (r0, r1) in enumerate(blocks):
        gm.set_distributed_host(rank, 2, lambda a: None)
        assert gm.vecchia_rows_info()["stored"] == 0   # dropped with the old structure
        part = gm.vecchia_partials(PARS, r0, r1)
        info = gm.vecchia_rows_info()
        assert info["stored"] == 1 and info["rows"] == r1 - r0 and info["bytes"] == (r1 - r0) * ROW_BYTES
        monkeypatch.setenv("GPBOOST_AMD_ROWS16_DIST", "0")
        assert np.array_equal(gm.vecchia_partials(PARS, r0, r1), part)
        monkeypatch.delenv("GPBOOST_AMD_ROWS16_DIST")
        sub = gm.vecchia_partials(PARS, r0 + 5, r1 - 3)   # a sub-range of a block that does not start at row 0
        ref = O.vecchia_partials(*_oracle_inputs(X, Y, m), r0 + 5, r1 - 3)
        assert _close(sub, ref), (rank, sub, ref)
        total += part
    print(f"m={m} d={d}: two blocks against one rank, max rel {np.max(np.abs(total - one) / np.abs(one)):.3e}")
    np.testing.assert_allclose(total, one, rtol=1e-10)


def _oracle_inputs(X, Y, m):
    perm, xv, nb = O.vecchia_setup(X, m, 0, True)
    return xv, np.ascontiguousarray(Y[perm]), nb, 0, O.transform(0, PARS)
