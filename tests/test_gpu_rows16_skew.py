"""How the 16-lane row kernel (vecchia_rows16.hip) shares a SIMD between its two resident waves: the waves in
even and in odd wave slots take turns, trip by trip, at the higher issue priority, and every wave lowers its
own for the elimination (VecchiaRowsArgs::prio, s_setprio). The start delay that this file was first meant
for (one wave of each SIMD sleeping before its first load) was measured and not built: the waves are not in
phase to begin with (profiles/rows16_phase/RESULTS.md). Priorities order the issue of instructions and touch
no arithmetic, no set assignment and no store, so every output must be bit-equal to
GPBOOST_AMD_ROWS16_PRIO=0, which leaves all waves at the default priority.

Models as in test_gpu_rows16_flush.py: n = 203 (51 problem sets, the last one partial) and n = 128 (32 full
sets), m in {17, 30} with the exponential kernel and m = 30 with matern15, d = 2, both
GPBOOST_AMD_ROWS16_DIST settings (the stored-distance and the on-the-fly kernel share the loop).
Grids: unset (one trip per wave, so no wave ever has a turn at the lower level), 2 (26 trips at n = 203, 16 at
n = 128: two waves, which may or may not share a SIMD) and 1 (51 and 32 trips, one wave alone).
Switch: unset (on), 1 (on), 0 (off).

No timing is asserted here: what the priorities buy is measured in profiles/rows16_phase/RESULTS.md.
"""
import numpy as np
import pytest

PARS = [0.3, 1.2, 0.15]
COVS = {"exponential": ("exponential", 0.5), "matern15": ("matern", 1.5)}
MODELS = [(n, m, cov) for n in (203, 128) for m, cov in ((17, "exponential"), (30, "exponential"), (30, "matern15"))]
GRIDS = [None, 2, 1]
DISTS = [None, "0"]
ON = [None, "1"]

_models = {}
_runs = {}


def _model(n, m, cov):
    key = (n, m, cov)
    if key not in _models:
        from gpboost_amd import GPModel, synthetic
        X = synthetic.bench_coords(n, 2)
        Y = synthetic.bench_gaussian_y(n)
        name, shape = COVS[cov]
        gm = GPModel(gp_coords=X, cov_function=name, cov_fct_shape=shape, gp_approx="vecchia", num_neighbors=m,
                     vecchia_ordering="random", seed=0)
        _models[key] = dict(gm=gm, Y=Y)
    return _models[key]


def _ranges(n):
    return [(7, min(150, n)), (13, n), (2, 3)]


def _run(n, m, cov, dist, grid, prio, monkeypatch):
    """nll, gradient and sigma2 of both modes, the three sub-range partials, D^-1 and B under one setting of the
    three switches, with what the full-range launch and the last sub-range launch reported; computed once and
    left unchanged."""
    key = (n, m, cov, dist, grid, prio)
    if key not in _runs:
        c = _model(n, m, cov)
        gm = c["gm"]
        monkeypatch.delenv("GPBOOST_AMD_ROWS16_DIST_MB", raising=False)
        for name, v in (("GPBOOST_AMD_ROWS16_DIST", dist), ("GPBOOST_AMD_ROWS16_GRID", grid),
                        ("GPBOOST_AMD_ROWS16_PRIO", prio)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
        out = []
        for mode in (0, 1):
            nll, g, s2 = gm.neg_log_likelihood_and_grad(PARS, c["Y"], profile_sigma2=bool(mode))
            out += [np.array([nll]), np.array(g, float), np.array([s2], float)]
        info = [gm.vecchia_rows_launch_info()]
        out += [np.array(gm.vecchia_partials(PARS, r0, r1), float) for r0, r1 in _ranges(n)]
        info.append(gm.vecchia_rows_launch_info())
        dinv, b = gm.vecchia_factor(PARS)
        out += [np.array(dinv, float), np.array(b, float)]
        for a in out:
            a.setflags(write=False)
        _runs[key] = (out, info)
    return _runs[key]


def _id(v):
    return "unset" if v is None else str(v)


def _trips(n, grid):
    sets = (n + 3) // 4
    return -(-sets // (sets if grid is None else min(grid, sets)))


@pytest.mark.gpu
@pytest.mark.parametrize("prio", ON, ids=lambda p: f"prio_{_id(p)}")
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid_{_id(g)}")
@pytest.mark.parametrize("dist", DISTS, ids=lambda d: f"dist_{_id(d)}")
@pytest.mark.parametrize("n,m,cov", MODELS)
def test_bit_equal_to_default_priority(n, m, cov, dist, grid, prio, monkeypatch):
    ref, info0 = _run(n, m, cov, dist, grid, "0", monkeypatch)
    got, info = _run(n, m, cov, dist, grid, prio, monkeypatch)
    # the two runs did differ in the switch, on the full range and on the one-row range, over the trips expected
    assert [i["prio"] for i in info0] == [0, 0] and [i["prio"] for i in info] == [1, 1]
    assert info[0]["trips"] == info0[0]["trips"] == _trips(n, grid)
    assert info[1]["trips"] == 1
    for k, (a, b) in enumerate(zip(got, ref)):
        diff = np.max(np.abs(a - b))
        print(f"n={n} m={m} {cov} dist={_id(dist)} grid={_id(grid)} prio={_id(prio)} output {k}: "
              f"max abs difference {diff:.3e}")
        assert np.array_equal(a, b), (k, diff)


@pytest.mark.gpu
def test_trip_counts_of_the_capped_grids(monkeypatch):
    """The grids above do give a wave one trip, an even and an odd number of trips: 1, 26 and 51 at n = 203."""
    n, m, cov = MODELS[1]
    assert n == 203
    for grid, trips in ((None, 1), (2, 26), (1, 51)):
        _, info = _run(n, m, cov, None, grid, None, monkeypatch)
        assert info[0] == dict(trips=trips, prio=1)
