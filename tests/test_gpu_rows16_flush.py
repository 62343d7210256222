"""What the 16-lane row kernel (vecchia_rows16.hip) carries from one problem set to the next: log(D) is
taken once per 16 trips of the set loop, from a register in which lane (trip & 15) of each 16-lane row
keeps that trip's D, and once more after the loop for the trips left over. A wave must therefore run
more than 16 trips before the in-loop flush is reached at all; GPBOOST_AMD_ROWS16_GRID caps the grid so
that a model of a few hundred rows gives one wave that many.

Models: n = 203 (51 problem sets, the last one partial, rows 0..29 with k < m) and n = 128 (32 full sets);
m in {17, 30} with the exponential kernel, m = 30 with matern15 and gaussian; d = 2; both
GPBOOST_AMD_ROWS16_DIST settings (the stored-distance and the on-the-fly kernel share the loop).
Grids: unset; 4 (13 trips, no flush inside the loop); 3 (17 trips at n = 203: one flush at trip 16 and one
value after it); 2 (n = 128: exactly 16 trips, the loop's flush and the final one coincide; n = 203: 26
and 25 trips); 1 (51 trips: three flushes and three values). The sub-range partials run the same loop
over fewer sets (36, 48 and 1 at n = 203); at n = 128 the range (7, 150) ends at row 128.

Against the oracle: test_gpu_rows16_edges.py's tolerances (nll, gradient, partial sums 1e-6; D^-1 rtol
1e-10; B rtol 1e-8 / atol 1e-11; padding entries of B exactly 0; the factor launch takes the kernel's
path without a likelihood, which keeps nothing between trips). Capped grid against the uncapped one:
1e-12 relative, the project's tolerance between row-kernel forms (test_gpu_vecchia.py): the rows are the
same, only their partition into per-wave sums changes; the factor is per row and must not move at all.
Stored against GPBOOST_AMD_ROWS16_DIST=0 on the same grid: bit-equal, as in test_gpu_rows16_dist.py.
"""
import numpy as np
import pytest

from oracle import oracle as O

RTOL = 1e-6
GRID_RTOL = 1e-12
PARS = [0.3, 1.2, 0.15]
COVS = {"exponential": ("exponential", 0.5, 0), "matern15": ("matern", 1.5, 1), "gaussian": ("gaussian", 0.5, 3)}
MODELS = [(n, m, cov) for n in (203, 128) for m, cov in ((17, "exponential"), (30, "exponential"), (30, "matern15"),
                                                        (30, "gaussian"))]
GRIDS = [None, 4, 3, 2, 1]
DISTS = [None, "0"]

_models = {}
_runs = {}


def _ranges(n):
    return [(7, min(150, n)), (13, n), (2, 3)]


def _model(n, m, cov):
    """Model, data and the oracle's results (both modes, factor, sub-range partials), computed once."""
    key = (n, m, cov)
    if key not in _models:
        from gpboost_amd import GPModel, synthetic
        X = synthetic.bench_coords(n, 2)
        Y = synthetic.bench_gaussian_y(n)
        name, shape, ct = COVS[cov]
        gm = GPModel(gp_coords=X, cov_function=name, cov_fct_shape=shape, gp_approx="vecchia", num_neighbors=m,
                     vecchia_ordering="random", seed=0)
        perm, xv, nb = O.vecchia_setup(X, m, 0, True)
        tp = O.transform(ct, PARS)
        yv = np.ascontiguousarray(Y[perm])
        ref = [O.vecchia_nll_grad(xv, yv, nb, ct, tp, mode, want_factor=(mode == 0)) for mode in (0, 1)]
        parts = [O.vecchia_partials(xv, yv, nb, ct, tp, r0, r1) for r0, r1 in _ranges(n)]
        _models[key] = dict(gm=gm, Y=Y, ref=ref, parts=parts)
    return _models[key]


def _run(n, m, cov, dist, grid, monkeypatch):
    """[nll, grad] of both modes, the three sub-range partials, D^-1 and B of one model under one setting
    of the two switches, computed once and left unchanged."""
    key = (n, m, cov, dist, grid)
    if key not in _runs:
        c = _model(n, m, cov)
        gm = c["gm"]
        monkeypatch.delenv("GPBOOST_AMD_ROWS16_DIST_MB", raising=False)
        for name, val in (("GPBOOST_AMD_ROWS16_DIST", dist), ("GPBOOST_AMD_ROWS16_GRID", grid)):
            if val is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(val))
        out = []
        for mode in (0, 1):
            nll, g, _ = gm.neg_log_likelihood_and_grad(PARS, c["Y"], profile_sigma2=bool(mode))
            out += [np.array([nll]), np.array(g, float)]
        out += [np.array(gm.vecchia_partials(PARS, r0, r1), float) for r0, r1 in _ranges(n)]
        dinv, b = gm.vecchia_factor(PARS)
        out += [np.array(dinv, float), np.array(b, float)]
        if dist is None:   # GPBOOST_AMD_ROWS16_DIST=0 leaves a buffer held, unused
            assert gm.vecchia_rows_info()["stored"] == 1
        for a in out:
            a.setflags(write=False)
        _runs[key] = out
    return _runs[key]


def _close(a, b, rtol=RTOL):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1.0))


def _id(v):
    return "unset" if v is None else str(v)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid_{_id(g)}")
@pytest.mark.parametrize("dist", DISTS, ids=lambda d: f"dist_{_id(d)}")
@pytest.mark.parametrize("n,m,cov", MODELS)
def test_matches_oracle(n, m, cov, dist, grid, monkeypatch):
    c = _model(n, m, cov)
    out = _run(n, m, cov, dist, grid, monkeypatch)
    tag = f"n={n} m={m} {cov} dist={_id(dist)} grid={_id(grid)}"
    for mode in (0, 1):
        ref = c["ref"][mode]
        nll, g = out[2 * mode][0], out[2 * mode + 1]
        print(f"{tag} mode={mode}: nll rel {abs(nll - ref['nll']) / abs(ref['nll']):.3e}, "
              f"grad abs {np.max(np.abs(g - ref['grad'])):.3e}")
        assert abs(nll - ref["nll"]) <= RTOL * abs(ref["nll"])
        assert _close(g, ref["grad"]), (g, ref["grad"])
    for (r0, r1), got, ref in zip(_ranges(n), out[4:7], c["parts"]):
        print(f"{tag} rows {r0}..{r1}: max rel {np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)):.3e}")
        assert _close(got, ref), (r0, r1, got, ref)
    dinv, b = out[7], out[8]
    rd, rb = c["ref"][0]["Dinv"], c["ref"][0]["B"]
    print(f"{tag}: Dinv rel {np.max(np.abs(dinv - rd) / np.abs(rd)):.3e}, "
          f"B excess over atol {np.max((np.abs(b - rb) - 1e-11) / np.maximum(np.abs(rb), 1e-300)):.3e}")
    np.testing.assert_allclose(dinv, rd, rtol=1e-10)
    np.testing.assert_allclose(b, rb, rtol=1e-8, atol=1e-11)
    k = np.minimum(np.arange(n), m)
    assert np.all(b[np.arange(m)[None, :] >= k[:, None]] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS[1:], ids=lambda g: f"grid_{_id(g)}")
@pytest.mark.parametrize("dist", DISTS, ids=lambda d: f"dist_{_id(d)}")
@pytest.mark.parametrize("n,m,cov", MODELS)
def test_capped_grid_matches_uncapped(n, m, cov, dist, grid, monkeypatch):
    full = _run(n, m, cov, dist, None, monkeypatch)
    capped = _run(n, m, cov, dist, grid, monkeypatch)
    for k, (a, b) in enumerate(zip(capped[:7], full[:7])):
        rel = np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))
        print(f"n={n} m={m} {cov} dist={_id(dist)} grid={grid} output {k}: max rel difference {rel:.3e}")
        np.testing.assert_allclose(a, b, rtol=GRID_RTOL, atol=0.0)
    assert np.array_equal(capped[7], full[7]) and np.array_equal(capped[8], full[8])


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid_{_id(g)}")
@pytest.mark.parametrize("n,m,cov", MODELS)
def test_stored_bit_equal_to_on_the_fly(n, m, cov, grid, monkeypatch):
    stored = _run(n, m, cov, None, grid, monkeypatch)
    fly = _run(n, m, cov, "0", grid, monkeypatch)
    for k, (a, b) in enumerate(zip(stored, fly)):
        diff = np.max(np.abs(a - b))
        print(f"n={n} m={m} {cov} grid={_id(grid)} output {k}: max abs difference {diff:.3e}")
        assert np.array_equal(a, b), (k, diff)
