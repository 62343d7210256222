"""The 16-lane row kernel (vecchia_rows16.hip) at the smallest shapes where its elimination can go
wrong, against the oracle's restatement on the CPU.

The A rows (matrix rows 0..15) take no part in pivots 16..29 and keep their columns 16..31 out of
pivots 0..15: their right-hand sides are finished by a block back-substitution with the original
columns 16..29 and a replay of the 16 stored row operations. n = 203 leaves the last set of four rows
partial and rows 0..29 with k < m; m in {1, 15, 16, 17, 29, 30} covers B rows (16..29) that are all
padding, exactly one real B row and exactly one padding pivot; d = 2 and d = 3 are the kernel's two
template forms.

Tolerances: nll, gradient and the row partials at test_gpu_vecchia.py's file-wide 1e-6 (the partial
sums are what nll and gradient are linear in, so they take the same bound); the factor at the
tolerances test_gpu_vecchia.py::test_vecchia_factor_matches_reference uses against the reference
(D^-1 rtol 1e-10, B rtol 1e-8 / atol 1e-11); padding entries of B exactly 0.
"""
import numpy as np
import pytest

from oracle import oracle as O

RTOL = 1e-6
N = 203
PARS = [0.3, 1.2, 0.15]
COVS = {"exponential": ("exponential", 0.5, 0), "matern15": ("matern", 1.5, 1), "matern25": ("matern", 2.5, 2),
        "gaussian": ("gaussian", 0.5, 3)}
CASES = [(m, d, "exponential") for m in (1, 15, 16, 17, 29, 30) for d in (2, 3)] + \
        [(30, d, c) for d in (2, 3) for c in ("matern15", "matern25", "gaussian")]

_cache = {}


def _case(m, d, cov):
    """Model, data and the oracle's results (both modes, factor), computed once per case."""
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
        _cache[key] = dict(gm=gm, Y=Y, xv=xv, yv=yv, nb=nb, ct=ct, tp=tp, ref=ref)
    return _cache[key]


def _close(a, b, rtol=RTOL):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1.0))


@pytest.mark.gpu
@pytest.mark.parametrize("m,d,cov", CASES)
def test_nll_grad_and_factor_match_oracle(m, d, cov):
    c = _case(m, d, cov)
    gm = c["gm"]
    for mode in (0, 1):
        ref = c["ref"][mode]
        nll, g, _ = gm.neg_log_likelihood_and_grad(PARS, c["Y"], profile_sigma2=bool(mode))
        print(f"m={m} d={d} {cov} mode={mode}: nll rel {abs(nll - ref['nll']) / abs(ref['nll']):.3e}, "
              f"grad abs {np.max(np.abs(np.asarray(g) - ref['grad'])):.3e}")
        assert abs(nll - ref["nll"]) <= RTOL * abs(ref["nll"])
        assert _close(g, ref["grad"]), (g, ref["grad"])
    dinv, b = gm.vecchia_factor(PARS)
    rd, rb = c["ref"][0]["Dinv"], c["ref"][0]["B"]
    print(f"m={m} d={d} {cov}: Dinv rel {np.max(np.abs(dinv - rd) / np.abs(rd)):.3e}, "
          f"B excess over atol {np.max((np.abs(b - rb) - 1e-11) / np.maximum(np.abs(rb), 1e-300)):.3e}")
    np.testing.assert_allclose(dinv, rd, rtol=1e-10)
    np.testing.assert_allclose(b, rb, rtol=1e-8, atol=1e-11)
    k = np.minimum(np.arange(N), m)
    pad = np.arange(m)[None, :] >= k[:, None]
    assert np.all(b[pad] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("m,d", [(30, 2), (17, 3)])
def test_row_subrange_matches_oracle_partials(m, d):
    """Rows r0..r1 with r0 no multiple of the kernel's 4-row set, r0 inside the k < m rows, and a partial last set."""
    c = _case(m, d, "exponential")
    gm = c["gm"]
    gm.neg_log_likelihood_and_grad(PARS, c["Y"])   # sets y
    for r0, r1 in [(7, 150), (13, N), (2, 3)]:
        got = gm.vecchia_partials(PARS, r0, r1)
        ref = O.vecchia_partials(c["xv"], c["yv"], c["nb"], c["ct"], c["tp"], r0, r1)
        print(f"m={m} d={d} rows {r0}..{r1}: max rel {np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)):.3e}")
        assert _close(got, ref), (r0, r1, got, ref)


def _solve_lazy_a(M, rhs):
    """The kernel's elimination order on a 30 x 30 system with two right-hand sides, in numpy: the 32 x 32
    symmetric bordered matrix [[M, rhs], [rhs^T, 0]], Gauss-Jordan without normalisation over pivots
    0..29, the pivot row's entries read from column j by symmetry; pivots 0..15 update the B rows
    (16..31, border rows included) in full but the A rows (0..15) only in columns < 16, each step's
    A-row multipliers stored; pivots 16..29 eliminate the B rows only; then z_A = rhs_A - M_AB x_B with
    the original M_AB, the 16 stored row operations replayed on z_A in pivot order, and x = z / pivot."""
    n, na = M.shape[0], 16
    W = np.zeros((n + 2, n + 2))
    W[:n, :n], W[:n, n:], W[n:, :n] = M, rhs, rhs.T
    orig = W.copy()
    mult = np.zeros((na, na))                    # mult[j, h]: row h's multiplier at pivot j
    piv = np.zeros(n)
    for j in range(n):
        piv[j] = W[j, j]
        f = W[:, j] / piv[j]
        f[j] = 0.0
        row = W[j + 1:, j].copy()                # M[j][c] = M[c][j], c = j + 1 .. 31
        if j < na:
            mult[j] = f[:na]
            W[:na, j + 1:na] -= np.outer(f[:na], row[:na - j - 1])
        W[na:, j + 1:] -= np.outer(f[na:], row)
    x = np.zeros((n, 2))
    x[na:] = W[na:n, n:] / piv[na:, None]
    z = orig[:na, n:] - orig[:na, na:n] @ x[na:]
    for j in range(na):
        z -= np.outer(mult[j], z[j])
    x[:na] = z / piv[:na, None]
    return x


def test_stored_multiplier_replay_solves_the_system():
    """The algebra of the A rows' deferred columns, independent of the kernel."""
    rng = np.random.default_rng(7)
    for _ in range(20):
        G = rng.standard_normal((30, 30))
        M = G @ G.T + 30.0 * np.eye(30)   # SPD, condition number of a few units
        rhs = rng.standard_normal((30, 2))
        x = _solve_lazy_a(M, rhs)
        ref = np.linalg.solve(M, rhs)
        assert np.max(np.abs(x - ref)) <= 1e-12 * np.max(np.abs(ref))
