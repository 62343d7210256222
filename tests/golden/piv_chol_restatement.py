"""numpy restatement of the pivoted Cholesky factorisation of the exact covariance that the
"pivoted_cholesky" CG preconditioner uses (Harbrecht et al. 2012; the reference's
PivotedCholsekyFactorizationSigma, CG_utils.h:438-488, restated from its rules):

* the pivot is the FIRST maximum of the remaining diagonal in the current order of the permutation,
  which starts as the Vecchia order and is changed by the swaps;
* entries with |L_jm| < 1e-12 before scaling are not stored and not divided, their unscaled square is
  still subtracted from the diagonal;
* err = sum |remaining diagonal| after the update, the loop runs while m == 0 or (m < k and err > tol);
* L[pi(m), m] = sqrt(diag(pi(m))) with the diagonal before this step's updates of the other rows.

Two variants decide whether a case is a sound fixture (make_golden_precond.py, test_precond_fixtures.py):
plain (float64, dot products accumulated forwards) and perturbed (covariance in longdouble, dot products
accumulated backwards). A case whose pivot sequence or rank differs between them depends on rounding and
cannot be a fixture.
"""
from __future__ import annotations

import numpy as np

STOP_TOL = 1e-6
DROP_TOL = 1e-12


def cov_values(cov_fct, shape, var, phi, dist, dtype):
    r = dist.astype(dtype)
    var = dtype(var)
    phi = dtype(phi)
    if cov_fct == "gaussian":
        return var * np.exp(-phi * r * r)
    if cov_fct == "exponential" or float(shape) == 0.5:
        return var * np.exp(-phi * r)
    x = phi * r
    if float(shape) == 1.5:
        return var * (1 + x) * np.exp(-x)
    if float(shape) == 2.5:
        return var * (1 + x + x * x / 3) * np.exp(-x)
    raise ValueError("covariance not covered")


def pivoted_cholesky(X, cov_fct, shape, var, phi, k, tol=STOP_TOL, perturbed=False):
    """X: coordinates in the order the permutation starts from (Vecchia order). (var, phi): the
    transformed parameters. Returns (L (n, k) float64, pivots, rank)."""
    dtype = np.longdouble if perturbed else np.float64
    X = np.asarray(X, dtype=dtype)
    n = X.shape[0]
    k = min(k, n)
    L = np.zeros((n, k), dtype=dtype)
    diag = np.full(n, var, dtype=dtype)
    pi = np.arange(n)
    piv = []
    m, err = 0, float(var) * n
    while m == 0 or (m < k and err > tol):
        i = m + int(np.argmax(diag[pi[m:]]))   # argmax: the first maximum
        pi[m], pi[i] = pi[i], pi[m]
        p = pi[m]
        if m + 1 < n:
            rows = pi[m + 1:]
            dist = np.sqrt(((X[rows] - X[p]) ** 2).sum(axis=1))
            l = cov_values(cov_fct, shape, var, phi, dist, dtype)
            if m > 0:
                prod = L[rows, :m] * L[p, :m]
                dot = np.zeros(rows.shape[0], dtype=dtype)
                for a in (range(m - 1, -1, -1) if perturbed else range(m)):
                    dot = dot + prod[:, a]
                l = l - dot
            small = np.abs(l) < DROP_TOL
            l = np.where(small, l, l / np.sqrt(diag[p]))
            L[rows, m] = np.where(small, 0, l)
            diag[rows] = diag[rows] - l * l
            err = float(np.abs(diag[rows]).sum())
        L[p, m] = np.sqrt(diag[p])
        piv.append(int(p))
        m += 1
    return L.astype(np.float64), piv, m
