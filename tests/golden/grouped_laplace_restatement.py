"""Dense numpy restatement of the Laplace-approximated negative log-likelihood of grouped random effects
under a non-Gaussian likelihood, matrix_inversion_method = "cholesky". Written from the formulas:

    b ~ N(0, Sigma), Sigma = diag(sigma_k^2 I_{m_k}), eta = F + Z b, y_i ~ p(. | eta_i)
    Psi(b) = sum_i log p(y_i | eta_i) - b^T Sigma^-1 b / 2
    Newton: A = Sigma^-1 + Z^T W Z (W = -d^2 log p / d eta^2 at the current b),
            delta = A^-1 (Z^T dlog p/d eta - Sigma^-1 b), b <- b + lr delta, lr halved (at most 20 times)
            while Psi(b + lr delta) < Psi(b) + 1e-4 lr delta^T grad;
            stop when the change of Psi is below 1e-8 |Psi| (its absolute value in the first step)
    nll = -(Psi(b) - sum log diag chol(A) + sum log diag(Sigma^-1) / 2), A at the final b.

Used by make_golden_grouped_laplace.py (the generator stops when it does not reproduce the reference) and by
tests/test_grouped_laplace_fixtures.py. Needs numpy and scipy.special only.
"""
from __future__ import annotations

import numpy as np
from scipy.special import gammaln, log_ndtr

MAXIT = 1000


def _logit(y, eta, aux):
    p = 1.0 / (1.0 + np.exp(-eta))
    return np.sum(y * eta - np.logaddexp(0.0, eta)), y - p, p * (1.0 - p)


def _probit(y, eta, aux):
    s = 2.0 * y - 1.0
    logcdf = log_ndtr(s * eta)
    r = np.exp(-0.5 * eta * eta - 0.5 * np.log(2.0 * np.pi) - logcdf)   # phi / Phi(s eta)
    return np.sum(logcdf), s * r, r * (s * eta + r)


def _poisson(y, eta, aux):
    mu = np.exp(eta)
    return np.sum(y * eta - mu - gammaln(y + 1.0)), y - mu, mu


def _gamma(y, eta, aux):
    t = y * np.exp(-eta)
    ll = np.sum(-aux * (eta + t) + (aux - 1.0) * np.log(y)) + y.size * (aux * np.log(aux) - gammaln(aux))
    return ll, aux * (t - 1.0), aux * t


LIKELIHOODS = {"bernoulli_logit": _logit, "bernoulli_probit": _probit, "poisson": _poisson, "gamma": _gamma}


def design(groups):
    """Z (n x M) with the levels of every effect numbered in order of first appearance."""
    n, K = groups.shape
    cols, m = [], []
    for k in range(K):
        _, first, inv = np.unique(groups[:, k], return_index=True, return_inverse=True)
        rank = np.argsort(np.argsort(first))   # order of first appearance
        lev = rank[inv]
        Zk = np.zeros((n, lev.max() + 1))
        Zk[np.arange(n), lev] = 1.0
        cols.append(Zk)
        m.append(Zk.shape[1])
    return np.hstack(cols), m


def laplace_nll(groups, y, sigma2, likelihood, aux=1.0, offset=None, delta=1e-8):
    """Returns (nll, newton_iterations, mode, W at the mode, Z)."""
    lik = LIKELIHOODS[likelihood]
    Z, m = design(np.asarray(groups))
    n, M = Z.shape
    F = np.zeros(n) if offset is None else np.asarray(offset, dtype=np.float64)
    sigi = np.concatenate([np.full(mk, 1.0 / s) for mk, s in zip(m, sigma2)])
    b = np.zeros(M)

    def psi(bb):
        return lik(y, F + Z @ bb, aux)[0] - 0.5 * np.dot(bb * sigi, bb)

    obj = psi(b)
    its = 0
    for it in range(MAXIT):
        _, d1, W = lik(y, F + Z @ b, aux)
        grad = Z.T @ d1 - sigi * b
        A = np.diag(sigi) + Z.T @ (W[:, None] * Z)
        step = np.linalg.solve(A, grad)
        slope = float(step @ grad)
        lr = 1.0
        for _ in range(20):
            new = psi(b + lr * step)
            if new < obj + 1e-4 * lr * slope or not np.isfinite(new):
                lr *= 0.5
            else:
                break
        b = b + lr * step
        its = it + 1
        done = abs(new - obj) < delta * abs(obj) if it == 0 else (new - obj) < delta * abs(obj)
        obj = new
        if done:
            break
    _, _, W = lik(y, F + Z @ b, aux)
    A = np.diag(sigi) + Z.T @ (W[:, None] * Z)
    L = np.linalg.cholesky(A)
    nll = -(obj - np.sum(np.log(np.diag(L))) + 0.5 * np.sum(np.log(sigi)))
    return float(nll), its, b, W, Z
