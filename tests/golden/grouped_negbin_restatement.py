"""Dense numpy restatement of the Laplace-approximated negative log-likelihood of grouped random effects under the
negative binomial likelihood (shape r, log link), matrix_inversion_method = "cholesky":

    log p(y | eta) = y eta - (y + r) log(e^eta + r) + lgamma(y + r) - lgamma(y + 1) + r log r - lgamma(r)
    d/d eta        = y - (y + r) mu / (mu + r),   mu = e^eta
    information    = (y + r) mu r / (mu + r)^2

written as the formulas stand (the fixtures' linear predictors are far from the ranges where that form fails). The
Newton iteration, its line search and stopping rule, and the value are those of grouped_laplace_restatement.laplace_nll,
which this module calls with the likelihood above.

Used by make_golden_grouped_negbin.py (the generator stops when it does not reproduce the reference) and by
tests/test_grouped_negbin_fixtures.py. Needs numpy and scipy.special only.
"""
from __future__ import annotations

import numpy as np
from scipy.special import gammaln

import grouped_laplace_restatement as base

MAXIT = base.MAXIT


def negbin(y, eta, r):
    mu = np.exp(eta)
    ll = np.sum(y * eta - (y + r) * np.log(mu + r) + gammaln(y + r) - gammaln(y + 1.0)) \
        + y.size * (r * np.log(r) - gammaln(r))
    return ll, y - (y + r) * mu / (mu + r), (y + r) * mu * r / (mu + r) ** 2


def laplace_nll(groups, y, sigma2, aux, offset=None, delta=1e-8):
    """(nll, newton_iterations, mode, W at the mode, Z) of base.laplace_nll for the negative binomial likelihood."""
    liks = dict(base.LIKELIHOODS, negative_binomial=negbin)
    saved = base.LIKELIHOODS
    base.LIKELIHOODS = liks
    try:
        return base.laplace_nll(groups, y, sigma2, "negative_binomial", aux=aux, offset=offset, delta=delta)
    finally:
        base.LIKELIHOODS = saved
