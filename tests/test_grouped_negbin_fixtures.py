"""CPU checks of the negative binomial grouped-Laplace fixtures (tests/golden/golden_grouped_negbin.json, written by
tests/golden/make_golden_grouped_negbin.py from the reference): no GPU and no reference needed.

Every fixture's response is what gpboost_amd.synthetic generates (bench_grouped_negbin_y; with covariates
bench_grouped_coef_y at shape 1.5), its sample variance exceeds its mean (the data are over-dispersed, which is what
the likelihood is for), and the dense numpy restatement (tests/golden/grouped_negbin_restatement.py: the likelihood as
its definition is written, the Newton loop of grouped_laplace_restatement.py) reproduces the reference's nll of every
Cholesky evaluation and fit to 1e-9 relative without reaching the Newton iteration cap.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from gpboost_amd import synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from grouped_negbin_restatement import MAXIT, laplace_nll  # noqa: E402

with open(os.path.join(HERE, "golden", "golden_grouped_negbin.json")) as _f:
    GOLDEN = json.load(_f)
EVAL = sorted(k for k, v in GOLDEN.items() if "grad" in v)
FITS = sorted(k for k, v in GOLDEN.items() if "aux_fit" in v)


def _data(case):
    g = synthetic.bench_groups(case["n"], tuple(case["levels"]))
    if "covariates" in case:
        X = synthetic.bench_covariates(case["n"], 2)
        y = synthetic.bench_grouped_coef_y(g, X, case["beta_data"], "negative_binomial", shape=case["data_shape"])
        return g, y, None
    y = synthetic.bench_grouped_negbin_y(g)
    fe = 0.5 * (synthetic.lcg_unif(case["n"], 0.77) - 0.5) if case["offset"] else None
    return g, y, fe


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_fixture_response_is_the_synthetic_one_and_over_dispersed(name):
    case = GOLDEN[name]
    _, y, _ = _data(case)
    assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest() == case["y_sha256"], (y.sum(), case["y_sum"])
    assert np.all(y >= 0) and np.all(y == np.floor(y))
    assert y.var(ddof=1) > y.mean(), (y.var(ddof=1), y.mean())


@pytest.mark.parametrize("name", EVAL)
def test_restatement_reproduces_reference_nll(name):
    case = GOLDEN[name]
    g, y, fe = _data(case)
    nll, its, _, _, _ = laplace_nll(g, y, case["cov_pars"], case["aux"], offset=fe)
    assert its < MAXIT
    if case.get("iterative"):   # a stochastic estimate: the fixture records the restatement's exact value beside it
        assert abs(nll - case["nll_exact"]) <= 1e-9 * abs(case["nll_exact"])
        assert abs(nll - case["nll"]) <= 1e-3 * abs(case["nll"])   # and the estimate is an estimate of that value
        return
    assert its == case["newton_its"]
    assert abs(nll - case["nll"]) <= 1e-9 * abs(case["nll"]), (nll, case["nll"])


@pytest.mark.parametrize("name", FITS)
def test_fits_are_reproducible_and_restated(name):
    """the reference reproduces its own fit ten times inside the GPU test's tolerance, and the restatement at the
    printed parameters (mode from zero) gives the stored value"""
    case = GOLDEN[name]
    assert case["fit_spread"] <= 1e-7
    g, y, _ = _data(case)
    nll, its, _, _, _ = laplace_nll(g, y, case["cov_pars"], case["aux_fit"][0])
    assert its < MAXIT
    assert abs(nll - case["nll_restated_at_fit"]) <= 1e-9 * abs(nll)
    assert abs(nll - case["nll"]) <= 1e-6 * abs(case["nll"])   # the fit's own value: a warm-started mode


def test_generator_is_deterministic():
    g = synthetic.bench_groups(3001, (60, 9))
    y = synthetic.bench_grouped_negbin_y(g)
    np.testing.assert_array_equal(y, synthetic.bench_grouped_negbin_y(g))
    assert synthetic.bench_grouped_negbin_y(g, shape=50.).var() < y.var()   # a larger shape: less over-dispersion
