"""CPU checks of the grouped-Laplace fixtures (tests/golden/golden_grouped_laplace.json, written by
tests/golden/make_golden_grouped_laplace.py from the reference): no GPU and no reference needed.

Every fixture's response is what gpboost_amd.synthetic generates, and the dense numpy restatement of the
Laplace-approximated nll (tests/golden/grouped_laplace_restatement.py: Newton from mode 0, Armijo halving, the
reference's stop rule) reproduces the reference's nll of every cholesky evaluation fixture to 1e-9 relative without
reaching the Newton iteration cap.
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
from grouped_laplace_restatement import MAXIT, laplace_nll  # noqa: E402

Y_OF = {"bernoulli_logit": synthetic.bench_grouped_bernoulli_y, "bernoulli_probit": synthetic.bench_grouped_bernoulli_y,
        "poisson": synthetic.bench_grouped_poisson_y, "gamma": synthetic.bench_grouped_gamma_y}

with open(os.path.join(HERE, "golden", "golden_grouped_laplace.json")) as _f:
    GOLDEN = json.load(_f)
EVAL = sorted(k for k, v in GOLDEN.items() if "grad" in v)


def _data(case):
    g = synthetic.bench_groups(case["n"], tuple(case["levels"]))
    y = Y_OF[case["likelihood"]](g)
    fe = 0.5 * (synthetic.lcg_unif(case["n"], 0.77) - 0.5) if case["offset"] else None
    return g, y, fe


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_fixture_response_is_the_synthetic_one(name):
    case = GOLDEN[name]
    _, y, _ = _data(case)
    assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest() == case["y_sha256"], (y.sum(), case["y_sum"])


@pytest.mark.parametrize("name", EVAL)
def test_restatement_reproduces_reference_nll(name):
    case = GOLDEN[name]
    g, y, fe = _data(case)
    nll, its, _, _, _ = laplace_nll(g, y, case["cov_pars"], case["likelihood"], aux=case["aux"] or 1.0, offset=fe)
    assert its < MAXIT
    if case.get("iterative"):   # a stochastic estimate: the fixture records the restatement's exact value beside it
        assert abs(nll - case["nll_exact"]) <= 1e-9 * abs(case["nll_exact"])
        return
    assert its == case["newton_its"]
    assert abs(nll - case["nll"]) <= 1e-9 * abs(case["nll"]), (nll, case["nll"])


def test_generators_are_deterministic_and_in_range():
    g = synthetic.bench_groups(3001, (60, 9))
    yb, yp, yg = (synthetic.bench_grouped_bernoulli_y(g), synthetic.bench_grouped_poisson_y(g),
                  synthetic.bench_grouped_gamma_y(g))
    assert set(np.unique(yb)) == {0.0, 1.0}
    assert np.all(yp >= 0) and np.all(yp == np.floor(yp))
    assert np.all(yg > 0) and np.all(np.isfinite(yg))
    np.testing.assert_array_equal(yg, synthetic.bench_grouped_gamma_y(g))
