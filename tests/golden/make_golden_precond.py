#!/usr/bin/env python3
"""Reference fixtures for cg_preconditioner_type = "pivoted_cholesky" (iterative Vecchia-Laplace and
vecchia_latent), from the reference itself (oracle/_ref/ref_harness built from the reference by
oracle/Makefile):

    make -C oracle ref && python3 tests/golden/make_golden_precond.py

All cases: num_rand_vec_trace = 50, seed_rand_vec_trace = 1, ordering = random; cg_delta_conv = 1e-10 unless
stated. The harness passes rank -1, so every case runs at the default rank 50.

Every case must be a sound fixture: its pivot sequence and rank may not depend on rounding. The numpy
restatement (piv_chol_restatement.py) is run plain and perturbed on the case's points in Vecchia order;
both must give the same pivots and rank, otherwise the generator stops (choose other parameters, do not
loosen). tests/test_precond_fixtures.py repeats the check without the reference. The pivots and rank of
the restatement are recorded with each case.

The default-tolerance case (cg_delta_conv = 1e-2) also records the reference's own gradient at covariance
parameters moved by 1e-14 relative: the spread that bounds the GPU test at that tolerance.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ROOT, fmt_pars, run_ref  # noqa: E402
from piv_chol_restatement import pivoted_cholesky  # noqa: E402

sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from gpboost_amd import synthetic  # noqa: E402
from oracle import oracle as O  # noqa: E402

OUT = os.path.join(HERE, "golden_precond.json")
RANK = 50
IT = dict(matrix_inversion_method="iterative", cg_preconditioner_type="pivoted_cholesky", num_rand_vec_trace="50",
          seed_rand_vec_trace="1", ordering="random")


def data(kind, n):
    X = synthetic.bench_coords(n)
    if kind == "bench_gauss":
        return X, synthetic.bench_gaussian_y(n)
    if kind == "bench_gamma":
        return X, synthetic.bench_gamma_y(X)
    return X, (synthetic.bench_poisson_y(X) if kind == "bench_pois" else synthetic.bench_bernoulli_y(X))


def pivot_check(X, cov_fct, shape, cp):
    """Pivots and rank of the restatement, plain and perturbed, on the points in Vecchia order."""
    perm = O.vecchia_order(X.shape[0], 0, True)
    var, phi = O.transform_latent(O.cov_code(cov_fct, shape), cp)
    xv = X[perm]
    _, piv_a, rank_a = pivoted_cholesky(xv, cov_fct, shape, var, phi, RANK)
    _, piv_b, rank_b = pivoted_cholesky(xv, cov_fct, shape, var, phi, RANK, perturbed=True)
    if piv_a != piv_b or rank_a != rank_b:
        raise SystemExit(f"pivots depend on rounding ({cov_fct} {cp}, n = {X.shape[0]}): not a fixture")
    return dict(pivots=piv_a, rank=rank_a)


def spec_of(lik, cov_fct, shape, m, gp_approx="vecchia"):
    return dict(cov_fct=cov_fct, shape=str(shape), num_neighbors=m, likelihood=lik, gp_approx=gp_approx, **IT)


def eval_case(kind, n, lik, cov_fct, shape, m, cp, dc=1e-10, aux=None, estimate_aux=False, gp_approx="vecchia",
              offset=False, sens=False):
    X, y = data(kind, n)
    fe = (0.3 * np.sin(3.0 * X[:, 0]) - 0.2) if offset else None
    spec = spec_of(lik, cov_fct, shape, m, gp_approx)
    extra = dict(cg_delta_conv=repr(dc))
    if aux is not None:
        extra.update(aux_pars=repr(float(aux)), estimate_aux=str(int(estimate_aux)))
    r = run_ref(X, y, fe=fe, cov_pars=fmt_pars(cp), mode="eval", **spec, **extra)
    out = dict(data=kind, n=n, likelihood=lik, cov_fct=cov_fct, shape=shape, num_neighbors=m, gp_approx=gp_approx,
               cov_pars=list(cp), cg_delta_conv=dc, aux=aux, estimate_aux=estimate_aux, offset=offset, nll=r["nll"],
               grad=r["grad"], **pivot_check(X, cov_fct, shape, cp))
    if offset:
        out["grad_f"] = run_ref(X, y, fe=fe, cov_pars=fmt_pars(cp), mode="grad_f", **spec, **extra)["grad_f"]
    if sens:   # the reference's own gradient a few ulps away (see make_golden_100k_sens.py)
        runs = []
        for pars in ([cp[0] * (1 + 1e-14), cp[1]], [cp[0] * (1 - 1e-14), cp[1]], [cp[0], cp[1] * (1 + 1e-14)],
                     [cp[0], cp[1] * (1 - 1e-14)]):
            rr = run_ref(X, y, cov_pars=",".join(repr(v) for v in pars), mode="eval", **spec, **extra)
            runs.append(dict(cov_pars=pars, nll=rr["nll"], grad=rr["grad"]))
        out["sensitivity"] = dict(rel_perturbation=1e-14, runs=runs)
    return out


def pred_case(kind, n, lik, cov_fct, shape, m, cp, npred, nsim, response):
    X, y = data(kind, n)
    Xp = synthetic.lcg_unif(npred * 2, 0.713).reshape(2, npred).T.copy()
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        f.write(np.array([npred], dtype=np.int32).tobytes())
        f.write(np.asfortranarray(Xp).T.astype(np.float64).tobytes())
        ppath = f.name
    ptype = "latent_order_obs_first_cond_obs_only"
    spec = spec_of(lik, cov_fct, shape, m)
    # one thread: the simulation draws one stream (likelihoods.h:6668-6700), which GPBOOST_AMD_PRED_DRAWS=reference repeats
    extra = dict(cg_delta_conv="1e-10", threads=1, vecchia_pred_type=ptype, nsim_var_pred=str(nsim), predict_var="1")
    if response:
        extra["predict_response"] = "1"
    try:
        r = run_ref(X, y, cov_pars=fmt_pars(cp), mode="predict", pred=ppath, **spec, **extra)
    finally:
        os.unlink(ppath)
    return dict(data=kind, n=n, likelihood=lik, cov_fct=cov_fct, shape=shape, num_neighbors=m, cov_pars=list(cp),
                npred=npred, nsim=nsim, ptype=ptype, response=response, mean=r["mean"], var=r["var"],
                **pivot_check(X, cov_fct, shape, cp))


def main():
    lo, po = "bernoulli_logit", "poisson"
    cases = {
        # n not a multiple of 64; far points tie exactly on the remaining diagonal
        "logit_short": eval_case("bench_bern", 600, lo, "exponential", 0.5, 10, (1.0, 0.1)),
        "pois_smooth": eval_case("bench_pois", 1999, po, "matern", 1.5, 15, (0.8, 0.1)),
        # the factorisation stops before rank 50
        "pois_early_stop": eval_case("bench_pois", 300, po, "gaussian", 0.0, 10, (0.5, 1.2)),
        "gamma_aux": eval_case("bench_gamma", 700, "gamma", "exponential", 0.5, 10, (1.0, 0.1), aux=2.0,
                               estimate_aux=True),
        "gauss_latent": eval_case("bench_gauss", 700, "gaussian", "exponential", 0.5, 10, (1.0, 0.1), aux=0.1,
                                  estimate_aux=True, gp_approx="vecchia_latent"),
        "logit_grad_f": eval_case("bench_bern", 600, lo, "exponential", 0.5, 10, (1.0, 0.1), offset=True),
        "logit_default_tol": eval_case("bench_bern", 600, lo, "exponential", 0.5, 10, (1.0, 0.1), dc=1e-2, sens=True),
        "pred_latent": pred_case("bench_bern", 700, lo, "matern", 1.5, 15, (1.0, 0.1), 20, 200, False),
        "pred_response": pred_case("bench_bern", 700, lo, "matern", 1.5, 15, (1.0, 0.1), 20, 200, True),
    }
    if not cases["pois_early_stop"]["rank"] < RANK:
        raise SystemExit("the early-stop case reached the full rank")
    for k, v in cases.items():
        print(k, v.get("nll"), v.get("grad", v.get("mean", [])[:2]), "rank", v["rank"], file=sys.stderr)
    with open(OUT, "w") as f:
        json.dump(cases, f)


if __name__ == "__main__":
    main()
