#!/usr/bin/env python3
"""Reference fixtures for linear regression covariates (GPB_OptimLinRegrCoefCovPar / GPB_GetCoef) under the two
low-rank approximations, gp_approx = "fitc" and "full_scale_vecchia" (Gaussian likelihood, cholesky), from the
reference itself (oracle/_ref/ref_harness). Build container only:

    make -C oracle ref && python3 tests/golden/make_golden_cov_lowrank.py

Every case is a default fit (lbfgs + wls, nugget profiled out) on the portable LCG data of
gpboost_amd/synthetic.py. A reference fit that ends at maxit or returns a non-finite value stops the
generator: such a case proves nothing about a fit and other parameters have to be chosen.
"""
from __future__ import annotations

import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ROOT, run_ref  # noqa: E402

sys.path.insert(0, ROOT)
from gpboost_amd import synthetic  # noqa: E402

OUT = os.path.join(HERE, "golden_cov_lowrank.json")
MAXIT = 1000   # the harness's default for mode = "fit"

CASES = [
    ("fitc_fit_X", 1000, dict(gp_approx="fitc", num_ind_points=50, cov_fct="exponential")),
    ("fitc_fit_X_matern15", 1500, dict(gp_approx="fitc", num_ind_points=37, cov_fct="matern", shape=1.5)),
    ("vif_fit_X", 1000, dict(gp_approx="full_scale_vecchia", num_ind_points=30, num_neighbors=10, ordering="random",
                             ind_points_selection="kmeans++", cov_fct="exponential")),
    ("vif_fit_X_gaussian", 1500, dict(gp_approx="full_scale_vecchia", num_ind_points=37, num_neighbors=15,
                                      ordering="random", ind_points_selection="kmeans++", cov_fct="gaussian")),
]


def flat(v):
    return [float(x) for x in (v if isinstance(v, (list, tuple)) else [v])]


def main():
    out = {}
    for name, n, spec in CASES:
        X = synthetic.bench_coords(n)
        Xc = synthetic.bench_covariates(n, 2)
        y = synthetic.bench_gaussian_y_cov(X, Xc)
        r = run_ref(X, y, X=Xc, mode="fit", maxit=MAXIT, seed=0, **spec)
        rec = dict(n=n, p=Xc.shape[1], spec=spec, maxit=MAXIT, cov_pars=r["cov_pars"], coef=r["coef"],
                   coef_std_dev=r["coef_std_dev"], init_cov_pars=r["init_cov_pars"], num_it=r["num_it"], nll=r["nll"])
        if not 0 < rec["num_it"] < MAXIT:
            raise SystemExit(f"{name}: the reference fit took {rec['num_it']} iterations (maxit {MAXIT})")
        for k in ("cov_pars", "coef", "coef_std_dev", "init_cov_pars", "nll"):
            if not all(math.isfinite(x) for x in flat(rec[k])):
                raise SystemExit(f"{name}: non-finite reference value in '{k}': {rec[k]}")
        out[name] = rec
        print(name, rec["cov_pars"], rec["coef"], rec["coef_std_dev"], rec["num_it"], rec["nll"], file=sys.stderr)
    with open(OUT, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
