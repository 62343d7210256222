#!/usr/bin/env python3
"""Reference fixtures for grouped random effects under the negative binomial likelihood (Laplace approximation, the
shape r as estimated auxiliary parameter) from the reference itself (oracle/_ref/ref_harness_grouped, which takes any
likelihood= string with aux_pars= / estimate_aux=):

    make -C oracle ref && python3 tests/golden/make_golden_grouped_negbin.py

Data: gpboost_amd.synthetic bench_groups with bench_grouped_negbin_y (drawn with shape 1.5, so that the marginal
variance clearly exceeds the mean) and, with covariates, bench_grouped_coef_y(..., "negative_binomial", shape=1.5).

The evaluation, prediction and training-data cases are those of make_golden_grouped_laplace.py (its eval_case /
pred_case / pred_train_case, run here with this likelihood's draw and restatement). A case is kept only if
  * the dense numpy restatement (grouped_negbin_restatement.py) reproduces every Cholesky nll to 1e-9 relative,
  * no Newton loop reaches its cap,
  * for fits, the reference's 1-thread fit and four 16-thread fits agree to 1e-7 ("fit_spread", written into the
    file): ten times inside the tests' tolerance, the condition make_golden_grouped_coef.py imposes.
The fit with covariates follows make_golden_grouped_coef.py: the harness stops before it prints aux_pars, nll and
num_it, so num_it is the smallest maxit of the 1-thread run that reproduces the unrestricted fit and the states after
every iteration ("trajectory") pin the fitted shape, which is never printed. That num_it is the optimizer's own count
unless its last iteration's line search finds no decrease (the parameters are put back and the iteration is counted,
LineSearchBacktracking.h:130-137): a sweep cannot see such an iteration, so the test applies the sweep's definition
to its own side as well.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from gpboost_amd import synthetic  # noqa: E402
import grouped_negbin_restatement as nbr  # noqa: E402
import make_golden_grouped_coef as C  # noqa: E402
import make_golden_grouped_laplace as L  # noqa: E402
from make_golden import run_ref  # noqa: E402

OUT = os.path.join(HERE, "golden_grouped_negbin.json")
NB = "negative_binomial"
DATA_SHAPE = 1.5
TIGHT = L.TIGHT

# make_golden_grouped_laplace's cases with this likelihood's draw and restatement
L.Y_OF[NB] = "bench_grouped_negbin_y"
L.laplace_nll = lambda g, y, cov_pars, likelihood, aux=1.0, offset=None: nbr.laplace_nll(g, y, cov_pars, aux,
                                                                                         offset=offset)


def fit_opts(aux, it, threads):
    o = dict(likelihood=NB, matrix_inversion_method="cholesky" if it is None else "iterative", threads=str(threads))
    if aux is not None:
        o.update(aux_pars=repr(float(aux)), estimate_aux="1")
    if it is not None:
        o.update(it)
    return o


def fit_case(n, levels, aux=None, it=None):
    """aux None: the shape initialised by the reference's own rule (FindInitialAuxPars, method of moments)"""
    g, y, _ = L.data(n, levels, NB, False)
    runs = [run_ref(None, y, groups=g, mode="fit", **fit_opts(aux, it, 1))]
    runs += [run_ref(None, y, groups=g, mode="fit", **fit_opts(aux, it, 16)) for _ in range(4)]
    r = runs[0]
    out = L.base(n, levels, NB, r["cov_pars"], aux, False, g, y)
    out.update(iterative=it, init_cov_pars=r["init_cov_pars"], nll=r["nll"], num_it=r["num_it"], aux_fit=r["aux_pars"])
    ref1 = np.asarray(r["cov_pars"] + r["aux_pars"])
    out["fit_spread"] = float(max(np.max(np.abs(np.asarray(q["cov_pars"] + q["aux_pars"]) / ref1 - 1.))
                                  for q in runs[1:]))
    if out["fit_spread"] > 1e-7 or any(q["num_it"] != r["num_it"] for q in runs[1:]):
        raise SystemExit(f"the reference's 1- and 16-thread fits differ by {out['fit_spread']:.3g} for {levels} {aux}: "
                         "choose data on which its optimizer path is stable")
    nll, its, _, _, _ = nbr.laplace_nll(g, y, r["cov_pars"], r["aux_pars"][0])
    if its >= nbr.MAXIT:
        raise SystemExit(f"Newton iteration cap reached at the fit of {levels}")
    out["nll_restated_at_fit"] = nll   # the mode from zero at the printed parameters: near the fit's own value
    return out


COEF_SPEC = (3001, (60, 9), NB, "icpt+2", (0.5, 0.4, -0.3), None, False, None)


def coef_case(spec):
    n, levels, likelihood, kind, beta, aux, offset, it = spec
    g = synthetic.bench_groups(n, levels)
    X = C.covariates(n, kind)
    y = synthetic.bench_grouped_coef_y(g, X, beta, likelihood, shape=DATA_SHAPE)
    out = dict(n=n, levels=list(levels), likelihood=likelihood, covariates=kind, beta_data=list(beta), aux=aux,
               data_shape=DATA_SHAPE, offset=False, iterative=it,
               y_sha256=hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest(), y_sum=float(y.sum()))
    runs = {}
    for threads, tag in ((1, ""), (16, "_16")):
        def fit(**extra):
            return C.run_fit_lines(y, X, None, g, **C.ref_opts(likelihood, aux, it, threads), **extra)
        r = runs[tag] = fit()
        out.update({"cov_pars" + tag: r["cov_pars"], "coef" + tag: r["coef"]})
        if threads == 1:
            out["num_it"], out["trajectory"] = C.sweep(fit, r)
        else:
            out["trajectory_16"] = [dict(cov_pars=q["cov_pars"], coef=q["coef"])
                                    for q in (fit(maxit=str(k)) for k in range(1, out["num_it"] + 1))]
    out["init_cov_pars"] = runs[""]["init_cov_pars"]
    ref1 = np.asarray(runs[""]["cov_pars"] + runs[""]["coef"])
    again = [runs["_16"]] + [C.run_fit_lines(y, X, None, g, **C.ref_opts(likelihood, aux, it, 16)) for _ in range(3)]
    out["fit_spread"] = float(max(np.max(np.abs(np.asarray(r["cov_pars"] + r["coef"]) / ref1 - 1.)) for r in again))
    if out["fit_spread"] > 1e-7:
        raise SystemExit(f"the reference's 1- and 16-thread fits differ by {out['fit_spread']:.3g} for {spec}: "
                         "choose data on which its optimizer path is stable")
    s1, s16 = np.asarray(runs[""]["coef_std_dev"]), np.asarray(runs["_16"]["coef_std_dev"])
    out.update(coef_std_dev=s1.tolist(), coef_std_dev_16=s16.tolist(),
               coef_std_dev_spread=float(np.max(np.abs(s1 - s16) / np.abs(s1))))
    return out


def main():
    cases = {
        "k1_nb_aux": L.eval_case(1001, (50,), NB, (0.8,), aux=2.0),
        "k2_nb_aux_chol": L.eval_case(3001, (60, 9), NB, (0.8, 0.3), aux=2.0),
        "k3_nb_aux_chol": L.eval_case(2000, (40, 9, 5), NB, (0.8, 0.3, 0.2), aux=2.0),
        "k2_nb_offset_chol": L.eval_case(3001, (60, 9), NB, (0.8, 0.3), aux=2.0, offset=True, grad_f=True),
        "k2_nb_aux_iter": L.eval_case(3001, (60, 9), NB, (0.8, 0.3), aux=2.0, it=TIGHT),
        "k2_nb_default_iter": L.eval_case(3001, (60, 9), NB, (0.8, 0.3), aux=2.0,
                                          it=dict(cg_delta_conv="1e-2", num_rand_vec_trace="50")),
        "fit_k1_nb": fit_case(1001, (50,)),
        "fit_k2_nb_chol": fit_case(3001, (60, 9)),
        "fit_k2_nb_init": fit_case(3001, (60, 9), aux=2.0),
        "k2_nb_icpt2_chol": coef_case(COEF_SPEC),
        "pred_k1_nb_resp": L.pred_case(1001, (50,), NB, (0.8,), 40, True, aux=2.0),
        "pred_k2_nb_chol_resp": L.pred_case(3001, (60, 9), NB, (0.8, 0.3), 48, True, aux=2.0),
        "pred_train_k2_nb_chol": pred_train_case(3001, (60, 9), (0.8, 0.3), 2.0),
    }
    for v in cases.values():   # the draw is over-dispersed
        g = synthetic.bench_groups(v["n"], tuple(v["levels"]))
        if "covariates" not in v:
            y = synthetic.bench_grouped_negbin_y(g)
            v["y_mean"], v["y_var"] = float(y.mean()), float(y.var(ddof=1))
            if not v["y_var"] > v["y_mean"]:
                raise SystemExit("the draw is not over-dispersed")
    for k, v in cases.items():
        print(k, v.get("nll"), v.get("newton_its"), v.get("num_it"), v.get("fit_spread"), v.get("aux_fit"),
              file=sys.stderr)
    with open(OUT, "w") as f:
        json.dump(cases, f)


def pred_train_case(n, levels, cov_pars, aux):
    """L.pred_train_case with the shape given (it passes none)"""
    g, y, _ = L.data(n, levels, NB, False)
    r = run_ref(None, y, groups=g, cov_pars=L.fmt_pars(cov_pars), mode="pred_train", **L.ref_opts(NB, aux, None))
    out = L.base(n, levels, NB, cov_pars, aux, False, g, y)
    out["iterative"] = None
    K = len(levels)
    mean = np.asarray(r["mean"]).reshape(K, n)
    per_level = []
    for k in range(K):
        _, first = np.unique(g[:, k], return_index=True)
        per_level.append(mean[k][np.sort(first)].tolist())
        lev_of_first = {int(g[i, k]): mean[k][i] for i in np.sort(first)}
        assert all(mean[k][i] == lev_of_first[int(g[i, k])] for i in range(n))
    out["level_means"] = per_level
    return out


if __name__ == "__main__":
    main()
