"""The reference fixtures of the covariate fits under gp_approx = "fitc" / "full_scale_vecchia"
(tests/golden/golden_cov_lowrank.json, make_golden_cov_lowrank.py) are complete and are fits: four cases, finite
values, and an iteration count strictly between 0 and the fit's maxit (a fit that stopped at maxit, or never moved,
would pin nothing)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"fitc_fit_X": ("fitc", 1000, 50), "fitc_fit_X_matern15": ("fitc", 1500, 37),
         "vif_fit_X": ("full_scale_vecchia", 1000, 30), "vif_fit_X_gaussian": ("full_scale_vecchia", 1500, 37)}


def test_cov_lowrank_fixtures_are_complete_and_finite():
    with open(os.path.join(HERE, "golden", "golden_cov_lowrank.json")) as f:
        g = json.load(f)
    assert sorted(g) == sorted(CASES)
    for name, (approx, n, m) in CASES.items():
        c = g[name]
        assert c["spec"]["gp_approx"] == approx and c["n"] == n and c["spec"]["num_ind_points"] == m, name
        p = c["p"]
        for key, size in (("cov_pars", 3), ("init_cov_pars", 3), ("coef", p), ("coef_std_dev", p), ("nll", 1)):
            v = np.atleast_1d(np.asarray(c[key], dtype=float))
            assert v.shape == (size,), (name, key)
            assert np.all(np.isfinite(v)), (name, key)
        assert np.all(np.asarray(c["cov_pars"]) > 0.) and np.all(np.asarray(c["coef_std_dev"]) > 0.), name
        assert isinstance(c["num_it"], int) and 0 < c["num_it"] < c["maxit"], (name, c["num_it"])
    assert g["vif_fit_X"]["spec"]["num_neighbors"] == 10 and g["vif_fit_X_gaussian"]["spec"]["num_neighbors"] == 15
    assert g["fitc_fit_X_matern15"]["spec"]["cov_fct"] == "matern" and g["fitc_fit_X_matern15"]["spec"]["shape"] == 1.5
    assert g["vif_fit_X_gaussian"]["spec"]["cov_fct"] == "gaussian"
