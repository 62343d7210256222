"""The refusals of a prediction call, by message, and one valid call, for every engine path behind
GPB_PredictREModel: a call that is wrong in one way reports the same message whichever engine serves it."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NP = 40, 4
PATHS = {
    "vecchia": dict(gp_approx="vecchia", num_neighbors=5),
    "vecchia_laplace": dict(gp_approx="vecchia", num_neighbors=5, likelihood="bernoulli_logit"),
    "dense": dict(gp_approx="none"),
    "dense_laplace": dict(gp_approx="none", likelihood="bernoulli_logit"),
    "fitc": dict(gp_approx="fitc", num_ind_points=8),
    "fitc_laplace": dict(gp_approx="fitc", num_ind_points=8, likelihood="bernoulli_logit"),
    "vif": dict(gp_approx="full_scale_vecchia", num_neighbors=5, num_ind_points=8),
    "vif_laplace": dict(gp_approx="full_scale_vecchia", num_neighbors=5, num_ind_points=8,
                        likelihood="bernoulli_logit"),
    "clusters": dict(gp_approx="none", cluster_ids=np.repeat([1, 2], N // 2)),
}
LAPLACE = [p for p in PATHS if p.endswith("_laplace")]

NO_Y = "response variable y has not been set (pass y or evaluate the likelihood first)"
NO_PARS = "cov_pars must be provided (no previous evaluation)"
COV_OF_RESPONSE = "predictive covariance matrices of the response are not supported for likelihood 'bernoulli_logit'"
NO_POINTS = "num_data_pred must be > 0"
NO_COORDS = "gp_coords_data_pred must be provided"


def _data(n=N):
    from gpboost_amd import synthetic
    X = synthetic.bench_coords(n + NP)
    return X[:n], X[n:]


def _model(path, n=N):
    """a fresh model of the path (no response, no evaluation), its response, parameters and prediction arguments"""
    from gpboost_amd import GPModel, synthetic
    kw = dict(PATHS[path])
    laplace = "likelihood" in kw
    X, Xp = _data(n)
    y = synthetic.bench_bernoulli_y(X) if laplace else synthetic.bench_gaussian_y(n)
    gm = GPModel(gp_coords=X, cov_function="exponential", **kw)
    pred = dict(gp_coords_pred=Xp)
    if path == "clusters":
        pred["cluster_ids_pred"] = np.array([1, 2, 1, 2])
    return gm, y, ([1.0, 0.2] if laplace else [0.1, 1.0, 0.2]), pred


def _c_predict(gm, y, n_pred, coords, cov_pars, cluster_ids=None):
    """GPB_PredictREModel itself: the Python layer derives num_data_pred from the coordinates it requires"""
    from gpboost_amd.basic import _dp, _ip, _safe_call, lib
    y, cp = np.ascontiguousarray(y, dtype=np.float64), np.asarray(cov_pars, dtype=np.float64)
    out = np.zeros(max(n_pred, 1))
    cm = np.ascontiguousarray(coords.T.reshape(-1)) if coords is not None else None
    cl = np.ascontiguousarray(cluster_ids, dtype=np.int32) if cluster_ids is not None else None
    no = ctypes.c_bool(False)
    _safe_call(lib().GPB_PredictREModel(
        gm.handle, _dp(y), ctypes.c_int32(n_pred), _dp(out), no, no, no, _ip(cl) if cl is not None else None, None, None,
        _dp(cm) if cm is not None else None, None, _dp(cp), None, no, None, None))
    return out


@pytest.mark.parametrize("path", list(PATHS))
def test_prediction_without_a_response(path):
    from gpboost_amd import GPBoostError
    gm, _, pars, pred = _model(path)
    with pytest.raises(GPBoostError) as e:
        gm.predict(cov_pars=pars, **pred)
    assert NO_Y in str(e.value)


@pytest.mark.parametrize("path", list(PATHS))
def test_prediction_without_parameters_or_an_evaluation(path):
    from gpboost_amd import GPBoostError
    gm, y, _, pred = _model(path)
    with pytest.raises(GPBoostError) as e:
        gm.predict(y=y, **pred)
    assert NO_PARS in str(e.value)


@pytest.mark.parametrize("path", LAPLACE)
def test_covariance_matrix_of_the_response(path):
    from gpboost_amd import GPBoostError
    gm, y, pars, pred = _model(path)
    with pytest.raises(GPBoostError) as e:
        gm.predict(y=y, cov_pars=pars, predict_cov_mat=True, predict_response=True, **pred)
    assert COV_OF_RESPONSE in str(e.value)


@pytest.mark.parametrize("path", list(PATHS))
def test_no_prediction_points_and_null_coordinates(path):
    from gpboost_amd import GPBoostError
    gm, y, pars, pred = _model(path)
    Xp, ids = pred["gp_coords_pred"], pred.get("cluster_ids_pred")
    for n_pred in (0, -1):
        with pytest.raises(GPBoostError) as e:
            _c_predict(gm, y, n_pred, Xp, pars, ids)
        assert NO_POINTS in str(e.value)
    with pytest.raises(GPBoostError) as e:
        _c_predict(gm, y, NP, None, pars, ids)
    assert NO_COORDS in str(e.value)


@pytest.mark.parametrize("pred_type,n,n_pred", [("order_obs_first_cond_obs_only", 70, NP),
                                                ("order_obs_first_cond_all", 70, NP),
                                                ("order_pred_first", N, 26),
                                                ("latent_order_obs_first_cond_obs_only", N, 26)])
def test_vecchia_more_than_64_prediction_neighbours(pred_type, n, n_pred):
    """num_neighbors_pred = 65 is first capped at the number of candidate points (the observations, or all earlier
    points), so the refusal needs 65 candidates: 70 observations, or 40 observations and 26 prediction points"""
    from gpboost_amd import GPBoostError, GPModel, synthetic
    X = synthetic.bench_coords(n + n_pred)
    gm = GPModel(gp_coords=X[:n], cov_function="exponential", gp_approx="vecchia", num_neighbors=5)
    gm.set_prediction_data(vecchia_pred_type=pred_type, num_neighbors_pred=65)
    with pytest.raises(GPBoostError) as e:
        gm.predict(y=synthetic.bench_gaussian_y(n), cov_pars=[0.1, 1.0, 0.2], gp_coords_pred=X[n:])
    assert "num_neighbors_pred = 65 > 64 is not supported by the GPU prediction kernel" in str(e.value)


def test_vecchia_65_prediction_neighbours_capped_at_the_observations():
    gm, y, pars, pred = _model("vecchia")
    gm.set_prediction_data(num_neighbors_pred=65)   # min(65, 40) = 40 neighbours: a valid call
    mu = gm.predict(y=y, cov_pars=pars, **pred)["mu"]
    assert mu.shape == (NP,) and np.all(np.isfinite(mu))


def test_full_scale_vecchia_prediction_points_first():
    from gpboost_amd import GPBoostError
    gm, y, pars, pred = _model("vif")
    gm.set_prediction_data(vecchia_pred_type="order_pred_first")
    with pytest.raises(GPBoostError) as e:
        gm.predict(y=y, cov_pars=pars, **pred)
    assert "not implemented when prediction locations appear first in the ordering" in str(e.value)


@pytest.mark.parametrize("path", list(PATHS))
def test_valid_call(path):
    gm, y, pars, pred = _model(path)
    r = gm.predict(y=y, cov_pars=pars, predict_var=True, predict_response=False, **pred)
    assert r["mu"].shape == (NP,) and r["var"].shape == (NP,)
    assert np.all(np.isfinite(r["mu"])) and np.all(np.isfinite(r["var"])) and np.all(r["var"] > 0.)
    r = gm.predict(cov_pars=pars, predict_cov_mat=True, predict_response=False, **pred)   # the response already set
    assert r["cov"].shape == (NP, NP) and np.all(np.isfinite(r["cov"]))
    out = _c_predict(gm, y, NP, pred["gp_coords_pred"], pars, pred.get("cluster_ids_pred"))
    assert out.shape == (NP,) and np.all(np.isfinite(out))
