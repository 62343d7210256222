// REModelAMD: predictions at new coordinates (GPB_PredictREModel).
//
// One call is a PredictCall; Predict and PredictClusters run the one prologue (argument checks, response,
// covariance parameters, for Laplace models the mode) and then one engine path. The paths share the
// coordinate, neighbour and factor-row helpers and the two epilogues (Laplace, Gaussian) below; what remains
// in a path is its own work around the engine's Predict.
#include <algorithm>
#include <cmath>

#include "cov.h"
#include "kernels.h"
#include "latent_kernels.h"
#include "re_model.h"
#include "vecchia_host.h"

namespace gpb_amd {

namespace {
// Gauss-Hermite rule of the given order (weight exp(-x^2)) by Newton iteration on the normalised
// Hermite recurrence; returns [nodes | weights * exp(nodes^2)] (the reference's GH_nodes_ and
// adaptive_GH_weights_ tables, likelihoods.h:12891-12980, reproduced to rounding).
std::vector<double> gauss_hermite_adaptive(int order) {
  std::vector<long double> x(order), w(order);
  const long double pim4 = 0.7511255444649424828587030047762276930510L;   // pi^-1/4
  long double z = 0.;
  const int half = (order + 1) / 2;
  for (int i = 0; i < half; ++i) {
    if (i == 0) z = std::sqrt((long double)(2 * order + 1)) - 1.85575L * std::pow((long double)(2 * order + 1), -0.16667L);
    else if (i == 1) z -= 1.14L * std::pow((long double)order, 0.426L) / z;
    else if (i == 2) z = 1.86L * z - 0.86L * x[0];
    else if (i == 3) z = 1.91L * z - 0.91L * x[1];
    else z = 2.L * z - x[i - 2];
    long double pp = 1.;
    for (int it = 0; it < 100; ++it) {
      long double p1 = pim4, p2 = 0.;
      for (int j = 1; j <= order; ++j) {
        const long double p3 = p2;
        p2 = p1;
        p1 = z * std::sqrt(2.L / j) * p2 - std::sqrt((long double)(j - 1) / j) * p3;
      }
      pp = std::sqrt(2.L * order) * p2;
      const long double z1 = z;
      z = z1 - p1 / pp;
      if (std::fabs(z - z1) <= 1e-18L) break;
    }
    x[i] = z;
    x[order - 1 - i] = -z;
    w[i] = w[order - 1 - i] = 2.L / (pp * pp);
  }
  std::vector<double> out((size_t)2 * order);
  for (int j = 0; j < order; ++j) {
    out[j] = (double)x[order - 1 - j];   // ascending, as the reference's table
    out[order + j] = (double)(w[order - 1 - j] * std::exp(x[order - 1 - j] * x[order - 1 - j]));
  }
  return out;
}
}  // namespace

// PredictResponse (likelihoods.h:7526-7580) on the latent predictive mean / variance (n_pred each, in place):
// bernoulli_logit by the adaptive Gauss-Hermite rule on the GPU, bernoulli_probit / poisson in closed form,
// gaussian (vecchia_latent) + the error variance (also on the covariance diagonal, cov nullable).
void response_transform(int lik, double aux_shape, double aux_gauss, double delta_conv, hipStream_t stream, int n_pred,
                        double* mean, double* var, double* cov) {
  if (lik == kLikBernoulliLogit) {
    static const std::vector<double> gh = gauss_hermite_adaptive(30);   // order_GH_ = 30 (likelihoods.h:12877)
    DevBuf<double> dmv((size_t)2 * n_pred), dgh(gh.size()), dout((size_t)2 * n_pred);
    HIP_CHECK(hipMemcpyAsync(dmv.get(), mean, sizeof(double) * n_pred, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(dmv.get() + n_pred, var, sizeof(double) * n_pred, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(dgh.get(), gh.data(), sizeof(double) * gh.size(), hipMemcpyHostToDevice, stream));
    launch_resp_logit(n_pred, dmv.get(), dmv.get() + n_pred, dgh.get(), dgh.get() + 30, 30, delta_conv,
                      dout.get(), dout.get() + n_pred, stream);
    HIP_CHECK(hipMemcpyAsync(mean, dout.get(), sizeof(double) * n_pred, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(var, dout.get() + n_pred, sizeof(double) * n_pred, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  } else if (lik == kLikBernoulliProbit) {   // :7531-7543
    for (int p = 0; p < n_pred; ++p) {
      mean[p] = 0.5 * std::erfc(-(mean[p] / std::sqrt(1. + var[p])) * M_SQRT1_2);
      var[p] = mean[p] * (1. - mean[p]);
    }
  } else if (lik == kLikGamma) {   // :7571-7584
    const double a = aux_shape;
    for (int p = 0; p < n_pred; ++p) {
      const double pm = std::exp(mean[p] + 0.5 * var[p]);
      var[p] = (std::exp(var[p]) - 1.) * pm * pm + std::exp(2 * mean[p] + 2 * var[p]) / a;
      mean[p] = pm;
    }
  } else if (lik == kLikNegBinomial) {   // :7585-7594, the variance as the reference has it (its last term included)
    const double r = aux_shape;
    for (int p = 0; p < n_pred; ++p) {
      const double pm = std::exp(mean[p] + 0.5 * var[p]);
      var[p] = std::exp(2 * (mean[p] + var[p])) * (1 + 1 / r) + pm * (1 - pm);
      mean[p] = pm;
    }
  } else if (lik == kLikPoisson) {   // :7557-7569
    for (int p = 0; p < n_pred; ++p) {
      const double pm = std::exp(mean[p] + 0.5 * var[p]);
      var[p] = pm * ((std::exp(var[p]) - 1.) * pm + 1.);
      mean[p] = pm;
    }
  } else {   // gaussian vecchia_latent: + the error variance
    const double aux = aux_gauss;
    for (int p = 0; p < n_pred; ++p) var[p] += aux;
    if (cov != nullptr)
      for (int p = 0; p < n_pred; ++p) cov[(size_t)p * n_pred + p] += aux;
  }
}

void REModelAMD::ResponseTransform(int n_pred, double* mean, double* var, double* cov) {
  response_transform(cfg_.lik, aux_pars_.empty() ? 1. : aux_pars_[0], aux_pars_.empty() ? 0. : aux_pars_[0],
                     iter.delta_conv_mode_finding, stream_, n_pred, mean, var, cov);
}

// ---- what every prediction call does first
// The checks, the response, the covariance parameters (given, or those of the last evaluation) and their
// transform; for Laplace models the mode at these parameters, found from zero (re_model.cpp:967-977 ->
// CalcCovFactorOrModeAndNegLL; SetYCalcCovCalcYAuxForPred, re_model_template.h:3306-3312).
PredictPars REModelAMD::PredictPrologue(const double* y, const double* cov_pars, const PredictCall& c) {
  if (world_ > 1) Fatal("predictions are only available on single-rank models");
  if (c.n_pred <= 0) Fatal("num_data_pred must be > 0");
  if (c.coords_pred == nullptr) Fatal("gp_coords_data_pred must be provided");
  UseDevice();
  if (y != nullptr) SetY(y);
  if (!y_set_) Fatal("response variable y has not been set (pass y or evaluate the likelihood first)");
  PredictPars p{};
  const int ncp = num_cov_pars();
  if (cov_pars != nullptr) std::copy(cov_pars, cov_pars + ncp, p.cp);
  else if ((int)last_cov_pars_.size() == ncp) std::copy(last_cov_pars_.begin(), last_cov_pars_.end(), p.cp);
  else Fatal("cov_pars must be provided (no previous evaluation)");
  if (!cfg_.latent) {
    double trafo[3];
    TransformCovPars(p.cp, trafo);
    p.sigma2 = trafo[0];
    p.var = trafo[1];
    p.phi = trafo[2];
    return p;
  }
  // only the Vecchia path has the Gaussian likelihood's (vecchia_latent) covariance of the response
  if (c.cov_mat && c.response && !(vecchia_ && cfg_.lik == kLikGaussian))
    Fatal("predictive covariance matrices of the response are not supported for likelihood '%s' by gpboost_amd "
          "(use predict_response = false or predict_var)", cfg_.likelihood.c_str());
  EvalLatent(p.cp, false);
  p.sigma2 = 1.;
  p.var = p.cp[0];
  p.phi = range_trafo(cfg_.cov_type, p.cp[1], cfg_.shape);
  return p;
}

// The prediction points row-major; n_obs > 0: stacked after (pred_first: before) the first n_obs model points
std::vector<double> REModelAMD::PredCoords(const PredictCall& c, int n_obs, bool pred_first) const {
  const int d = cfg_.d, n_pred = c.n_pred;
  std::vector<double> x((size_t)(n_obs + n_pred) * d);
  double* xp = x.data() + (pred_first ? 0 : (size_t)n_obs * d);
  for (int p = 0; p < n_pred; ++p)
    for (int q = 0; q < d; ++q) xp[(size_t)p * d + q] = c.coords_pred[(size_t)q * n_pred + p];
  std::copy(coords_vo_.begin(), coords_vo_.begin() + (size_t)n_obs * d, x.begin() + (pred_first ? (size_t)n_pred * d : 0));
  return x;
}

// mp neighbours of rows [row_begin, na) of xa among the earlier points up to end_at (-1: all of them), by the
// reference's sweep on the GPU (find_nearest_neighbors_Vecchia_fast, Vecchia_utils.cpp:1729-1737). The Vecchia
// paths' row kernel takes at most 64; the full-scale model takes more (the search is on the GPU up to 128, on the
// host beyond that), and the unused slots of its first rows (fewer candidates than mp) are -1.
std::vector<int> REModelAMD::PredNeighbors(const std::vector<double>& xa, int na, int mp, int row_begin, int end_at) {
  if (mp > 64 && !vif_) Fatal("num_neighbors_pred = %d > 64 is not supported by the GPU prediction kernel", mp);
  const int d = cfg_.d;
  std::vector<int> nb((size_t)(na - row_begin) * mp, -1);
  if (d <= 3 && mp <= 128) vecchia_neighbors_gpu(xa.data(), na, d, mp, row_begin, na, nb.data(), stream_, end_at);
  else vecchia_neighbors(xa.data(), na, d, mp, row_begin, na, nb.data(), end_at);
  if (vif_ && end_at < 0)
    for (int i = row_begin; i < na; ++i)
      for (int r = std::min(i, mp); r < mp; ++r) nb[(size_t)(i - row_begin) * mp + r] = -1;
  return nb;
}

// The factor rows (B, D^-1) of rows [r0, na) of xa with the neighbours nb, by the likelihood's row kernel.
// jitter = false: the nugget on the between-neighbour covariance, D starts at 1 (Vecchia_utils.cpp:1877, :1797-1798,
// :2189, :2124-2125); jitter = true: the latent process, no nugget, the between-neighbour diagonal times
// JITTER_MULT_VECCHIA, D = sigma1^2 - A c (utils.h:36, Vecchia_utils.cpp:1894-1898, :2382).
void REModelAMD::PredFactorRows(const std::vector<double>& xa, int na, const std::vector<int>& nb, int mp, int r0,
                                const PredictPars& p, bool jitter, FactorRows& f) {
  f.X.alloc(xa.size());
  f.nbr.alloc(nb.size());
  f.B.alloc(nb.size());
  f.Dinv.alloc(na - r0);
  HIP_CHECK(hipMemcpyAsync(f.X.get(), xa.data(), sizeof(double) * xa.size(), hipMemcpyHostToDevice, stream_));
  HIP_CHECK(hipMemcpyAsync(f.nbr.get(), nb.data(), sizeof(int) * nb.size(), hipMemcpyHostToDevice, stream_));
  VecchiaRowsArgs a{};
  a.X = f.X.get();
  a.Y = nullptr;   // factor rows only
  a.nbr = f.nbr.get();
  a.n = na;
  a.d = cfg_.d;
  a.m = mp;
  a.r0 = r0;
  a.r1 = na;
  a.var = p.var;
  a.phi = p.phi;
  a.diag_mult = jitter ? 1. + 1e-10 : 1.;
  a.diag_add = jitter ? 0. : 1.;
  a.d_nugget = jitter ? 0. : 1.;
  a.B_out = f.B.get();
  a.Dinv_out = f.Dinv.get();
  a.row_base = r0;
  a.mg = cfg_.mg;
  launch_vecchia_rows(cfg_.cov_type, a, stream_);
}

// The factor rows on the host, with the model's response (y non-null; Gaussian models)
void REModelAMD::DownloadFactorRows(const FactorRows& f, std::vector<double>& B, std::vector<double>& Dinv,
                                    std::vector<double>* y) {
  B.resize(f.B.size());
  Dinv.resize(f.Dinv.size());
  HIP_CHECK(hipMemcpyAsync(B.data(), f.B.get(), sizeof(double) * B.size(), hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipMemcpyAsync(Dinv.data(), f.Dinv.get(), sizeof(double) * Dinv.size(), hipMemcpyDeviceToHost, stream_));
  if (y != nullptr) {
    y->resize(cfg_.n);
    HIP_CHECK(hipMemcpyAsync(y->data(), d_y_.get(), sizeof(double) * cfg_.n, hipMemcpyDeviceToHost, stream_));
  }
  HIP_CHECK(hipStreamSynchronize(stream_));
}

// Laplace epilogue: the prediction points' fixed effects / linear predictor on the latent mean
// (re_model_template.h:3929-3946), the response transform (PredictResponse, likelihoods.h:7544-7556), the copy
void REModelAMD::LaplaceTail(const PredictCall& c, std::vector<double>& mean, std::vector<double>& var,
                             std::vector<double>& cov) {
  if (c.mean_add != nullptr)
    for (int p = 0; p < c.n_pred; ++p) mean[p] += c.mean_add[p];
  if (c.response) ResponseTransform(c.n_pred, mean.data(), var.data(), c.cov_mat ? cov.data() : nullptr);
  std::copy(mean.begin(), mean.end(), c.out);
  if (c.cov_mat) std::copy(cov.begin(), cov.end(), c.out + c.n_pred);
  else if (c.var) std::copy(var.begin(), var.begin() + c.n_pred, c.out + c.n_pred);
}

// Gaussian epilogue (re_model_template.h:3956, :3967, :3776-3815): the mean (+ mean_add), variances (v + shift) s2
// and the covariance times s2 with shift on its diagonal, where shift = +-1 adds the nugget for the response or
// removes it for the latent process. The paths round the diagonal differently and each keeps its form:
// scale_first c s2 + shift s2, else (c + shift) s2.
void REModelAMD::GaussianTail(const PredictCall& c, const double* mean, const double* var, std::vector<double>& cov,
                              double s2, double shift, bool scale_first) {
  const int n_pred = c.n_pred;
  double* o = c.out + n_pred;
  for (int p = 0; p < n_pred; ++p) c.out[p] = c.mean_add != nullptr ? mean[p] + c.mean_add[p] : mean[p];
  if (c.cov_mat) {
    if (!scale_first && shift != 0.)
      for (int p = 0; p < n_pred; ++p) cov[(size_t)p * n_pred + p] += shift;
    for (size_t e = 0; e < cov.size(); ++e) o[e] = cov[e] * s2;
    if (scale_first && shift != 0.)
      for (int p = 0; p < n_pred; ++p) o[(size_t)p * n_pred + p] += shift * s2;
  } else if (c.var) {
    for (int p = 0; p < n_pred; ++p) o[p] = (shift != 0. ? var[p] + shift : var[p]) * s2;
  }
}

void REModelAMD::Predict(const double* y, int n_pred, const double* coords_pred, const double* cov_pars,
                         bool predict_cov_mat, bool predict_var, bool predict_response, double* out,
                         const double* mean_add) {
  if (clustered())
    Fatal("cluster_ids_pred (cluster_ids_data_pred) must be provided for predictions of a model with several clusters");
  const PredictCall c{n_pred, coords_pred, predict_cov_mat, predict_var, predict_response, out, mean_add};
  const PredictPars p = PredictPrologue(y, cov_pars, c);
  if (vif_) PredictVif(c, p);
  else if (fitc_) PredictFitc(c, p);
  else if (!vecchia_) PredictDense(c, p);
  else if (!cfg_.latent && vecchia_pred_type_ == "order_pred_first") PredictPredFirst(c, p);
  else if (!cfg_.latent && vecchia_pred_type_.rfind("latent_", 0) == 0) PredictLatentGaussian(c, p);
  else PredictObsFirst(c, p);
}

// Vecchia_utils.cpp:1634-1931 (CondObsOnly = true, Gaussian, no full-scale part) and
// re_model_template.h:3787-3803, 3960-4071: neighbours of the prediction points among the
// observed points (GPU sweep, end_search_at = n - 1), the per-point rows (A, Dp) by the
// likelihood's row kernel (rows n .. n + n_pred - 1 of [observed; prediction] coordinates), then
// mean = A . y_nbr and var = (Dp - [latent: 1]) sigma2 (predict_mean_var_kernel).
void REModelAMD::PredictObsFirst(const PredictCall& c, const PredictPars& pp) {
  const bool latent = cfg_.latent;
  // observed points: the latent variables' locations (unique, Vecchia order) / the observations
  const int n = latent ? nu_ : cfg_.n, n_pred = c.n_pred, na = n + n_pred;
  const int mp = std::min(num_neighbors_pred_, n);   // end_search_at + 1 (Vecchia_utils.cpp:754-757)
  // order_obs_first_cond_all: neighbours among the observed AND the earlier prediction points
  // (find_nearest_neighbors_Vecchia_fast end_search_at = -1, Vecchia_utils.cpp:1729-1737)
  const bool cond_all = vecchia_pred_type_ == "order_obs_first_cond_all" ||
                        vecchia_pred_type_ == "latent_order_obs_first_cond_all";
  const std::vector<double> xa = PredCoords(c, n);
  const std::vector<int> nb = PredNeighbors(xa, na, mp, n, cond_all ? -1 : n - 1);
  FactorRows f;
  PredFactorRows(xa, na, nb, mp, n, pp, latent, f);
  if (latent && (cond_all || c.cov_mat || latent_->cholesky())) {
    PredictLatentSim(c, n, mp, nb, f, cond_all);
    return;
  }
  std::vector<double> mean(n_pred), var(n_pred), cov;
  if (cond_all) {
    // the covariance of cond_all is assembled on the host from the rows of Bp^-1 (they fill in): bounded like the
    // latent forms (PredictLatentSim) rather than running O(n_pred^3) host work unannounced
    if (c.cov_mat && n_pred > 20000)
      Fatal("order_obs_first_cond_all with predict_cov_mat is limited to num_data_pred <= 20000 in gpboost_amd");
    PredictCondAll(c, n, mp, nb, f, mean, var, cov);
    GaussianTail(c, mean.data(), var.data(), cov, pp.sigma2, c.response ? 0. : -1., true);
    return;
  }
  DevBuf<double> dout((size_t)2 * n_pred), dmode;
  if (latent) {   // mean = -Bpo mode (likelihoods.h:6609), Dp (no nugget to remove)
    std::vector<double> mode(n);
    latent_->GetMode(mode.data());
    dmode.alloc(n);
    HIP_CHECK(hipMemcpyAsync(dmode.get(), mode.data(), sizeof(double) * n, hipMemcpyHostToDevice, stream_));
  }
  launch_predict_mean_var(n_pred, mp, f.nbr.get(), f.B.get(), f.Dinv.get(), latent ? dmode.get() : d_y_.get(),
                          pp.sigma2, latent ? 0. : (c.response ? 0. : 1.), dout.get(), stream_);
  HIP_CHECK(hipMemcpyAsync(mean.data(), dout.get(), sizeof(double) * n_pred, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipMemcpyAsync(var.data(), dout.get() + n_pred, sizeof(double) * n_pred, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  if (latent) {
    if (c.var || c.response) {
      // + the simulation term of PredictLaplaceApproxVecchia (iterative, likelihoods.h:6628-6746)
      std::vector<double> acc(n_pred);
      latent_->PredVarSim(nsim_var_pred_, iter.num_rand_vec_trace, iter.cg_delta_conv, iter.cg_max_num_it,
                          pred_seed_++, n_pred, mp, nb.data(), f.B.get(), acc.data(), nullptr, RefDraws());
      for (int p = 0; p < n_pred; ++p) var[p] += acc[p] / nsim_var_pred_;
    }
    LaplaceTail(c, mean, var, cov);
    return;
  }
  if (c.cov_mat) {   // conditioning on observed points only: the predictive covariance is diagonal
    cov.assign((size_t)n_pred * n_pred, 0.);
    for (int p = 0; p < n_pred; ++p) cov[(size_t)p * n_pred + p] = var[p];
  }
  GaussianTail(c, mean.data(), var.data(), cov, 1., 0., true);   // the kernel has scaled the variances
}

// Latent models (Laplace, iterative) with latent_order_obs_first_cond_all or a predictive covariance
// (PredictLaplaceApproxVecchia, likelihoods.h:6576-6749): with the prediction rows' B split into Bpo
// (observed neighbours) and Bp (earlier prediction points; identity for cond_obs_only),
//   mean = -Bp^-1 Bpo mode (forward substitution in prediction order, :6610-6616)
//   var / cov = (1/nsim) sum_draws (Bp^-1 Bpo z)(.)^T + Bp^-1 diag(Dp) Bp^-T, z ~ N(0, (Sigma^-1 + W)^-1)
// with the draws of PredVarSim kept as an n_pred x nsim matrix on the device and the moments on the
// dense path (latent_pred_moments); then the response transform as in Predict.
void REModelAMD::PredictLatentSim(const PredictCall& c, int n, int mp, const std::vector<int>& nb, const FactorRows& f,
                                  bool cond_all) {
  const int n_pred = c.n_pred;
  if (cond_all && n_pred > 20000)
    Fatal("latent_order_obs_first_cond_all is limited to num_data_pred <= 20000 in gpboost_amd (dense Bp^-1)");
  if (c.cov_mat && n_pred > 40000)
    Fatal("predictive covariance matrices are limited to num_data_pred <= 40000 in gpboost_amd");
  std::vector<double> B, Dinv, mode(n);
  DownloadFactorRows(f, B, Dinv, nullptr);
  latent_->GetMode(mode.data());
  std::vector<double> mean(n_pred), D(n_pred), Bpo(B), Bp;
  if (cond_all) Bp.assign((size_t)n_pred * n_pred, 0.);
  for (int p = 0; p < n_pred; ++p) {
    D[p] = 1. / Dinv[p];
    double b = 0.;
    for (int r = 0; r < mp; ++r) {
      const int j = nb[(size_t)p * mp + r];
      const double v = B[(size_t)p * mp + r];
      if (j < n) {
        b += v * mode[j];
      } else {   // an earlier prediction point (cond_all)
        Bpo[(size_t)p * mp + r] = 0.;
        Bp[(size_t)(j - n) * n_pred + p] = v;
        b -= v * mean[j - n];   // mean holds x = Bp^-1 (Bpo mode) for the earlier points
      }
    }
    mean[p] = b;
    if (cond_all) Bp[(size_t)p * n_pred + p] = 1.;
  }
  for (int p = 0; p < n_pred; ++p) mean[p] = 0. - mean[p];
  const bool want_var = c.var || c.response;
  std::vector<double> var(n_pred), cov(c.cov_mat ? (size_t)n_pred * n_pred : 0);
  if (want_var || c.cov_mat) {
    // iterative: nsim simulation draws; cholesky: the exact term through L^-1 Bpo^T (likelihoods.h:6751-6811),
    // as n "draws" whose second moment is Bpo (Sigma^-1 + W)^-1 Bpo^T
    const bool chol = latent_->cholesky();
    const int nsim = chol ? n : nsim_var_pred_;
    if (chol && (double)n_pred * n > 4e9)
      Fatal("latent Vecchia predictions with matrix_inversion_method = 'cholesky' are limited to num_data_pred * "
            "num_data <= 4e9 in gpboost_amd (predict in batches)");
    DevBuf<double> dBpo(Bpo.size()), dV((size_t)n_pred * nsim);
    HIP_CHECK(hipMemcpyAsync(dBpo.get(), Bpo.data(), sizeof(double) * Bpo.size(), hipMemcpyHostToDevice, stream_));
    if (chol)
      latent_->PredVarChol(n_pred, mp, nb.data(), dBpo.get(), dV.get());
    else
      latent_->PredVarSim(nsim, iter.num_rand_vec_trace, iter.cg_delta_conv, iter.cg_max_num_it, pred_seed_++, n_pred,
                          mp, nb.data(), dBpo.get(), nullptr, dV.get(), RefDraws());
    latent_pred_moments(stream_, n_pred, cond_all ? Bp.data() : nullptr, D.data(), dV.get(), nsim, want_var,
                        c.cov_mat, var.data(), cov.data());
  }
  LaplaceTail(c, mean, var, cov);
}

// gp_approx = "none" (CalcPred, re_model_template.h:3894-3898 -> the dense conditional Gaussian):
// mean = Sigma_po Psi^-1 y, cov = Sigma_pp - Sigma_po Psi^-1 Sigma_op (+ the nugget for the response),
// times sigma^2 (:3956, :3967), on the dense path's factor (DenseSolver::Predict).
// With a Laplace likelihood (CalcPred, re_model_template.h:10026- -> PredictLaplaceApproxStable,
// likelihoods.h:5610-5676): latent means Sigma_po d1 and (co)variances from the factor of I + W^1/2 Sigma W^1/2.
void REModelAMD::PredictDense(const PredictCall& c, const PredictPars& p) {
  if (cfg_.cov_type == kMaternGeneral)
    Fatal("predictions with gp_approx = 'none' are not supported for cov_fct 'matern' with cov_fct_shape = %g by "
          "gpboost_amd (use gp_approx = 'vecchia'; supported shapes: 0.5, 1.5, 2.5)", cfg_.shape);
  const int n_pred = c.n_pred;
  const std::vector<double> xp = PredCoords(c);
  const bool want_var = c.var || (cfg_.latent && c.response);
  std::vector<double> mean(n_pred), var(want_var ? n_pred : 0), cov(c.cov_mat ? (size_t)n_pred * n_pred : 0);
  if (dense_lap_) {
    dense_lap_->Predict(cfg_.cov_type, p.var, p.phi, xp.data(), n_pred, want_var, c.cov_mat, mean.data(), var.data(),
                        cov.data());
    LaplaceTail(c, mean, var, cov);
    return;
  }
  dense_->Predict(cfg_.cov_type, p.var, p.phi, d_y_.get(), xp.data(), n_pred, c.var && !c.cov_mat, c.cov_mat,
                  mean.data(), var.data(), cov.data());
  GaussianTail(c, mean.data(), var.data(), cov, p.sigma2, c.response ? 1. : 0., true);
}

// FITC: the training point whose coordinates equal prediction point p's, or -1 (CalcPredFITC_FSA,
// re_model_template.h:10643-10691: TwoNumbersAreEqual on the coordinate sums, then per coordinate,
// utils.h:52-54 with EPSILON_NUMBERS = 1e-10); candidates by sorted coordinate sums.
std::vector<int> REModelAMD::FitcMatch(const std::vector<double>& xp, int n_pred) const {
  const int n = cfg_.n, d = cfg_.d;
  auto equal = [](double a, double b) {
    return std::fabs(a - b) < 1e-10 * std::max({1.0, std::fabs(a), std::fabs(b)});
  };
  std::vector<std::pair<double, int>> sums(n);
  for (int i = 0; i < n; ++i) {
    double s = 0.;
    for (int q = 0; q < d; ++q) s += coords_[(size_t)i * d + q];
    sums[i] = {s, i};
  }
  std::sort(sums.begin(), sums.end());
  std::vector<int> match(n_pred, -1);
  for (int p = 0; p < n_pred; ++p) {
    double sp = 0.;
    for (int q = 0; q < d; ++q) sp += xp[(size_t)p * d + q];
    const double tol = 1e-10 * std::max(1.0, std::fabs(sp)) * 2. + 1e-300;
    auto it = std::lower_bound(sums.begin(), sums.end(), std::make_pair(sp - tol, -1));
    for (; it != sums.end() && it->first <= sp + tol; ++it) {
      if (!equal(sp, it->first)) continue;
      bool same = true;
      for (int q = 0; q < d; ++q) same = same && equal(xp[(size_t)p * d + q], coords_[(size_t)it->second * d + q]);
      if (same) {
        match[p] = it->second;   // training coordinates are unique (FITC requires it)
        break;
      }
    }
  }
  return match;
}

// FITC (CalcPredFITC_FSA, re_model_template.h:10600-10828 via Predict :3890-3893): means, variances or the
// covariance matrix, times sigma^2 (:3956, :3967); prediction points that coincide with a training point
// (FitcMatch) get the FITC diagonal correction.
// With a Laplace likelihood (CalcPredFITC_FSA, re_model_template.h:10600-10760, then PredictLaplaceApproxFITC,
// likelihoods.h:7157-7232): latent means / variances / covariance by FitcLaplace::Predict.
void REModelAMD::PredictFitc(const PredictCall& c, const PredictPars& p) {
  const int n_pred = c.n_pred;
  const std::vector<double> xp = PredCoords(c);
  const std::vector<int> match = FitcMatch(xp, n_pred);
  const bool want_var = c.var || (cfg_.latent && c.response);
  std::vector<double> mean(n_pred), var(want_var ? n_pred : 0), cov(c.cov_mat ? (size_t)n_pred * n_pred : 0);
  if (fitc_lap_) {
    fitc_lap_->Predict(cfg_.cov_type, p.var, p.phi, xp.data(), n_pred, match, want_var, c.cov_mat, mean.data(),
                       var.data(), cov.data());
    LaplaceTail(c, mean, var, cov);
    return;
  }
  fitc_->Predict(cfg_.cov_type, p.var, p.phi, d_y_.get(), xp.data(), n_pred, match, c.var, c.cov_mat, c.response,
                 mean.data(), var.data(), cov.data());
  GaussianTail(c, mean.data(), var.data(), cov, p.sigma2, 0., false);   // FitcSolver::Predict has placed the nugget
}

// gp_approx = "full_scale_vecchia" (re_model_template.h:3708-3752 -> CalcPredVecchiaObservedFirstOrder with the
// full-scale branches, Vecchia_utils.cpp:1634-1980): the prediction points follow the observed ones in the model
// order; neighbours among the observed points (cond_obs_only) or the observed and earlier prediction points
// (cond_all) by the reference's sweep; VifSolver::Predict on the transformed scale, then times sigma^2 with the
// nugget removed for the latent process (:3776-3792).
// With a Laplace likelihood (re_model_template.h:3811-3846 -> CalcPredVecchiaObservedFirstOrder for Bpo / Bp / Dp of
// the latent residual and PredictLaplaceApproxFSVA, likelihoods.h:6060-6551): latent means, variances or covariance
// matrices by VifLaplace::Predict.
void REModelAMD::PredictVif(const PredictCall& c, const PredictPars& p) {
  const bool latent = cfg_.latent;
  const std::string& t = vecchia_pred_type_;
  const bool cond_all = t == "order_obs_first_cond_all" || (latent && t == "latent_order_obs_first_cond_all");
  if (!cond_all && t != "order_obs_first_cond_obs_only" && !(latent && t == "latent_order_obs_first_cond_obs_only")) {
    if (latent) Fatal("Prediction type '%s' is not supported for the Veccia approximation.", t.c_str());   // :3848-3850
    if (t == "order_pred_first")   // re_model_template.h:3748-3750
      Fatal("The full-scale Vecchia approximation is currently not implemented when prediction locations appear "
            "first in the ordering. Please use vecchia_pred_type = order_obs_first_cond_all or vecchia_pred_type = "
            "order_obs_first_cond_obs_only");
    Fatal("The full-scale Vecchia approximation for latent process(es) is currently not implemented");   // :3761-3763
  }
  const int n = cfg_.n, n_pred = c.n_pred, na = n + n_pred;
  const int mp = std::min(num_neighbors_pred_, cond_all ? na - 1 : n);
  const std::vector<double> xa = PredCoords(c, n);
  const std::vector<int> nb = PredNeighbors(xa, na, mp, n, cond_all ? -1 : n - 1);
  const double* xp = xa.data() + (size_t)n * cfg_.d;
  const bool want_var = c.var || (latent && c.response);
  std::vector<double> mean(n_pred), var(want_var ? n_pred : 0), cov(c.cov_mat ? (size_t)n_pred * n_pred : 0);
  double* pvar = want_var ? var.data() : nullptr;
  double* pcov = c.cov_mat ? cov.data() : nullptr;
  if (latent) {
    vif_lap_->Predict(cfg_.cov_type, p.var, p.phi, xp, n_pred, nb.data(), mp, cond_all, mean.data(), pvar, pcov);
    LaplaceTail(c, mean, var, cov);
    return;
  }
  vif_->Predict(cfg_.cov_type, p.var, p.phi, d_y_.get(), xp, n_pred, nb.data(), mp, cond_all, mean.data(), pvar, pcov);
  GaussianTail(c, mean.data(), var.data(), cov, p.sigma2, c.response ? 0. : -1., false);
}

// order_pred_first, Gaussian likelihood (CalcPredVecchiaPredictedFirstOrder, Vecchia_utils.cpp:2018-2239):
// the prediction points first (given order), then the observations (Vecchia order); every point's
// neighbours among ALL earlier points (GPU sweep from row 0); the rows' (B, D^-1) by the row kernel.
// With Bp (prediction rows, prediction columns), Bop / Bo (observation rows, prediction /
// observation columns):
//   cond_prec = Bp^T Dp^-1 Bp + Bop^T Do^-1 Bop,  mean = -cond_prec^-1 Bop^T Do^-1 Bo y,
//   cov = cond_prec^-1 (variances its diagonal), less the nugget unless predict_response, times
// sigma^2 (re_model_template.h:3788-3815). cond_prec is assembled on the host (O((n + n_pred) m^2))
// and factorized densely on the GPU (POTRF / TRTRI / GEMM). The reference factorizes it with a
// fill-reducing (AMD) permutation and reads the variances / covariance off the inverse of the
// permuted factor, i.e. in AMD-permuted order; here they come in prediction-point order.
void REModelAMD::PredictPredFirst(const PredictCall& c, const PredictPars& pp) {
  const int n = cfg_.n, n_pred = c.n_pred, na = n + n_pred;
  const int mp = std::min(num_neighbors_pred_, na - 1);
  const std::vector<double> xa = PredCoords(c, n, true);
  const std::vector<int> nb = PredNeighbors(xa, na, mp, 0, -1);
  FactorRows f;
  PredFactorRows(xa, na, nb, mp, 0, pp, false, f);
  std::vector<double> B, Dinv, y;
  DownloadFactorRows(f, B, Dinv, &y);
  // cond_prec (column-major n_pred x n_pred) and y_aux = Bop^T Do^-1 Bo y
  std::vector<double> P((size_t)n_pred * n_pred, 0.), yaux(n_pred, 0.);
  std::vector<int> pc;        // prediction columns of one row (incl. the diagonal of a prediction row)
  std::vector<double> pv;
  for (int i = 0; i < na; ++i) {
    const int k = std::min(i, mp);
    pc.clear();
    pv.clear();
    double boy = 0.;   // (Bo y)_i for an observation row
    if (i < n_pred) {
      pc.push_back(i);
      pv.push_back(1.);
    } else {
      boy = y[i - n_pred];
    }
    for (int r = 0; r < k; ++r) {
      const int j = nb[(size_t)i * mp + r];
      const double b = B[(size_t)i * mp + r];
      if (j < n_pred) {
        pc.push_back(j);
        pv.push_back(b);
      } else {
        boy += b * y[j - n_pred];
      }
    }
    const double w = Dinv[i];
    for (size_t u = 0; u < pc.size(); ++u) {
      for (size_t v = 0; v < pc.size(); ++v) P[(size_t)pc[v] * n_pred + pc[u]] += pv[u] * w * pv[v];
      if (i >= n_pred) yaux[pc[u]] += pv[u] * w * boy;
    }
  }
  std::vector<double> mean(n_pred), var(n_pred), cov(c.cov_mat ? (size_t)n_pred * n_pred : 0);
  spd_solve_inverse(stream_, n_pred, P.data(), yaux.data(), mean.data(), var.data(), c.cov_mat ? cov.data() : nullptr);
  for (int p = 0; p < n_pred; ++p) mean[p] = 0. - mean[p];
  GaussianTail(c, mean.data(), var.data(), cov, pp.sigma2, c.response ? 0. : -1., true);
}

// latent_order_obs_first_cond_obs_only / latent_order_obs_first_cond_all with the Gaussian likelihood
// (CalcPredVecchiaLatentObservedFirstOrder, Vecchia_utils.cpp:2241-2442, dispatched at
// re_model_template.h:3755-3786): a Vecchia approximation of the LATENT process over the observed
// (Vecchia order) then the prediction points, num_neighbors_pred neighbours for every point among the
// earlier observed points (cond_obs_only) or all earlier points (cond_all), no nugget (between-neighbour
// diagonal times JITTER_MULT_VECCHIA, D = sigma1^2 - A c); then Sigma = B^-1 D B^-T and the Gaussian
// conditional given y = latent + N(0, 1): mean = Sigma_po (Sigma_oo + I)^-1 y, cov = Sigma_pp -
// Sigma_po (Sigma_oo + I)^-1 Sigma_op (+ I for the response), times sigma^2. The reference forms
// B^-1 as a sparse matrix with fill; here B is dense and everything runs on the GPU's dense path, so
// the observed plus prediction points are bounded (N <= 20000).
void REModelAMD::PredictLatentGaussian(const PredictCall& c, const PredictPars& pp) {
  const int n = cfg_.n, d = cfg_.d, n_pred = c.n_pred, N = n + n_pred;
  if (N > 20000)
    Fatal("vecchia_pred_type '%s' with the Gaussian likelihood is limited to num_data + num_data_pred <= 20000 in "
          "gpboost_amd (dense latent covariance)", vecchia_pred_type_.c_str());
  const bool cond_all = vecchia_pred_type_ == "latent_order_obs_first_cond_all";
  const int mp = std::min(num_neighbors_pred_, N - 1);
  const std::vector<double> xa = PredCoords(c, n);
  {
    std::vector<int> uniq, idx;
    unique_locations(xa.data(), N, d, uniq, idx);
    if ((int)uniq.size() < N)
      Fatal("Duplicates found among training and test coordinates. This is not supported for predictions with a "
            "Vecchia approximation for the latent process ('latent_') in gpboost_amd ");
  }
  const std::vector<int> nb = PredNeighbors(xa, N, mp, 0, cond_all ? -1 : n - 1);
  FactorRows f;
  PredFactorRows(xa, N, nb, mp, 0, pp, true, f);
  std::vector<double> Bv, Dinv, y;
  DownloadFactorRows(f, Bv, Dinv, &y);
  std::vector<double> Bd((size_t)N * N, 0.), D(N);
  for (int i = 0; i < N; ++i) {
    Bd[(size_t)i * N + i] = 1.;
    const int k = std::min(i, mp);
    for (int r = 0; r < k; ++r) {
      const int j = nb[(size_t)i * mp + r];
      if (j >= 0) Bd[(size_t)j * N + i] += Bv[(size_t)i * mp + r];
    }
    D[i] = 1. / Dinv[i];
  }
  std::vector<double> mean(n_pred), var(n_pred), cov(c.cov_mat ? (size_t)n_pred * n_pred : 0);
  vecchia_latent_dense_pred(stream_, N, n, Bd.data(), D.data(), y.data(), c.var, c.cov_mat, mean.data(), var.data(),
                            cov.data());
  GaussianTail(c, mean.data(), var.data(), cov, pp.sigma2, c.response ? 1. : 0., true);
}

// order_obs_first_cond_all, Gaussian likelihood (Vecchia_utils.cpp:1776-1803 the B rows split into
// Bpo (observed neighbours) and Bp (earlier prediction points), :1977-2006 the moments): the rows
// (A = -B, Dp) come from the row kernel like the obs-only type; then on the host
//   mean = -Bp^-1 Bpo y                         (sp_L_solve: forward substitution in prediction order)
//   cov  = Bp^-1 diag(Dp) Bp^-T, var its diagonal (rows of Bp^-1 by the same recursion)
// on the transformed scale with the nugget (the caller's GaussianTail removes it, re_model_template.h:3789-3815).
void REModelAMD::PredictCondAll(const PredictCall& c, int n, int mp, const std::vector<int>& nb, const FactorRows& f,
                                std::vector<double>& mu, std::vector<double>& var, std::vector<double>& cov) {
  const int n_pred = c.n_pred;
  std::vector<double> B, Dinv, y;
  DownloadFactorRows(f, B, Dinv, &y);
  for (int p = 0; p < n_pred; ++p) {   // -Bpo y
    double s = 0.;
    for (int r = 0; r < mp; ++r) {
      const int j = nb[(size_t)p * mp + r];
      if (j < n) s -= B[(size_t)p * mp + r] * y[j];
    }
    mu[p] = s;
  }
  for (int p = 0; p < n_pred; ++p)   // Bp mu = -Bpo y, unit lower triangular in prediction order
    for (int r = 0; r < mp; ++r) {
      const int j = nb[(size_t)p * mp + r];
      if (j >= n) mu[p] -= B[(size_t)p * mp + r] * mu[j - n];
    }
  if (!c.var && !c.cov_mat) return;
  // rows of Bp^-1: R_p = e_p - sum_{j in pred nbrs(p)} B_pj R_j (sparse, column indices ascending)
  std::vector<std::vector<std::pair<int, double>>> R(n_pred);
  std::vector<double> acc(n_pred, 0.);
  std::vector<int> touched;
  std::vector<char> on(n_pred, 0);
  for (int p = 0; p < n_pred; ++p) {
    touched.clear();
    acc[p] = 1.;
    on[p] = 1;
    touched.push_back(p);
    for (int r = 0; r < mp; ++r) {
      const int j = nb[(size_t)p * mp + r];
      if (j < n) continue;
      const double b = B[(size_t)p * mp + r];
      for (const auto& e : R[j - n]) {
        if (!on[e.first]) { on[e.first] = 1; acc[e.first] = 0.; touched.push_back(e.first); }
        acc[e.first] -= b * e.second;
      }
    }
    std::sort(touched.begin(), touched.end());
    R[p].reserve(touched.size());
    for (int k : touched) {
      R[p].emplace_back(k, acc[k]);
      on[k] = 0;
    }
  }
  std::vector<double> Dp(n_pred);
  for (int p = 0; p < n_pred; ++p) Dp[p] = 1. / Dinv[p];
  for (int p = 0; p < n_pred; ++p) {
    double v = 0.;
    for (const auto& e : R[p]) v += e.second * e.second * Dp[e.first];
    var[p] = v;
  }
  if (!c.cov_mat) return;
  // cov = Bp^-1 diag(Dp) Bp^-T on the dense path (unit-lower inverse + MFMA GEMM; the host product of
  // the filled-in rows was O(n_pred^3)); Bp column-major with its unit diagonal, as PredictLatentSim
  std::vector<double> Bp((size_t)n_pred * n_pred, 0.);
  for (int p = 0; p < n_pred; ++p) {
    Bp[(size_t)p * n_pred + p] = 1.;
    for (int r = 0; r < mp; ++r) {
      const int j = nb[(size_t)p * mp + r];
      if (j >= n) Bp[(size_t)(j - n) * n_pred + p] = B[(size_t)p * mp + r];
    }
  }
  cov.assign((size_t)n_pred * n_pred, 0.);
  latent_pred_moments(stream_, n_pred, Bp.data(), Dp.data(), nullptr, 0, false, true, nullptr, cov.data());
}

}  // namespace gpb_amd
