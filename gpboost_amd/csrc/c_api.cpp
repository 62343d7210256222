// extern "C" boundary: the GPB_* / LGBM_* symbols of include/gpboost_amd.h.
// Error convention of the reference (src/LightGBM/c_api.cpp:54-58, include/LightGBM/c_api.h:1798-1810):
// every call returns 0 / -1, the message goes to a 512-byte thread-local buffer read by
// LGBM_GetLastError. Logging goes through LGBM_RegisterLogCallback when registered
// (log.h:171-191 semantics: "[GPBoost] [Info] ..."), else stderr.
#include "gpboost_amd.h"

#include <cmath>
#include <cstdarg>
#include <cstring>
#include <exception>
#include <limits>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "coef.h"
#include "grouped_model.h"
#include "laplace_newton.h"
#include "latent_test.h"
#include "re_model.h"
#include "sparse_chol.h"
#include "grouped_test.h"
#include "lik_test.h"
#include "fitc_test.h"
#include "vif_test.h"

using gpb_amd::GroupedModel;
using gpb_amd::REModelAMD;

namespace {

// Handles of grouped-random-effects models (GroupedModel); every other handle is an REModelAMD.
std::mutex g_grouped_mu;
std::unordered_set<const void*> g_grouped;

GroupedModel* as_grouped(REModelHandle h) {
  std::lock_guard<std::mutex> lk(g_grouped_mu);
  return g_grouped.count(h) ? reinterpret_cast<GroupedModel*>(h) : nullptr;
}

// Prediction data saved by GPB_SetPredictionData for GPB_PredictREModel(use_saved_data = true)
// (REModelTemplate::SetPredictionData / Predict, re_model_template.h:3061-3119, 3168-3206): copies, per
// handle; a later call replaces the kinds of data it gives.
struct SavedPred {
  int num_data_pred = 0;
  std::vector<double> gp_coords;     // column-major num_data_pred x dim
  std::vector<double> covariates;    // column-major num_data_pred x p
  std::vector<char> re_group;        // num_data_pred x K NUL-terminated level strings, effect-major
  std::vector<double> re_group_rand_coef;   // column-major num_data_pred x R (grouped models with random slopes)
  std::vector<int32_t> cluster_ids;         // num_data_pred (GP models with several clusters)
};
std::mutex g_saved_mu;
std::unordered_map<const void*, SavedPred> g_saved;

thread_local char g_last_error[512] = "Everything is fine";
void (*g_log_callback)(const char*) = nullptr;

void set_last_error(const char* msg) {
  std::strncpy(g_last_error, msg, sizeof(g_last_error) - 1);
  g_last_error[sizeof(g_last_error) - 1] = '\0';
}

void vlog(const char* level, const char* fmt, va_list ap) {
  char buf[1024];
  int k = std::snprintf(buf, sizeof(buf), "[GPBoost] [%s] ", level);
  std::vsnprintf(buf + k, sizeof(buf) - k, fmt, ap);
  std::strncat(buf, "\n", sizeof(buf) - std::strlen(buf) - 1);
  if (g_log_callback) g_log_callback(buf);
  else std::fputs(buf, stderr);
}

REModelAMD* model(REModelHandle h) {
  if (h == nullptr) gpb_amd::Fatal("REModelHandle is NULL");
  if (as_grouped(h) != nullptr)
    gpb_amd::Fatal("this function is not supported for models with grouped random effects by gpboost_amd");
  return reinterpret_cast<REModelAMD*>(h);
}

std::string str_or(const char* s, const char* def) { return s ? std::string(s) : std::string(def); }

void copy_name(const std::string& name, char* out_str, int* num_char) {
  if (num_char) *num_char = (int)name.size() + 1;
  if (out_str) std::memcpy(out_str, name.c_str(), name.size() + 1);
}

}  // namespace

namespace gpb_amd {

void Fatal(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  throw std::runtime_error(buf);
}

void Info(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vlog("Info", fmt, ap);
  va_end(ap);
}

void Warning(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vlog("Warning", fmt, ap);
  va_end(ap);
}

}  // namespace gpb_amd

#define API_BEGIN() try {
#define API_END()                                  \
  }                                                \
  catch (std::exception & ex) {                    \
    set_last_error(ex.what());                     \
    return -1;                                     \
  }                                                \
  catch (std::string & ex) {                       \
    set_last_error(ex.c_str());                    \
    return -1;                                     \
  }                                                \
  catch (...) {                                    \
    set_last_error("unknown exception");           \
    return -1;                                     \
  }                                                \
  return 0;

extern "C" {

const char* LGBM_GetLastError(void) { return g_last_error; }

int LGBM_RegisterLogCallback(void (*callback)(const char*)) {
  API_BEGIN();
  g_log_callback = callback;
  API_END();
}

int GPB_CreateREModel(int32_t num_data, const int32_t* cluster_ids_data, const char* re_group_data,
                      int32_t num_re_group, const double* re_group_rand_coef_data,
                      const int32_t* ind_effect_group_rand_coef, int32_t num_re_group_rand_coef,
                      const int* drop_intercept_group_rand_effect, int32_t num_gp, const double* gp_coords_data,
                      const int dim_gp_coords, const double* gp_rand_coef_data, int32_t num_gp_rand_coef,
                      const char* cov_fct, double cov_fct_shape, const char* gp_approx, double cov_fct_taper_range,
                      double cov_fct_taper_shape, int num_neighbors, const char* vecchia_ordering,
                      int num_ind_points, double cover_tree_radius, const char* ind_points_selection,
                      const char* likelihood, double likelihood_additional_param,
                      const char* matrix_inversion_method, int seed, int num_parallel_threads, bool GPU_use,
                      bool has_weights, const double* weights, double likelihood_learning_rate,
                      REModelHandle* out) {
  API_BEGIN();
  (void)cov_fct_taper_range; (void)cov_fct_taper_shape;
  (void)likelihood_additional_param; (void)num_parallel_threads; (void)GPU_use;
  (void)weights; (void)likelihood_learning_rate;
  if (out == nullptr) gpb_amd::Fatal("'out' is NULL");
  if (num_gp_rand_coef > 0 || gp_rand_coef_data != nullptr)
    gpb_amd::Fatal("GP random coefficients (gp_rand_coef_data) are out of scope for gpboost_amd (SURVEY.md §8)");
  if (num_re_group_rand_coef < 0) gpb_amd::Fatal("num_re_group_rand_coef must be >= 0");
  if (num_re_group_rand_coef > 0 && (num_re_group <= 0 || re_group_data == nullptr))
    gpb_amd::Fatal("grouped random coefficients (group_rand_coef_data) need group_data");
  if (num_re_group_rand_coef > 0 && cluster_ids_data != nullptr)
    gpb_amd::Fatal("cluster_ids together with grouped random coefficients (group_rand_coef_data) are not supported "
                   "by gpboost_amd");
  if (has_weights) gpb_amd::Fatal("'weights' are not supported by gpboost_amd");
  // several clusters: GP models only (REModelAMD, re_model_cluster.cpp)
  if (cluster_ids_data != nullptr && (num_re_group > 0 || re_group_data != nullptr)) {
    for (int32_t i = 1; i < num_data; ++i)
      if (cluster_ids_data[i] != cluster_ids_data[0])
        gpb_amd::Fatal("multiple clusters (cluster_ids) with grouped random effects (group_data) are out of scope for "
                       "gpboost_amd");
  }
  if (seed < 0) gpb_amd::Fatal("seed must be >= 0");
  if (num_re_group > 0 || re_group_data != nullptr) {   // grouped random effects (GroupedModel)
    if (num_re_group <= 0 || re_group_data == nullptr) gpb_amd::Fatal("re_group_data and num_re_group must be given together");
    if ((num_gp > 0) != (gp_coords_data != nullptr)) gpb_amd::Fatal("num_gp and gp_coords_data must be given together");
    if (num_gp > 1) gpb_amd::Fatal("gpboost_amd supports at most one GP component (num_gp = 1)");
    if (num_gp == 1 && num_re_group_rand_coef > 0)
      gpb_amd::Fatal("group_rand_coef_data together with gp_coords (a Gaussian process beside grouped random effects) "
                     "is not supported by gpboost_amd");
    if (num_gp == 1 && str_or(gp_approx, "none") != "none")
      gpb_amd::Fatal("GP + grouped random effects models with gp_approx = '%s' are not supported (the reference "
                     "allows only 'none' there, re_model_template.h:236-239)", gp_approx);
    // non-Gaussian likelihoods: the Laplace approximation of GroupedLaplace; names outside parse_likelihood's fail there
    const std::string lik_name = str_or(likelihood, "gaussian");
    if (lik_name != "gaussian") {
      const int lik_code = gpb_amd::parse_likelihood(lik_name);
      if (num_gp == 1) gpb_amd::refuse_grouped_only_likelihood(lik_code, lik_name);
      if (num_gp == 1)
        gpb_amd::Fatal("a Gaussian process beside grouped random effects (gp_coords with group_data) is not supported "
                       "for likelihood '%s' by gpboost_amd", lik_name.c_str());
    }
    if (num_data <= 0) gpb_amd::Fatal("num_data must be > 0");
    std::vector<std::unordered_map<std::string, int>> index;
    auto levels = gpb_amd::parse_group_levels(num_data, num_re_group, re_group_data, &index);
    std::string mim = str_or(matrix_inversion_method, "default");
    if (num_gp == 1 && mim == "default") mim = "cholesky";   // a GP beside: the dense path
    gpb_amd::GroupedSlopes slopes;
    slopes.R = num_re_group_rand_coef;
    slopes.data = re_group_rand_coef_data;
    slopes.ind = ind_effect_group_rand_coef;
    slopes.drop = drop_intercept_group_rand_effect;
    std::unique_ptr<GroupedModel> gm(
        new GroupedModel(num_data, levels, mim, seed, std::move(index), lik_name, slopes));
    if (num_gp == 1)
      gm->AttachGP(dim_gp_coords, gp_coords_data, gpb_amd::parse_cov(str_or(cov_fct, "exponential"), cov_fct_shape),
                   seed);
    auto* g = gm.release();
    {
      std::lock_guard<std::mutex> lk(g_grouped_mu);
      g_grouped.insert(g);
    }
    *out = g;
    return 0;   // (inside API_BEGIN's try; API_END's trailing return is not reached)
  }
  if (num_gp != 1 || gp_coords_data == nullptr) gpb_amd::Fatal("gpboost_amd requires exactly one GP component (num_gp = 1)");
  gpb_amd::ModelConfig cfg;
  cfg.n = num_data;
  cfg.d = dim_gp_coords;
  cfg.cov_fct = str_or(cov_fct, "exponential");
  cfg.shape = cov_fct_shape;
  cfg.gp_approx = str_or(gp_approx, "none");
  cfg.num_neighbors = num_neighbors;
  cfg.vecchia_ordering = str_or(vecchia_ordering, "random");
  cfg.likelihood = str_or(likelihood, "gaussian");
  cfg.matrix_inversion_method = str_or(matrix_inversion_method, "default");
  cfg.seed = seed;
  cfg.num_ind_points = num_ind_points;
  cfg.cover_tree_radius = cover_tree_radius;
  cfg.ind_points_selection = str_or(ind_points_selection, "kmeans++");
  *out = new REModelAMD(cfg, gp_coords_data, cluster_ids_data);
  API_END();
}

int GPB_REModelFree(REModelHandle handle) {
  API_BEGIN();
  {
    std::lock_guard<std::mutex> lk(g_saved_mu);
    g_saved.erase(handle);
  }
  if (GroupedModel* g = as_grouped(handle)) {
    {
      std::lock_guard<std::mutex> lk(g_grouped_mu);
      g_grouped.erase(handle);
    }
    delete g;
    return 0;
  }
  delete reinterpret_cast<REModelAMD*>(handle);
  API_END();
}

int GPB_SetOptimConfig(REModelHandle handle, double* init_cov_pars, double lr, double acc_rate_cov, int max_iter,
                       double delta_rel_conv, bool use_nesterov_acc, int nesterov_schedule_version, bool trace,
                       const char* optimizer, int momentum_offset, const char* convergence_criterion,
                       int num_covariates, double* init_coef, double lr_coef, double acc_rate_coef,
                       const char* optimizer_coef, int cg_max_num_it, int cg_max_num_it_tridiag,
                       double cg_delta_conv, int num_rand_vec_trace, bool reuse_rand_vec_trace,
                       const char* cg_preconditioner_type, int seed_rand_vec_trace, int piv_chol_rank,
                       double* init_aux_pars, bool estimate_aux_pars, const int* estimate_cov_par_index,
                       int m_lbfgs, double delta_conv_mode_finding) {
  // re_model.cpp:234-332 / re_model_template.h:686-823: the settings of the likelihood path and
  // of the covariance-parameter optimizer (GPB_OptimCovPar; "lbfgs" only). Settings of the
  // gradient-descent / Nesterov / coefficient optimizers have no effect here (no covariates).
  API_BEGIN();
  // acc_rate_cov / use_nesterov_acc / nesterov_schedule_version / momentum_offset / convergence_criterion drive the
  // internal optimizers ("gradient_descent", "fisher_scoring"); L-BFGS always tests the relative change of the
  // objective (optim_utils.h:656-657)
  (void)trace;
  (void)lr_coef; (void)acc_rate_coef;
  if (GroupedModel* g = as_grouped(handle)) {   // coefficients: Laplace models, optimizer_coef "lbfgs"; aux: the shape of gamma / negative_binomial
    (void)piv_chol_rank;
    (void)num_covariates;
    g->SetOptimizerCoef(optimizer_coef, init_coef != nullptr);   // checked when covariates are given
    if (g->laplace()) {
      g->SetPreconditioner(cg_preconditioner_type);
      if (delta_conv_mode_finding > 0.) g->iter.delta_conv_mode_finding = delta_conv_mode_finding;
      if (init_aux_pars != nullptr) g->SetInitAuxPars(init_aux_pars);
      g->estimate_aux_pars = estimate_aux_pars;
    }
    g->SetOptimSettings(init_cov_pars, lr, max_iter, delta_rel_conv, optimizer, m_lbfgs);
    g->SetInternalOptimSettings(acc_rate_cov, use_nesterov_acc, nesterov_schedule_version, momentum_offset,
                                convergence_criterion);
    if (g->iterative()) {
      g->SetPreconditioner(cg_preconditioner_type);
      g->iter.cg_max_num_it = cg_max_num_it;
      g->iter.cg_max_num_it_tridiag = cg_max_num_it_tridiag;
      g->iter.cg_delta_conv = cg_delta_conv;
    }
    if (num_rand_vec_trace <= 0) gpb_amd::Fatal("num_rand_vec_trace must be > 0");
    g->iter.num_rand_vec_trace = num_rand_vec_trace;
    g->iter.seed_rand_vec_trace = seed_rand_vec_trace;
    g->iter.reuse_rand_vec_trace = reuse_rand_vec_trace;
    g->SetCovParIndexGiven(estimate_cov_par_index != nullptr && estimate_cov_par_index[0] >= 0);
    if (estimate_cov_par_index != nullptr && estimate_cov_par_index[0] >= 0) {
      for (int k = 0; k < g->num_cov_pars(); ++k)
        if (estimate_cov_par_index[k] <= 0) gpb_amd::Fatal("estimate_cov_par_index: fixing covariance parameters is not supported by gpboost_amd");
    }
    return 0;
  }
  REModelAMD* m = model(handle);
  (void)num_covariates; (void)init_coef;   // the "wls" coefficient update profiles beta out at every evaluation
  const bool iterative = m->config().matrix_inversion_method == "iterative";
  std::string precond;   // canonical name (ParsePreconditionerAlias, re_model_template.h:6756-6787); "": unchanged
  if (iterative && cg_preconditioner_type != nullptr && std::string(cg_preconditioner_type) != "") {
    const std::string p(cg_preconditioner_type);
    if (p == "vadu" || p == "VADU" || p == "vecchia_approximation_with_diagonal_update" || p == "Sigma_inv_plus_BtWB")
      precond = "vadu";
    else if (p == "pivoted_cholesky" || p == "piv_chol" || p == "piv_chol_on_Sigma")
      precond = "pivoted_cholesky";
    else
      gpb_amd::Fatal("cg_preconditioner_type '%s' is not supported by gpboost_amd (supported: vadu, pivoted_cholesky)",
                     p.c_str());
    if (precond == "pivoted_cholesky" && m->world_size() > 1)
      gpb_amd::Fatal("cg_preconditioner_type = 'pivoted_cholesky' is not supported on multi-rank (sharded) models by "
                     "gpboost_amd (use 'vadu')");
  }
  m->SetOptimSettings(init_cov_pars, lr, max_iter, delta_rel_conv, optimizer, m_lbfgs);
  m->SetInternalOptimSettings(acc_rate_cov, use_nesterov_acc, nesterov_schedule_version, momentum_offset,
                              convergence_criterion);
  // validated above; the canonical preconditioner name is recorded for iterative models only
  m->SetOptimizerNames(optimizer, optimizer_coef, precond.empty() ? nullptr : precond.c_str());
  if (iterative) {   // :775-801
    if (!precond.empty()) m->iter.piv_chol = precond == "pivoted_cholesky";
    // fitc_piv_chol_preconditioner_rank (:789-800): a value > 0, else default_piv_chol_preconditioner_rank_ = 50
    m->iter.piv_chol_rank = piv_chol_rank > 0 ? piv_chol_rank : 50;
    if (m->iter.piv_chol && m->iter.piv_chol_rank > m->num_latent())   // :8464-8467
      gpb_amd::Fatal("'fitc_piv_chol_preconditioner_rank' cannot be larger than the dimension of the mode (= number of "
                     "unique locations) ");
    m->iter.cg_max_num_it = cg_max_num_it;
    m->iter.cg_max_num_it_tridiag = cg_max_num_it_tridiag;
    m->iter.cg_delta_conv = cg_delta_conv;
  }
  if (num_rand_vec_trace <= 0) gpb_amd::Fatal("num_rand_vec_trace must be > 0");
  m->iter.num_rand_vec_trace = num_rand_vec_trace;   // :771-773
  m->iter.seed_rand_vec_trace = seed_rand_vec_trace;
  m->iter.reuse_rand_vec_trace = reuse_rand_vec_trace;
  if (delta_conv_mode_finding > 0.) m->iter.delta_conv_mode_finding = delta_conv_mode_finding;   // :820-822
  if (init_aux_pars != nullptr) m->SetInitAuxPars(init_aux_pars);
  m->estimate_aux_pars = estimate_aux_pars;   // :803
  if (estimate_cov_par_index != nullptr && estimate_cov_par_index[0] >= 0)   // SetOptimConfig :806-816
    m->SetEstimateCovParIndex(std::vector<int>(estimate_cov_par_index, estimate_cov_par_index + m->num_cov_pars()));
  API_END();
}

int GPB_EvalNegLogLikelihood(REModelHandle handle, const double* y_data, double* cov_pars,
                             const double* fixed_effects, double* negll) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    if (cov_pars == nullptr)
      gpb_amd::Fatal("cov_pars is NULL: evaluating at the initial values is not supported for grouped random effects "
                     "models by gpboost_amd");
    if (fixed_effects != nullptr && y_data == nullptr)
      gpb_amd::Fatal("EvalNegLogLikelihood: 'y_data' cannot nullptr when 'fixed_effects' is provided");
    g->SetResponseAndOffset(y_data, fixed_effects);
    negll[0] = g->Eval(cov_pars, false, 0).nll;
    return 0;
  }
  REModelAMD* m = model(handle);
  if (fixed_effects != nullptr && y_data == nullptr && !m->config().latent)
    gpb_amd::Fatal("EvalNegLogLikelihood: 'y_data' cannot nullptr when 'fixed_effects' is provided");
  m->SetResponseAndOffset(y_data, fixed_effects);
  if (cov_pars == nullptr) {   // re_model.cpp:598-605: the current parameters, initialised if not defined
    if (y_data != nullptr) m->InitCovParsIfNotDefined(y_data, fixed_effects);
    else if (m->config().latent) m->InitCovParsIfNotDefined(nullptr, nullptr);
    if (m->current_cov_pars().empty()) gpb_amd::Fatal("Covariance parameters have not been initialized");
    const std::vector<double> cp = m->current_cov_pars();
    negll[0] = m->Eval(cp.data(), false, 0).nll;
    return 0;
  }
  negll[0] = m->Eval(cov_pars, false, 0).nll;
  API_END();
}

int GPB_SetPredictionData(REModelHandle handle, int32_t num_data_pred, const int32_t* cluster_ids_data_pred,
                          const char* re_group_data_pred, const double* re_group_rand_coef_data_pred,
                          double* gp_coords_data_pred, const double* gp_rand_coef_data_pred,
                          const double* covariate_data_pred, const char* vecchia_pred_type, int num_neighbors_pred,
                          double cg_delta_conv_pred, int nsim_var_pred, int rank_pred_approx_matrix_lanczos) {
  API_BEGIN();
  (void)cg_delta_conv_pred;   // the Vecchia-Laplace draws use the model's cg_delta_conv (likelihoods.h:12052)
  (void)rank_pred_approx_matrix_lanczos;
  if (handle == nullptr) gpb_amd::Fatal("REModelHandle is NULL");
  GroupedModel* g = as_grouped(handle);
  // cluster ids: saved for GP models with several clusters only
  const bool clusters_ok = cluster_ids_data_pred != nullptr && g == nullptr && model(handle)->clustered();
  if ((cluster_ids_data_pred != nullptr && !clusters_ok) || gp_rand_coef_data_pred != nullptr ||
      (re_group_rand_coef_data_pred != nullptr && g == nullptr))
    gpb_amd::Fatal("GPB_SetPredictionData: clusters and random coefficients are not supported by gpboost_amd");
  if (re_group_rand_coef_data_pred != nullptr && !g->has_slopes())
    gpb_amd::Fatal("group_rand_coef_data_pred is given but the model has no grouped random coefficients");
  const bool has_data = re_group_data_pred != nullptr || gp_coords_data_pred != nullptr ||
                        covariate_data_pred != nullptr || re_group_rand_coef_data_pred != nullptr ||
                        cluster_ids_data_pred != nullptr;
  if (has_data) {
    if (num_data_pred <= 0) gpb_amd::Fatal("num_data_pred must be > 0 when prediction data is given");   // CHECK :3075
    if (g != nullptr && gp_coords_data_pred != nullptr && !g->has_gp())
      gpb_amd::Fatal("GP coordinates or covariates for a grouped random effects model are not supported by gpboost_amd");
    if (g != nullptr && covariate_data_pred != nullptr && !g->laplace())
      gpb_amd::Fatal("GP coordinates or covariates for a grouped random effects model are not supported by gpboost_amd");
    if (g == nullptr && re_group_data_pred != nullptr)
      gpb_amd::Fatal("grouped random effects data for a GP model are not supported by gpboost_amd");
    SavedPred sp;
    {
      std::lock_guard<std::mutex> lk(g_saved_mu);
      auto it = g_saved.find(handle);
      if (it != g_saved.end()) sp = it->second;
    }
    if (sp.num_data_pred != num_data_pred) {   // kinds saved for another size would be read past their end
      if (gp_coords_data_pred == nullptr) sp.gp_coords.clear();
      if (covariate_data_pred == nullptr) sp.covariates.clear();
      if (re_group_data_pred == nullptr) sp.re_group.clear();
      if (re_group_rand_coef_data_pred == nullptr) sp.re_group_rand_coef.clear();
      if (cluster_ids_data_pred == nullptr) sp.cluster_ids.clear();
    }
    sp.num_data_pred = num_data_pred;
    if (cluster_ids_data_pred != nullptr)
      sp.cluster_ids.assign(cluster_ids_data_pred, cluster_ids_data_pred + num_data_pred);
    if (gp_coords_data_pred != nullptr) {
      const size_t cnt = (size_t)num_data_pred * (g != nullptr ? g->gp_dim() : model(handle)->config().d);
      sp.gp_coords.assign(gp_coords_data_pred, gp_coords_data_pred + cnt);
    }
    if (covariate_data_pred != nullptr) {
      const int p = g != nullptr ? g->num_covariates() : model(handle)->num_covariates();
      if (p <= 0) gpb_amd::Fatal("Covariate data 'X_pred' is provided but the model has no covariates");
      sp.covariates.assign(covariate_data_pred, covariate_data_pred + (size_t)num_data_pred * p);
    }
    if (re_group_data_pred != nullptr) {   // num_data_pred x K NUL-terminated strings
      const char* e = re_group_data_pred;
      for (long k = 0; k < (long)num_data_pred * g->num_groups(); ++k) e += std::strlen(e) + 1;
      sp.re_group.assign(re_group_data_pred, e);
    }
    if (re_group_rand_coef_data_pred != nullptr)
      sp.re_group_rand_coef.assign(re_group_rand_coef_data_pred,
                                   re_group_rand_coef_data_pred + (size_t)num_data_pred * g->num_slopes());
    std::lock_guard<std::mutex> lk(g_saved_mu);
    g_saved[handle] = std::move(sp);
  }
  if (g == nullptr) model(handle)->SetPredictionData(vecchia_pred_type, num_neighbors_pred, nsim_var_pred);
  API_END();
}

int GPB_PredictREModel(REModelHandle handle, const double* y_data, int32_t num_data_pred, double* out_predict,
                       bool predict_cov_mat, bool predict_var, bool predict_response,
                       const int32_t* cluster_ids_data_pred, const char* re_group_data_pred,
                       const double* re_group_rand_coef_data_pred, double* gp_coords_data_pred,
                       const double* gp_rand_coef_data_pred, const double* cov_pars,
                       const double* covariate_data_pred, bool use_saved_data, const double* fixed_effects,
                       const double* fixed_effects_pred) {
  API_BEGIN();
  if (out_predict == nullptr) gpb_amd::Fatal("out_predict is NULL");
  SavedPred saved;
  if (use_saved_data) {   // re_model_template.h:3168-3206: the saved data replaces the arguments
    {
      std::lock_guard<std::mutex> lk(g_saved_mu);
      auto it = g_saved.find(handle);
      if (it == g_saved.end() || it->second.num_data_pred <= 0)
        gpb_amd::Fatal("No data has been set for making predictions. Call set_prediction_data first");
      saved = it->second;
    }
    if (num_data_pred > 0 && num_data_pred != saved.num_data_pred)
      gpb_amd::Fatal("num_data_pred (%d) differs from the saved prediction data (%d)", num_data_pred, saved.num_data_pred);
    num_data_pred = saved.num_data_pred;
    cluster_ids_data_pred = saved.cluster_ids.empty() ? nullptr : saved.cluster_ids.data();
    re_group_rand_coef_data_pred = saved.re_group_rand_coef.empty() ? nullptr : saved.re_group_rand_coef.data();
    gp_rand_coef_data_pred = nullptr;
    re_group_data_pred = saved.re_group.empty() ? nullptr : saved.re_group.data();
    gp_coords_data_pred = saved.gp_coords.empty() ? nullptr : saved.gp_coords.data();
    covariate_data_pred = saved.covariates.empty() ? nullptr : saved.covariates.data();
  }
  if (GroupedModel* g = as_grouped(handle)) {
    if (cluster_ids_data_pred != nullptr || gp_rand_coef_data_pred != nullptr ||
        (covariate_data_pred != nullptr && !g->laplace()))
      gpb_amd::Fatal("predictions with clusters, GP random coefficients or covariates are not supported "
                     "for grouped random effects models by gpboost_amd");
    // Laplace models with covariates: the mode is found with the offset F + X beta (GroupedModel::
    // SetResponseAndOffset) and X_pred beta joins fixed_effects_pred before the response transformation
    std::vector<double> mean_add;
    if (g->has_covariates()) {
      if (covariate_data_pred == nullptr)
        gpb_amd::Fatal("Covariate data 'X_pred' is not provided but the model has covariates");
      if (num_data_pred <= 0) gpb_amd::Fatal("num_data_pred must be > 0");
      mean_add.assign(num_data_pred, 0.);
      g->AddLinearPredictor(covariate_data_pred, num_data_pred, mean_add.data());
      if (fixed_effects_pred != nullptr)
        for (int i = 0; i < num_data_pred; ++i) mean_add[i] += fixed_effects_pred[i];
      fixed_effects_pred = mean_add.data();
    } else if (covariate_data_pred != nullptr) {
      gpb_amd::Fatal("Covariate data 'X_pred' is provided but the model has no covariates");
    }
    g->Predict(y_data, num_data_pred, re_group_data_pred, gp_coords_data_pred, cov_pars, predict_cov_mat, predict_var,
               predict_response, fixed_effects, fixed_effects_pred, out_predict, re_group_rand_coef_data_pred);
    return 0;
  }
  REModelAMD* m = model(handle);
  if ((cluster_ids_data_pred != nullptr && !m->clustered()) || re_group_data_pred != nullptr ||
      re_group_rand_coef_data_pred != nullptr || gp_rand_coef_data_pred != nullptr)
    gpb_amd::Fatal("predictions with clusters, grouped random effects or random coefficients are not "
                   "supported by gpboost_amd");
  if (m->clustered() && covariate_data_pred != nullptr)
    m->RefuseClusters("linear regression covariates (X_pred)");
  std::vector<double> r;
  const double* y = y_data;
  if (m->has_covariates()) {   // y - X beta - offset (SetYCalcCovCalcYAuxForPred, re_model_template.h:3386-3410)
    if (covariate_data_pred == nullptr)
      gpb_amd::Fatal("Covariate data 'X_pred' is not provided but the model has covariates");
    r = m->ResidualResponse(y_data, fixed_effects);
    y = r.data();
  } else if (covariate_data_pred != nullptr) {
    gpb_amd::Fatal("Covariate data 'X_pred' is provided but the model has no covariates");
  } else if (m->config().latent) {   // non-Gaussian: F is the offset of the location parameter (the mode);
    m->SetLatentOffset(m->ResolveOffset(fixed_effects));   // none given: the saved one (re_model_template.h:3306-3312)
  } else if (fixed_effects != nullptr) {   // the GP part of the response (re_model_template.h:3386-3393)
    if (y_data == nullptr) gpb_amd::Fatal("'y_data' cannot be NULL when 'fixed_effects' is provided");
    r.resize(m->config().n);
    for (int i = 0; i < m->config().n; ++i) r[i] = y_data[i] - fixed_effects[i];
    y = r.data();
  }
  // fixed_effects_pred (and X_pred beta) join the predictive mean before any response transform
  // (re_model_template.h:3929-3946)
  std::vector<double> mean_add;
  if (m->has_covariates() || fixed_effects_pred != nullptr) {
    mean_add.assign(num_data_pred, 0.);
    if (m->has_covariates()) m->AddLinearPredictor(covariate_data_pred, num_data_pred, mean_add.data());
    if (fixed_effects_pred != nullptr)
      for (int i = 0; i < num_data_pred; ++i) mean_add[i] += fixed_effects_pred[i];
  }
  if (m->clustered()) {   // a missing cluster_ids_data_pred fails there, naming it
    m->PredictClusters(y, num_data_pred, gp_coords_data_pred, cluster_ids_data_pred, cov_pars, predict_cov_mat,
                       predict_var, predict_response, out_predict, mean_add.empty() ? nullptr : mean_add.data());
    return 0;
  }
  m->Predict(y, num_data_pred, gp_coords_data_pred, cov_pars, predict_cov_mat, predict_var, predict_response,
             out_predict, mean_add.empty() ? nullptr : mean_add.data());
  API_END();
}

int GPB_EvalNegLogLikelihoodGrad(REModelHandle handle, const double* y_data, const double* cov_pars,
                                 const double* fixed_effects, int profile_sigma2, double* negll, double* grad,
                                 double* sigma2_out) {
  API_BEGIN();
  if (cov_pars == nullptr || negll == nullptr || grad == nullptr) gpb_amd::Fatal("NULL argument");
  gpb_amd::EvalResult res;
  if (GroupedModel* g = as_grouped(handle)) {
    g->SetResponseAndOffset(y_data, fixed_effects);
    res = g->Eval(cov_pars, true, profile_sigma2 ? 1 : 0);
  } else {
    REModelAMD* m = model(handle);
    m->SetResponseAndOffset(y_data, fixed_effects);
    res = m->Eval(cov_pars, true, profile_sigma2 ? 1 : 0);
  }
  negll[0] = res.nll;
  for (size_t k = 0; k < res.grad.size(); ++k) {
    double g = res.grad[k];
    if (std::isnan(g) || std::isinf(g)) {  // re_model_template.h:1944-1955
      gpb_amd::Warning("NaN or Inf occurred in gradient wrt covariance parameter number %d; it is set to 0", (int)k);
      g = 0.;
    }
    grad[k] = g;
  }
  if (sigma2_out) sigma2_out[0] = res.sigma2;
  API_END();
}

int GPB_GetCurrentNegLogLikelihood(REModelHandle handle, double* negll) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    negll[0] = g->last_nll();
    return 0;
  }
  negll[0] = model(handle)->last_nll();
  API_END();
}

int GPB_GetCovPar(REModelHandle handle, double* cov_par, bool calc_std_dev) {
  API_BEGIN();
  // re_model.cpp:767-811: cov_par[0, P) = parameters, cov_par[P, 2P) = std devs if calc_std_dev
  if (GroupedModel* g = as_grouped(handle)) {
    const auto& p = g->last_cov_pars();
    if (p.empty()) gpb_amd::Fatal("Covariance parameters have not been estimated or correctly set ");
    for (size_t k = 0; k < p.size(); ++k) cov_par[k] = p[k];
    if (calc_std_dev) g->StdDevCovPars(p.data(), cov_par + p.size());
    return 0;
  }
  REModelAMD* m = model(handle);
  const auto p = m->last_cov_pars();
  if (p.empty()) gpb_amd::Fatal("Covariance parameters have not been estimated or correctly set ");
  for (size_t k = 0; k < p.size(); ++k) cov_par[k] = p[k];
  if (calc_std_dev) m->StdDevCovPars(p.data(), cov_par + p.size());
  API_END();
}

int GPB_GetNumIt(REModelHandle handle, int* num_it) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    num_it[0] = g->num_it();
    return 0;
  }
  num_it[0] = model(handle)->num_it();
  API_END();
}

int GPB_GetInitCovPar(REModelHandle handle, double* init_cov_pars) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    g->GetInitCovPar(init_cov_pars);
    return 0;
  }
  model(handle)->GetInitCovPar(init_cov_pars);
  API_END();
}

int GPB_OptimCovPar(REModelHandle handle, const double* y_data, const double* fixed_effects) {
  // c_api.cpp GPB_OptimCovPar -> REModel::OptimCovPar(y, fixed_effects, false, false)
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    g->OptimCovPar(y_data, fixed_effects);
    return 0;
  }
  model(handle)->OptimCovPar(y_data, fixed_effects);
  API_END();
}

int GPB_OptimLinRegrCoefCovPar(REModelHandle handle, const double* y_data, const double* covariate_data,
                               int num_covariates, const double* fixed_effects) {
  // c_api.cpp:2843-2852 -> REModel::OptimLinRegrCoefCovPar (re_model.cpp:403-469)
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    if (covariate_data != nullptr && num_covariates > 0) {
      if (!g->laplace() || g->has_gp())   // the Gaussian grouped model's GLS is not implemented
        gpb_amd::Fatal("linear regression covariates with grouped random effects are not supported by gpboost_amd");
      g->OptimLinRegrCoefCovPar(y_data, covariate_data, num_covariates, fixed_effects);
      return 0;
    }
    g->OptimCovPar(y_data, fixed_effects);
    return 0;
  }
  model(handle)->OptimLinRegrCoefCovPar(y_data, covariate_data, num_covariates, fixed_effects);
  API_END();
}

int GPB_OptimCovParBoosting(REModelHandle handle, const double* y_data, const double* fixed_effects,
                            bool called_in_GPBoost_algorithm, bool reuse_learning_rates_from_previous_call) {
  // REModel::OptimCovPar(y, F, called_in_GPBoost_algorithm, reuse) (re_model.cpp:339-401)
  API_BEGIN();
  if (as_grouped(handle) != nullptr)
    gpb_amd::Fatal("the GPBoost-algorithm covariance update (GPB_OptimCovParBoosting) is not supported for grouped "
                   "random effects models by gpboost_amd");
  model(handle)->RefuseClusters("the GPBoost-algorithm covariance update (GPB_OptimCovParBoosting)");
  model(handle)->OptimCovPar(y_data, fixed_effects, called_in_GPBoost_algorithm, reuse_learning_rates_from_previous_call);
  API_END();
}

int GPB_GetInducingPoints(REModelHandle handle, int32_t* num_ind_points, double* ind_points) {
  API_BEGIN();
  if (as_grouped(handle) != nullptr) gpb_amd::Fatal("model does not use gp_approx = 'fitc'");
  const std::vector<double>& Z = model(handle)->InducingPoints();
  const int d = model(handle)->config().d;
  if (num_ind_points != nullptr) *num_ind_points = (int32_t)(Z.size() / d);
  if (ind_points != nullptr) std::copy(Z.begin(), Z.end(), ind_points);
  API_END();
}

int GPB_CalcGradientF(REModelHandle handle, double* y, const double* fixed_effects, bool calc_cov_factor) {
  // REModel::CalcGradient (re_model.cpp:667-680), the call the boosting objective makes
  // (regression_objective.hpp:164-179)
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    if (g->laplace()) {
      g->CalcGradientF(y, fixed_effects, calc_cov_factor);
      return 0;
    }
  }
  model(handle)->CalcGradientF(y, fixed_effects, calc_cov_factor);
  API_END();
}

int GPB_CanCalculateStandardErrorsCovPars(REModelHandle handle, int* out) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {   // cholesky: exact Fisher information; iterative: refused
    out[0] = (int)g->CanCalculateStandardErrorsCovPars();
    return 0;
  }
  out[0] = (int)model(handle)->CanCalculateStandardErrorsCovPars();
  API_END();
}

int GPB_GetCoef(REModelHandle handle, double* optim_coef, bool calc_std_dev) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    g->GetCoef(optim_coef, calc_std_dev);
    return 0;
  }
  model(handle)->GetCoef(optim_coef, calc_std_dev);
  API_END();
}

int GPB_GetNumCoef(REModelHandle handle, int* num_coef) {
  API_BEGIN();
  if (num_coef == nullptr) gpb_amd::Fatal("GPB_GetNumCoef: num_coef is NULL");
  GroupedModel* g = as_grouped(handle);
  num_coef[0] = g != nullptr ? g->num_covariates() : model(handle)->num_covariates();
  API_END();
}

int GPB_EvalNegLogLikelihoodGradCoef(REModelHandle handle, const double* cov_pars, const double* aux_pars,
                                     const double* coef, const double* y_data, const double* covariate_data,
                                     int num_covariates, const double* fixed_effects, double* negll, double* grad_cov,
                                     double* grad_aux, double* grad_coef) {
  API_BEGIN();
  GroupedModel* g = as_grouped(handle);
  if (g == nullptr)
    gpb_amd::Fatal("GPB_EvalNegLogLikelihoodGradCoef: the model needs grouped random effects with a non-Gaussian "
                   "likelihood");
  if (negll == nullptr || grad_coef == nullptr) gpb_amd::Fatal("GPB_EvalNegLogLikelihoodGradCoef: NULL argument");
  negll[0] = g->EvalGradCoef(cov_pars, aux_pars, coef, y_data, covariate_data, num_covariates, fixed_effects, grad_cov,
                             grad_aux, grad_coef);
  API_END();
}

int GPB_TestCoefOps(int n, int p, const double* X, const double* beta, const double* dir, const double* F,
                    const double* gF, double* eta0, double* g, double* mom) {
  API_BEGIN();
  gpb_amd::test_coef_ops(n, p, X, beta, dir, F, gF, eta0, g, mom);
  API_END();
}

int GPB_TestCoefHost(int op, int lik, int n, int p, const double* X, const double* y, const double* F,
                     const double* in, double* out) {
  // host only: 0 scaling (out = [intercept_col, scaled, loc (p), scale (p), scaled X row-major (n p)]);
  // 1 / 2 TransformCoef / TransformBackCoef of in (p) -> out (p); 3 the initial intercept with in[0] = the random
  // effects' total variance -> out[0]; 4 C_mu, C_sigma2 -> out[0 .. 1]; 5 the step cap from in = [4 sums, C_mu,
  // C_sigma2] over n observations -> out[0]
  API_BEGIN();
  if (out == nullptr) gpb_amd::Fatal("GPB_TestCoefHost: out is NULL");
  if (op >= 0 && op <= 2) {
    std::vector<double> Xs;
    const gpb_amd::CoefScaling sc(n, p, X, op == 0 ? &Xs : nullptr);
    if (op == 0) {
      out[0] = sc.intercept_col;
      out[1] = sc.scaled ? 1. : 0.;
      std::copy(sc.loc.begin(), sc.loc.end(), out + 2);
      std::copy(sc.scale.begin(), sc.scale.end(), out + 2 + p);
      std::copy(Xs.begin(), Xs.end(), out + 2 + 2 * p);
    } else {
      if (in == nullptr) gpb_amd::Fatal("GPB_TestCoefHost: in is NULL");
      const std::vector<double> b(in, in + p);
      const std::vector<double> r = op == 1 ? sc.ToScaled(b) : sc.ToOriginal(b);
      std::copy(r.begin(), r.end(), out);
    }
  } else if (op == 3) {
    if (y == nullptr || in == nullptr || n < 1) gpb_amd::Fatal("GPB_TestCoefHost: invalid argument");
    out[0] = gpb_amd::coef_initial_intercept(lik, n, y, F, in[0]);
  } else if (op == 4) {
    if (y == nullptr || n < 1) gpb_amd::Fatal("GPB_TestCoefHost: invalid argument");
    gpb_amd::coef_cap_constants(lik, n, y, out, out + 1);
  } else if (op == 5) {
    if (in == nullptr || n < 1) gpb_amd::Fatal("GPB_TestCoefHost: invalid argument");
    out[0] = gpb_amd::coef_max_learning_rate(in, n, in[4], in[5]);
  } else {
    gpb_amd::Fatal("GPB_TestCoefHost: unknown op %d", op);
  }
  API_END();
}

int GPB_PredictREModelTrainingDataRandomEffects(REModelHandle handle, const double* cov_pars_pred, const double* y_obs,
                                                double* out_predict, const double* fixed_effects, bool calc_var) {
  API_BEGIN();
  if (out_predict == nullptr) gpb_amd::Fatal("out_predict is NULL");
  if (GroupedModel* g = as_grouped(handle)) {
    g->PredictTrainingDataRandomEffects(cov_pars_pred, y_obs, out_predict, fixed_effects, calc_var);
    return 0;
  }
  model(handle)->PredictTrainingDataRandomEffects(cov_pars_pred, y_obs, out_predict, fixed_effects, calc_var);
  API_END();
}

int GPB_GetOptimizerCovPars(REModelHandle handle, char* out_str, int* num_char) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {   // InitializeOptimSettings (re_model_template.h:7463-7474)
    copy_name(g->optimizer_cov(), out_str, num_char);
    return 0;
  }
  copy_name(model(handle)->optimizer_cov(), out_str, num_char);
  API_END();
}

int GPB_GetOptimizerCoef(REModelHandle handle, char* out_str, int* num_char) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {   // a Laplace model fitted with covariates: they sat in the L-BFGS vector
    copy_name(g->has_covariates() ? g->optimizer_coef() : "wls", out_str, num_char);
    return 0;
  }
  copy_name(model(handle)->optimizer_coef(), out_str, num_char);
  API_END();
}

int GPB_GetCGPreconditionerType(REModelHandle handle, char* out_str, int* num_char) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    copy_name(g->cg_preconditioner_type(), out_str, num_char);
    return 0;
  }
  copy_name(model(handle)->cg_preconditioner_type(), out_str, num_char);
  API_END();
}

int GPB_GetPivotedCholeskyInfo(REModelHandle handle, double* out, int* pivots) {
  API_BEGIN();
  model(handle)->PivCholInfo(out, pivots);
  API_END();
}

int GPB_GetGroupedLaplaceInfo(REModelHandle handle, int32_t* dims, int32_t* rowptr, int32_t* col, double* diag,
                              double* vals) {
  API_BEGIN();
  GroupedModel* g = as_grouped(handle);
  if (g == nullptr) gpb_amd::Fatal("GPB_GetGroupedLaplaceInfo: the model has no grouped random effects");
  g->GetLaplaceInfo(dims, rowptr, col, diag, vals);
  API_END();
}

int GPB_PivotedCholeskyHost(const double* coords, int n, int d, int cov_type, double var, double phi, int rank,
                            double tol, double* L, int* pivots, int* out_rank) {
  API_BEGIN();
  if (n < 1 || d < 1 || rank < 1 || cov_type < 0 || cov_type > 3) gpb_amd::Fatal("GPB_PivotedCholeskyHost: invalid argument");
  *out_rank = gpb_amd::pivoted_cholesky_host(cov_type, coords, n, d, var, phi, rank, tol, L, pivots);
  API_END();
}

int GPB_TestNewtonLineSearch(int it, double obj, double gdd, double delta, int max_shrink, const double* trial_objs,
                             int n_trials, double* out) {
  API_BEGIN();
  if (it < 0 || max_shrink < 1 || n_trials < 0 || out == nullptr || (n_trials > 0 && trial_objs == nullptr))
    gpb_amd::Fatal("GPB_TestNewtonLineSearch: invalid argument");
  for (int k = 0; k < n_trials; ++k) out[5 + k] = std::numeric_limits<double>::quiet_NaN();
  const gpb_amd::LineSearchResult r =
      gpb_amd::newton_line_search(it, obj, gdd, delta, max_shrink, [&](double lam, int ih) {
        if (ih >= n_trials) gpb_amd::Fatal("GPB_TestNewtonLineSearch: trial %d asked for, %d scripted", ih, n_trials);
        out[5 + ih] = lam;
        return trial_objs[ih];
      });
  out[0] = r.obj_new;
  out[1] = r.lam;
  out[2] = r.trials;
  out[3] = r.terminate ? 1. : 0.;
  out[4] = r.nan ? 1. : 0.;
  API_END();
}

int GPB_TestDenseGemm(int variant, int M, int N, int K, double alpha, const double* A, int64_t a_len, int lda,
                      int transA, const double* B, int64_t b_len, int ldb, int transB, double beta, double* C,
                      int64_t c_len, int ldc, int lower_out, int a_lower, int a_upper, int b_lower, int c_alias_a) {
  API_BEGIN();
  if (a_len < 0 || b_len < 0 || c_len < 0) gpb_amd::Fatal("GPB_TestDenseGemm: negative extent");
  gpb_amd::test_dense_gemm(variant, M, N, K, alpha, A, (long)a_len, lda, transA, B, (long)b_len, ldb, transB, beta, C,
                           (long)c_len, ldc, lower_out, a_lower, a_upper, b_lower, c_alias_a);
  API_END();
}

int GPB_TestDenseGemmSplitK(int variant, int M, int N, int K, const double* A, int64_t a_len, int lda, int transA,
                            const double* B, int64_t b_len, int ldb, int transB, double* C, int64_t c_len, int ldc,
                            int64_t cstride, int nslabs, int target_blocks, int max_chunks, int* out_chunks) {
  API_BEGIN();
  if (a_len < 0 || b_len < 0 || c_len < 0 || cstride < 0) gpb_amd::Fatal("GPB_TestDenseGemmSplitK: negative extent");
  if (out_chunks == nullptr) gpb_amd::Fatal("GPB_TestDenseGemmSplitK: out_chunks is NULL");
  *out_chunks = gpb_amd::test_dense_splitk(variant, M, N, K, A, (long)a_len, lda, transA, B, (long)b_len, ldb, transB,
                                           C, (long)c_len, ldc, (long)cstride, nslabs, target_blocks, max_chunks);
  API_END();
}

int GPB_TestDenseChol(int n, int ld, double* A, double* W, int want_inverse, double* logdet, int* out_info) {
  API_BEGIN();
  if (out_info == nullptr) gpb_amd::Fatal("GPB_TestDenseChol: out_info is NULL");
  *out_info = gpb_amd::test_dense_chol(n, ld, A, W, want_inverse, logdet);
  API_END();
}

int GPB_TestDenseSpdSolveInverse(int n, const double* A, const double* b, double* x, double* diag, double* inv) {
  API_BEGIN();
  gpb_amd::test_dense_spd_solve_inverse(n, A, b, x, diag, inv);
  API_END();
}

int GPB_TestWeightedTallSkinny(int m, int n, int c, const double* A, int64_t a_len, const double* w, const double* U,
                               double* T_out, double* G0_out) {
  API_BEGIN();
  gpb_amd::test_weighted_tall_skinny(m, n, c, A, (long)a_len, w, U, T_out, G0_out);
  API_END();
}

int GPB_TestSparseCholPlan(int n, int m, const int32_t* nbr, int64_t nbr_len, int d, const double* X, int64_t x_len,
                           const int64_t* opts, int t, int mode, int32_t* perm, int32_t* sfirst, int32_t* sparent,
                           int64_t* rptr, int32_t* rows, int64_t rows_cap, int32_t* lvl_ptr, int32_t* lvl_sup,
                           int64_t* stats, int64_t stats_len) {
  API_BEGIN();
  gpb_amd::test_sparse_chol_check_graph("GPB_TestSparseCholPlan", n, m, nbr, nbr_len, d, X, x_len);
  if (perm == nullptr || sfirst == nullptr || sparent == nullptr || rptr == nullptr || lvl_ptr == nullptr ||
      lvl_sup == nullptr || stats == nullptr)
    gpb_amd::Fatal("GPB_TestSparseCholPlan: an output is NULL");
  if (stats_len != gpb_amd::kTestCholStats)
    gpb_amd::Fatal("GPB_TestSparseCholPlan: stats holds %lld entries, not %d", (long long)stats_len, gpb_amd::kTestCholStats);
  gpb_amd::test_sparse_chol_plan(n, m, nbr, d, X, gpb_amd::test_sparse_chol_options(opts), t, mode, perm, sfirst, sparent,
                                 rptr, rows, rows_cap, lvl_ptr, lvl_sup, stats);
  API_END();
}

static gpb_amd::TestSparseChol* test_chol(void* handle, const char* fn) {
  if (handle == nullptr) gpb_amd::Fatal("%s: handle is NULL", fn);
  return static_cast<gpb_amd::TestSparseChol*>(handle);
}

int GPB_TestSparseCholCreate(int n, int m, const int32_t* nbr, int64_t nbr_len, int d, const double* X, int64_t x_len,
                             const int64_t* opts, void** out) {
  API_BEGIN();
  gpb_amd::test_sparse_chol_check_graph("GPB_TestSparseCholCreate", n, m, nbr, nbr_len, d, X, x_len);
  if (out == nullptr) gpb_amd::Fatal("GPB_TestSparseCholCreate: out is NULL");
  *out = new gpb_amd::TestSparseChol(n, m, nbr, d, X, gpb_amd::test_sparse_chol_options(opts));
  API_END();
}

int GPB_TestSparseCholFree(void* handle) {
  API_BEGIN();
  delete static_cast<gpb_amd::TestSparseChol*>(handle);
  API_END();
}

int GPB_TestSparseCholSetB(void* handle, const double* Bv, int64_t bv_len, const double* Dinv, int64_t dinv_len,
                           const double* dBv, int64_t dbv_len, const double* dD, int64_t dd_len) {
  API_BEGIN();
  const char* fn = "GPB_TestSparseCholSetB";
  gpb_amd::TestSparseChol* c = test_chol(handle, fn);
  const int64_t nm = (int64_t)c->n() * c->m(), n = c->n();
  if (Bv == nullptr || Dinv == nullptr || bv_len != nm || dinv_len != n)
    gpb_amd::Fatal("%s: Bv / Dinv hold %lld / %lld entries, n m = %lld, n = %lld", fn, (long long)bv_len,
                   (long long)dinv_len, (long long)nm, (long long)n);
  if ((dBv == nullptr) != (dD == nullptr)) gpb_amd::Fatal("%s: dBv and dD go together", fn);
  if (dBv != nullptr && (dbv_len != nm || dd_len != n))
    gpb_amd::Fatal("%s: dBv / dD hold %lld / %lld entries, n m = %lld, n = %lld", fn, (long long)dbv_len, (long long)dd_len,
                   (long long)nm, (long long)n);
  c->SetB(Bv, Dinv, dBv, dD);
  API_END();
}

int GPB_TestSparseCholFactor(void* handle, const double* W, int64_t w_len, int* out_info, double* logdet) {
  API_BEGIN();
  const char* fn = "GPB_TestSparseCholFactor";
  gpb_amd::TestSparseChol* c = test_chol(handle, fn);
  if (out_info == nullptr) gpb_amd::Fatal("%s: out_info is NULL", fn);
  if (W != nullptr && w_len != c->n()) gpb_amd::Fatal("%s: W holds %lld entries, n = %d", fn, (long long)w_len, c->n());
  *out_info = c->Factor(W, logdet);
  API_END();
}

int GPB_TestSparseCholSolve(void* handle, int op, int nrhs, int inplace, const double* b, int64_t b_len, double* x,
                            int64_t x_len) {
  API_BEGIN();
  const char* fn = "GPB_TestSparseCholSolve";
  gpb_amd::TestSparseChol* c = test_chol(handle, fn);
  if (op < 0 || op > 3 || nrhs < 1 || (op == 0 && nrhs != 1)) gpb_amd::Fatal("%s: op = %d, nrhs = %d", fn, op, nrhs);
  const int64_t len = (int64_t)c->n() * nrhs;
  if (b == nullptr || x == nullptr || b_len != len || x_len != len)
    gpb_amd::Fatal("%s: b / x hold %lld / %lld entries, n nrhs = %lld", fn, (long long)b_len, (long long)x_len,
                   (long long)len);
  c->Solve(op, nrhs, inplace, b, x);
  API_END();
}

int GPB_TestSparseCholSelectedInverse(void* handle, double* tr_bdb, double* tr_da, double* diagS, int64_t diag_len) {
  API_BEGIN();
  const char* fn = "GPB_TestSparseCholSelectedInverse";
  gpb_amd::TestSparseChol* c = test_chol(handle, fn);
  if (diagS != nullptr && diag_len != c->n())
    gpb_amd::Fatal("%s: diagS holds %lld entries, n = %d", fn, (long long)diag_len, c->n());
  c->SelectedInverse(tr_bdb, tr_da, diagS);
  API_END();
}

int GPB_TestSparseCholDense(void* handle, int which, double* out, int64_t out_len) {
  API_BEGIN();
  const char* fn = "GPB_TestSparseCholDense";
  gpb_amd::TestSparseChol* c = test_chol(handle, fn);
  if (which < 0 || which > 2) gpb_amd::Fatal("%s: which = %d", fn, which);
  if (out == nullptr || out_len != (int64_t)c->n() * c->n())
    gpb_amd::Fatal("%s: out holds %lld entries, n n = %lld", fn, (long long)out_len, (long long)c->n() * c->n());
  c->Dense(which, out);
  API_END();
}

static gpb_amd::TestLatentOps* test_latent(void* handle, const char* fn) {
  if (handle == nullptr) gpb_amd::Fatal("%s: handle is NULL", fn);
  return static_cast<gpb_amd::TestLatentOps*>(handle);
}

int GPB_TestLatentOpsCreate(int n, int m, const int32_t* nbr, int64_t nbr_len, int d, const double* X, int64_t x_len,
                            const int64_t* opts, void** out) {
  API_BEGIN();
  const char* fn = "GPB_TestLatentOpsCreate";
  gpb_amd::test_latent_check_graph(fn, n, m, nbr, nbr_len, d, X, x_len);
  if (out == nullptr) gpb_amd::Fatal("%s: out is NULL", fn);
  const gpb_amd::LatentOptions o = gpb_amd::test_latent_options(fn, opts, n);
  *out = new gpb_amd::TestLatentOps(n, m, nbr, d, X, o);
  API_END();
}

int GPB_TestLatentOpsFree(void* handle) {
  API_BEGIN();
  delete static_cast<gpb_amd::TestLatentOps*>(handle);
  API_END();
}

int GPB_TestLatentOpsSetValues(void* handle, const double* Bv, int64_t bv_len, const double* Dinv, const double* W,
                               const double* dw, int64_t vec_len, const double* alt_vals, int64_t alt_len) {
  API_BEGIN();
  const char* fn = "GPB_TestLatentOpsSetValues";
  gpb_amd::TestLatentOps* c = test_latent(handle, fn);
  const int64_t nm = (int64_t)c->n() * c->m(), n = c->n();
  if (Bv == nullptr || Dinv == nullptr || W == nullptr || dw == nullptr) gpb_amd::Fatal("%s: an input is NULL", fn);
  if (bv_len != nm || vec_len != n || (alt_vals != nullptr && alt_len != nm))
    gpb_amd::Fatal("%s: Bv / vectors / alt_vals hold %lld / %lld / %lld entries, n m = %lld, n = %lld", fn,
                   (long long)bv_len, (long long)vec_len, (long long)alt_len, (long long)nm, (long long)n);
  c->lv().TestSetValues(Bv, Dinv, W, dw, alt_vals);
  API_END();
}

int GPB_TestLatentOpsInfo(void* handle, int64_t* stats, int64_t stats_len, int32_t* vo, int64_t vo_len) {
  API_BEGIN();
  const char* fn = "GPB_TestLatentOpsInfo";
  gpb_amd::TestLatentOps* c = test_latent(handle, fn);
  if (stats == nullptr || stats_len != gpb_amd::kTestLatentStats)
    gpb_amd::Fatal("%s: stats holds %lld entries, not %d", fn, (long long)stats_len, gpb_amd::kTestLatentStats);
  if (vo != nullptr && vo_len != c->n()) gpb_amd::Fatal("%s: vo holds %lld entries, n = %d", fn, (long long)vo_len, c->n());
  c->lv().TestInfo(stats, vo);
  API_END();
}

int GPB_TestLatentOpsApply(void* handle, int op, int form, int t, int unit, int use_alt_vals, const double* X,
                           const double* pre, const double* scale, const double* W, int64_t vec_len, const double* H,
                           double* Y, double* Y2, int64_t block_len, int* guard_flag) {
  API_BEGIN();
  const char* fn = "GPB_TestLatentOpsApply";
  gpb_amd::TestLatentOps* c = test_latent(handle, fn);
  if (t < 1 || t > 1024) gpb_amd::Fatal("%s: t = %d", fn, t);
  if (block_len != (int64_t)c->n() * t)
    gpb_amd::Fatal("%s: the blocks hold %lld entries, n t = %lld", fn, (long long)block_len, (long long)c->n() * t);
  if ((pre != nullptr || scale != nullptr || W != nullptr) && vec_len != c->n())
    gpb_amd::Fatal("%s: the vectors hold %lld entries, n = %d", fn, (long long)vec_len, c->n());
  c->lv().TestApply(op, form, t, unit, use_alt_vals, X, pre, scale, W, H, Y, Y2, guard_flag);
  API_END();
}

int GPB_TestLatentOpsVector(int op, int n, int t, int np, int ia, int ib, double alpha, double beta,
                            const double* const* blocks, int64_t block_len, const double* sv0, const double* sv1,
                            const int32_t* act, int64_t small_len, double* out0, double* out1, double* small_out,
                            int64_t small_out_len, int* guard_flag) {
  API_BEGIN();
  const char* fn = "GPB_TestLatentOpsVector";
  if (n < 1 || t < 1 || t > 1024) gpb_amd::Fatal("%s: n = %d, t = %d", fn, n, t);
  if (block_len != (int64_t)n * t) gpb_amd::Fatal("%s: the blocks hold %lld entries, n t = %lld", fn, (long long)block_len, (long long)n * t);
  if ((sv0 != nullptr || sv1 != nullptr || act != nullptr) && small_len != t)
    gpb_amd::Fatal("%s: the column vectors hold %lld entries, t = %d", fn, (long long)small_len, t);
  const int64_t so = op == gpb_amd::kVecColdots ? (int64_t)np * t : op == gpb_amd::kVecCgUpdate ? t
                     : op == gpb_amd::kVecAlpha ? 2 * t : op == gpb_amd::kVecBeta ? 3 * t : 0;
  if (small_out != nullptr && small_out_len != so)
    gpb_amd::Fatal("%s: small_out holds %lld entries, op %d writes %lld", fn, (long long)small_out_len, op, (long long)so);
  gpb_amd::test_latent_vector(op, n, t, np, ia, ib, alpha, beta, blocks, sv0, sv1, act, out0, out1, small_out, guard_flag);
  API_END();
}

int GPB_TestLatentOpsPcg(void* handle, int t, int n_single, double delta, int pmax_single, int pmax_block,
                         const double* RHS, double* U, int64_t block_len, int* its, int* flags) {
  API_BEGIN();
  const char* fn = "GPB_TestLatentOpsPcg";
  gpb_amd::TestLatentOps* c = test_latent(handle, fn);
  if (t < 1 || t > 1024) gpb_amd::Fatal("%s: t = %d", fn, t);
  if (block_len != (int64_t)c->n() * t)
    gpb_amd::Fatal("%s: the blocks hold %lld entries, n t = %lld", fn, (long long)block_len, (long long)c->n() * t);
  c->lv().TestPcg(t, n_single, delta, pmax_single, pmax_block, RHS, U, its, flags);
  API_END();
}

int GPB_TestVifRows(int n_total, int d, int i0, int nn, int m, const double* X, int64_t x_len, const int32_t* nbr,
                    int64_t nbr_len, const double* V, const double* P0, const double* P1, int64_t mat_len, int cov_type,
                    double var, double phi, double nugget, double cjit, int grad, int form, int order, double pad_fill,
                    double* D, double* Bv, double* dD0, double* dD1, double* dBv0, double* dBv1, int64_t rows_len,
                    int* guard_flag) {
  API_BEGIN();
  const gpb_amd::VifRowsTest t{n_total, d,   i0,     nn,   m,    X,     nbr,      V, P0, P1,  cov_type, var,
                               phi,     nugget, cjit, grad, form, order, pad_fill, D, Bv, dD0, dD1,      dBv0, dBv1};
  gpb_amd::test_vif_rows(t, x_len, nbr_len, mat_len, rows_len, guard_flag);
  API_END();
}

int GPB_TestVifApply(int op, int n, int nn, int m, const int32_t* nbr, int64_t nbr_len, const double* coef,
                     int64_t coef_len, const double* D, const double* in, int64_t in_len, double self, int div,
                     int want_div, const double* X, int d, int order, double pad_fill, double* out, double* out2,
                     int64_t out_len, int* guard_flag) {
  API_BEGIN();
  gpb_amd::test_vif_apply(op, n, nn, m, nbr, nbr_len, coef, coef_len, D, in, in_len, self, div, want_div, X, d, order,
                          pad_fill, out, out2, out_len, guard_flag);
  API_END();
}

int GPB_TestVifVector(int op, int n, int m, int d, int cov_type, double var, double phi, double pad_fill,
                      const double* const* arrays, const int64_t* lens, int n_arrays, const int32_t* sum_ops, int nt,
                      double* out, int64_t out_len, int* guard_flag) {
  API_BEGIN();
  gpb_amd::test_vif_vector(op, n, m, d, cov_type, var, phi, pad_fill, arrays, lens, n_arrays, sum_ops, nt, out, out_len,
                           guard_flag);
  API_END();
}

int GPB_TestFitcVector(int op, int n, int m, int d, int cov_type, double var, double phi, double extra, double pad_fill,
                       const double* const* arrays, const int64_t* lens, int n_arrays, const int32_t* ints,
                       int64_t ints_len, double* const* outs, const int64_t* out_lens, int n_outs, int* guard_flag) {
  API_BEGIN();
  gpb_amd::test_fitc_vector(op, n, m, d, cov_type, var, phi, extra, pad_fill, arrays, lens, n_arrays, ints, ints_len,
                            outs, out_lens, n_outs, guard_flag);
  API_END();
}

int GPB_TestFitcKmeans(int op, int n, int k, int d, const double* X, int64_t x_len, const double* mu, const double* mu_a,
                       const double* mu_b, int64_t mu_len, const int32_t* cluster_in, int64_t cluster_len, int scan,
                       int max_it, double* mu_out, int32_t* ints_out, int64_t ints_len, int* its, int* guard_flag) {
  API_BEGIN();
  gpb_amd::test_fitc_kmeans(op, n, k, d, X, x_len, mu, mu_a, mu_b, mu_len, cluster_in, cluster_len, scan, max_it, mu_out,
                            ints_out, ints_len, its, guard_flag);
  API_END();
}

int GPB_TestFitcStages(int stage, int n, int m, int d, int cov_type, double var, double phi, double var2, double phi2,
                       const double* X, const double* Z, const double* y, int np, const double* Xp, const int32_t* match,
                       double* const* outs, const int64_t* out_lens, int n_outs) {
  API_BEGIN();
  gpb_amd::test_fitc_stages(stage, n, m, d, cov_type, var, phi, var2, phi2, X, Z, y, np, Xp, match, outs, out_lens,
                            n_outs);
  API_END();
}

int GPB_TestDenseBatch(int cov_type, int C, int d, const int32_t* ptr, int64_t ptr_len, const double* X, int64_t x_len,
                       const double* y, int64_t y_len, double var, double phi, int want_grad, double* sums,
                       int64_t sums_len, double* u, int64_t u_len, int32_t* info, int64_t info_len) {
  API_BEGIN();
  gpb_amd::test_dense_batch(cov_type, C, d, ptr, ptr_len, X, x_len, y, y_len, var, phi, want_grad, sums, sums_len, u,
                            u_len, info, info_len);
  API_END();
}

int GPB_GetClusterInfo(REModelHandle handle, int32_t* out) {
  API_BEGIN();
  if (out == nullptr) gpb_amd::Fatal("out is NULL");
  model(handle)->GetClusterInfo(out);
  API_END();
}

int GPB_TestLikPoint(int lik, double aux, int n, const double* y, const double* loc, double* loglik, double* d1,
                     double* info, double* dinfo, double* dinfo_lowrank, int* guard_flag) {
  API_BEGIN();
  gpb_amd::test_lik_point(lik, aux, n, y, loc, loglik, d1, info, dinfo, dinfo_lowrank, guard_flag);
  API_END();
}

int GPB_TestLikAuxPoint(int lik, double aux, int n, const double* y, const double* loc, double* dd1_aux,
                        double* dinfo_aux, double* aux_term, int* guard_flag) {
  API_BEGIN();
  gpb_amd::test_lik_aux_point(lik, aux, n, y, loc, dd1_aux, dinfo_aux, aux_term, guard_flag);
  API_END();
}

int GPB_TestLikPath(int path, int kernel, int n, int lik, double aux, const double* y, const double* mode,
                    const double* offset, const double* const* vecs, int n_vecs, const int32_t* idx, int64_t idx_len,
                    const double* arr0, const double* arr1, int64_t arr_len, const double* mats, int64_t mats_len,
                    double lam, const int32_t* opts, int n_opts, double* const* outs, int n_outs, double* scalars,
                    int n_scalars, int* guard_flag) {
  API_BEGIN();
  const gpb_amd::LikPathTest t{path, kernel, n,       lik,  aux,      y,   mode, offset, vecs,   n_vecs, idx,     idx_len,
                               arr0, arr1,   arr_len, mats, mats_len, lam, opts, n_opts, outs,   n_outs, scalars, n_scalars};
  gpb_amd::test_lik_path(t, guard_flag);
  API_END();
}

int GPB_TestGroupedCreate(int n, int K, const int32_t* levels, int64_t levels_len, void** out) {
  API_BEGIN();
  const char* fn = "GPB_TestGroupedCreate";
  if (out == nullptr || levels == nullptr) gpb_amd::Fatal("%s: levels or out is NULL", fn);
  if (n < 1 || n > (1 << 22) || K < 1 || K > 16) gpb_amd::Fatal("%s: n = %d, K = %d", fn, n, K);
  if (levels_len != (int64_t)n * K)
    gpb_amd::Fatal("%s: levels holds %lld entries, not K n = %lld", fn, (long long)levels_len, (long long)n * K);
  for (int64_t e = 0; e < levels_len; ++e)
    if (levels[e] < 0 || levels[e] >= n) gpb_amd::Fatal("%s: levels[%lld] = %d is not in 0..n-1", fn, (long long)e, levels[e]);
  *out = new gpb_amd::GroupedTest(n, K, levels);
  API_END();
}

int GPB_TestGroupedCreateWeighted(int n, int K, const int32_t* levels, int64_t levels_len, const double* weights,
                                  int64_t weights_len, const int32_t* has_weight, void** out) {
  API_BEGIN();
  const char* fn = "GPB_TestGroupedCreateWeighted";
  if (out == nullptr || levels == nullptr || weights == nullptr || has_weight == nullptr)
    gpb_amd::Fatal("%s: levels, weights, has_weight or out is NULL", fn);
  if (n < 1 || n > (1 << 22) || K < 1 || K > 16) gpb_amd::Fatal("%s: n = %d, K = %d", fn, n, K);
  if (levels_len != (int64_t)n * K || weights_len != (int64_t)n * K)
    gpb_amd::Fatal("%s: levels / weights hold %lld / %lld entries, not K n = %lld", fn, (long long)levels_len,
                   (long long)weights_len, (long long)n * K);
  for (int64_t e = 0; e < levels_len; ++e)
    if (levels[e] < 0 || levels[e] >= n) gpb_amd::Fatal("%s: levels[%lld] = %d is not in 0..n-1", fn, (long long)e, levels[e]);
  bool any = false;
  for (int k = 0; k < K; ++k) {
    if (has_weight[k] == 0) continue;
    any = true;
    for (int i = 0; i < n; ++i)
      if (!std::isfinite(weights[(size_t)k * n + i])) gpb_amd::Fatal("%s: weights[%d, %d] is not finite", fn, k, i);
  }
  *out = new gpb_amd::GroupedTest(n, K, levels, any ? weights : nullptr, has_weight);
  API_END();
}

static gpb_amd::GroupedTest* grouped_test(void* handle, const char* fn) {
  if (handle == nullptr) gpb_amd::Fatal("%s: handle is NULL", fn);
  return static_cast<gpb_amd::GroupedTest*>(handle);
}

int GPB_TestGroupedFree(void* handle) {
  API_BEGIN();
  delete static_cast<gpb_amd::GroupedTest*>(handle);
  API_END();
}

int GPB_TestGroupedInfo(void* handle, int t, int64_t* stats, int64_t stats_len, int32_t* ints, int64_t ints_len,
                        double* dbls, int64_t dbls_len) {
  API_BEGIN();
  grouped_test(handle, "GPB_TestGroupedInfo")->Info(t, stats, stats_len, ints, ints_len, dbls, dbls_len);
  API_END();
}

int GPB_TestGroupedApply(void* handle, int op, int t, const double* val, const double* dg_or_D, const double* dis,
                         const double* In, double* Out0, double* Out1, int64_t block_len, int* guard_flag) {
  API_BEGIN();
  grouped_test(handle, "GPB_TestGroupedApply")->Apply(op, t, val, dg_or_D, dis, In, Out0, Out1, block_len, guard_flag);
  API_END();
}

int GPB_TestGroupedSmall(void* handle, int op, const double* const* in, const int64_t* in_len, int n_in,
                         double* const* out, const int64_t* out_len, int n_out, int* guard_flag) {
  API_BEGIN();
  grouped_test(handle, "GPB_TestGroupedSmall")->Small(op, in, in_len, n_in, out, out_len, n_out, guard_flag);
  API_END();
}

int GPB_TestGroupedDense(void* handle, int op, int ld, int np, const int32_t* idx, const double* const* in,
                         const int64_t* in_len, int n_in, double* const* out, const int64_t* out_len, int n_out,
                         int* guard_flag) {
  API_BEGIN();
  grouped_test(handle, "GPB_TestGroupedDense")->Dense(op, ld, np, idx, in, in_len, n_in, out, out_len, n_out, guard_flag);
  API_END();
}

int GPB_TestGroupedSolve(void* handle, const double* val, const double* cnt, const double* D, const double* dis,
                         const double* rhs, int warm, const double* u0, int pmax, double delta, double* u, int* its,
                         int* guard_flag) {
  API_BEGIN();
  grouped_test(handle, "GPB_TestGroupedSolve")->Solve(val, cnt, D, dis, rhs, warm, u0, pmax, delta, u, its, guard_flag);
  API_END();
}

int GPB_TestGroupedLaplaceOps(void* handle, int op, int sub, int t, int ld, double alpha, const double* const* in,
                              const int64_t* in_len, int n_in, double* const* out, const int64_t* out_len, int n_out,
                              int* guard_flag) {
  API_BEGIN();
  grouped_test(handle, "GPB_TestGroupedLaplaceOps")
      ->LaplaceOps(op, sub, t, ld, alpha, in, in_len, n_in, out, out_len, n_out, guard_flag);
  API_END();
}

int GPB_GetVifFactor(REModelHandle handle, const double* cov_pars, int32_t* perm, int32_t* neighbors, double* D,
                     double* B_vals, double* dD, double* dB_vals) {
  API_BEGIN();
  if (cov_pars == nullptr || D == nullptr || B_vals == nullptr || dD == nullptr || dB_vals == nullptr)
    gpb_amd::Fatal("GPB_GetVifFactor: an argument is NULL");
  model(handle)->GetVifFactor(cov_pars, perm, neighbors, D, B_vals, dD, dB_vals);
  API_END();
}

int GPB_GetNumCGSteps(REModelHandle handle, int* num_cg_steps) {
  // re_model_template.h:527-537: defined for models of several grouped random effects only
  API_BEGIN();
  GroupedModel* g = as_grouped(handle);
  if (g == nullptr) (void)model(handle);
  if (g == nullptr || !g->iterative())
    gpb_amd::Fatal("GetNumCGStepLast: this function is currently only implemented when having multiple grouped random "
                   "effects and iterative methods are used ");
  num_cg_steps[0] = g->num_cg_steps();
  API_END();
}

int GPB_GetNumCGStepsTridiag(REModelHandle handle, int* num_cg_steps) {
  API_BEGIN();   // re_model_template.h:542-552
  GroupedModel* g = as_grouped(handle);
  if (g == nullptr) (void)model(handle);
  if (g == nullptr || !g->iterative())
    gpb_amd::Fatal("GetNumCGStepLast: this function is currently only implemented when having multiple grouped random "
                   "effects and iterative methods are used ");
  num_cg_steps[0] = g->num_cg_steps_tridiag();
  API_END();
}

int GPB_SetLikelihood(REModelHandle handle, const char* likelihood) {
  API_BEGIN();
  if (likelihood == nullptr) gpb_amd::Fatal("likelihood is NULL");
  if (GroupedModel* g = as_grouped(handle)) {
    if (std::string(likelihood) != g->likelihood())
      gpb_amd::Fatal("changing the likelihood of a grouped random effects model ('%s' to '%s') is not supported by "
                     "gpboost_amd (create a new model)", g->likelihood().c_str(), likelihood);
    return 0;
  }
  model(handle)->SetLikelihood(std::string(likelihood));
  API_END();
}

int GPB_GetResponseData(REModelHandle handle, double* response_data) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    g->GetResponseData(response_data);
    return 0;
  }
  model(handle)->GetResponseData(response_data);
  API_END();
}

int GPB_GetCovariateData(REModelHandle handle, double* covariate_data) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    g->GetCovariateData(covariate_data);
    return 0;
  }
  model(handle)->GetCovariateData(covariate_data);
  API_END();
}

int GPB_GetOffsetData(REModelHandle handle, double* fixed_effects) {
  API_BEGIN();
  model(handle)->GetOffsetData(fixed_effects);
  API_END();
}

int GPB_SetOffsetData(REModelHandle handle, const double* fixed_effects) {
  API_BEGIN();
  model(handle)->SetOffsetData(fixed_effects);
  API_END();
}

int GPB_GetInitAuxPars(REModelHandle handle, double* aux_pars) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    g->GetInitAuxPars(aux_pars);
    return 0;
  }
  model(handle)->GetInitAuxPars(aux_pars);
  API_END();
}

int GPB_GetLikelihoodName(REModelHandle handle, char* out_str, int* num_char) {
  API_BEGIN();
  GroupedModel* g = as_grouped(handle);
  const std::string s = g != nullptr ? g->likelihood() : model(handle)->config().likelihood;
  std::memcpy(out_str, s.c_str(), s.size() + 1);
  num_char[0] = (int)s.size() + 1;
  API_END();
}

int GPB_GetNumAuxPars(REModelHandle handle, int* num_aux_pars) {
  API_BEGIN();
  GroupedModel* g = as_grouped(handle);
  num_aux_pars[0] = g != nullptr ? g->num_aux_pars() : model(handle)->num_aux_pars();
  API_END();
}

int GPB_GetAuxPars(REModelHandle handle, double* aux_pars, char* out_str) {
  API_BEGIN();
  if (GroupedModel* g = as_grouped(handle)) {
    const auto& a = g->aux_pars();
    for (size_t k = 0; k < a.size(); ++k) aux_pars[k] = a[k];
    const std::string name = g->aux_par_name();
    if (out_str != nullptr) std::memcpy(out_str, name.c_str(), name.size() + 1);
    return 0;
  }
  REModelAMD* m = model(handle);
  const auto& a = m->aux_pars();
  for (size_t k = 0; k < a.size(); ++k) aux_pars[k] = a[k];
  const std::string name = m->aux_par_name();
  if (out_str != nullptr) std::memcpy(out_str, name.c_str(), name.size() + 1);
  API_END();
}

int GPB_GetLatentVecchiaFactor(REModelHandle handle, const double* cov_pars, double* D_inv, double* B_vals,
                               double* dD_range, double* dB_range_vals) {
  API_BEGIN();
  model(handle)->GetLatentVecchiaFactor(cov_pars, D_inv, B_vals, dD_range, dB_range_vals);
  API_END();
}

int GPB_GetLastIterationInfo(REModelHandle handle, double* info) {
  API_BEGIN();
  model(handle)->GetLastIterationInfo(info);
  API_END();
}

int GPB_GetCholeskyPlanInfo(REModelHandle handle, double* info) {
  API_BEGIN();
  if (info == nullptr) gpb_amd::Fatal("NULL argument");
  model(handle)->CholeskyPlanInfo(info);
  API_END();
}

int GPB_GetNumCovPars(REModelHandle handle, int* num_cov_pars) {
  API_BEGIN();
  GroupedModel* g = as_grouped(handle);
  num_cov_pars[0] = g != nullptr ? g->num_cov_pars() : model(handle)->num_cov_pars();
  API_END();
}

int GPB_EvalVecchiaPartials(REModelHandle handle, const double* cov_pars, int32_t row_begin, int32_t row_end,
                            double* sums) {
  API_BEGIN();
  model(handle)->EvalVecchiaPartials(cov_pars, row_begin, row_end, sums);
  API_END();
}

int GPB_GetVecchiaStructure(REModelHandle handle, int32_t* perm, int32_t* neighbors) {
  API_BEGIN();
  model(handle)->GetVecchiaStructure(perm, neighbors);
  API_END();
}

int GPB_GetVecchiaFactor(REModelHandle handle, const double* cov_pars, double* D_inv, double* B_vals) {
  API_BEGIN();
  model(handle)->GetVecchiaFactor(cov_pars, D_inv, B_vals);
  API_END();
}

int GPB_GetVecchiaRowsInfo(REModelHandle handle, double* out) {
  API_BEGIN();
  model(handle)->GetVecchiaRowsInfo(out);
  API_END();
}

int GPB_GetLastKernelTimes(REModelHandle handle, double* kernel_ms) {
  API_BEGIN();
  model(handle)->GetLastKernelTimes(kernel_ms);
  API_END();
}

int GPB_GetLastGramTimes(REModelHandle handle, double* gram_ms) {
  API_BEGIN();
  if (gram_ms == nullptr) gpb_amd::Fatal("GPB_GetLastGramTimes: gram_ms is NULL");
  model(handle)->GetLastGramTimes(gram_ms);
  API_END();
}

int GPB_BenchLatentOperators(REModelHandle handle, int t, int reps, double* out) {
  API_BEGIN();
  model(handle)->BenchLatentOperators(t, reps, out);
  API_END();
}

int GPB_CommIdSize(void) { return (int)sizeof(ncclUniqueId); }

int GPB_CommCreateId(char* id_out) {
  API_BEGIN();
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) gpb_amd::Fatal("ncclGetUniqueId failed: %s", ncclGetErrorString(r));
  std::memcpy(id_out, &id, sizeof(id));
  API_END();
}

int GPB_SetDistributed(REModelHandle handle, int rank, int world_size, const char* comm_id) {
  API_BEGIN();
  ncclUniqueId id;
  std::memset(&id, 0, sizeof(id));
  if (world_size > 1 && comm_id == nullptr) gpb_amd::Fatal("comm_id is NULL");
  if (comm_id != nullptr) std::memcpy(&id, comm_id, sizeof(id));
  // a given id joins an RCCL communicator even at world_size 1 (one-rank communicator: the same
  // in-library all-reduce path, which the single-GPU tests exercise)
  model(handle)->SetDistributed(rank, world_size, id, comm_id != nullptr);
  API_END();
}

int GPB_SetDistributedHostReduce(REModelHandle handle, int rank, int world_size,
                                 void (*allreduce)(double* buf, int count, void* user), void* user) {
  API_BEGIN();
  model(handle)->SetDistributedHost(rank, world_size, allreduce, user);
  API_END();
}

int GPB_PartitionRows(int32_t num_data, int world_size, int rank, int32_t* row_begin, int32_t* row_end) {
  API_BEGIN();
  if (world_size < 1 || rank < 0 || rank >= world_size) gpb_amd::Fatal("invalid rank/world_size");
  const int base = num_data / world_size, rem = num_data % world_size;
  row_begin[0] = rank * base + (rank < rem ? rank : rem);
  row_end[0] = row_begin[0] + base + (rank < rem ? 1 : 0);
  API_END();
}

int GPB_CombinePartials(const double* sums, int32_t num_data, double sigma2, int profile_sigma2, double* negll,
                        double* grad, double* sigma2_out) {
  API_BEGIN();
  gpb_amd::combine_partials(sums, num_data, sigma2, profile_sigma2 ? 1 : 0, negll, grad, sigma2_out);
  API_END();
}

}  // extern "C"
