// GroupedModel: the model object behind the GPB_* C ABI for Gaussian models whose random effects
// are K grouped (crossed or nested) effects — the reference's REModelTemplate<sp_mat_rm_t, ...>
// with num_re_group > 0 and no GP (re_model.cpp:21-111, re_model_template.h:95-465). Parameters
// (original scale): [sigma^2 (error variance), sigma_1^2, ..., sigma_K^2]; transformed scale
// [sigma^2, tau_1, ..., tau_K], tau_k = sigma_k^2 / sigma^2 (TransformCovPars). The likelihood runs
// on the device in GroupedRE (grouped.h); this class keeps the configuration, the response and the
// optimizer state.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "coef.h"
#include "grouped.h"
#include "grouped_laplace.h"
#include "optim.h"
#include "re_model.h"

namespace gpb_amd {

// Random slopes (group_rand_coef_data; re_model_template.h:246-273, 6845-6872): R covariates (data column-major
// n x R), slope r on grouping variable ind[r] (counted from 1); drop[k] > 0 (nullable, K entries) removes the
// intercept of grouping variable k, which must have a slope. The model's components are then the K intercepts in
// column order, the R slopes in column order, minus the dropped intercept: component c has the levels of its
// grouping variable, the value z_c[i] of Z (1 or the covariate) and one variance.
struct GroupedSlopes {
  int R = 0;
  const double* data = nullptr;
  const int32_t* ind = nullptr;
  const int* drop = nullptr;
};

class GroupedModel {
 public:
  // levels: K x n level indices (order of first appearance, as RECompGroup numbers its labels,
  // re_comp.h:245-264). matrix_inversion_method: "default" -> "iterative" for K >= 2, "cholesky"
  // for K == 1 (UseIterativeByDefault, re_model_template.h:6719-6724).
  // likelihood other than "gaussian" (bernoulli_logit, bernoulli_probit, poisson, gamma, negative_binomial and its
  // aliases): the Laplace approximation of GroupedLaplace (grouped_laplace.h) for K == 1 and for K >= 2 with
  // "cholesky"; there is no error term then, the parameters are [sigma_1^2 .. sigma_K^2] on both scales, and the
  // shape of gamma / negative_binomial is the auxiliary parameter.
  GroupedModel(int n, const std::vector<std::vector<int>>& levels, const std::string& matrix_inversion_method,
               int seed, std::vector<std::unordered_map<std::string, int>> label_index = {},
               const std::string& likelihood = "gaussian", const GroupedSlopes& slopes = GroupedSlopes());
  // K(): the components (one variance each); num_groups(): the grouping variables (the label columns of
  // re_group_data and re_group_data_pred); num_slopes(): the columns of the slope data
  int num_groups() const { return G_; }
  int num_slopes() const { return (int)slope_data_.size(); }
  bool has_slopes() const { return !slope_data_.empty(); }
  ~GroupedModel();
  // Combined model (re_model_template.h:236-239 allows grouped random effects beside a GP for
  // gp_approx = "none"): one dense GP component on coords (host column-major n x d, as GPB_CreateREModel passes
  // them) with covariance cov_type. Parameters [sigma^2, sigma_1^2 .. sigma_K^2, sigma_gp^2, rho] (the
  // reference's component order: grouped effects first); the likelihood on DenseSolver with the grouped term.
  void AttachGP(int d, const double* coords_colmajor, int cov_type, int seed);
  bool has_gp() const { return dense_ != nullptr; }
  int gp_dim() const { return gp_d_; }

  int n() const { return n_; }
  int K() const { return re_->K(); }
  int num_cov_pars() const { return laplace() ? re_->K() : 1 + re_->K() + (has_gp() ? 2 : 0); }
  bool laplace() const { return lap_ != nullptr; }
  const std::string& likelihood() const { return likelihood_; }
  int num_aux_pars() const { return (int)aux_pars_.size(); }
  const std::vector<double>& aux_pars() const { return aux_pars_; }
  std::string aux_par_name() const { return aux_pars_.empty() ? "" : "shape"; }
  void SetInitAuxPars(const double* aux);
  void GetInitAuxPars(double* aux) const;
  bool estimate_aux_pars = true;
  // GPB_CalcGradientF for non-Gaussian likelihoods (re_model_template.h:3021-3043): the gradient of the
  // Laplace-approximated nll wrt the fixed effects F at the current covariance parameters, written to y.
  // calc_cov_factor = false keeps the mode of the last evaluation. fixed_effects null keeps the offset of the last call
  // that gave y or an offset (the rule of every call without y and offset, Predict included). Laplace models only.
  void CalcGradientF(double* y, const double* fixed_effects, bool calc_cov_factor);
  // test hook (GPB_GetGroupedLaplaceInfo): dims = [M, nnz]; the CSR of the off-diagonal part of Z^T Z and the
  // diagonal / off-diagonal values of Z^T W Z of the last evaluation (each nullable)
  void GetLaplaceInfo(int* dims, int* rowptr, int* col, double* diag, double* vals);
  // the objective of the L-BFGS fit: x = log(sigma_1^2 .. sigma_K^2 [, shape])
  EvalResult EvalLaplace(const double* sigma2, bool want_grad, GroupedLaplace::Start start, bool fatal_on_nan,
                         double* grad_f = nullptr);
  void SetAuxPars(const double* aux) { aux_pars_[0] = aux[0]; aux_pars_set_ = true; }
  void ResetLaplaceModeToPrevious() { lap_->ResetModeToPrevious(); }
  const std::string& matrix_inversion_method() const { return mim_; }
  bool iterative() const { return mim_ == "iterative"; }
  std::string cg_preconditioner_type() const { return iterative() ? "ssor" : ""; }
  const std::vector<int>& levels_per_effect() const { return re_->levels_per_effect(); }

  // y - fixed_effects (nullable) is the response; y (nullable: keep) is stored for GetResponseData.
  void SetResponseAndOffset(const double* y, const double* fixed_effects);
  bool HasY() const { return y_set_; }
  void GetResponseData(double* y) const;

  // cov_pars on the original scale. profile: 0 -> gradient wrt log of all 1 + K parameters
  // (include_error_var), 1 -> sigma^2 profiled out, gradient wrt log tau (the L-BFGS unit).
  EvalResult Eval(const double* cov_pars_orig, bool want_grad, int profile);
  EvalResult EvalTrafo(const double* trafo, bool want_grad, int profile, bool fatal_on_nan = true);

  void SetOptimSettings(const double* init_cov_pars, double lr, int max_iter, double delta_rel_conv,
                        const char* optimizer, int m_lbfgs);
  void SetPreconditioner(const char* preconditioner);
  void SetInternalOptimSettings(double acc_rate, bool nesterov, int schedule, int momentum_offset,
                                const char* convergence_criterion) {
    isettings_.acc_rate = acc_rate;
    isettings_.nesterov = nesterov;
    isettings_.schedule = schedule;
    isettings_.momentum_offset = momentum_offset;
    if (convergence_criterion != nullptr && convergence_criterion[0] != '\0')
      isettings_.crit_params = check_convergence_criterion(convergence_criterion);
  }
  // Fisher information of the log transformed parameters (Fisher scoring; cholesky, no GP), row-major
  std::vector<double> FisherTrafo(const double* trafo);
  const std::string& optimizer_cov() const { return optimizer_name_; }
  // OptimCovPar (re_model.cpp:339-401 -> OptimExternal "lbfgs", optim_utils.h:561-706): L-BFGS on
  // log tau with sigma^2 profiled out (EvalLLforLBFGSpp, optim_utils.h:269-313).
  void OptimCovPar(const double* y, const double* fixed_effects);
  // OptimLinRegrCoefCovPar for Laplace models (re_model_template.h:926-1647 with optimizer_cov = optimizer_coef =
  // "lbfgs"): the coefficients of the p covariates X (column-major n x p, p <= 31) join the L-BFGS vector as
  // [log cov pars, beta, log aux pars] (EvalLLforLBFGSpp, optim_utils.h:243-364), on centred and scaled covariates
  // (CoefLayer, coef.h); the offset F + X beta and the gradient X^T grad_F stay on the device.
  void OptimLinRegrCoefCovPar(const double* y, const double* X, int p, const double* fixed_effects);
  bool has_covariates() const { return coef_ != nullptr && !beta_.empty(); }
  int num_covariates() const { return has_covariates() ? coef_->p() : 0; }
  // coefficients on the original scale; calc_std_dev: then their standard deviations by central differences of the
  // coefficient gradient (CalcStdDevCoefNonGaussian, re_model_template.h:9825-9854; K == 1 and cholesky)
  void GetCoef(double* out, bool calc_std_dev);
  void GetCovariateData(double* out) const;
  // mean_add[i] += sum_j X_pred[i, j] beta_j (X_pred column-major n_pred x p)
  void AddLinearPredictor(const double* X_pred, int n_pred, double* mean_add) const;
  // GPB_EvalNegLogLikelihoodGradCoef: one evaluation at the given parameters and coefficients on the unscaled X
  // (column-major n x p), the mode started from zero; grad = [d/dlog cov pars (K), d/dlog aux (if estimated)],
  // grad_coef = X^T grad_F (p). Like GPB_EvalNegLogLikelihood it is an evaluation of the model: y (when given)
  // becomes the stored response, aux (when given) the auxiliary parameters, cov_pars the last evaluated ones. The
  // covariates and coefficients of a fit stay, and the fit's offset F + X beta is put back before the call returns
  // or throws; a model without fitted coefficients is left with the offset fixed_effects + X coef, as after a call
  // that gives fixed_effects.
  double EvalGradCoef(const double* cov_pars, const double* aux, const double* coef, const double* y, const double* X,
                      int p, const double* fixed_effects, double* grad_cov, double* grad_aux, double* grad_coef);
  // NULL or "": the default ("lbfgs" for Laplace models)
  void SetOptimizerCoef(const char* optimizer_coef, bool init_coef_given);
  const std::string& optimizer_coef() const { return optimizer_coef_; }
  void SetCovParIndexGiven(bool given) { cov_par_index_given_ = given; }
  // hooks of the L-BFGS objective: beta on the optimizer's (scaled) scale
  void CoefWriteOffset(const double* beta);
  void CoefGradient(double* grad_beta);
  double CoefMaxLearningRate(const double* beta, const double* dir);
  void SetNumIter(int it) { num_iter_ = it; }
  int num_it() const { return num_it_; }
  double last_nll() const { return last_nll_; }
  const std::vector<double>& last_cov_pars() const { return last_cov_pars_; }
  void GetInitCovPar(double* out) const;
  // GPB_GetNumCGSteps / GetNumCGStepsTridiag (re_model_template.h:527-552)
  int num_cg_steps() const { return last_cg_its_; }
  int num_cg_steps_tridiag() const { return last_lanczos_; }
  // GPB_PredictREModelTrainingDataRandomEffects (re_model.cpp -> PredictTrainingDataRandomEffects,
  // grouped branch re_model_template.h:4065-4167): out[k n + i] = posterior mean of effect k at
  // observation i's level; calc_var (cholesky only, as the reference's iterative branch refuses it):
  // out[K n + k n + i] = its posterior variance. cov_pars original scale (null: the last ones).
  // With random slopes: one block per component; a slope's block holds the slope effect b, not x b.
  void PredictTrainingDataRandomEffects(const double* cov_pars, const double* y, double* out,
                                        const double* fixed_effects, bool calc_var);
  // GPB_PredictREModel with re_group_data_pred (re_model_template.h:3146 -> CalcPred :10026-10535, Woodbury branch): means; with
  // predict_var / predict_cov_mat (cholesky only; iterative: the reference's simulation, refused) the
  // predictive (co)variances nugget [predict_response] + sum_k tau_k [new level, same label] + e_p^T A^-1 e_q,
  // e_p the indicator of p's seen levels (derivation in grouped.h), times sigma^2.
  // Combined models: gp_coords_pred (column-major n_pred x d) required; mean = Sigma_po Psi^-1 y, (co)variances
  // from the dense factor with the grouped cross-covariances (DenseSolver::Predict).
  // Random slopes: slope_data_pred (column-major n_pred x R, required then) gives Z's values z_c(p) of the
  // prediction points: mean = sum_c z_c(p) b_c[level], e_p holds z_c(p), and a new label adds tau_c z_c(p) z_c(q).
  void Predict(const double* y, int n_pred, const char* re_group_data_pred, const double* gp_coords_pred,
               const double* cov_pars, bool predict_cov_mat, bool predict_var, bool predict_response,
               const double* fixed_effects, const double* fixed_effects_pred, double* out,
               const double* slope_data_pred = nullptr);
  // GPB_GetCovPar(calc_std_dev) (CalcStdDevCovPar re_model_template.h:9775-9789 ->
  // CalcFisherInformation_Only_Grouped_REs_Woodbury :9559-9651): sqrt(diag(FI^-1)) at the original-scale
  // cov_pars; cholesky only (the iterative branch is a stochastic estimate: refused)
  void StdDevCovPars(const double* cov_pars, double* sd);
  bool CanCalculateStandardErrorsCovPars() const { return !iterative() && !has_gp() && !laplace(); }
  IterativeConfig iter;

 private:
  void UseDevice() const;
  void FindInitCovPar(const double* y, double* trafo) const;
  // transformed <-> original scale: tau_k = sigma_k^2 / sigma^2, v = sigma_gp^2 / sigma^2, phi = range_trafo(rho)
  void ToTrafo(const double* orig, double* trafo) const;
  void ToOrig(const double* trafo, double sigma2, double* orig) const;
  EvalResult EvalDense(const double* trafo, bool want_grad, int profile, bool fatal_on_nan);
  // the prediction points' level indices (K x n_pred, effect-major; -1 - id for labels not seen in training,
  // equal ids for equal new labels) and the per-effect label strings (nullable)
  void PredictCombined(const double* y, int n_pred, const char* re_group_data_pred, const double* gp_coords_pred,
                       const double* cov_pars, bool predict_cov_mat, bool predict_var, bool predict_response,
                       const double* fixed_effects, const double* fixed_effects_pred, double* out);
  std::vector<int> PredLevels(int n_pred, const char* re_group_data_pred, std::vector<std::vector<std::string>>* labels) const;
  std::vector<double> Blup(const double* cov_pars, const double* y, const double* fixed_effects,
                           std::vector<double>* var);

  int n_;
  int device_ = 0;
  std::string mim_;
  hipStream_t stream_ = nullptr;
  std::unique_ptr<GroupedRE> re_;
  // non-Gaussian likelihood
  std::unique_ptr<GroupedLaplace> lap_;
  std::string likelihood_ = "gaussian";
  int lik_ = 0;
  std::vector<double> aux_pars_, init_aux_pars_;
  bool aux_pars_set_ = false;
  // with_coef: coef_ holds the covariates of this fit and beta joins the optimizer's vector
  void OptimCovParLaplace(const double* y, const double* fixed_effects, bool with_coef = false);
  // optimizer_cov = "gradient_descent" for Laplace models (with or without Nesterov acceleration; no covariates):
  // start = the initial variances, the auxiliary parameter from aux_pars_
  void GradientDescentLaplace(const std::vector<double>& start, bool with_aux);
  void PredictLaplace(const double* y, int n_pred, const char* re_group_data_pred, const double* cov_pars,
                      bool predict_var, bool predict_response, const double* fixed_effects,
                      const double* fixed_effects_pred, double* out, const double* slope_data_pred);
  // The prediction points per component: idx (np x C, global level index or -1 for a label not in the training
  // data), wt (np x C, Z's values; empty without slopes) and, when asked, fresh (C x np: ids of the new labels,
  // equal for equal labels of one grouping variable, -1 for seen ones)
  void PredComponents(int n_pred, const char* re_group_data_pred, const double* slope_data_pred, std::vector<int>& idx,
                      std::vector<double>& wt, std::vector<std::vector<int>>* fresh) const;
  std::vector<double> LaplaceCovPars(const double* cov_pars) const;
  // linear regression coefficients (Laplace models): the layer of the last fit and its coefficients (original scale)
  std::unique_ptr<CoefLayer> coef_;
  std::vector<double> beta_, fit_offset_;   // fit_offset_: F of the fit (empty: none)
  void RefreshCoefOffset();   // the device offset := F of the fit + X beta
  std::string optimizer_coef_ = "lbfgs";
  bool cov_par_index_given_ = false, init_coef_given_ = false;
  std::vector<std::vector<int>> levels_;                       // C x n, per component
  std::vector<std::unordered_map<std::string, int>> label_index_;   // label -> level, per grouping variable
  int G_ = 0;                                  // grouping variables
  std::vector<int> comp_group_, comp_slope_;   // per component: its grouping variable, its slope column (-1: intercept)
  std::vector<std::vector<double>> slope_data_;   // R x n
  std::vector<double> y_raw_, y_;
  bool y_set_ = false;

  LbfgsSettings optim_;
  InternalSettings isettings_;
  std::string optimizer_name_ = "lbfgs";
  std::vector<double> init_cov_pars_, cov_pars_orig_, init_used_, last_cov_pars_;
  bool cov_pars_initialized_ = false;
  int num_it_ = 0;
  int num_iter_ = 0;   // the reference's num_iter_ (warm starts of the A^-1 Z^T y solve)
  double last_nll_ = 0.;
  int last_cg_its_ = 0, last_lanczos_ = 0;
  // combined GP + grouped (AttachGP)
  std::unique_ptr<DenseSolver> dense_;
  int gp_d_ = 0, cov_type_ = 0, seed_ = 0;
  std::vector<double> coords_;   // row-major n x d
  DevBuf<double> d_X_, d_y_;
  DevBuf<int> d_lev_;            // K x n
};

// Parses re_group_data (column-major K x n NUL-terminated labels, re_model_template.h:6246-6270)
// into level indices numbered in order of first appearance per effect.
// label_index (nullable) receives the per-effect label -> level maps.
std::vector<std::vector<int>> parse_group_levels(int n, int K, const char* re_group_data,
                                                 std::vector<std::unordered_map<std::string, int>>* label_index = nullptr);

}  // namespace gpb_amd
