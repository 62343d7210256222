/*
 * gpboost_amd — MI355X-native GP / mixed-effects likelihood engine.
 * C-ABI drop-in boundary (plain pointers and sizes, no torch or HIP types).
 *
 * Every GPB_* / LGBM_* entry point below has the signature and semantics of the
 * reference GPBoost C API it replaces (cited per function, paths relative to the
 * reference repository), so GPBoost's Python/R packages can bind this library
 * instead of lib_gpboost.so for the REModel likelihood path. Functions marked
 * EXTENSION do not exist in the reference (the reference exposes
 * no gradient entry point); they are additive.
 *
 * Conventions (identical to the reference): every function returns 0 on success
 * and -1 on failure; the failure message is kept in a thread-local buffer that
 * LGBM_GetLastError() returns (include/LightGBM/c_api.h:1798-1810,
 * src/LightGBM/c_api.cpp:54-58). Input arrays are borrowed for the duration of
 * the call and copied; output arrays are caller-allocated. A handle is not
 * thread-safe.
 *
 * All 29 GPB_* functions of the reference (include/LightGBM/c_api.h:1358-1786) are exported with
 * their signatures. Scope of this build: one GP component (num_gp = 1) with
 * cov_fct in {exponential, matern (shape 0.5/1.5/2.5), gaussian}; gp_approx "none" (dense
 * Cholesky) and "vecchia" with likelihood "gaussian" (exact), "vecchia" with "bernoulli_logit" and
 * "vecchia_latent" with "gaussian" (Laplace approximation, iterative methods); linear regression
 * covariates for the Gaussian likelihood (GLS, optimizer_coef "wls"); OR grouped random effects
 * (num_gp = 0, re_group_data with num_re_group >= 1 grouping variables, Gaussian likelihood; K = 1
 * closed form, K >= 2 iterative SSOR-PCG + SLQ as the reference's default). Grouped handles also accept
 * likelihood "bernoulli_logit", "bernoulli_probit", "poisson" and "gamma" (Laplace approximation on
 * A = Sigma^-1 + Z^T W Z: K = 1 closed form per level, K >= 2 "iterative" (the default: SSOR-PCG Newton solves,
 * SLQ, stochastic traces; cg_* / num_rand_vec_trace / seed_rand_vec_trace / reuse_rand_vec_trace honoured) or
 * "cholesky" (dense factor). Such a model has no error term: cov_pars =
 * [sigma_1^2 .. sigma_K^2]; gamma's shape is its auxiliary parameter (init_aux_pars / estimate_aux_pars of
 * GPB_SetOptimConfig, GPB_GetAuxPars). GPB_EvalNegLogLikelihood[Grad], GPB_OptimCovPar (optimizer "lbfgs"),
 * GPB_CalcGradientF, GPB_PredictREModel (latent and response means and variances, unseen labels) and
 * GPB_PredictREModelTrainingDataRandomEffects (means) serve them; fixed_effects is the offset of the location
 * parameter. Refused: a GP beside the grouped effects, profile_sigma2, standard deviations of the covariance
 * parameters, predictive covariance matrices, predictive variances with "iterative", GPB_OptimCovParBoosting. Latent models accept
 * repeated coordinates (the reference's unique-location form). Anything else fails with -1 and a
 * message naming the unsupported option.
 * The compute path is HIP on gfx950; there is no CPU fallback: if no GPU is
 * visible, GPB_CreateREModel fails.
 */
#ifndef GPBOOST_AMD_H_
#define GPBOOST_AMD_H_

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPBOOST_AMD_EXPORT __attribute__((visibility("default")))

typedef void* REModelHandle;

/* ---------------------------------------------------------------- errors / logging */

/* replaces LGBM_GetLastError (include/LightGBM/c_api.h:54; c_api.cpp:1008) */
GPBOOST_AMD_EXPORT const char* LGBM_GetLastError(void);

/* replaces LGBM_RegisterLogCallback (include/LightGBM/c_api.h:61; c_api.cpp:1012) */
GPBOOST_AMD_EXPORT int LGBM_RegisterLogCallback(void (*callback)(const char*));

/* ---------------------------------------------------------------- model lifecycle */

/* replaces GPB_CreateREModel (include/LightGBM/c_api.h:1358-1390; c_api.cpp:2693-2762).
 * Grouped random slopes: re_group_rand_coef_data is column-major num_data x num_re_group_rand_coef (0: none),
 * ind_effect_group_rand_coef the grouping variable of every slope, counted from 1. The components (one variance
 * each) are the intercepts, then the slopes, minus the intercept dropped by drop_intercept_group_rand_effect
 * (num_re_group entries, nullable; at most one, of a variable that has a slope). Not with gp_coords or several
 * clusters.
 * cluster_ids_data (nullable, num_data) with more than one distinct value: independent realisations of the GP that
 * share the covariance parameters (clusters in order of first appearance, re_model_template.h:6211-6243), for GP
 * models with likelihood "gaussian" and gp_approx "none" or "vecchia"; clusters of at most 64 points are evaluated
 * by one launch of a batched kernel (GPBOOST_AMD_NO_CLUSTER_BATCH=1: one engine per cluster). Such a model refuses,
 * naming the option: other likelihoods and approximations, covariates, optimizer "fisher_scoring", standard
 * deviations of the covariance parameters, GPB_PredictREModelTrainingDataRandomEffects, GPB_OptimCovParBoosting,
 * GPB_CalcGradientF, GPB_SetDistributed*, grouped random effects. One distinct value: the model without ids. */
GPBOOST_AMD_EXPORT int GPB_CreateREModel(int32_t num_data,
    const int32_t* cluster_ids_data,
    const char* re_group_data,
    int32_t num_re_group,
    const double* re_group_rand_coef_data,
    const int32_t* ind_effect_group_rand_coef,
    int32_t num_re_group_rand_coef,
    const int* drop_intercept_group_rand_effect,
    int32_t num_gp,
    const double* gp_coords_data,
    const int dim_gp_coords,
    const double* gp_rand_coef_data,
    int32_t num_gp_rand_coef,
    const char* cov_fct,
    double cov_fct_shape,
    const char* gp_approx,
    double cov_fct_taper_range,
    double cov_fct_taper_shape,
    int num_neighbors,
    const char* vecchia_ordering,
    int num_ind_points,
    double cover_tree_radius,
    const char* ind_points_selection,
    const char* likelihood,
    double likelihood_additional_param,
    const char* matrix_inversion_method,
    int seed,
    int num_parallel_threads,
    bool GPU_use,
    bool has_weights,
    const double* weights,
    double likelihood_learning_rate,
    REModelHandle* out);

/* replaces GPB_REModelFree (include/LightGBM/c_api.h:1397; c_api.cpp:2764-2768) */
GPBOOST_AMD_EXPORT int GPB_REModelFree(REModelHandle handle);

/* replaces GPB_SetOptimConfig (include/LightGBM/c_api.h:1433-1462; c_api.cpp:2770-2830).
 * Stored: the iterative-solver fields (cg_*, num_rand_vec_trace, seed_rand_vec_trace,
 * delta_conv_mode_finding), init_aux_pars / estimate_aux_pars, and the covariance-parameter
 * optimizer fields GPB_OptimCovPar uses: init_cov_pars (original scale), lr (L-BFGS initial
 * step factor, < 0: 1), max_iter, delta_rel_conv (< 0: 1e-6), optimizer (NULL / "" / "lbfgs";
 * others fail), optimizer_coef (NULL / "" / "wls"), m_lbfgs (<= 0: 6). init_coef has no effect:
 * the "wls" update profiles the coefficients out at every evaluation. */
GPBOOST_AMD_EXPORT int GPB_SetOptimConfig(REModelHandle handle,
    double* init_cov_pars,
    double lr,
    double acc_rate_cov,
    int max_iter,
    double delta_rel_conv,
    bool use_nesterov_acc,
    int nesterov_schedule_version,
    bool trace,
    const char* optimizer,
    int momentum_offset,
    const char* convergence_criterion,
    int num_covariates,
    double* init_coef,
    double lr_coef,
    double acc_rate_coef,
    const char* optimizer_coef,
    int cg_max_num_it,
    int cg_max_num_it_tridiag,
    double cg_delta_conv,
    int num_rand_vec_trace,
    bool reuse_rand_vec_trace,
    const char* cg_preconditioner_type,
    int seed_rand_vec_trace,
    int piv_chol_rank,
    double* init_aux_pars,
    bool estimate_aux_pars,
    const int* estimate_cov_par_index,
    int m_lbfgs,
    double delta_conv_mode_finding);

/* ---------------------------------------------------------------- likelihood evaluation */

/* replaces GPB_EvalNegLogLikelihood (include/LightGBM/c_api.h:1500; c_api.cpp:2854-2863).
 * cov_pars on the ORIGINAL scale: (sigma2, sigma1^2, rho) for the Gaussian likelihood,
 * (sigma1^2, rho) for latent models (likelihood "bernoulli_logit", or gp_approx
 * "vecchia_latent" whose error variance is the aux par set by GPB_SetOptimConfig's
 * init_aux_pars); for latent models negll is the Laplace-approximated value computed with
 * iterative methods (PCG + stochastic Lanczos quadrature, likelihoods.h:2765-3076).
 * nll written to negll[0]. y may be NULL to reuse the response set by the previous call. */
GPBOOST_AMD_EXPORT int GPB_EvalNegLogLikelihood(REModelHandle handle,
    const double* y_data,
    double* cov_pars,
    const double* fixed_effects,
    double* negll);

/* EXTENSION. nll and its gradient in one evaluation.
 * profile_sigma2 == 0: gradient with respect to log of every covariance parameter on the
 *   reference's transformed scale (sigma2, sigma1^2/sigma2, range transform), i.e.
 *   REModelTemplate::CalcGradPars(..., include_error_var=true) (re_model_template.h:1748-1818);
 *   grad has num_cov_pars entries.
 * profile_sigma2 == 1: the reference's L-BFGS objective unit
 *   (include/GPBoost/optim_utils.h:243-364): sigma2 is profiled out (yT Psi^-1 y / n),
 *   negll is the profiled nll, grad has num_cov_pars-1 entries (sigma2 excluded), and
 *   sigma2_out (may be NULL) receives the profiled sigma2.
 * Latent models (profile_sigma2 must be 0): gradient of the approximate negative marginal
 *   log-likelihood with respect to log(sigma1^2), log(range transform) and, for
 *   "vecchia_latent" with estimate_aux_pars, log(error variance) — what
 *   CalcGradPars -> CalcGradNegMargLikelihoodLaplaceApproxVecchia returns
 *   (likelihoods.h:4951-5206); grad needs num_cov_pars + num_aux_pars entries.
 * y may be NULL (reuse). */
GPBOOST_AMD_EXPORT int GPB_EvalNegLogLikelihoodGrad(REModelHandle handle,
    const double* y_data,
    const double* cov_pars,
    const double* fixed_effects,
    int profile_sigma2,
    double* negll,
    double* grad,
    double* sigma2_out);

/* replaces GPB_GetCurrentNegLogLikelihood (include/LightGBM/c_api.h:1512) */
GPBOOST_AMD_EXPORT int GPB_GetCurrentNegLogLikelihood(REModelHandle handle, double* negll);

/* replaces GPB_GetCovPar (include/LightGBM/c_api.h:1526; re_model.cpp:767-811): the estimated (or
 * last evaluated) cov_pars on the original scale in cov_par[0, P); calc_std_dev = true also writes
 * their standard deviations to cov_par[P, 2P) — square roots of the diagonal of the inverse Fisher
 * information (CalcStdDevCovPar re_model_template.h:9775-9789), computed on the device for dense
 * Gaussian models (gp_approx "none"); other models fail with a message. */
GPBOOST_AMD_EXPORT int GPB_GetCovPar(REModelHandle handle, double* cov_par, bool calc_std_dev);

/* replaces GPB_GetNumIt (include/LightGBM/c_api.h:1559): iterations of the last GPB_OptimCovPar */
GPBOOST_AMD_EXPORT int GPB_GetNumIt(REModelHandle handle, int* num_it);

/* replaces GPB_GetInitCovPar (include/LightGBM/c_api.h:1537; re_model.cpp:813-834): the initial
 * covariance parameters on the original scale (given by GPB_SetOptimConfig or determined by the
 * last GPB_OptimCovPar), -1 each when there are none yet */
GPBOOST_AMD_EXPORT int GPB_GetInitCovPar(REModelHandle handle, double* init_cov_pars);

/* replaces GPB_OptimCovPar (include/LightGBM/c_api.h:1471; c_api.cpp GPB_OptimCovPar ->
 * re_model.cpp:339-401): estimates the covariance parameters (and, for "vecchia_latent", the
 * error variance aux par) with the reference's default optimizer "lbfgs" (optim_utils.h:561-706:
 * L-BFGS on the log of the transformed parameters, Armijo backtracking, nugget profiled out for
 * the Gaussian likelihood). Initial values: init_cov_pars of GPB_SetOptimConfig, the previous
 * estimate, or the reference's FindInitCovPar heuristic (re_model_template.h:4388-4504). y may be
 * NULL to reuse the response already set; fixed_effects (length n) is an offset (Gaussian:
 * subtracted from y). Results: GPB_GetCovPar, GPB_GetAuxPars, GPB_GetNumIt,
 * GPB_GetCurrentNegLogLikelihood. */
GPBOOST_AMD_EXPORT int GPB_OptimCovPar(REModelHandle handle, const double* y_data, const double* fixed_effects);

/* replaces GPB_GetLikelihoodName (include/LightGBM/c_api.h:1659) */
GPBOOST_AMD_EXPORT int GPB_GetLikelihoodName(REModelHandle handle, char* out_str, int* num_char);

/* replaces GPB_GetNumAuxPars (include/LightGBM/c_api.h:1776) */
GPBOOST_AMD_EXPORT int GPB_GetNumAuxPars(REModelHandle handle, int* num_aux_pars);

/* replaces GPB_GetAuxPars (include/LightGBM/c_api.h:1766; c_api.cpp:3098-3107): aux_pars
 * caller-allocated (num_aux_pars), out_str receives the name of the first parameter. */
GPBOOST_AMD_EXPORT int GPB_GetAuxPars(REModelHandle handle, double* aux_pars, char* out_str);

/* replaces GPB_OptimLinRegrCoefCovPar (include/LightGBM/c_api.h:1485; c_api.cpp:2843-2852 ->
 * re_model.cpp:403-469): covariance parameters by L-BFGS (nugget profiled out) with the linear
 * regression coefficients profiled out by generalised least squares at every objective evaluation
 * (the reference's default optimizer_coef "wls" for the Gaussian likelihood,
 * re_model_template.h:7467-7470, optim_utils.h:297-313). covariate_data column-major
 * num_data x num_covariates (num_covariates + 1 <= 32); fixed_effects: an offset (nullable).
 * Gaussian likelihood only; results through GPB_GetCovPar / GPB_GetCoef. */
GPBOOST_AMD_EXPORT int GPB_OptimLinRegrCoefCovPar(REModelHandle handle,
    const double* y_data,
    const double* covariate_data,
    int num_covariates,
    const double* fixed_effects);

/* replaces GPB_CanCalculateStandardErrorsCovPars (include/LightGBM/c_api.h:1515; c_api.cpp:2873-2879;
 * re_model_template.h:1630-1632): out[0] = 1 for Gaussian-likelihood models, 0 for latent ones. */
GPBOOST_AMD_EXPORT int GPB_CanCalculateStandardErrorsCovPars(REModelHandle handle, int* out);

/* replaces GPB_GetCoef (include/LightGBM/c_api.h:1548; re_model.cpp:836-870): the coefficients
 * estimated by GPB_OptimLinRegrCoefCovPar in optim_coef[0, p); calc_std_dev also writes their
 * standard deviations sqrt(diag((X^T Psi^-1 X / sigma^2)^-1)) to optim_coef[p, 2p)
 * (CalcStdDevCoef, re_model_template.h:9797-9814). */
GPBOOST_AMD_EXPORT int GPB_GetCoef(REModelHandle handle, double* optim_coef, bool calc_std_dev);

/* Grouped random effects with a non-Gaussian likelihood (Laplace): GPB_OptimLinRegrCoefCovPar estimates the
 * coefficients inside the L-BFGS vector [log cov pars, beta, log aux pars] (optimizer_coef "lbfgs",
 * optim_utils.h:243-364) on centred and scaled covariates (num_covariates <= 31); GPB_GetCoef returns them on the
 * original scale, calc_std_dev by central differences of the coefficient gradient (CalcStdDevCoefNonGaussian,
 * re_model_template.h:9825-9854; not for matrix_inversion_method "iterative"). After such a fit
 * GPB_EvalNegLogLikelihood, GPB_CalcGradientF, GPB_PredictREModel (with covariate_data_pred) and
 * GPB_PredictREModelTrainingDataRandomEffects use fixed_effects + X beta as the offset.
 * GPB_GetNumCoef: the number of coefficients of the last fit (0: none), for every handle. */
GPBOOST_AMD_EXPORT int GPB_GetNumCoef(REModelHandle handle, int* num_coef);

/* Extension (grouped random effects, non-Gaussian likelihood): one evaluation of the Laplace-approximated negative
 * log-likelihood at cov_pars (K), aux_pars (NULL: the current ones) and coef (p) on the covariates as given
 * (column-major num_data x p, not scaled), the mode found from zero. grad_cov (K, nullable): d/dlog cov_pars;
 * grad_aux (1, nullable; when auxiliary parameters are estimated): d/dlog aux; grad_coef (p) = X^T grad_F. y_data
 * NULL: the stored response. It is an evaluation of the model like GPB_EvalNegLogLikelihood: y_data, aux_pars and
 * cov_pars given become the model's; the covariates, coefficients and offset of an earlier fit stay. */
GPBOOST_AMD_EXPORT int GPB_EvalNegLogLikelihoodGradCoef(REModelHandle handle, const double* cov_pars,
    const double* aux_pars, const double* coef, const double* y_data, const double* covariate_data,
    int num_covariates, const double* fixed_effects, double* negll, double* grad_cov, double* grad_aux,
    double* grad_coef);

/* replaces GPB_PredictREModelTrainingDataRandomEffects (include/LightGBM/c_api.h:1645;
 * re_model.cpp PredictTrainingDataRandomEffects): cov_pars_pred on the original scale (NULL: the
 * estimated / last evaluated ones), y_obs NULL: the stored response. Gaussian likelihood (dense and
 * Vecchia): out[0, n) = y - Psi^-1 y (minus X beta and the offset first), with calc_var
 * out[n, 2n) = sigma^2 (1 - diag(Psi^-1)); latent models: out[0, n) = the posterior mode
 * (calc_var fails). */
GPBOOST_AMD_EXPORT int GPB_PredictREModelTrainingDataRandomEffects(REModelHandle handle,
    const double* cov_pars_pred,
    const double* y_obs,
    double* out_predict,
    const double* fixed_effects,
    bool calc_var);

/* replace GPB_GetOptimizerCovPars / GPB_GetOptimizerCoef / GPB_GetCGPreconditionerType
 * (include/LightGBM/c_api.h:1670, 1681, 1692; re_model.cpp:174-208): the optimizer names ("" until
 * set or fitted, then "lbfgs" / "wls" for the Gaussian, "lbfgs" for latent models) and the CG
 * preconditioner ("vadu" for latent Vecchia models, "" otherwise). out_str must hold the name;
 * num_char receives its length + 1. */
GPBOOST_AMD_EXPORT int GPB_GetOptimizerCovPars(REModelHandle handle, char* out_str, int* num_char);
GPBOOST_AMD_EXPORT int GPB_GetOptimizerCoef(REModelHandle handle, char* out_str, int* num_char);
GPBOOST_AMD_EXPORT int GPB_GetCGPreconditionerType(REModelHandle handle, char* out_str, int* num_char);

/* replace GPB_GetNumCGSteps / GPB_GetNumCGStepsTridiag (include/LightGBM/c_api.h:1702, 1711): as in
 * the reference (re_model_template.h:527-552) they are defined for models with several grouped
 * random effects only and fail with the reference's message here. */
GPBOOST_AMD_EXPORT int GPB_GetNumCGSteps(REModelHandle handle, int* num_cg_steps);
GPBOOST_AMD_EXPORT int GPB_GetNumCGStepsTridiag(REModelHandle handle, int* num_cg_steps);

/* replaces GPB_SetLikelihood (include/LightGBM/c_api.h:1720; re_model.cpp:142-160): switches between
 * "gaussian" and "bernoulli_logit" before a model is estimated (Vecchia: exact <-> Laplace). */
GPBOOST_AMD_EXPORT int GPB_SetLikelihood(REModelHandle handle, const char* likelihood);

/* replace GPB_GetResponseData / GPB_GetCovariateData / GPB_GetOffsetData / GPB_SetOffsetData
 * (include/LightGBM/c_api.h:1729, 1738, 1747, 1756; re_model_template.h:5762-5825): the stored
 * response (original order, n), covariates (column-major n x p) and offset (n). */
GPBOOST_AMD_EXPORT int GPB_GetResponseData(REModelHandle handle, double* response_data);
GPBOOST_AMD_EXPORT int GPB_GetCovariateData(REModelHandle handle, double* covariate_data);
GPBOOST_AMD_EXPORT int GPB_GetOffsetData(REModelHandle handle, double* fixed_effects);
GPBOOST_AMD_EXPORT int GPB_SetOffsetData(REModelHandle handle, const double* fixed_effects);

/* replaces GPB_GetInitAuxPars (include/LightGBM/c_api.h:1785; re_model.cpp:1226-1238): the aux
 * parameters given by GPB_SetOptimConfig's init_aux_pars, -1 each when none were given. */
GPBOOST_AMD_EXPORT int GPB_GetInitAuxPars(REModelHandle handle, double* aux_pars);

/* EXTENSION (the reference has it as a C++ method only): REModel::OptimCovPar(y, fixed_effects,
 * called_in_GPBoost_algorithm, reuse_learning_rates_from_previous_call) (re_model.cpp:339-401), the
 * covariance update the GPBoost boosting objective runs every boosting round
 * (regression_objective.hpp:164, 178: Gaussian OptimCovPar(F - label, NULL, true, reuse), latent
 * OptimCovPar(NULL, score, true, reuse); reuse = the booster's reuse_learning_rates_gp_model, default
 * true). With called_in_GPBoost_algorithm the offset is not saved for prediction
 * (re_model_template.h:1051); with reuse as well, the L-BFGS inverse-Hessian approximation of the
 * previous call seeds the first direction at step 1 when both calls estimated the covariance
 * parameters (:880-881; LBFGS.h:158-171). GPB_OptimCovPar is this call with both flags false. */
GPBOOST_AMD_EXPORT int GPB_OptimCovParBoosting(REModelHandle handle, const double* y_data, const double* fixed_effects,
    bool called_in_GPBoost_algorithm, bool reuse_learning_rates_from_previous_call);

/* EXTENSION: the inducing points of a gp_approx = "fitc" model (the reference keeps them in
 * REModelTemplate::gp_coords_ip_mat_, chosen by CreateREComponentsFITC_FSA re_model_template.h:6931-7073:
 * kmeans++ GP_utils.cpp:269-295 or random utils.h:323-337). *num_ind_points receives m; ind_points
 * (nullable) receives them row-major m x dim_gp_coords. */
GPBOOST_AMD_EXPORT int GPB_GetInducingPoints(REModelHandle handle, int32_t* num_ind_points, double* ind_points);

/* EXTENSION (the reference has it as a C++ method only): REModel::CalcGradient (re_model.cpp:667-680
 * -> CalcGradientF re_model_template.h:3021-3043), what the GPBoost boosting objective calls after
 * GPB_OptimCovPar(handle, NULL, score) (regression_objective.hpp:164-179): the gradient of the
 * (approximate marginal) negative log-likelihood wrt the fixed effects F at the current covariance
 * parameters, written on y (length n, original order). Gaussian likelihood: input y = F - label,
 * output Psi^-1 y / sigma^2; latent models (Laplace): y is output only and F = fixed_effects, output
 * -dlog p(y|mode+F)/dF + the stochastic implicit-derivative terms (likelihoods.h:5337-5367).
 * calc_cov_factor = false (the booster's call after GPB_OptimCovParBoosting) keeps the Laplace mode
 * of the last evaluation; true re-runs the mode finding from it. */
GPBOOST_AMD_EXPORT int GPB_CalcGradientF(REModelHandle handle, double* y, const double* fixed_effects,
    bool calc_cov_factor);

/* ---------------------------------------------------------------- EXTENSION: introspection */

/* Number of covariance parameters (incl. sigma2) of the model. */
GPBOOST_AMD_EXPORT int GPB_GetNumCovPars(REModelHandle handle, int* num_cov_pars);

/* Vecchia ordering permutation (perm[i] = original index of the i-th point in the
 * Vecchia order) and neighbour lists (n x num_neighbors, -1 padded) exactly as the
 * reference builds them (Vecchia_utils.cpp:1094-1161). Arrays caller-allocated. */
GPBOOST_AMD_EXPORT int GPB_GetVecchiaStructure(REModelHandle handle, int32_t* perm, int32_t* neighbors);

/* Vecchia factor at the given cov_pars (original scale): D^-1 (n, Vecchia order) and
 * B values (n x num_neighbors; B(i, nbr) = -A_i, 0-padded). Computed on the GPU. */
GPBOOST_AMD_EXPORT int GPB_GetVecchiaFactor(REModelHandle handle, const double* cov_pars,
    double* D_inv, double* B_vals);

/* Stored pair distances of the exact Vecchia row kernel (num_neighbors 17..30; built at the first
 * evaluation): out[0] 1 if this model holds them, out[1] their bytes of device memory, out[2] the
 * rows they cover (this rank's), out[3] the milliseconds the one-time distance kernel took. Then the
 * model's last likelihood or partial-sum launch of that kernel: out[4] the problem sets (4 rows) each wave
 * ran, out[5] 1 if the waves took turns at the issue priority (the default), 0 if
 * GPBOOST_AMD_ROWS16_PRIO=0 switched that off. out holds 6 doubles. */
GPBOOST_AMD_EXPORT int GPB_GetVecchiaRowsInfo(REModelHandle handle, double* out);

/* Latent Vecchia factor at cov_pars = (sigma1^2, rho) (latent models): D^-1 (n), B values
 * (n x num_neighbors) and their derivatives with respect to log(range transform)
 * (Vecchia_utils.cpp:1307-1632 with gauss_likelihood = false). Computed on the GPU. */
GPBOOST_AMD_EXPORT int GPB_GetLatentVecchiaFactor(REModelHandle handle, const double* cov_pars,
    double* D_inv, double* B_vals, double* dD_range, double* dB_range_vals);

/* Iterative-method statistics of the last latent evaluation: info[0] Newton iterations,
 * info[1] mode-finding (and gradient) CG iterations, info[2] Lanczos steps of the SLQ
 * block CG, info[3] the estimate of log|Sigma W + I|. */
GPBOOST_AMD_EXPORT int GPB_GetLastIterationInfo(REModelHandle handle, double* info);

/* Latent Vecchia models with matrix_inversion_method = "cholesky" (the sparse Cholesky of Sigma^-1 + W;
 * replaces the reference's SimplicialLLT analyzePattern / factorize, likelihoods.h:2946-2950): statistics of
 * the symbolic plan (built on first use): info[0] supernodes, info[1] levels of the supernodal tree,
 * info[2] entries of L (incl. amalgamation zeros), info[3] doubles of the dense fronts, info[4]
 * factorization flops, info[5] largest front, info[6] widest supernode, info[7] host analysis time (ms),
 * info[8] device time of the last factorization (ms). No reference counterpart (measurement only). */
GPBOOST_AMD_EXPORT int GPB_GetCholeskyPlanInfo(REModelHandle handle, double* info);

/* Timing of the last evaluation's dominant kernel (ms, HIP events on the model's stream),
 * for the benchmark's live roofline. kernel_ms[0] = factor/Cholesky kernel,
 * kernel_ms[1] = whole device-side evaluation. Exact Vecchia models record the events only for
 * evaluations after the first call of this function (they cost ~10 us of host time each);
 * before that it returns zeros. */
GPBOOST_AMD_EXPORT int GPB_GetLastKernelTimes(REModelHandle handle, double* kernel_ms);
/* Measurement only: device time (HIP events, ms) of the last covariate Gram matrix [X | y]^T Psi^-1 [X | y] of
 * a gp_approx = "fitc" / "full_scale_vecchia" model: gram_ms[0] = its factorization (which the evaluation that
 * follows reuses), gram_ms[1] = the whole call. Zeros before the first one. */
GPBOOST_AMD_EXPORT int GPB_GetLastGramTimes(REModelHandle handle, double* gram_ms);

/* Benchmark support (latent Vecchia, iterative): device time of the operator
 * A = B^T D^-1 B + W and of the VADU preconditioner on t columns, on the factor of the last
 * evaluation (HIP events, averaged over reps). out[0] = ms per A application, out[1] = ms
 * per preconditioner application, out[2] = nnz(B) incl. the unit diagonal, out[3] = dependent
 * kernel launches per preconditioner application (level sets of the tail + the head
 * kernels). No reference counterpart (measurement only). */
GPBOOST_AMD_EXPORT int GPB_BenchLatentOperators(REModelHandle handle, int t, int reps, double* out);

/* cg_preconditioner_type = "pivoted_cholesky" (latent Vecchia, iterative): the factorisation of the last
 * evaluation. out[0] = reached rank (0: no such evaluation yet), out[1] = its device time in ms (HIP
 * events); pivots (nullable, >= rank entries): the pivots in Vecchia order. After such an evaluation
 * GPB_BenchLatentOperators times the CG's operator W^-1 + Sigma (out[0]) and the preconditioner
 * (W^-1 + L_k L_k^T)^-1 (out[1]). No reference counterpart (measurement and tests). */
GPBOOST_AMD_EXPORT int GPB_GetPivotedCholeskyInfo(REModelHandle handle, double* out, int* pivots);

/* Grouped random effects with a non-Gaussian likelihood: the structure and the weighted values of
 * A - Sigma^-1 = Z^T W Z of the last evaluation. dims[0] = M (number of random effects), dims[1] = nnz of the
 * off-diagonal part; rowptr (M + 1) and col (nnz): its CSR over the random effects (effect-major, columns
 * ascending); diag (M) and vals (nnz): the values at the mode. Every array is nullable (diag and vals are
 * filled together). No reference counterpart (tests). */
GPBOOST_AMD_EXPORT int GPB_GetGroupedLaplaceInfo(REModelHandle handle, int32_t* dims, int32_t* rowptr, int32_t* col,
                                                 double* diag, double* vals);

/* Host restatement of the reference's PivotedCholsekyFactorizationSigma (CG_utils.h:438-488), the rules
 * the device factorisation follows; needs no GPU. coords: row-major n x d in the order the permutation
 * starts from; cov_type 0 / 1 / 2 Matern 0.5 / 1.5 / 2.5, 3 Gaussian; (var, phi) on the transformed
 * scale. L: row-major n x min(rank, n), pivots: min(rank, n) entries, out_rank: the reached rank. */
GPBOOST_AMD_EXPORT int GPB_PivotedCholeskyHost(const double* coords, int n, int d, int cov_type, double var,
                                               double phi, int rank, double tol, double* L, int* pivots,
                                               int* out_rank);

/* The line search and convergence rule of the Laplace mode finding (likelihoods.h:1910-1928, 11820-11870) as every
 * driver runs it, on a scripted sequence of trial objectives; needs no GPU. it: the Newton iteration, obj: the
 * objective before the step, gdd: the Armijo slope, delta: delta_conv_mode_finding, max_shrink: the number of trials
 * allowed; trial k returns trial_objs[k] (an error when more than n_trials are asked for). out (5 + n_trials):
 * [objective of the last trial, its learning rate, trials used, terminate (0 / 1), NaN or Inf (0 / 1)], then the
 * learning rate passed to each trial (NaN for the trials not run). No reference counterpart (tests). */
GPBOOST_AMD_EXPORT int GPB_TestNewtonLineSearch(int it, double obj, double gdd, double delta, int max_shrink,
                                                const double* trial_objs, int n_trials, double* out);

/* Test hooks of the coefficient layer (coef.h). GPB_TestCoefOps: the three device passes over X (row-major n x p,
 * p <= 31) with host arrays in and out: eta0 (n) = F + X beta (F nullable), g (p) = X^T gF, mom (4) = [sum X dir,
 * sum X beta, sum (X dir)^2, sum (X dir)(X beta)]; each output nullable.
 * GPB_TestCoefHost makes no device call (X column-major n x p): op 0 scaling, out = [intercept column or -1,
 * scaled 0/1, loc (p), scale (p), scaled X row-major (n p)]; 1 / 2 TransformCoef / TransformBackCoef of in (p) to
 * out (p); 3 the initial intercept of likelihood lik (1 bernoulli_logit, 2 bernoulli_probit, 3 poisson, 4 gamma)
 * with in[0] the random effects' total variance; 4 out = [C_mu, C_sigma2]; 5 the step cap from in = [the four sums,
 * C_mu, C_sigma2] over n observations. */
GPBOOST_AMD_EXPORT int GPB_TestCoefOps(int n, int p, const double* X, const double* beta, const double* dir,
    const double* F, const double* gF, double* eta0, double* g, double* mom);
GPBOOST_AMD_EXPORT int GPB_TestCoefHost(int op, int lik, int n, int p, const double* X, const double* y,
    const double* F, const double* in, double* out);

/* The dense fp64 building blocks (C = alpha op(A) op(B) + beta C on MFMA tiles with triangle masks, its
 * split-K form, the blocked Cholesky with the triangular inverse and the log-determinant, the SPD solve /
 * inverse) on host arrays, one call each: column-major, copied to the device and back, synchronised. Extents
 * (*_len, in doubles) are checked against the sizes, transposes and leading dimensions; a violation is an
 * error return. No reference counterpart (tests).
 * GPB_TestDenseGemm: variant 0 = the production dispatch, 1 = unpipelined 64 x 64 tiles, 2 = pipelined 64 x 64
 * tiles, 3 = 128 x 128 tiles, forced at any size. C (c_len >= ldc * N doubles, all copied both ways) is in /
 * out. lower_out: elements above the diagonal are not written; a_lower / a_upper: op(A)[i][k] is taken as 0
 * for k > i / k < i; b_lower: op(B)[k][j] is taken as 0 for k < j (never read). c_alias_a = 1: the product
 * overwrites A on the device (transA = 0, N <= 64, ldc = lda, c_len = a_len) and is returned in C. */
GPBOOST_AMD_EXPORT int GPB_TestDenseGemm(int variant, int M, int N, int K, double alpha, const double* A,
                                         int64_t a_len, int lda, int transA, const double* B, int64_t b_len,
                                         int ldb, int transB, double beta, double* C, int64_t c_len, int ldc,
                                         int lower_out, int a_lower, int a_upper, int b_lower, int c_alias_a);
/* Chunk z of K writes op(A) op(B) over its K range to C + z * cstride (M x N, ldc); C holds nslabs >=
 * max_chunks slabs (c_len = nslabs * cstride, cstride >= ldc * N), all copied both ways. variant 0 = the
 * production tile rule, 1 = 64 x 64 tiles, 2 = 128 x 128 tiles. out_chunks: the number of chunks. */
GPBOOST_AMD_EXPORT int GPB_TestDenseGemmSplitK(int variant, int M, int N, int K, const double* A, int64_t a_len,
                                               int lda, int transA, const double* B, int64_t b_len, int ldb,
                                               int transB, double* C, int64_t c_len, int ldc, int64_t cstride,
                                               int nslabs, int target_blocks, int max_chunks, int* out_chunks);
/* Cholesky of the lower triangle of A (order n, ld x ld doubles, ld a multiple of 64, in / out: L); W (ld x ld,
 * in / out): the inverses of L's 64 x 64 diagonal blocks and, with want_inverse = 1, all of L^-1. logdet
 * (nullable): 2 sum log L_ii. out_info: non-zero exactly when some pivot was not positive and finite (not the
 * number of such pivots: the default kernel adds to it at most once per wave and diagonal block). */
GPBOOST_AMD_EXPORT int GPB_TestDenseChol(int n, int ld, double* A, double* W, int want_inverse, double* logdet,
                                         int* out_info);
/* A: n x n (ld = n). x = A^-1 b (b and x nullable together), diag = diag(A^-1) (nullable), inv = A^-1
 * (n x n, nullable). Fails if A is not positive definite. */
GPBOOST_AMD_EXPORT int GPB_TestDenseSpdSolveInverse(int n, const double* A, const double* b, double* x,
                                                    double* diag, double* inv);
/* The weighted tall-skinny product behind the covariate Gram matrix of gp_approx = "fitc" / "full_scale_vecchia"
 * on host arrays: T_out (m x c row-major) = A diag(w) U and G0_out (c x c row-major) = U^T diag(w) U. A: m x n
 * column-major with leading dimension round_up(m, 64) (a_len doubles, checked); w: n; U: n x c row-major,
 * 1 <= c <= 32. No reference counterpart (tests). */
GPBOOST_AMD_EXPORT int GPB_TestWeightedTallSkinny(int m, int n, int c, const double* A, int64_t a_len,
                                                  const double* w, const double* U, double* T_out, double* G0_out);

/* The sparse multifrontal Cholesky of A = B^T D^-1 B + diag(W) (matrix_inversion_method = "cholesky") on host
 * arrays: its plan alone, and the numeric operations on a small handle. No reference counterpart (tests).
 * Graph: nbr is n x m row-major (row i holds min(i, m) entries, entries < 0 skipped), X the coordinates n x d
 * row-major. Checked on the host before anything else, a violation being an error return: n >= 1,
 * 1 <= m <= 254, d >= 1, nbr_len = n m, x_len = n d, -1 <= nbr[i][r] < i for r < min(i, m), and every other
 * *_len against the size it names.
 * opts (nullable): {leaf, small_panel, fuse_vec, k64, poison}; an entry < 0 keeps the default, which for the
 * first four is what GPBOOST_AMD_CHOL_LEAF / _SMALL_PANEL / _FWDVEC / _K64 give. poison = 1 / 0 fills every
 * device scratch and output buffer a phase (Factor, a solve, SelectedInverse) writes with NaN / zeros before the
 * phase; default: left as they are.
 * GPB_TestSparseCholPlan makes no device call. perm, sparent, lvl_sup: n entries; sfirst, rptr, lvl_ptr: n + 1
 * (nsup + 1, nsup + 1, levels + 1 used); rows (nullable; rows_cap entries, at least stats[5]): the supernodes'
 * row structures. stats (stats_len = 63): nsup, levels, max_fs, max_ns, nnz_l, rptr[nsup], then for the factor,
 * the selected-inverse and the solve schedule of t right-hand sides (mode 0 full, 1 forward only, 2 backward
 * only) 19 entries each: the number of ops of each of the 17 CholOpType values (csrc/sparse_chol.h), the largest
 * nslices of a split-K reduction, the largest chunk count of a kOpBwdVecFin task. */
GPBOOST_AMD_EXPORT int GPB_TestSparseCholPlan(int n, int m, const int32_t* nbr, int64_t nbr_len, int d,
                                              const double* X, int64_t x_len, const int64_t* opts, int t, int mode,
                                              int32_t* perm, int32_t* sfirst, int32_t* sparent, int64_t* rptr,
                                              int32_t* rows, int64_t rows_cap, int32_t* lvl_ptr, int32_t* lvl_sup,
                                              int64_t* stats, int64_t stats_len);
GPBOOST_AMD_EXPORT int GPB_TestSparseCholCreate(int n, int m, const int32_t* nbr, int64_t nbr_len, int d,
                                                const double* X, int64_t x_len, const int64_t* opts, void** out);
GPBOOST_AMD_EXPORT int GPB_TestSparseCholFree(void* handle);
/* Bv, dBv: n x m row-major (B(i, nbr[i][r]), unit diagonal implicit); Dinv, dD: n. dBv and dD are nullable
 * together (no derivative: tr_da of the selected inverse is 0). */
GPBOOST_AMD_EXPORT int GPB_TestSparseCholSetB(void* handle, const double* Bv, int64_t bv_len, const double* Dinv,
                                              int64_t dinv_len, const double* dBv, int64_t dbv_len, const double* dD,
                                              int64_t dd_len);
/* Factor A + diag(W) (W nullable = 0). out_info: non-zero exactly when some pivot was not positive and finite;
 * logdet (nullable): 2 sum log L_ii. */
GPBOOST_AMD_EXPORT int GPB_TestSparseCholFactor(void* handle, const double* W, int64_t w_len, int* out_info,
                                                double* logdet);
/* op 0: Solve (nrhs = 1), 1: SolveMulti, 2: ForwardCols, 3: BackwardCols; b, x: n x nrhs column-major in the
 * matrix labels (ForwardCols' result: elimination position k at label perm[k]). inplace = 1: x aliases b on
 * the device. An error before the first factorization. */
GPBOOST_AMD_EXPORT int GPB_TestSparseCholSolve(void* handle, int op, int nrhs, int inplace, const double* b,
                                               int64_t b_len, double* x, int64_t x_len);
/* tr(S B^T D^-1 B), tr(S dA), diag(S) in the matrix labels; each output nullable. */
GPBOOST_AMD_EXPORT int GPB_TestSparseCholSelectedInverse(void* handle, double* tr_bdb, double* tr_da, double* diagS,
                                                         int64_t diag_len);
/* which = 0: the factor L, exact zeros outside its structure; 1: the selected inverse, NaN outside the lower
 * structure of L; 2: the same entries of the selected inverse read from their mirrored (upper) copies in the
 * fronts. n x n column-major in elimination positions (row / column k = label perm[k]). */
GPBOOST_AMD_EXPORT int GPB_TestSparseCholDense(void* handle, int which, double* out, int64_t out_len);

/* The operator layer of the iterative latent-Vecchia path on host arrays: the sparse operators
 * Y = diag(scale)(unit X + V X) and Y = unit pre.*X + V^T (pre.*X) + W.*H in every selectable kernel form, their
 * production composition (B^T D^-1 B + W) X, and the VADU preconditioner. No reference counterpart (tests).
 * Graph: nbr is n x m row-major (row i holds min(i, m) entries), X the coordinates n x d row-major (used only
 * by the storage relabelling). Checked on the host before any device call, a violation being an error return:
 * 1 <= n < 2^24, m >= 1, d >= 1, nbr_len = n m, x_len = n d, 0 <= nbr[i][r] < i and distinct within a row for
 * r < min(i, m), finite coordinates, and every other *_len against the size it names.
 * opts (nullable, 9 entries): {relabel (0: storage order = Vecchia order), dense_rows, head_rows, tail_merge,
 * seg_form (0 block, 1 wave), tail_order (0 row, 1 level), tail_form (0 launch, 1 persist), tail_w, no_graph};
 * an entry < 0 keeps what GPBOOST_AMD_NO_RELABEL / _DENSE_ROWS / _HEAD_ROWS / _TAIL_MERGE / _SEG_FORM /
 * _TAIL_ORDER / _TAIL_FORM / _TAIL_W / _NO_GRAPH give. */
GPBOOST_AMD_EXPORT int GPB_TestLatentOpsCreate(int n, int m, const int32_t* nbr, int64_t nbr_len, int d,
                                               const double* X, int64_t x_len, const int64_t* opts, void** out);
GPBOOST_AMD_EXPORT int GPB_TestLatentOpsFree(void* handle);
/* The per-evaluation refresh of an evaluation on given values, all in Vecchia order: Bv (n x m: B(i, nbr[i][r]),
 * unit diagonal implicit), Dinv, W, dw (n each, vec_len = n), alt_vals (nullable, n x m: a second value array on
 * B's pattern for the operators' use_alt_vals paths). */
GPBOOST_AMD_EXPORT int GPB_TestLatentOpsSetValues(void* handle, const double* Bv, int64_t bv_len, const double* Dinv,
                                                  const double* W, const double* dw, int64_t vec_len,
                                                  const double* alt_vals, int64_t alt_len);
/* stats (stats_len = 22): nnz, the longest and the shortest transposed list, lists longer than 64 (long-row
 * waves), runs of the segmented t = 1 form, runs closed by the entry limit / by the row limit, runs that are
 * one list longer than the entry limit, pad entries of the paired layout, {tiles, fallback rows, largest union}
 * of the B and of the B^T tile plan, K0, K, the dense head's padded order, merged tail levels of the B^T and of
 * the lower solve, segment passes, launches per preconditioner application. vo (nullable, vo_len = n): the
 * Vecchia row of storage row p. */
GPBOOST_AMD_EXPORT int GPB_TestLatentOpsInfo(void* handle, int64_t* stats, int64_t stats_len, int32_t* vo,
                                             int64_t vo_len);
/* One application on n x t row-major blocks in Vecchia order (block_len = n t, vec_len = n for each given vector).
 * op 0: Y = diag(scale)(unit X + V X); op 1: Y = unit pre.*X + V^T (pre.*X) + W.*H (W and H go together);
 * V = Bv's values, or alt_vals' with use_alt_vals. op 2: Y = (B^T D^-1 B + W) X of the set values (form 0 the
 * production dispatch, 1 the LDS-tiled pair). op 3: Y = P^-1 X of the VADU plan and Y2 = the plan's scratch, B^-T X on
 * the Vecchia rows >= K0 (the dense head's rows hold the head's input); with graphs on, a second call at the same t replays the captured graph. form 0 = the production dispatch, other values the
 * kernels listed in csrc/latent_test.h (LatentBForm / LatentBtForm); a form the shape or the arguments do not
 * admit is an error return. Outputs start as NaN between 64 guard doubles on either side; guard_flag = 1 when a
 * guard word changed. */
GPBOOST_AMD_EXPORT int GPB_TestLatentOpsApply(void* handle, int op, int form, int t, int unit, int use_alt_vals,
                                              const double* X, const double* pre, const double* scale,
                                              const double* W, int64_t vec_len, const double* H, double* Y,
                                              double* Y2, int64_t block_len, int* guard_flag);
/* The block-CG vector kernels on host arrays of any n and t (no structure; ops: LatentVecOp in
 * csrc/latent_test.h): 0 coldots (np = 1..3 pairs of blocks, small_out np t), 1 cg_update (blocks H, V, U, R,
 * sv0 = a; out0 = U, out1 = R, small_out = rr), 2 h_update (blocks Z, H, sv0 = b; out0 = H), 3 cg_alpha
 * (sv0 = rz, sv1 = hv, act; small_out = a, hist), 4 cg_beta (sv0 = rz_new, sv1 = rz, act; small_out = b, hist,
 * rz), 5 axpby (blocks X, Y; out0), 6 cap_mode_change (blocks mode, mnew; out0), 7 pack_columns (np columns
 * from column ia of blocks[0] to column ib of blocks[1]; out0). blocks: 6 pointers (unused ones NULL), each
 * n x t row-major with block_len = n t; sv0, sv1, act: t entries (small_len = t); act nullable (all active). */
GPBOOST_AMD_EXPORT int GPB_TestLatentOpsVector(int op, int n, int t, int np, int ia, int ib, double alpha,
                                               double beta, const double* const* blocks, int64_t block_len,
                                               const double* sv0, const double* sv1, const int32_t* act,
                                               int64_t small_len, double* out0, double* out1, double* small_out,
                                               int64_t small_out_len, int* guard_flag);
/* The PCG of the iterative path on the handle's operator (B^T D^-1 B + W) and VADU preconditioner from a zero
 * start: RHS, U n x t row-major in Vecchia order (block_len = n t); columns [0, n_single) stop by the
 * single-vector rule (||r|| < delta, pmax_single), the others by the block rule (mean ||r|| < delta,
 * pmax_block). its: {single, block} iteration counts; flags: {NaN met, zero right-hand side (t = 1)}. */
GPBOOST_AMD_EXPORT int GPB_TestLatentOpsPcg(void* handle, int t, int n_single, double delta, int pmax_single,
                                            int pmax_block, const double* RHS, double* U, int64_t block_len,
                                            int* its, int* flags);

/* The full-scale Vecchia ("VIF") row factor, sparse products and vector kernels on host arrays, launched by the
 * host launch functions VifSolver uses (csrc/vif.h). No reference counterpart (tests). Everything is checked on
 * the host before any device call, a violation being an error return. Matrices that the device holds as m x n
 * with leading dimension ldm = round_up(m, 64) are host arrays n x m row-major (point i's m entries contiguous);
 * the hook fills the ldm - m padding entries of every input column with pad_fill. Outputs and scratch start as
 * NaN between 64 guard doubles on either side; guard_flag = 1 when a guard word changed.
 *
 * GPB_TestVifRows: the residual rows i0 .. n_total - 1 of the points X (n_total x d, x_len = n_total d, d in
 * 1..3, finite). nbr: (n_total - i0) x nn, the row of point i holding min(i, nn) distinct indices in [0, i) and
 * -1 after them (nbr_len). V, P0, P1: n_total x m (mat_len = n_total m; P0 and P1 given exactly when grad = 1).
 * nn in 1..48 with grad, 1..64 without; m in 1..4096; cov_type 0..3 (CovType of csrc/cov.h); var, phi > 0;
 * nugget >= 0; cjit > 0. form 0: the production dispatch, 1: the MFMA form (refused for nn > 31), 2: the
 * LDS-staged form; order 1: the rows in Morton order, XCD-chunked, as VifSolver processes them (with more than
 * one row), 0: in index order. Outputs (rows_len = n_total - i0): D, Bv (rows x nn) and with grad dD0, dD1,
 * dBv0, dBv1 (NULL otherwise). */
GPBOOST_AMD_EXPORT int GPB_TestVifRows(int n_total, int d, int i0, int nn, int m, const double* X, int64_t x_len,
                                       const int32_t* nbr, int64_t nbr_len, const double* V, const double* P0,
                                       const double* P1, int64_t mat_len, int cov_type, double var, double phi,
                                       double nugget, double cjit, int grad, int form, int order, double pad_fill,
                                       double* D, double* Bv, double* dD0, double* dD1, double* dBv0, double* dBv1,
                                       int64_t rows_len, int* guard_flag);
/* One sparse product on the graph nbr (n x nn, nbr_len = n nn, row i holding min(i, nn) distinct indices < i)
 * with the coefficients coef (n x nn, coef_len). op 0 (BRow): out[i] = self in[i] + sum_r coef[i][r] in[nbr[i][r]]
 * over m-vectors (in: n x m, in_len = n m), div = 1: times 1 / D_i; want_div = 1: out2 = the same times 1 / D_i.
 * op 1 (BCol): out[j] = self in[j] + sum over the rows i that hold j of coef(i, j) in[i], the coefficients
 * gathered into column order on the device. op 2 (BVec): out_i = (self x_i + sum_r coef[i][r] x[nbr[i][r]])
 * (/ D_i with D), in: n entries. op 3 (BtVec): the transposed vector product. D: n entries or NULL. X (nullable,
 * n x d) with order = 1: the columns in Morton order as VifSolver processes them. out / out2: n x ldm for ops 0
 * and 1 (the padding entries are returned as they are left), n for ops 2 and 3 (out_len). n < 2^22, m in 1..4096. */
GPBOOST_AMD_EXPORT int GPB_TestVifApply(int op, int n, int nn, int m, const int32_t* nbr, int64_t nbr_len,
                                        const double* coef, int64_t coef_len, const double* D, const double* in,
                                        int64_t in_len, double self, int div, int want_div, const double* X, int d,
                                        int order, double pad_fill, double* out, double* out2, int64_t out_len,
                                        int* guard_flag);
/* The small kernels (ops: VifVecOp in csrc/vif_test.h): 0 gemv (arrays M n x m, x n; out m), 1 column dots with
 * a vector (M, w m; out n), 2 column dots of two matrices (M, M2; out n), 3 z = (e - dD u) / D (dD, u, e, D; out
 * n), 4 sums of nt in 1..8 terms (arrays a_t, b_t, c_t for each term, b / c nullable; sum_ops[t] in 0..4: a b c,
 * log a, a b / c, a b^2 / c^2, a b / c^2; out nt), 5 dK_mn / dlog phi (X n x d, Z m x d; out n x ldm, padding as
 * left). lens[k]: the entries of arrays[k] (0 for NULL). */
GPBOOST_AMD_EXPORT int GPB_TestVifVector(int op, int n, int m, int d, int cov_type, double var, double phi,
                                         double pad_fill, const double* const* arrays, const int64_t* lens,
                                         int n_arrays, const int32_t* sum_ops, int nt, double* out, int64_t out_len,
                                         int* guard_flag);
/* The FITC kernels (csrc/fitc_kernels.hip, csrc/fitc_fisher.hip) on host arrays, launched by the host launch
 * functions FitcSolver and fitc_inducing_points use (csrc/fitc.h). No reference counterpart (tests). Everything is
 * checked on the host before any device call, a violation being an error return. Matrices that the device holds as
 * m x n with leading dimension ldm = round_up(m, 64) are host arrays n x m row-major, the m x m ones m x m row-major
 * (row k = the device's column k); the hook fills the padding of every input with pad_fill, and outputs of these
 * shapes come back as n x ldm / m x ldm with the padding as it was left. Outputs and scratch start as NaN between 64
 * guard doubles on either side; guard_flag = 1 when a guard word changed.
 *
 * GPB_TestFitcVector: one kernel per op (FitcVecOp in csrc/fitc_test.h, which lists every op's arrays, ints, extra
 * and outs). n in 1..2^22 - 1, m in 1..4096, d in 1..3 and cov_type 0..3 for the ops that take coordinates; lens[k]:
 * the entries of arrays[k] (0 for NULL), out_lens[k] those of outs[k]. The pairs of op pred_corr name prediction
 * points in 0..np - 1, each at most once, and training points in 0..n - 1. */
GPBOOST_AMD_EXPORT int GPB_TestFitcVector(int op, int n, int m, int d, int cov_type, double var, double phi,
                                          double extra, double pad_fill, const double* const* arrays,
                                          const int64_t* lens, int n_arrays, const int32_t* ints, int64_t ints_len,
                                          double* const* outs, const int64_t* out_lens, int n_outs, int* guard_flag);
/* The k-means steps of the inducing-point search on the points X (n x d) and the centres mu (k x d, k <= n <
 * 2^22, k <= 4096, d in 1..3, all finite); ops: FitcKmeansOp in csrc/fitc_test.h. 0 assign: ints_out = the cluster of
 * every point (n). 1 means: the new means of the assignment cluster_in (n entries in 0..k - 1) in mu_out, mu being
 * the old means; scan = 1: the scanning kernel (ints_len = 0), scan = 0: the member-list path, ints_out = cnt, off
 * (nbk x k each, nbk = ceil(n / 256)), tot (k), base (k + 1), list (n). 2 cmp: ints_out = [any(mu != mu_a), any(mu
 * != mu_b)]. 3 lloyd: the whole loop of fitc_inducing_points from the seeds mu with at most max_it (1..1000)
 * iterations; mu_out = the final means, its = the iterations run (no guard bands: the loop owns its buffers).
 * Integer outputs start as a negative fill between guard words. */
GPBOOST_AMD_EXPORT int GPB_TestFitcKmeans(int op, int n, int k, int d, const double* X, int64_t x_len, const double* mu,
                                          const double* mu_a, const double* mu_b, int64_t mu_len,
                                          const int32_t* cluster_in, int64_t cluster_len, int scan, int max_it,
                                          double* mu_out, int32_t* ints_out, int64_t ints_len, int* its,
                                          int* guard_flag);
/* A FitcSolver on the points X (n x d, n <= 65536), the inducing points Z (m x d, m <= min(n, 1024)) and the response
 * y (n) runs one stage (FitcStage in csrc/fitc_test.h: 0 Factor, 1 Eval with the gradient, 2 Gram then Eval at the
 * same parameters, 3 Gram at (var2, phi2) then Eval at (var, phi), 4 Predict at Xp (np x d, np <= 4096) with match
 * (np entries in -1..n - 1)); then the solver's buffers are copied out as they stand into the non-NULL outs[k]
 * (FitcStageOut of csrc/fitc_test.h names them; n_outs = 24; matrices with their padding, n x ldm or m x ldm; sums
 * = Eval's six; mean / var / cov (np, np, np x np column-major) are Predict's, var and cov computed when asked for).
 * Everything is checked on the host before any device call. */
GPBOOST_AMD_EXPORT int GPB_TestFitcStages(int stage, int n, int m, int d, int cov_type, double var, double phi,
                                          double var2, double phi2, const double* X, const double* Z, const double* y,
                                          int np, const double* Xp, const int32_t* match, double* const* outs,
                                          const int64_t* out_lens, int n_outs);
/* The batched dense kernel of models with several clusters (csrc/dense_batch.hip) on caller-given clusters. No
 * reference counterpart (tests). C clusters, cluster c holding the rows ptr[c] .. ptr[c + 1] - 1 (ptr: C + 1 entries
 * from 0, 1 .. 64 rows per cluster) of X (N x d row-major, d in 1..3) and y (N); cov_type 0..3, var and phi > 0 on
 * the transformed scale. sums (C x 6): [log|Psi_c|, y_c' Psi_c^-1 y_c, -1/2 u' dPsi/dlog var u, -1/2 u' dPsi/dlog phi
 * u, tr(Psi^-1 dPsi/dlog var), tr(Psi^-1 dPsi/dlog phi)] with Psi_c = var corr + I and u = Psi_c^-1 y_c (the last four
 * 0 without want_grad); u (N, nullable); info (C): 1 for a cluster with a pivot that is not positive and finite (its
 * sums and u are NaN), else 0. Every extent is checked on the host before the launch. */
GPBOOST_AMD_EXPORT int GPB_TestDenseBatch(int cov_type, int C, int d, const int32_t* ptr, int64_t ptr_len,
                                          const double* X, int64_t x_len, const double* y, int64_t y_len, double var,
                                          double phi, int want_grad, double* sums, int64_t sums_len, double* u,
                                          int64_t u_len, int32_t* info, int64_t info_len);
/* EXTENSION (no reference counterpart): out = [clusters, clusters served by the batched kernel, clusters with an
 * engine of their own] of a GP model (1, 0, 0 without several clusters). GPBOOST_AMD_NO_CLUSTER_BATCH=1, read when
 * the model is created, gives every cluster an engine. */
GPBOOST_AMD_EXPORT int GPB_GetClusterInfo(REModelHandle handle, int32_t* out);
/* The likelihood layer of the Laplace paths (csrc/lik_device.h) on host arrays. No reference counterpart (tests).
 * Everything is checked on the host before any device call, a violation being an error return; outputs and
 * scratch start as NaN between 64 guard doubles on either side; guard_flag = 1 when a guard word changed or a
 * scalar that was not asked for was written. lik: LatentLik of csrc/latent_kernels.h (0 gaussian, 1
 * bernoulli_logit, 2 bernoulli_probit, 3 poisson, 4 gamma, 5 negative_binomial: GPB_TestLikPoint,
 * GPB_TestLikAuxPoint and path 0 of GPB_TestLikPath only, as grouped random effects alone have it; every other
 * path refuses it before any device call); aux finite and > 0; n < 2^22.
 *
 * GPB_TestLikPoint: log-likelihood, first derivative, information and the information's derivative at (y_i,
 * loc_i), i < n, from a kernel that calls the four device functions and nothing else; dinfo_lowrank: the same
 * derivative from the low-rank preconditioner's launch_lik_dinfo (lik 5: left NaN, that path does not have it). */
GPBOOST_AMD_EXPORT int GPB_TestLikPoint(int lik, double aux, int n, const double* y, const double* loc, double* loglik,
                                        double* d1, double* info, double* dinfo, double* dinfo_lowrank,
                                        int* guard_flag);
/* lik 5 only (the likelihood whose shape gradient takes the general form): the derivatives of d1 and of the
 * information with respect to log(aux), and log(mu + aux) + (y + aux) / (mu + aux), the per-observation term of
 * the explicit shape gradient, at (y_i, loc_i), i < n. */
GPBOOST_AMD_EXPORT int GPB_TestLikAuxPoint(int lik, double aux, int n, const double* y, const double* loc,
                                           double* dd1_aux, double* dinfo_aux, double* aux_term, int* guard_flag);
/* One production kernel (set) of a Laplace path on its production grid (LikPath / LikKernel of csrc/lik_test.h).
 * y, mode, offset (nullable), every vecs[k] and every outs[k]: n entries; an output is given exactly when its
 * option asks for it (NULL otherwise). lam in (0, 1]. idx / arr0 / arr1 / mats are NULL (lengths 0) unless named.
 *   path 0 grouped (mode NULL, offset = F; idx = glev, K x n with entries in [0, arr_len), arr0 = b; opts = {K,
 *     want_dW}): kernel 0 glp_obs_kernel<true>, outs = {d1, W, dW}; kernel 1 glp_obs_kernel<false>, no outs; both
 *     followed by glp_finish_kernel, scalars = {sum loglik}; kernel 2 (lik 5 only; opts = {K}) glp_nb_aux_kernel,
 *     outs = {dd1 / dlog aux, dW / dlog aux}, then glp_finish_kernel, scalars = {sum of the explicit term}.
 *   path 1 full-scale Vecchia: kernel 0 vl_prep_kernel (opts = {want_dW, want_rhs, want_count}, outs = {d1, W,
 *     dW, rhs}, scalars = {#(W == 0)} with want_count); kernel 1 vl_trial_kernel (vecs = {upd}, opts = {first,
 *     cap}, outs = {trial}, scalars = {sum loglik}).
 *   path 2 FITC: kernel 0 fl_prep_kernel (vecs = {dvec, stored W (nullable with w_update)}, opts = {w_update,
 *     want_rhs}, outs = {d1, W, wdw, DW, rhs}); kernel 1 fl_trial_kernel (vecs = {a, mupd, aupd}, outs = {mnew,
 *     anew}, scalars = {a^T mode, sum loglik}); kernel 2 fl_final_kernel (vecs = {dvec}, outs = {d1, W, DW, dpwi},
 *     scalars = {sum log dpwi, sum log W, #(W == 0)}).
 *   path 3 dense: kernel 0 dl_prep_kernel (opts = {want_rhs}, outs = {d1, W, sqrt W, rhs}); kernel 1
 *     dl_trial_kernel (as FITC's); kernel 2 dl_dmll_kernel (n <= 2048, opts = {ld >= n, want_dg}, mats = C then S,
 *     ld x n column-major each, mats_len = 2 ld n, outs = {dmll, dg}).
 *   path 4 sparse Vecchia: kernel 0 newton_prep_kernel (vecs = {Dinv, stored W (nullable with W_update)}, opts =
 *     {W_update, want_rhs, want_dw, want_sdw}, outs = {d1, W, rhs, dw, sdw}; with an ObsMap idx = ptr (n + 1
 *     entries, 0 .. arr_len ascending), arr0 = the observations' y, arr1 = their offset or NULL).
 * The stored W is what a kernel reads with (w / W)_update = 0; outs[1] returns the block as the kernel left it. */
GPBOOST_AMD_EXPORT int GPB_TestLikPath(int path, int kernel, int n, int lik, double aux, const double* y,
                                       const double* mode, const double* offset, const double* const* vecs, int n_vecs,
                                       const int32_t* idx, int64_t idx_len, const double* arr0, const double* arr1,
                                       int64_t arr_len, const double* mats, int64_t mats_len, double lam,
                                       const int32_t* opts, int n_opts, double* const* outs, int n_outs,
                                       double* scalars, int n_scalars, int* guard_flag);
/* The grouped random-effects engine (csrc/grouped_kernels.hip, csrc/grouped_laplace.hip) on host arrays, through
 * the production launch functions. No reference counterpart (tests). Everything is checked on the host before any
 * device call, a violation being an error return. Outputs and scratch (the chunk partials included) start as NaN
 * between 64 guard doubles on either side; guard_flag = 1 when a guard word changed. Dense matrices are host M x M
 * column-major; the hook places them at leading dimension ld >= M and fills the ld - M padding with NaN.
 *
 * GPB_TestGroupedCreate: a GroupedRE on a stream of its own for levels (K x n, levels_len = K n, each in 0..n-1,
 * taken as given: an index that no observation uses is a row with count 0 and no entries).
 * GPB_TestGroupedInfo: stats (14): M, nnz, n, K, then for the lane split of t columns tc, the chunk length, the
 * chunk counts of the full / lower / upper plan, the entries of ints, and the segmented sums' long level
 * destinations, their chunks, all long destinations, all chunks. ints (nullable together with dbls): cum (K + 1),
 * rowptr (M + 1), split (M), col (nnz), the observation lists' ptr (M + 1) and entries (n K), then e0, e1 (chunk
 * count each) and ptr (M + 1) of the full, the lower and the upper plan, lower_q and upper_q (K + 1 each), all as
 * the device holds them; dbls: val (nnz), cnt (M). */
GPBOOST_AMD_EXPORT int GPB_TestGroupedCreate(int n, int K, const int32_t* levels, int64_t levels_len, void** out);
/* GPB_TestGroupedCreateWeighted: the same with the values of Z (random slopes): weights (K x n, finite) gives
 * Z[i, level of i in effect k] = weights[k n + i] for every effect with has_weight[k] != 0; an effect with
 * has_weight[k] == 0 is an intercept (all ones, no array). Two effects may share their levels. Every op of the
 * GPB_TestGrouped* entries then runs the weighted kernels: op 0 of Small gives Z^T y with Z's values, the assembly
 * of LaplaceOps the sums of z_k[i] w_i (diag_only) or of z_a[i] z_b[i] w_i (full), q / row trace / grad_F the weighted
 * gathers, and ops 2 and 3 of Dense take one more input, wt (np K): column k of point p enters with wt[p K + k].
 * dbls of Info then holds the weighted values of Z^T Z. */
GPBOOST_AMD_EXPORT int GPB_TestGroupedCreateWeighted(int n, int K, const int32_t* levels, int64_t levels_len,
                                                     const double* weights, int64_t weights_len,
                                                     const int32_t* has_weight, void** out);
GPBOOST_AMD_EXPORT int GPB_TestGroupedFree(void* handle);
GPBOOST_AMD_EXPORT int GPB_TestGroupedInfo(void* handle, int t, int64_t* stats, int64_t stats_len, int32_t* ints,
                                           int64_t ints_len, double* dbls, int64_t dbls_len);
/* One product on M x t row-major blocks (block_len = M t, t in 1..1024), K >= 2. val: the nnz off-diagonal values
 * in CSR order, NULL: the model's counts. op 0 apply: Out0 = (diag(dg) + offdiag) In; 1 the same with the lower
 * off-diagonal part; 2 Out0 = (L D^-1/2) In; 3 the SSOR sweeps: Out0 = X = (L D^-1/2)^-1 In, Out1 = Z =
 * (L D^-1/2)^-T X; 4 Out0 = D^-1 (upper triangle of A) In; 5 GroupedRE::Precond after SetOperator(val, NULL, D,
 * dis) (Out0 = its scratch X, Out1 = Z). dis: M entries for ops 2, 3 and 5 (independent of D), NULL otherwise;
 * Out1: for ops 3 and 5 only. */
GPBOOST_AMD_EXPORT int GPB_TestGroupedApply(void* handle, int op, int t, const double* val, const double* dg_or_D,
                                            const double* dis, const double* In, double* Out0, double* Out1,
                                            int64_t block_len, int* guard_flag);
/* op 0 launch_gre_zty: in = y (n); out = Z^T y (M). 1 launch_gre_diag: in = cnt (M), tau (K, > 0); out = D (M),
 * dis (M), sums (2 K). 2 launch_gre_single on m = in_len[0] rows: in = zty, cnt, D (m each); out = u (m), sums (2).
 * 3 launch_gre_residual: in = rhs, V (any equal length); out = rhs - V. */
GPBOOST_AMD_EXPORT int GPB_TestGroupedSmall(void* handle, int op, const double* const* in, const int64_t* in_len,
                                            int n_in, double* const* out, const int64_t* out_len, int n_out,
                                            int* guard_flag);
/* M <= 4096, M <= ld <= 8192. op 0 launch_gre_dense_build: in = val (nnz, or length 0: the model's counts), D (M);
 * out = the M columns of ld entries, zero before the launch. 1 launch_gre_inv_diag: in = Li (M x M); out (M).
 * 2 / 3 launch_gre_pred_cols with E / with var: idx (np x K, -1..M-1), in = Li; out = E (np columns of ld entries,
 * the padding as left) / var (np). 4 launch_gre_fisher_cols: in = sc (M), Ainv (M x M); out = part (M x K), diag (M). */
GPBOOST_AMD_EXPORT int GPB_TestGroupedDense(void* handle, int op, int ld, int np, const int32_t* idx,
                                            const double* const* in, const int64_t* in_len, int n_in,
                                            double* const* out, const int64_t* out_len, int n_out, int* guard_flag);
/* SetOperator(val, cnt, D, dis) (val / cnt NULL: the model's) and SolveVec(rhs, u, pmax, delta, warm); warm = 1:
 * u starts from u0. its: the iterations run. */
GPBOOST_AMD_EXPORT int GPB_TestGroupedSolve(void* handle, const double* val, const double* cnt, const double* D,
                                            const double* dis, const double* rhs, int warm, const double* u0,
                                            int pmax, double delta, double* u, int* its, int* guard_flag);
/* A GroupedLaplace on the handle's engine (K <= 8). op 0 Assemble: sub = diag_only, in = w (n); out (M, or M + nnz:
 * the levels, then the CSR slots). 1 glp_q_kernel<sub = AUX> and glp_finish_kernel on the production block count:
 * in = Ainv (M x M at ld; length 0 for K = 1), D (M), W, dW (n), Wa (n, length 0 without AUX); out = dwq (n), sums
 * (K, + 1 with AUX). 2 glp_row_trace_kernel: in = U, V (M x t), dW (n); out (n). 3 glp_grad_f_kernel: in = d1, dwq,
 * W (n), v (M); out (n). 4 glp_vec_kernel, sub = form (0 1/sigma2 + x, 1 x - y / sigma2, 2 x / y, 3 x + alpha y,
 * 4 sqrt(1 / x)): in = sigma2 (K), x (M), y (M, length 0 for forms 0 and 4); out (M). 5 glp_effect_dots_kernel,
 * sub = mode (0 x y, 1 log x, 2 1 / x, 3 x / y): in = sigma2 (K), x (M), y (M, length 0 for modes 1 and 2); out (K). */
GPBOOST_AMD_EXPORT int GPB_TestGroupedLaplaceOps(void* handle, int op, int sub, int t, int ld, double alpha,
                                                 const double* const* in, const int64_t* in_len, int n_in,
                                                 double* const* out, const int64_t* out_len, int n_out,
                                                 int* guard_flag);
/* The residual factor of a gp_approx = "full_scale_vecchia" model at cov_pars (original scale) in the model
 * order: perm (n, nullable: perm[i] = original index of the i-th point), neighbors (n x num_neighbors, nullable),
 * D (n), B_vals (n x num_neighbors, B(i, nbr) = -A_i, 0-padded) and their derivatives with respect to log var and
 * log phi on the transformed scale (dD: 2 x n, dB_vals: 2 x n x num_neighbors). Runs the GEMM chain of an
 * evaluation with the gradient (V, P_k), then the rows. */
GPBOOST_AMD_EXPORT int GPB_GetVifFactor(REModelHandle handle, const double* cov_pars, int32_t* perm,
                                        int32_t* neighbors, double* D, double* B_vals, double* dD, double* dB_vals);

/* ---------------------------------------------------------------- prediction */

/* replaces GPB_SetPredictionData (include/LightGBM/c_api.h:1578; c_api.cpp). Only the settings
 * are supported: vecchia_pred_type (NULL: unchanged; supported: "order_obs_first_cond_obs_only",
 * the reference's default for Gaussian likelihoods, and "latent_order_obs_first_cond_obs_only", its
 * default for latent models, re_model_template.h:6485-6490), num_neighbors_pred (<= 0: unchanged;
 * default 2 * num_neighbors, :299) and nsim_var_pred (<= 0: unchanged; default 1000, :5374: draws of
 * the latent models' predictive-variance simulation). Prediction data must be NULL / 0 (pass it to
 * GPB_PredictREModel); cg_delta_conv_pred and rank_pred_approx_matrix_lanczos are accepted and
 * ignored (the Vecchia-Laplace draws use the model's cg_delta_conv, likelihoods.h:12043-12053).
 * cluster_ids_data_pred (num_data_pred) is saved for GP models with several clusters and refused otherwise. */
GPBOOST_AMD_EXPORT int GPB_SetPredictionData(REModelHandle handle,
    int32_t num_data_pred,
    const int32_t* cluster_ids_data_pred,
    const char* re_group_data_pred,
    const double* re_group_rand_coef_data_pred,
    double* gp_coords_data_pred,
    const double* gp_rand_coef_data_pred,
    const double* covariate_data_pred,
    const char* vecchia_pred_type,
    int num_neighbors_pred,
    double cg_delta_conv_pred,
    int nsim_var_pred,
    int rank_pred_approx_matrix_lanczos);

/* replaces GPB_PredictREModel (include/LightGBM/c_api.h:1617; Vecchia_utils.cpp:1634-2442,
 * re_model_template.h:3700-4071; dense CalcPred, FITC CalcPredFITC_FSA, grouped CalcPred): predictive mean
 * (out_predict[0 .. num_data_pred)) and, if predict_var, variances (out_predict[num_data_pred ..
 * 2 num_data_pred)), or, if predict_cov_mat, the num_data_pred^2 covariance (column-major).
 * gp_coords_data_pred column-major num_data_pred x dim_gp_coords. cov_pars on the original scale (NULL: those
 * of the last evaluation); y_data NULL: the response set before; use_saved_data: the data of
 * GPB_SetPredictionData. Exact Gaussian models: predict_response = false removes the nugget variance (latent
 * process). Every vecchia_pred_type is supported: order_obs_first_cond_obs_only / _cond_all, order_pred_first,
 * latent_order_obs_first_cond_obs_only / _cond_all (Gaussian and Laplace models). Latent Vecchia models
 * (PredictLaplaceApproxVecchia likelihoods.h:6576-6813): the Laplace mode at cov_pars, mean = -Bpo mode
 * (cond_all: Bp^-1 on top); with matrix_inversion_method = "iterative" predict_var / predict_cov_mat add the
 * reference's simulation term (nsim_var_pred draws; statistically equivalent, or the reference's own one-thread
 * stream with GPBOOST_AMD_PRED_DRAWS=reference), with "cholesky" the exact term ||L^-1 Bpo^T e_p||^2 on the
 * sparse Cholesky factor of Sigma^-1 + W (:6751-6811); predict_response gives the response mean / variance.
 * Deviation from the reference, by design: with vecchia_pred_type = "order_pred_first" the variances and the
 * covariance matrix are returned in prediction-point order (row p = the p-th prediction point); the
 * reference returns them in the order of its sparse factor's AMD permutation (an artefact of its
 * SimplicialLLT; the means are in prediction-point order on both sides). Unsupported inputs (clusters,
 * GP random coefficients, full_scale_vecchia, num_neighbors_pred > 64) return -1 with a message.
 * GP models with several clusters need cluster_ids_data_pred and gp_coords_data_pred: every prediction point uses
 * the training data of its own cluster, an id without training data gets mean 0 (or fixed_effects_pred) and the
 * prior covariance (plus the nugget with predict_response), and covariances between clusters are 0
 * (re_model_template.h:3292-3420); a call without the ids fails with a message naming them.
 * Grouped models with random slopes need re_group_rand_coef_data_pred (column-major num_data_pred x
 * num_re_group_rand_coef; also accepted and saved by GPB_SetPredictionData): the values of Z at the prediction
 * points. GPB_PredictREModelTrainingDataRandomEffects returns one block of num_data means per component (a
 * slope's block holds the slope effect, not its product with the covariate), then the variances where supported. */
GPBOOST_AMD_EXPORT int GPB_PredictREModel(REModelHandle handle,
    const double* y_data,
    int32_t num_data_pred,
    double* out_predict,
    bool predict_cov_mat,
    bool predict_var,
    bool predict_response,
    const int32_t* cluster_ids_data_pred,
    const char* re_group_data_pred,
    const double* re_group_rand_coef_data_pred,
    double* gp_coords_data_pred,
    const double* gp_rand_coef_data_pred,
    const double* cov_pars,
    const double* covariate_data_pred,
    bool use_saved_data,
    const double* fixed_effects,
    const double* fixed_effects_pred);

/* ---------------------------------------------------------------- EXTENSION: multi-GPU */

/* Size of the opaque communicator id (bytes). */
GPBOOST_AMD_EXPORT int GPB_CommIdSize(void);
/* Create a communicator id on one rank (to be broadcast to all ranks by the caller). */
GPBOOST_AMD_EXPORT int GPB_CommCreateId(char* id_out);
/* Join the model to an RCCL communicator. Exact Vecchia: rows (observations in Vecchia order)
 * are split into world_size contiguous blocks; this rank evaluates block `rank` and the
 * per-rank partial sums are all-reduced over RCCL (one all-reduce of 6 doubles per
 * evaluation). Latent Vecchia (iterative): every rank holds the whole factor and runs its
 * share of the num_rand_vec_trace probe columns; one all-reduce of 1 double per PCG iteration
 * (block stopping rule) and of the per-probe terms at the end (SURVEY.md §8e Option A).
 * Must be called before the first evaluation. comm_id may be NULL only at world_size 1 (no
 * communicator); a non-NULL id at world_size 1 creates a one-rank communicator (same data
 * path). */
GPBOOST_AMD_EXPORT int GPB_SetDistributed(REModelHandle handle, int rank, int world_size, const char* comm_id);
/* As GPB_SetDistributed, with the cross-rank sums done by `allreduce` on host buffers (it must
 * replace buf[0..count) by the element-wise sum over all ranks, e.g. a gloo all-reduce) instead
 * of RCCL: a transport for tests with several ranks on one GPU, where RCCL refuses to run. */
GPBOOST_AMD_EXPORT int GPB_SetDistributedHostReduce(REModelHandle handle, int rank, int world_size,
    void (*allreduce)(double* buf, int count, void* user), void* user);
/* The six per-row partial sums over Vecchia rows [row_begin, row_end) at cov_pars (original
 * scale), without any all-reduce: for callers that run their own communication. The
 * response must have been set by a previous evaluation. */
GPBOOST_AMD_EXPORT int GPB_EvalVecchiaPartials(REModelHandle handle, const double* cov_pars,
    int32_t row_begin, int32_t row_end, double* sums);
/* Host-side partition of n rows over world_size ranks (block distribution). */
GPBOOST_AMD_EXPORT int GPB_PartitionRows(int32_t num_data, int world_size, int rank, int32_t* row_begin, int32_t* row_end);
/* Host-side final assembly from all-reduced partial sums (exposed so the reduction
 * contract can be tested without a GPU): sums = [logdet, q, s1_var, s1_range, s2_var, s2_range]. */
GPBOOST_AMD_EXPORT int GPB_CombinePartials(const double* sums, int32_t num_data, double sigma2,
    int profile_sigma2, double* negll, double* grad, double* sigma2_out);

#ifdef __cplusplus
}
#endif
#endif /* GPBOOST_AMD_H_ */
