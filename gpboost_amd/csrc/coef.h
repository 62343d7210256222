// Linear regression coefficients (fixed effects) of Laplace-approximated models, estimated inside the L-BFGS vector
// [log cov pars, beta, log aux pars] (optimizer_coef = "lbfgs", EvalLLforLBFGSpp, optim_utils.h:243-364):
//   - the device passes over the scaled covariate matrix X (coef_kernels.hip): the offset F + X beta the Laplace
//     driver reads, the coefficient gradient X^T grad_F, and the four sums of MaximalLearningRateCoef;
//   - CoefLayer (coef.cpp): intercept detection, centring and scaling with its inverse, the initial intercept, the
//     constants C_mu / C_sigma2 and the step cap (re_model_template.h:976-1000, 1084-1153, 4952-4981, 7273-7315;
//     likelihoods.h:747-802, 1658-1685).
// CoefLayer knows no model: a driver gives it a device offset buffer, a device grad_F buffer and a stream.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"
#include "covariates.h"

namespace gpb_amd {

constexpr int kCoefMaxCols = kCovMaxCols - 1;   // 31
constexpr int kCoefRows = 256;                  // rows of X per tile (one per thread of a block)
constexpr int kCoefMaxBlocks = 1024;
constexpr double kCoefMaxChange = 10.;          // C_MAX_CHANGE_COEF_ (re_model_template.h:5293)

// Blocks of the three passes: a function of n alone, so that equal inputs give equal bits.
int coef_blocks(int n);
// Doubles of `partial` scratch the two reductions need: coef_blocks(n) * max(p, 4).
size_t coef_partial_len(int n, int p);

// X: n x p row-major on the device, 1 <= p <= kCoefMaxCols; beta, dir: p doubles on the device.
// eta0_i = F_i + sum_j X_ij beta_j (F nullable: 0).
void launch_coef_offset(int n, int p, const double* X, const double* beta, const double* F, double* eta0,
                        hipStream_t s);
// g_j = sum_i X_ij gF_i: per-block partials (tiles in ascending order inside a block), summed in block order.
void launch_coef_grad(int n, int p, const double* X, const double* gF, double* partial, double* g, hipStream_t s);
// mom = [sum (X dir)_i, sum (X beta)_i, sum (X dir)_i^2, sum (X dir)_i (X beta)_i], same order of summation.
void launch_coef_step_moments(int n, int p, const double* X, const double* beta, const double* dir, double* partial,
                              double* mom, hipStream_t s);

// Test entry (GPB_TestCoefOps): host arrays in and out, the default stream, synchronised. X row-major n x p.
// eta0 (n), g (p), mom (4) each nullable; F nullable; gF needed for g, beta for eta0 / mom, dir for mom.
void test_coef_ops(int n, int p, const double* X, const double* beta, const double* dir, const double* F,
                   const double* gF, double* eta0, double* g, double* mom);

// ---- host layer

// Step cap of MaximalLearningRateCoef from the four sums over n observations.
double coef_max_learning_rate(const double mom[4], int n, double C_mu, double C_sigma2);
// FindInitialIntercept (lik: kLik* of lik_device.h; y, F host, F nullable)
double coef_initial_intercept(int lik, int n, const double* y, const double* F, double rand_eff_var);
// FindConstantsCapTooLargeLearningRateCoef
void coef_cap_constants(int lik, int n, const double* y, double* C_mu, double* C_sigma2);

// Intercept detection and the centring / scaling of the covariates (host only, no device call).
struct CoefScaling {
  // X_colmajor: n x p as the C ABI passes it. The intercept is the first constant column (TwoNumbersAreEqual against
  // its first entry); every other column is centred and scaled by its population standard deviation unless the
  // intercept is the only column. Xs (nullable) receives the scaled matrix, row-major.
  // transform = false: the columns stay as given (only the intercept is looked for).
  CoefScaling(int n, int p, const double* X_colmajor, std::vector<double>* Xs, bool transform = true);
  bool has_intercept() const { return intercept_col >= 0; }
  // TransformCoef / TransformBackCoef (identity when the covariates are not scaled)
  std::vector<double> ToScaled(const std::vector<double>& beta) const;
  std::vector<double> ToOriginal(const std::vector<double>& beta) const;
  int n, p, intercept_col = -1;
  bool scaled = false;
  std::vector<double> loc, scale;
};

class CoefLayer {
 public:
  // Uploads the scaled matrix (CoefScaling) row-major; keeps X as given for the calls outside the optimizer.
  // transform = false: X is uploaded as given (evaluations at coefficients on the original scale).
  CoefLayer(int n, int p, const double* X_colmajor, hipStream_t s, bool transform = true);
  ~CoefLayer();
  CoefLayer(const CoefLayer&) = delete;
  CoefLayer& operator=(const CoefLayer&) = delete;
  int n() const { return n_; }
  int p() const { return p_; }
  const CoefScaling& scaling() const { return sc_; }
  bool has_intercept() const { return sc_.has_intercept(); }
  const std::vector<double>& X_colmajor() const { return X_; }   // as given (original scale)
  std::vector<double> ToScaled(const std::vector<double>& beta) const { return sc_.ToScaled(beta); }
  std::vector<double> ToOriginal(const std::vector<double>& beta) const { return sc_.ToOriginal(beta); }
  // Initial beta on the optimizer's scale: 0, the intercept from FindInitialIntercept; also sets C_mu / C_sigma2.
  std::vector<double> Init(int lik, const double* y, const double* F, double tot_var);
  // Host: out_i = (F_i) + sum_j X_ij beta_j with the original X and beta, for the calls outside the optimizer.
  void LinearPredictor(const double* beta_orig, const double* F, double* out) const;
  // Device: the offset F + X beta (beta on the optimizer's scale) written to d_off (n). F host-side is uploaded once
  // by SetF.
  void SetF(const double* F);
  void WriteOffset(const double* beta, double* d_off);
  // Device: grad_beta = X^T gF (host, p) for the device gradient gF of the driver.
  void Gradient(const double* d_gradf, double* grad_beta);
  // GetMaximalLearningRate's coefficient part for the step direction dir (the optimizer's drt, not negated: the
  // cap depends on |.| and squares only).
  double MaxLearningRate(const double* beta, const double* dir);
  double C_mu() const { return C_mu_; }
  double C_sigma2() const { return C_sigma2_; }

 private:
  int n_, p_;
  hipStream_t s_;
  std::vector<double> X_, Xs_;   // Xs_: the scaled rows, released after the upload
  CoefScaling sc_;
  double C_mu_ = 1., C_sigma2_ = 1.;
  DevBuf<double> d_X_, d_F_, d_beta_, d_dir_, d_partial_, d_out_;
  bool has_F_ = false;
  // GPBOOST_AMD_TIMING: HIP events around every pass, the device time of each printed to stderr
  bool timing_ = false;
  void ReportTime(const char* pass);
  hipEvent_t ev_[2] = {nullptr, nullptr};
};

}  // namespace gpb_amd
