// Host side of the coefficient layer (coef.h): intercept detection, centring / scaling and its inverse, the
// initial intercept, the step-cap constants and the cap itself, restated from the reference's
// OptimLinRegrCoefCovPar set-up (re_model_template.h:976-1000, 1084-1153), TransformCoef / TransformBackCoef
// (:7273-7315), MaximalLearningRateCoef (:4952-4981), FindInitialIntercept (likelihoods.h:747-802) and
// FindConstantsCapTooLargeLearningRateCoef (:1658-1685).
#include "coef.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "latent_kernels.h"

namespace gpb_amd {

namespace {

// TwoNumbersAreEqual (utils.h:50-54)
bool nearly_equal(double a, double b) {
  return std::fabs(a - b) < 1e-10 * std::max({1.0, std::fabs(a), std::fabs(b)});
}

double horner(const double* c, int deg, double x) {   // c[deg] x^deg + ... + c[0]
  double v = c[deg];
  for (int k = deg - 1; k >= 0; --k) v = v * x + c[k];
  return v;
}

// Standard normal quantile, Wichura's algorithm AS 241 (PPND16, Applied Statistics 37 (1988) 477-484): rational
// approximations in q = p - 1/2 for |q| <= 0.425 and in r = sqrt(-log(min(p, 1 - p))) for the tails.
double normal_quantile(double p) {
  static const double a[8] = {3.3871328727963666080, 1.3314166789178437745e2, 1.9715909503065514427e3,
                              1.3731693765509461125e4, 4.5921953931549871457e4, 6.7265770927008700853e4,
                              3.3430575583588128105e4, 2.5090809287301226727e3};
  static const double b[8] = {1., 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3,
                              2.1213794301586595867e4, 3.9307895800092710610e4, 2.8729085735721942674e4,
                              5.2264952788528545610e3};
  static const double c[8] = {1.42343711074968357734, 4.63033784615654529590, 5.76949722146069140550,
                              3.64784832476320460504, 1.27045825245236838258, 2.41780725177450611770e-1,
                              2.27238449892691845833e-2, 7.74545014278341407640e-4};
  static const double d[8] = {1., 2.05319162663775882187, 1.67638483018380384940, 6.89767334985100004550e-1,
                              1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4,
                              1.05075007164441684324e-9};
  static const double e[8] = {6.65790464350110377720, 5.46378491116411436990, 1.78482653991729133580,
                              2.96560571828504891230e-1, 2.65321895265761230930e-2, 1.24266094738807843860e-3,
                              2.71155556874348757815e-5, 2.01033439929228813265e-7};
  static const double f[8] = {1., 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2,
                              7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7,
                              2.04426310338993978564e-15};
  const double q = p - 0.5;
  if (std::fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    return q * horner(a, 7, r) / horner(b, 7, r);
  }
  double r = std::sqrt(-std::log(q < 0. ? p : 1. - p));
  double v;
  if (r <= 5.) {
    r -= 1.6;
    v = horner(c, 7, r) / horner(d, 7, r);
  } else {
    r -= 5.;
    v = horner(e, 7, r) / horner(f, 7, r);
  }
  return q < 0. ? -v : v;
}

}  // namespace

double coef_max_learning_rate(const double mom[4], int n, double C_mu, double C_sigma2) {
  const double mean_change = mom[0] / n, mean_lag1 = mom[1] / n;
  const double var_change = mom[2] / n - mean_change * mean_change;
  const double cov = mom[3] / n - mean_change * mean_lag1;
  const double max_lr_mu = C_mu * kCoefMaxChange / std::fabs(mean_change);
  const double max_lr_var =
      (std::fabs(cov) + std::sqrt(cov * cov + 4 * var_change * C_sigma2 * kCoefMaxChange)) / 2 / var_change;
  return std::min({max_lr_mu, max_lr_var});   // std::min: a NaN second argument keeps the first (as the reference)
}

double coef_initial_intercept(int lik, int n, const double* y, const double* F, double rand_eff_var) {
  if (!(rand_eff_var > 0.)) Fatal("the total variance of the random effects must be > 0");
  if (lik == kLikBernoulliLogit || lik == kLikBernoulliProbit) {
    double swy = 0.;
    for (int i = 0; i < n; ++i) swy += y[i];
    double pavg = swy > 0. ? swy / n : 0.5;
    pavg = std::min(std::max(pavg, 1e-12), 1. - 1e-12);
    const double v = lik == kLikBernoulliLogit ? std::log(pavg / (1. - pavg)) : normal_quantile(pavg);
    return std::min(std::max(v, -3.), 3.);
  }
  if (lik == kLikPoisson || lik == kLikGamma || lik == kLikNegBinomial) {
    double avg = 0.;
    for (int i = 0; i < n; ++i) avg += F == nullptr ? y[i] : y[i] / std::exp(F[i]);
    avg = std::max(avg / n, 1e-12);
    return std::log(avg) - 0.5 * rand_eff_var;
  }
  Fatal("the initial intercept is not defined for this likelihood");
}

void coef_cap_constants(int lik, int n, const double* y, double* C_mu, double* C_sigma2) {
  if (lik == kLikPoisson || lik == kLikGamma || lik == kLikNegBinomial) {
    double mean = 0., sec = 0.;
    for (int i = 0; i < n; ++i) {
      mean += y[i];
      sec += y[i] * y[i];
    }
    mean /= n;
    sec /= n;
    const double var = sec - mean * mean;
    const double inf = std::numeric_limits<double>::infinity();
    *C_mu = std::fabs(mean > 0. ? std::log(mean) : -inf);
    *C_sigma2 = std::fabs(var > 0. ? std::log(var) : -inf);
    return;
  }
  *C_mu = 1.;
  *C_sigma2 = 1.;
}

CoefScaling::CoefScaling(int n_in, int p_in, const double* X, std::vector<double>* Xs, bool do_transform)
    : n(n_in), p(p_in) {
  if (n < 1) Fatal("covariate data needs at least one observation");
  if (p < 1 || p > kCoefMaxCols)
    Fatal("num_covariates = %d is not supported by gpboost_amd for likelihoods other than 'gaussian' (1 .. %d)", p,
          kCoefMaxCols);
  if (X == nullptr) Fatal("covariate_data is NULL");
  for (size_t e = 0; e < (size_t)n * p; ++e)
    if (std::isnan(X[e]) || std::isinf(X[e])) Fatal("NaN or Inf in covariate data 'X'");
  for (int j = 0; j < p && intercept_col < 0; ++j) {
    const double* col = X + (size_t)j * n;
    bool constant = true;
    for (int i = 1; i < n && constant; ++i) constant = nearly_equal(col[i], col[0]);
    if (constant) intercept_col = j;
  }
  scaled = do_transform && !(has_intercept() && p == 1);
  loc.assign(p, 0.);
  scale.assign(p, 1.);
  if (Xs != nullptr) Xs->resize((size_t)n * p);
  for (int j = 0; j < p; ++j) {
    const double* col = X + (size_t)j * n;
    const bool transform = scaled && j != intercept_col;
    if (transform) {
      double sum = 0.;
      for (int i = 0; i < n; ++i) sum += col[i];
      loc[j] = sum / n;
      double ss = 0.;
      for (int i = 0; i < n; ++i) ss += (col[i] - loc[j]) * (col[i] - loc[j]);
      scale[j] = std::sqrt(ss / n);
    }
    if (Xs != nullptr)
      for (int i = 0; i < n; ++i) (*Xs)[(size_t)i * p + j] = transform ? (col[i] - loc[j]) / scale[j] : col[i];
  }
}

std::vector<double> CoefScaling::ToScaled(const std::vector<double>& beta) const {
  std::vector<double> t = beta;
  if (!scaled) return t;
  for (int j = 0; j < p; ++j) {
    if (j == intercept_col) continue;
    if (has_intercept()) t[intercept_col] += t[j] * loc[j];
    t[j] *= scale[j];
  }
  if (has_intercept()) t[intercept_col] *= scale[intercept_col];
  return t;
}

std::vector<double> CoefScaling::ToOriginal(const std::vector<double>& beta) const {
  std::vector<double> o = beta;
  if (!scaled) return o;
  if (has_intercept()) o[intercept_col] /= scale[intercept_col];
  for (int j = 0; j < p; ++j) {
    if (j == intercept_col) continue;
    o[j] /= scale[j];
    if (has_intercept()) o[intercept_col] -= o[j] * loc[j];
  }
  return o;
}

CoefLayer::CoefLayer(int n, int p, const double* X_colmajor, hipStream_t s, bool transform)
    : n_(n), p_(p), s_(s), sc_(n, p, X_colmajor, &Xs_, transform) {
  X_.assign(X_colmajor, X_colmajor + (size_t)n * p);
  timing_ = std::getenv("GPBOOST_AMD_TIMING") != nullptr;
  d_X_.alloc(Xs_.size());
  d_beta_.alloc(kCovMaxCols);
  d_dir_.alloc(kCovMaxCols);
  d_partial_.alloc(coef_partial_len(n, p));
  d_out_.alloc(kCovMaxCols + 4);
  HIP_CHECK(hipMemcpyAsync(d_X_.get(), Xs_.data(), sizeof(double) * Xs_.size(), hipMemcpyHostToDevice, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
  std::vector<double>().swap(Xs_);
  if (timing_)
    for (auto& e : ev_) HIP_CHECK(hipEventCreate(&e));
}

CoefLayer::~CoefLayer() {
  for (auto& e : ev_)
    if (e != nullptr) (void)hipEventDestroy(e);
}

std::vector<double> CoefLayer::Init(int lik, const double* y, const double* F, double tot_var) {
  std::vector<double> beta(p_, 0.);
  if (has_intercept()) beta[sc_.intercept_col] = coef_initial_intercept(lik, n_, y, F, tot_var);
  coef_cap_constants(lik, n_, y, &C_mu_, &C_sigma2_);
  return beta;
}

void CoefLayer::LinearPredictor(const double* beta_orig, const double* F, double* out) const {
  for (int i = 0; i < n_; ++i) out[i] = F != nullptr ? F[i] : 0.;
  for (int j = 0; j < p_; ++j) {
    const double* col = X_.data() + (size_t)j * n_;
    for (int i = 0; i < n_; ++i) out[i] += col[i] * beta_orig[j];
  }
}

void CoefLayer::ReportTime(const char* pass) {
  float ms = 0.f;
  HIP_CHECK(hipEventSynchronize(ev_[1]));
  HIP_CHECK(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
  std::fprintf(stderr, "[coef] %s: %.4f ms (n = %d, p = %d)\n", pass, ms, n_, p_);
}

void CoefLayer::SetF(const double* F) {
  has_F_ = F != nullptr;
  if (!has_F_) return;
  d_F_.alloc(n_);
  HIP_CHECK(hipMemcpyAsync(d_F_.get(), F, sizeof(double) * n_, hipMemcpyHostToDevice, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
}

void CoefLayer::WriteOffset(const double* beta, double* d_off) {
  HIP_CHECK(hipMemcpyAsync(d_beta_.get(), beta, sizeof(double) * p_, hipMemcpyHostToDevice, s_));
  if (timing_) HIP_CHECK(hipEventRecord(ev_[0], s_));
  launch_coef_offset(n_, p_, d_X_.get(), d_beta_.get(), has_F_ ? d_F_.get() : nullptr, d_off, s_);
  if (timing_) {
    HIP_CHECK(hipEventRecord(ev_[1], s_));
    ReportTime("offset");
  }
  // beta is pageable host memory: the copy above has been staged when the call returns
}

void CoefLayer::Gradient(const double* d_gradf, double* grad_beta) {
  if (timing_) HIP_CHECK(hipEventRecord(ev_[0], s_));
  launch_coef_grad(n_, p_, d_X_.get(), d_gradf, d_partial_.get(), d_out_.get(), s_);
  if (timing_) HIP_CHECK(hipEventRecord(ev_[1], s_));
  HIP_CHECK(hipMemcpyAsync(grad_beta, d_out_.get(), sizeof(double) * p_, hipMemcpyDeviceToHost, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
  if (timing_) ReportTime("gradient");
}

double CoefLayer::MaxLearningRate(const double* beta, const double* dir) {
  HIP_CHECK(hipMemcpyAsync(d_beta_.get(), beta, sizeof(double) * p_, hipMemcpyHostToDevice, s_));
  HIP_CHECK(hipMemcpyAsync(d_dir_.get(), dir, sizeof(double) * p_, hipMemcpyHostToDevice, s_));
  if (timing_) HIP_CHECK(hipEventRecord(ev_[0], s_));
  launch_coef_step_moments(n_, p_, d_X_.get(), d_beta_.get(), d_dir_.get(), d_partial_.get(), d_out_.get(), s_);
  if (timing_) HIP_CHECK(hipEventRecord(ev_[1], s_));
  double mom[4];
  HIP_CHECK(hipMemcpyAsync(mom, d_out_.get(), sizeof(double) * 4, hipMemcpyDeviceToHost, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
  if (timing_) ReportTime("step moments");
  return coef_max_learning_rate(mom, n_, C_mu_, C_sigma2_);
}

}  // namespace gpb_amd
