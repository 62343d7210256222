// GroupedModel implementation: configuration, response handling, the combination of GroupedRE's
// device sums into the negative log-likelihood and its gradient, and the L-BFGS fit.
#include "grouped_model.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <unordered_map>

namespace gpb_amd {

std::vector<std::vector<int>> parse_group_levels(int n, int K, const char* re_group_data,
                                                 std::vector<std::unordered_map<std::string, int>>* label_index) {
  if (re_group_data == nullptr) Fatal("re_group_data is NULL");
  std::vector<std::vector<int>> levels(K, std::vector<int>(n));
  if (label_index) label_index->assign(K, {});
  const char* p = re_group_data;
  for (int k = 0; k < K; ++k) {
    std::unordered_map<std::string, int> local;
    std::unordered_map<std::string, int>& index = label_index ? (*label_index)[k] : local;
    index.reserve(1024);
    for (int i = 0; i < n; ++i) {
      std::string label(p);
      p += label.size() + 1;
      auto it = index.find(label);
      if (it == index.end()) it = index.emplace(std::move(label), (int)index.size()).first;
      levels[k][i] = it->second;
    }
  }
  return levels;
}

GroupedModel::GroupedModel(int n, const std::vector<std::vector<int>>& levels, const std::string& mim, int seed,
                           std::vector<std::unordered_map<std::string, int>> label_index, const std::string& likelihood,
                           const GroupedSlopes& slopes)
    : n_(n), mim_(mim), likelihood_(likelihood), label_index_(std::move(label_index)) {
  (void)seed;   // grouped models draw no random numbers at construction (probes use seed_rand_vec_trace)
  if (n <= 0) Fatal("num_data must be > 0");
  G_ = (int)levels.size();
  if (G_ < 1) Fatal("num_re_group must be > 0");
  // components (re_model_template.h:6833-6872): the intercepts, the slopes, then the dropped intercept removed
  for (int k = 0; k < G_; ++k) {
    comp_group_.push_back(k);
    comp_slope_.push_back(-1);
  }
  if (slopes.R > 0) {
    if (slopes.data == nullptr || slopes.ind == nullptr)
      Fatal("group_rand_coef_data and ind_effect_group_rand_coef must be given together");
    std::vector<bool> has_slope(G_, false);
    for (int r = 0; r < slopes.R; ++r) {
      if (slopes.ind[r] < 1 || slopes.ind[r] > G_)   // :252-254
        Fatal("ind_effect_group_rand_coef[%d] = %d is not in 1..%d (the grouping variables, counted from 1)", r,
              slopes.ind[r], G_);
      has_slope[slopes.ind[r] - 1] = true;
      const double* col = slopes.data + (size_t)r * n;
      for (int i = 0; i < n; ++i)
        if (std::isnan(col[i]) || std::isinf(col[i])) Fatal("NaN or Inf in group_rand_coef_data");
      slope_data_.emplace_back(col, col + n);
      comp_group_.push_back(slopes.ind[r] - 1);
      comp_slope_.push_back(r);
    }
    int dropped = -1;
    for (int k = 0; slopes.drop != nullptr && k < G_; ++k) {
      if (!(slopes.drop[k] > 0)) continue;
      if (!has_slope[k])   // the intent of :258-265
        Fatal("Cannot drop intercept random effect number %d (drop_intercept_group_rand_effect) as this random effect "
              "has no corresponding random coefficients", k + 1);
      if (dropped >= 0)
        Fatal("drop_intercept_group_rand_effect: dropping more than one intercept is not supported by gpboost_amd (the "
              "reference removes other components than the documented ones then)");
      dropped = k;
    }
    if (dropped >= 0) {
      comp_group_.erase(comp_group_.begin() + dropped);
      comp_slope_.erase(comp_slope_.begin() + dropped);
    }
    if (comp_group_.size() == 1)
      Fatal("group_rand_coef_data: a model whose only random effect is a random slope (one grouping variable, one "
            "slope, its intercept dropped) is not supported by gpboost_amd");
  }
  const int K = (int)comp_group_.size();
  std::vector<const double*> weights;
  for (int c = 0; c < K; ++c) {
    levels_.push_back(levels[comp_group_[c]]);
    if (has_slopes()) weights.push_back(comp_slope_[c] >= 0 ? slope_data_[comp_slope_[c]].data() : nullptr);
  }
  lik_ = parse_likelihood(likelihood_);
  if (lik_ == kLikNegBinomial) likelihood_ = "negative_binomial";   // the aliases' name (ParseLikelihoodAlias)
  if (mim_ == "default") mim_ = K > 1 ? "iterative" : "cholesky";
  if (mim_ != "iterative" && mim_ != "cholesky")
    Fatal("Matrix inversion method '%s' is not supported.", mim_.c_str());
  if (mim_ == "iterative" && K == 1)   // CheckCompatibilitySpecialOptions (re_model_template.h:6698-6702)
    Fatal("Cannot use matrix_inversion_method = 'iterative' if there is only a single-level grouped random effects. "
          "Use matrix_inversion_method = 'cholesky' instead (this is very fast). Iterative methods are for multiple "
          "grouped random effects ");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    Fatal("no HIP device visible: gpboost_amd has no CPU fallback");
  if (const char* dev = std::getenv("GPBOOST_AMD_DEVICE")) {
    device_ = std::atoi(dev);
    if (device_ < 0 || device_ >= ndev) Fatal("GPBOOST_AMD_DEVICE=%d but %d device(s) visible", device_, ndev);
  } else {
    HIP_CHECK(hipGetDevice(&device_));
  }
  UseDevice();
  HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  re_.reset(new GroupedRE(n, levels_, stream_, weights));
  if (lik_ != kLikGaussian) {
    lap_.reset(new GroupedLaplace(re_.get(), levels_, lik_, weights));
    if (lik_ == kLikGamma || lik_ == kLikNegBinomial) {
      aux_pars_ = {1.};   // aux_pars_ = {1.} until set or estimated (likelihoods.h:181-192)
      init_aux_pars_ = {-1.};
    }
  }
}

GroupedModel::~GroupedModel() {
  lap_.reset();
  re_.reset();
  if (stream_) (void)hipStreamDestroy(stream_);
}

void GroupedModel::UseDevice() const { HIP_CHECK(hipSetDevice(device_)); }

void GroupedModel::AttachGP(int d, const double* coords_colmajor, int cov_type, int seed) {
  if (has_slopes())
    Fatal("group_rand_coef_data together with gp_coords (a Gaussian process beside grouped random effects) is not "
          "supported by gpboost_amd");
  if (laplace())
    Fatal("a Gaussian process beside grouped random effects (gp_coords with group_data) is not supported for "
          "likelihood '%s' by gpboost_amd", likelihood_.c_str());
  if (d < 1 || d > 3) Fatal("dim_gp_coords = %d is not supported by gpboost_amd's dense path (1..3)", d);
  if (coords_colmajor == nullptr) Fatal("gp_coords_data is NULL");
  if (re_->K() > 8) Fatal("GP + grouped random effects: at most 8 grouped effects are supported by gpboost_amd");
  if (iterative())
    Fatal("matrix_inversion_method = 'iterative' is not supported for GP + grouped random effects models by "
          "gpboost_amd (use 'cholesky')");
  UseDevice();
  gp_d_ = d;
  cov_type_ = cov_type;
  seed_ = seed;
  coords_.resize((size_t)n_ * d);
  for (int i = 0; i < n_; ++i)
    for (int q = 0; q < d; ++q) coords_[(size_t)i * d + q] = coords_colmajor[(size_t)q * n_ + i];
  const int K = re_->K();
  std::vector<int> lev((size_t)K * n_);
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < n_; ++i) lev[(size_t)k * n_ + i] = levels_[k][i];
  d_X_.alloc(coords_.size());
  d_lev_.alloc(lev.size());
  d_y_.alloc(n_);
  HIP_CHECK(hipMemcpyAsync(d_X_.get(), coords_.data(), sizeof(double) * coords_.size(), hipMemcpyHostToDevice, stream_));
  HIP_CHECK(hipMemcpyAsync(d_lev_.get(), lev.data(), sizeof(int) * lev.size(), hipMemcpyHostToDevice, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  dense_.reset(new DenseSolver(n_, d, d_X_.get(), stream_));
}

void GroupedModel::ToTrafo(const double* orig, double* trafo) const {
  const int K = re_->K();
  trafo[0] = orig[0];
  for (int k = 0; k < K; ++k) trafo[1 + k] = orig[1 + k] / orig[0];
  if (has_gp()) {
    trafo[1 + K] = orig[1 + K] / orig[0];
    trafo[2 + K] = range_trafo(cov_type_, orig[2 + K]);
  }
}

void GroupedModel::ToOrig(const double* trafo, double sigma2, double* orig) const {
  const int K = re_->K();
  orig[0] = sigma2;
  for (int k = 0; k < K; ++k) orig[1 + k] = trafo[1 + k] * sigma2;
  if (has_gp()) {
    orig[1 + K] = trafo[1 + K] * sigma2;
    orig[2 + K] = range_back(cov_type_, trafo[2 + K]);
  }
}

void GroupedModel::SetResponseAndOffset(const double* y, const double* fixed_effects) {
  if (y == nullptr && fixed_effects == nullptr) {
    if (!y_set_) Fatal("response variable y has not been set");
    return;
  }
  if (y != nullptr) y_raw_.assign(y, y + n_);
  if (y_raw_.empty()) Fatal("response variable y has not been set");
  if (laplace()) {   // F is the offset of the location parameter, not a shift of y
    for (int i = 0; i < n_; ++i)
      if (std::isnan(y_raw_[i]) || std::isinf(y_raw_[i])) Fatal("NaN or Inf in response variable / label ");
    UseDevice();
    if (y != nullptr) lap_->SetY(y_raw_.data());
    if (has_covariates()) {   // the location parameter's offset is F + X beta (has_covariates_, re_model_template.h:3306-3312)
      std::vector<double> off(n_);
      coef_->LinearPredictor(beta_.data(), fixed_effects, off.data());
      lap_->SetOffset(off.data());
    } else {
      lap_->SetOffset(fixed_effects);
    }
    y_set_ = true;
    return;
  }
  y_ = y_raw_;
  if (fixed_effects != nullptr)
    for (int i = 0; i < n_; ++i) y_[i] -= fixed_effects[i];
  for (int i = 0; i < n_; ++i)
    if (std::isnan(y_[i]) || std::isinf(y_[i])) Fatal("NaN or Inf in response variable / label ");
  UseDevice();
  re_->SetY(y_.data());
  if (has_gp()) {
    HIP_CHECK(hipMemcpyAsync(d_y_.get(), y_.data(), sizeof(double) * n_, hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }
  y_set_ = true;
}

void GroupedModel::GetResponseData(double* y) const {
  if (y_raw_.empty()) Fatal("response variable y has not been set");
  std::copy(y_raw_.begin(), y_raw_.end(), y);
}

EvalResult GroupedModel::Eval(const double* cov_pars_orig, bool want_grad, int profile) {
  const int P = num_cov_pars();
  for (int k = 0; k < P; ++k)
    if (!(cov_pars_orig[k] > 0.)) Fatal("covariance parameters must be > 0");
  if (laplace()) {   // an explicit evaluation starts the mode finding from zero (InitializeModeAvec)
    if (profile)
      Fatal("profile_sigma2 is not available for likelihood '%s': there is no error variance to profile out",
            likelihood_.c_str());
    EvalResult r = EvalLaplace(cov_pars_orig, want_grad, GroupedLaplace::Start::kZero, /*fatal_on_nan=*/true);
    last_cov_pars_.assign(cov_pars_orig, cov_pars_orig + P);
    return r;
  }
  std::vector<double> trafo(P);   // TransformCovPars (re_comp.h: sigma_k^2 / sigma^2; the GP range transform)
  ToTrafo(cov_pars_orig, trafo.data());
  EvalResult r = EvalTrafo(trafo.data(), want_grad, profile);
  last_cov_pars_.assign(cov_pars_orig, cov_pars_orig + P);
  if (profile) ToOrig(trafo.data(), r.sigma2, last_cov_pars_.data());
  return r;
}

EvalResult GroupedModel::EvalTrafo(const double* trafo, bool want_grad, int profile, bool fatal_on_nan) {
  if (!y_set_) Fatal("response variable y has not been set");
  UseDevice();
  if (has_gp()) return EvalDense(trafo, want_grad, profile, fatal_on_nan);
  const int K = re_->K();
  GroupedParts parts;
  re_->Eval(trafo + 1, want_grad, iterative(), num_iter_ > 0, iter, parts);
  last_cg_its_ = parts.cg_its;
  last_lanczos_ = parts.lanczos_steps;
  const double q = parts.yTPsiInvy;
  const double sigma2 = profile ? q / n_ : trafo[0];   // ProfileOutSigma2 (re_model_template.h:2407)
  EvalResult res;
  res.sigma2 = sigma2;
  // CalcNegLogLikelihood (Gaussian, re_model_template.h:2880-2890)
  res.nll = q / 2. / sigma2 + parts.logdet / 2. + n_ / 2. * (std::log(sigma2) + std::log(2. * M_PI));
  if (!std::isfinite(res.nll)) {
    if (fatal_on_nan) Fatal("NaN or Inf occurred in the negative log-likelihood");
    res.nll = std::numeric_limits<double>::quiet_NaN();
  }
  if (want_grad) {   // CalcGradPars_Only_Grouped_REs_Woodbury_GaussLikelihood_Cluster_i (:2242-2391)
    int off = 0;
    res.grad.assign(profile ? K : K + 1, 0.);
    if (!profile) {
      res.grad[0] = -q / sigma2 / 2. + n_ / 2.;
      off = 1;
    }
    for (int k = 0; k < K; ++k) res.grad[off + k] = -parts.quad[k] / sigma2 / 2. + parts.trace[k] / 2.;
  }
  last_nll_ = res.nll;
  return res;
}

EvalResult GroupedModel::EvalDense(const double* trafo, bool want_grad, int profile, bool fatal_on_nan) {
  // Psi = sum_k tau_k Z_k Z_k^T + v K(phi) + I on the dense path; gradient wrt the log of the transformed
  // parameters [nugget], tau_1 .. tau_K, v, phi (CalcGradPars dense, re_model_template.h:1798-1818, with the
  // grouped components' dPsi / dlog tau_k = tau_k Z_k Z_k^T)
  const int K = re_->K();
  for (int k = 1; k < K + 3; ++k)
    if (!(trafo[k] > 0.)) Fatal("covariance parameters must be > 0");
  dense_->SetGrouped(K, d_lev_.get(), trafo + 1);
  double sums[6], kms[2];
  dense_->Eval(cov_type_, trafo[1 + K], trafo[2 + K], d_y_.get(), want_grad, sums, kms);
  const double q = sums[1];
  const double sigma2 = profile ? q / n_ : trafo[0];
  EvalResult res;
  res.sigma2 = sigma2;
  res.nll = q / 2. / sigma2 + sums[0] / 2. + n_ / 2. * (std::log(sigma2) + std::log(2. * M_PI));
  if (!std::isfinite(res.nll)) {
    if (fatal_on_nan) Fatal("NaN or Inf occurred in the negative log-likelihood");
    res.nll = std::numeric_limits<double>::quiet_NaN();
  }
  if (want_grad) {
    std::vector<double> s2(K), yaux(n_);
    dense_->GroupedTraces(s2.data(), yaux.data());
    const int off = profile ? 0 : 1;
    res.grad.assign(off + K + 2, 0.);
    if (!profile) res.grad[0] = -q / sigma2 / 2. + n_ / 2.;
    for (int k = 0; k < K; ++k) {   // y_aux^T dPsi_k y_aux = tau_k sum over levels of (sum of y_aux)^2
      std::vector<double> lsum(re_->levels_per_effect()[k], 0.);
      for (int i = 0; i < n_; ++i) lsum[levels_[k][i]] += yaux[i];
      double quad = 0.;
      for (double v : lsum) quad += v * v;
      quad *= trafo[1 + k];
      res.grad[off + k] = -quad / sigma2 / 2. + s2[k] / 2.;
    }
    res.grad[off + K] = sums[2] / sigma2 + sums[4] / 2.;
    res.grad[off + K + 1] = sums[3] / sigma2 + sums[5] / 2.;
  }
  last_nll_ = res.nll;
  return res;
}

void GroupedModel::SetOptimSettings(const double* init_cov_pars, double lr, int max_iter, double delta_rel_conv,
                                    const char* optimizer, int m_lbfgs) {
  if (optimizer != nullptr && optimizer[0] != '\0') {
    const std::string o(optimizer);
    if (laplace() && o != "lbfgs" && o != "gradient_descent")
      Fatal("Optimizer option '%s' is not supported for covariance parameters of grouped random effects with "
            "likelihood '%s' by gpboost_amd (supported: lbfgs, gradient_descent)", optimizer, likelihood_.c_str());
    if (o != "lbfgs" && o != "nelder_mead" && !is_internal_optimizer(o))
      Fatal("Optimizer option '%s' is not supported for covariance parameters by gpboost_amd (supported: lbfgs, "
            "gradient_descent, fisher_scoring, nelder_mead)", optimizer);
    isettings_.optimizer = o == "lbfgs" ? "" : o;
    optimizer_name_ = o;
  }
  isettings_.lr = lr;
  isettings_.max_iter = max_iter;
  isettings_.delta = delta_rel_conv < 0. ? (isettings_.optimizer == "nelder_mead" ? 1e-8 : 1e-6) : delta_rel_conv;
  if (init_cov_pars != nullptr) {
    init_cov_pars_.assign(init_cov_pars, init_cov_pars + num_cov_pars());
    for (double v : init_cov_pars_)
      if (!(v > 0.)) Fatal("init_cov_pars must be > 0");
    cov_pars_orig_ = init_cov_pars_;
    cov_pars_initialized_ = true;
  }
  optim_.initial_step_factor = lr < 0. ? 1. : lr;
  optim_.max_iterations = max_iter;
  optim_.delta = delta_rel_conv < 0. ? 1e-6 : delta_rel_conv;
  if (m_lbfgs > 0) optim_.m = m_lbfgs;
}

void GroupedModel::SetPreconditioner(const char* preconditioner) {
  if (preconditioner == nullptr || preconditioner[0] == '\0') return;
  const std::string p(preconditioner);
  if (p != "ssor")   // SUPPORTED_PRECONDITIONERS_GROUPED_RE_ (re_model_template.h:5410) minus the ones not built
    Fatal("cg_preconditioner_type '%s' is not supported for grouped random effects by gpboost_amd (supported: ssor)",
          p.c_str());
}

void GroupedModel::FindInitCovPar(const double* y, double* trafo) const {
  // re_model_template.h:4388-4485 (Gaussian): sigma^2 = sample variance / 2, every component's marginal
  // variance 1 / num_comps on the transformed scale; the GP range from the median distance (cov_fcts.h
  // FindInitCovPar, draws from the model's mt19937(seed) when n > 1000)
  double mean = 0., var = 0.;
  for (int i = 0; i < n_; ++i) mean += y[i];
  mean /= n_;
  for (int i = 0; i < n_; ++i) var += (y[i] - mean) * (y[i] - mean);
  var /= (n_ - 1);
  const int K = re_->K(), comps = K + (has_gp() ? 1 : 0);
  trafo[0] = var / 2.;
  for (int k = 0; k < K; ++k) trafo[1 + k] = 1. / comps;
  if (has_gp()) {
    trafo[1 + K] = 1. / comps;
    std::mt19937 rng((std::mt19937::result_type)seed_);
    trafo[2 + K] = init_range_trafo(coords_, gp_d_, cov_type_, rng);
  }
}

void GroupedModel::GetInitCovPar(double* out) const {
  const std::vector<double>& v = !init_cov_pars_.empty() ? init_cov_pars_ : init_used_;
  for (int k = 0; k < num_cov_pars(); ++k) out[k] = v.empty() ? -1. : v[k];
}

namespace {

// EvalLLforLBFGSpp with the error variance profiled out (optim_utils.h:269-313): x = log tau. The
// value and gradient come from one device evaluation, as the reference's gradient call reuses the
// state of the preceding likelihood evaluation at the same point.
class GroupedProfiledObjective : public LbfgsObjective {
 public:
  explicit GroupedProfiledObjective(GroupedModel* m) : m_(m) {}
  double Eval(const std::vector<double>& x, std::vector<double>& grad, bool eval_ll, bool calc_grad,
              bool) override {
    if (eval_ll || !(has_ && x == x_)) {
      std::vector<double> trafo(1 + x.size());
      trafo[0] = 1.;
      for (size_t k = 0; k < x.size(); ++k) trafo[1 + k] = std::exp(x[k]);
      EvalResult r = m_->EvalTrafo(trafo.data(), true, 1, /*fatal_on_nan=*/false);
      x_ = x;
      nll_ = r.nll;
      sigma2_ = r.sigma2;
      grad_ = r.grad;
      has_ = true;
    }
    if (calc_grad) grad = grad_;
    return nll_;
  }
  void SetLag1ProfiledOutVariables() override { sigma2_lag1_ = sigma2_; }
  void ResetProfiledOutVariablesToLag1() override { sigma2_ = sigma2_lag1_; }
  void SetNumIter(int it) override { m_->SetNumIter(it); }
  double sigma2() const { return sigma2_; }

 private:
  GroupedModel* m_;
  std::vector<double> x_, grad_;
  double nll_ = 0., sigma2_ = 1., sigma2_lag1_ = 1.;
  bool has_ = false;
};

class GroupedInternalAdapter : public InternalObjective {
 public:
  explicit GroupedInternalAdapter(GroupedModel* m) : m_(m) {}
  double Nll(const std::vector<double>& t) override { return m_->EvalTrafo(t.data(), false, 0, false).nll; }
  std::vector<double> Grad(const std::vector<double>& t, bool profile, double* sigma2) override {
    EvalResult r = m_->EvalTrafo(t.data(), true, profile ? 1 : 0, false);
    if (sigma2) *sigma2 = r.sigma2;
    return r.grad;
  }
  std::vector<double> FisherTrafo(const std::vector<double>& t) override { return m_->FisherTrafo(t.data()); }

 private:
  GroupedModel* m_;
};

}  // namespace

std::vector<double> GroupedModel::FisherTrafo(const double* trafo) {
  // CalcFisherInformation_Only_Grouped_REs_Woodbury with transf_scale = true (re_model_template.h:9579-9586,
  // 9638-9647): FI_00 = n / 2, FI_0j = tau_j tr(Z_j^T Psi^-1 Z_j) / 2 = (m_j - t_j) / 2,
  // FI_jk = tau_j tau_k ||Z_j^T Psi^-1 Z_k||^2 / 2 = (F_jk + delta_jk (m_j - 2 t_j)) / 2 (grouped.h)
  UseDevice();
  const int K = re_->K(), P = 1 + K;
  std::vector<double> F, tr;
  re_->FisherParts(trafo + 1, F, tr);
  std::vector<double> FI((size_t)P * P, 0.);
  FI[0] = n_ / 2.;
  for (int j = 0; j < K; ++j) {
    const double mj = re_->levels_per_effect()[j];
    FI[j + 1] = FI[(size_t)(j + 1) * P] = (mj - tr[j]) / 2.;
    for (int k = 0; k < K; ++k)
      FI[(size_t)(j + 1) * P + k + 1] = (F[(size_t)j * K + k] + (j == k ? mj - 2. * tr[j] : 0.)) / 2.;
  }
  return FI;
}

void GroupedModel::OptimCovPar(const double* y, const double* fixed_effects) {
  UseDevice();
  if (laplace()) {
    OptimCovParLaplace(y, fixed_effects);
    return;
  }
  if (y == nullptr && y_raw_.empty()) Fatal("response variable y has not been set");
  SetResponseAndOffset(y != nullptr ? y : y_raw_.data(), fixed_effects);
  const int P = num_cov_pars();
  num_iter_ = 0;   // re_model_template.h:974
  std::vector<double> trafo(P);
  if (cov_pars_initialized_) ToTrafo(cov_pars_orig_.data(), trafo.data());
  else FindInitCovPar(y_.data(), trafo.data());
  std::vector<double> start_orig(P);
  ToOrig(trafo.data(), trafo[0], start_orig.data());
  if (!cov_pars_initialized_) init_used_ = start_orig;
  if (optim_.max_iterations <= 0) {
    num_it_ = 0;
    cov_pars_orig_ = start_orig;
    cov_pars_initialized_ = true;
    last_cov_pars_ = cov_pars_orig_;
    return;
  }
  if (isettings_.optimizer == "nelder_mead") {   // OptimExternal "nelder_mead" with the nugget profiled out
    if (iterative())
      Fatal("optimizer_cov = 'nelder_mead' is supported by gpboost_amd for grouped random effects with "
            "matrix_inversion_method = 'cholesky' only (use 'lbfgs')");
    const double tol_obj = isettings_.crit_params ? 1e-20 : isettings_.delta;
    const double tol_sol = isettings_.crit_params ? isettings_.delta : 1e-20;
    std::vector<double> x(P - 1);
    for (int k = 0; k < P - 1; ++k) x[k] = std::log(trafo[1 + k]);
    double s2 = 1., fx = 0.;
    auto fn = [&](const std::vector<double>& v) {
      std::vector<double> t(P, 1.);
      for (int k = 0; k < P - 1; ++k) t[1 + k] = std::exp(v[k]);
      EvalResult r = EvalTrafo(t.data(), false, 1, /*fatal_on_nan=*/false);
      s2 = r.sigma2;
      return r.nll;
    };
    num_it_ = nelder_mead(fn, x, isettings_.max_iter, tol_obj, tol_sol, &fx);
    fn(x);   // the profiled sigma^2 at the solution (optim_utils.h:683-686)
    for (int k = 0; k < P - 1; ++k) trafo[1 + k] = std::exp(x[k]);
    cov_pars_orig_.assign(P, 0.);
    ToOrig(trafo.data(), s2, cov_pars_orig_.data());
    cov_pars_initialized_ = true;
    last_nll_ = fx;
    last_cov_pars_ = cov_pars_orig_;
    return;
  }
  if (!isettings_.optimizer.empty()) {   // "gradient_descent" / "fisher_scoring" (re_model_template.h:1287-1549)
    if (isettings_.optimizer == "fisher_scoring" && (has_gp() || iterative()))
      Fatal("optimizer_cov = 'fisher_scoring' is supported by gpboost_amd for grouped random effects with "
            "matrix_inversion_method = 'cholesky' only (use 'lbfgs')");
    GroupedInternalAdapter obj(this);
    double fx = 0.;
    num_it_ = internal_optimize(obj, trafo, isettings_, &fx);
    cov_pars_orig_.assign(P, 0.);
    ToOrig(trafo.data(), trafo[0], cov_pars_orig_.data());
    cov_pars_initialized_ = true;
    last_nll_ = fx;
    last_cov_pars_ = cov_pars_orig_;
    return;
  }
  std::vector<double> x(P - 1);   // log of the transformed parameters, sigma^2 profiled out
  for (int k = 0; k < P - 1; ++k) x[k] = std::log(trafo[1 + k]);
  double fx = 0.;
  GroupedProfiledObjective obj(this);
  num_it_ = lbfgs_minimize(obj, x, fx, optim_);
  for (double v : x)
    if (std::isnan(v) || std::isinf(v))
      Fatal("NaN or Inf occurred in covariance parameter optimization using 'lbfgs' (the reference's nelder_mead "
            "restart is not supported by gpboost_amd)");
  for (int k = 0; k < P - 1; ++k) trafo[1 + k] = std::exp(x[k]);
  cov_pars_orig_.assign(P, 0.);
  ToOrig(trafo.data(), obj.sigma2(), cov_pars_orig_.data());
  cov_pars_initialized_ = true;
  last_nll_ = fx;
  last_cov_pars_ = cov_pars_orig_;
}

std::vector<double> GroupedModel::Blup(const double* cov_pars, const double* y, const double* fixed_effects,
                                       std::vector<double>* var) {
  UseDevice();
  const int K = re_->K();
  std::vector<double> cp;
  if (cov_pars != nullptr) cp.assign(cov_pars, cov_pars + 1 + K);
  else if (!last_cov_pars_.empty()) cp = last_cov_pars_;
  else Fatal("Covariance parameters have not been estimated or correctly set ");
  for (double v : cp)
    if (!(v > 0.)) Fatal("covariance parameters must be > 0");
  if (y != nullptr || fixed_effects != nullptr) SetResponseAndOffset(y, fixed_effects);
  if (!y_set_) Fatal("Response variable data is not provided and has not been set before");
  std::vector<double> tau(K);
  for (int k = 0; k < K; ++k) tau[k] = cp[1 + k] / cp[0];
  std::vector<double> b(re_->M());
  if (var) var->assign(re_->M(), 0.);
  re_->Blup(tau.data(), iterative(), num_iter_ > 0, iter, b.data(), var ? var->data() : nullptr);
  if (var)
    for (double& v : *var) v *= cp[0];   // transformed -> original scale (cov_pars[0] x ..., :4095)
  return b;
}

void GroupedModel::PredictTrainingDataRandomEffects(const double* cov_pars, const double* y, double* out,
                                                    const double* fixed_effects, bool calc_var) {
  const int K = re_->K();
  if (has_gp())
    Fatal("PredictTrainingDataRandomEffects() for GP + grouped random effects models is not supported by "
          "gpboost_amd (call predict())");
  if (calc_var && iterative())
    Fatal("PredictTrainingDataRandomEffects() is currently not implemented for matrix_inversion_method_ == '%s' and "
          "likelihood == 'Gaussian'. Call the predict() function instead.", mim_.c_str());
  if (laplace()) {   // the mode at the parameters, found from zero; means only
    if (calc_var)
      Fatal("variances (predict_var / calc_var) of the training-data random effects are not supported for likelihood "
            "'%s' with grouped random effects by gpboost_amd (call predict() with predict_var)", likelihood_.c_str());
    const std::vector<double> cp = LaplaceCovPars(cov_pars);
    if (y != nullptr || fixed_effects != nullptr) SetResponseAndOffset(y, fixed_effects);
    EvalLaplace(cp.data(), false, GroupedLaplace::Start::kZero, true);
    std::vector<double> b(re_->M());
    lap_->GetMode(b.data());
    int off = 0;
    for (int k = 0; k < K; ++k) {   // a slope's block holds the slope effect itself (re_model_template.h:4266-4280)
      for (int i = 0; i < n_; ++i) out[(size_t)k * n_ + i] = b[off + levels_[k][i]];
      off += re_->levels_per_effect()[k];
    }
    return;
  }
  std::vector<double> var;
  const std::vector<double> b = Blup(cov_pars, y, fixed_effects, calc_var ? &var : nullptr);
  const std::vector<int>& cum_m = re_->levels_per_effect();
  int off = 0;
  for (int k = 0; k < K; ++k) {
    for (int i = 0; i < n_; ++i) {
      out[(size_t)k * n_ + i] = b[off + levels_[k][i]];
      if (calc_var) out[(size_t)K * n_ + (size_t)k * n_ + i] = var[off + levels_[k][i]];
    }
    off += cum_m[k];
  }
}

void GroupedModel::PredComponents(int n_pred, const char* re_group_data_pred, const double* slope_data_pred,
                                  std::vector<int>& idx, std::vector<double>& wt,
                                  std::vector<std::vector<int>>* fresh) const {
  const int K = re_->K();
  if ((int)label_index_.size() != G_) Fatal("the model has no label index (created without re_group_data)");
  if (has_slopes() && slope_data_pred == nullptr)   // re_model_template.h:3086-3089
    Fatal("No random coefficient data 'group_rand_coef_data_pred' has been provided for making predictions with a "
          "model that has grouped random coefficients (group_rand_coef_data)");
  if (!has_slopes() && slope_data_pred != nullptr)
    Fatal("group_rand_coef_data_pred is given but the model has no grouped random coefficients");
  if (has_slopes())
    for (size_t e = 0; e < (size_t)n_pred * num_slopes(); ++e)
      if (std::isnan(slope_data_pred[e]) || std::isinf(slope_data_pred[e]))
        Fatal("NaN or Inf in group_rand_coef_data_pred");
  // labels column-major, as re_group_data (re_model_template.h:3081-3085): seen levels to their level, new labels
  // to -1 - id; the id numbers the distinct new labels of a grouping variable (the same-new-label covariance terms
  // compare these ids, not the strings)
  std::vector<std::vector<int>> glev(G_, std::vector<int>(n_pred));
  const char* p = re_group_data_pred;
  for (int g = 0; g < G_; ++g) {
    std::unordered_map<std::string, int> fresh_ids;
    for (int i = 0; i < n_pred; ++i) {
      std::string label(p);
      p += label.size() + 1;
      auto it = label_index_[g].find(label);
      if (it != label_index_[g].end()) glev[g][i] = it->second;
      else glev[g][i] = -1 - fresh_ids.emplace(std::move(label), (int)fresh_ids.size()).first->second;
    }
  }
  idx.assign((size_t)n_pred * K, -1);
  wt.clear();
  if (has_slopes()) wt.assign((size_t)n_pred * K, 1.);
  if (fresh) fresh->assign(K, std::vector<int>(n_pred, -1));
  int off = 0;
  for (int c = 0; c < K; ++c) {
    const int g = comp_group_[c];
    for (int i = 0; i < n_pred; ++i) {
      if (glev[g][i] >= 0) idx[(size_t)i * K + c] = off + glev[g][i];
      else if (fresh) (*fresh)[c][i] = -1 - glev[g][i];
      if (comp_slope_[c] >= 0) wt[(size_t)i * K + c] = slope_data_pred[(size_t)comp_slope_[c] * n_pred + i];
    }
    off += re_->levels_per_effect()[c];
  }
}

void GroupedModel::Predict(const double* y, int n_pred, const char* re_group_data_pred, const double* gp_coords_pred,
                           const double* cov_pars, bool predict_cov_mat, bool predict_var, bool predict_response,
                           const double* fixed_effects, const double* fixed_effects_pred, double* out,
                           const double* slope_data_pred) {
  if (has_gp()) {
    if (slope_data_pred != nullptr)
      Fatal("group_rand_coef_data_pred is given but the model has no grouped random coefficients");
    PredictCombined(y, n_pred, re_group_data_pred, gp_coords_pred, cov_pars, predict_cov_mat, predict_var,
                    predict_response, fixed_effects, fixed_effects_pred, out);
    return;
  }
  if (gp_coords_pred != nullptr) Fatal("gp_coords_pred given for a model without a Gaussian process");
  if (laplace()) {
    if (predict_cov_mat)
      Fatal("predictive covariance matrices (predict_cov_mat) are not supported for likelihood '%s' with grouped "
            "random effects by gpboost_amd (use predict_var)", likelihood_.c_str());
    PredictLaplace(y, n_pred, re_group_data_pred, cov_pars, predict_var, predict_response, fixed_effects,
                   fixed_effects_pred, out, slope_data_pred);
    return;
  }
  if ((predict_cov_mat || predict_var) && iterative())
    Fatal("predictive (co)variances for grouped random effects with matrix_inversion_method = 'iterative' (the "
          "reference's simulation-based estimate) are not supported by gpboost_amd (use 'cholesky')");
  if (n_pred <= 0) Fatal("num_data_pred must be > 0");
  if (re_group_data_pred == nullptr) Fatal("re_group_data_pred must be provided for grouped random effects");
  const int K = re_->K();
  const bool want_unc = predict_cov_mat || predict_var;
  if (predict_cov_mat && n_pred > 40000)
    Fatal("predictive covariance matrices are limited to 40000 prediction points by gpboost_amd");
  std::vector<int> idx;
  std::vector<double> wt;
  std::vector<std::vector<int>> fresh;
  PredComponents(n_pred, re_group_data_pred, slope_data_pred, idx, wt, want_unc ? &fresh : nullptr);
  const bool wtd = !wt.empty();
  const std::vector<double> b = Blup(cov_pars, y, fixed_effects, nullptr);
  std::vector<double> mu(n_pred, 0.);
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < n_pred; ++i) {
      const int a = idx[(size_t)i * K + k];
      if (a >= 0) mu[i] += wtd ? wt[(size_t)i * K + k] * b[a] : b[a];   // a new level contributes 0
    }
  for (int i = 0; i < n_pred; ++i) out[i] = mu[i] + (fixed_effects_pred ? fixed_effects_pred[i] : 0.);
  if (!want_unc) return;
  std::vector<double> cp;
  if (cov_pars != nullptr) cp.assign(cov_pars, cov_pars + 1 + K);
  else cp = last_cov_pars_;
  std::vector<double> tau(K);
  for (int k = 0; k < K; ++k) tau[k] = cp[1 + k] / cp[0];
  const double nug = predict_response ? 1. : 0., s2 = cp[0];
  double* o = out + n_pred;
  re_->PredCov(n_pred, idx, predict_cov_mat, o, nullptr, wtd ? wt.data() : nullptr);
  if (predict_cov_mat) {
    for (int q = 0; q < n_pred; ++q)
      for (int i = 0; i < n_pred; ++i) {
        double v = o[(size_t)q * n_pred + i] + (i == q ? nug : 0.);
        for (int k = 0; k < K; ++k)
          if (fresh[k][i] >= 0 && fresh[k][i] == fresh[k][q])
            v += wtd ? tau[k] * wt[(size_t)i * K + k] * wt[(size_t)q * K + k] : tau[k];
        o[(size_t)q * n_pred + i] = v * s2;
      }
  } else {
    for (int i = 0; i < n_pred; ++i) {
      double v = o[i] + nug;
      for (int k = 0; k < K; ++k)
        if (idx[(size_t)i * K + k] < 0) v += wtd ? tau[k] * wt[(size_t)i * K + k] * wt[(size_t)i * K + k] : tau[k];
      o[i] = v * s2;
    }
  }
}


std::vector<int> GroupedModel::PredLevels(int n_pred, const char* re_group_data_pred,
                                          std::vector<std::vector<std::string>>* labels) const {
  const int K = re_->K();
  std::vector<int> lev((size_t)K * n_pred, -1);
  if (labels) labels->assign(K, std::vector<std::string>(n_pred));
  const char* p = re_group_data_pred;
  for (int k = 0; k < K; ++k) {
    std::unordered_map<std::string, int> fresh;
    for (int i = 0; i < n_pred; ++i) {
      std::string label(p);
      p += label.size() + 1;
      auto it = label_index_[k].find(label);
      if (it != label_index_[k].end()) {
        lev[(size_t)k * n_pred + i] = it->second;
      } else {
        auto f = fresh.emplace(label, (int)fresh.size()).first;
        lev[(size_t)k * n_pred + i] = -1 - f->second;
      }
      if (labels) (*labels)[k][i] = std::move(label);
    }
  }
  return lev;
}

void GroupedModel::PredictCombined(const double* y, int n_pred, const char* re_group_data_pred,
                                   const double* gp_coords_pred, const double* cov_pars, bool predict_cov_mat,
                                   bool predict_var, bool predict_response, const double* fixed_effects,
                                   const double* fixed_effects_pred, double* out) {
  // CalcPred, !use_woodbury_identity_ branch (re_model_template.h:10165-10244, 10265-10266, 10361-10365,
  // 10526-10534): cross-covariance = grouped indicators + GP cross-covariance, mean = cross_cov Psi^-1 y,
  // cov = Sigma_pp - cross_cov Psi^-1 cross_cov^T, times sigma^2, plus the nugget for responses
  if (n_pred <= 0) Fatal("num_data_pred must be > 0");
  if (re_group_data_pred == nullptr || gp_coords_pred == nullptr)
    Fatal("predictions of GP + grouped random effects models need both group_data_pred and gp_coords_pred");
  if (predict_cov_mat && n_pred > 40000)
    Fatal("predictive covariance matrices are limited to 40000 prediction points by gpboost_amd");
  UseDevice();
  const int K = re_->K(), P = num_cov_pars();
  std::vector<double> cp;
  if (cov_pars != nullptr) cp.assign(cov_pars, cov_pars + P);
  else if (!last_cov_pars_.empty()) cp = last_cov_pars_;
  else Fatal("Covariance parameters have not been estimated or correctly set ");
  for (double v : cp)
    if (!(v > 0.)) Fatal("covariance parameters must be > 0");
  if (y != nullptr || fixed_effects != nullptr) SetResponseAndOffset(y, fixed_effects);
  if (!y_set_) Fatal("Response variable data is not provided and has not been set before");
  std::vector<double> trafo(P);
  ToTrafo(cp.data(), trafo.data());
  const std::vector<int> plev = PredLevels(n_pred, re_group_data_pred, nullptr);
  DevBuf<int> d_plev(plev.size());
  HIP_CHECK(hipMemcpyAsync(d_plev.get(), plev.data(), sizeof(int) * plev.size(), hipMemcpyHostToDevice, stream_));
  std::vector<double> xp((size_t)n_pred * gp_d_);
  for (int i = 0; i < n_pred; ++i)
    for (int q = 0; q < gp_d_; ++q) xp[(size_t)i * gp_d_ + q] = gp_coords_pred[(size_t)q * n_pred + i];
  dense_->SetGrouped(K, d_lev_.get(), trafo.data() + 1);
  dense_->SetGroupedPred(n_pred, d_plev.get());
  std::vector<double> mean(n_pred), var(predict_var && !predict_cov_mat ? n_pred : 0),
      cov(predict_cov_mat ? (size_t)n_pred * n_pred : 0);
  dense_->Predict(cov_type_, trafo[1 + K], trafo[2 + K], d_y_.get(), xp.data(), n_pred,
                  predict_var && !predict_cov_mat, predict_cov_mat, mean.data(), var.data(), cov.data());
  dense_->SetGroupedPred(0, nullptr);
  const double nug = predict_response ? 1. : 0., s2 = cp[0];
  for (int i = 0; i < n_pred; ++i) out[i] = mean[i] + (fixed_effects_pred ? fixed_effects_pred[i] : 0.);
  if (predict_cov_mat) {
    for (int q = 0; q < n_pred; ++q)
      for (int i = 0; i < n_pred; ++i)
        out[n_pred + (size_t)q * n_pred + i] = (cov[(size_t)q * n_pred + i] + (i == q ? nug : 0.)) * s2;
  } else if (predict_var) {
    for (int i = 0; i < n_pred; ++i) out[n_pred + i] = (var[i] + nug) * s2;
  }
}

void GroupedModel::StdDevCovPars(const double* cov_pars, double* sd) {
  if (laplace())
    Fatal("standard deviations of covariance parameters (std_err) are not supported for likelihood '%s' with "
          "grouped random effects by gpboost_amd", likelihood_.c_str());
  if (has_gp())
    Fatal("standard deviations of covariance parameters for GP + grouped random effects models are not "
          "supported by gpboost_amd");
  if (iterative())
    Fatal("standard deviations of covariance parameters for grouped random effects with matrix_inversion_method = "
          "'iterative' (the reference's stochastic estimate) are not supported by gpboost_amd (use 'cholesky')");
  UseDevice();
  const int K = re_->K(), P = 1 + K;
  for (int k = 0; k < P; ++k)
    if (!(cov_pars[k] > 0.)) Fatal("covariance parameters must be > 0");
  std::vector<double> tau(K), FI((size_t)P * P);
  for (int k = 0; k < K; ++k) tau[k] = cov_pars[1 + k] / cov_pars[0];
  re_->Fisher(tau.data(), cov_pars[0], FI.data());
  // FI.inverse() (re_model_template.h:9788): Gauss-Jordan with partial pivoting on the small P x P matrix
  std::vector<double> inv((size_t)P * P, 0.);
  for (int i = 0; i < P; ++i) inv[(size_t)i * P + i] = 1.;
  for (int c = 0; c < P; ++c) {
    int piv = c;
    for (int r = c + 1; r < P; ++r)
      if (std::fabs(FI[(size_t)r * P + c]) > std::fabs(FI[(size_t)piv * P + c])) piv = r;
    if (!(FI[(size_t)piv * P + c] != 0.) || !std::isfinite(FI[(size_t)piv * P + c]))
      Fatal("the Fisher information is singular");
    for (int j = 0; j < P; ++j) {
      std::swap(FI[(size_t)c * P + j], FI[(size_t)piv * P + j]);
      std::swap(inv[(size_t)c * P + j], inv[(size_t)piv * P + j]);
    }
    const double d = FI[(size_t)c * P + c];
    for (int j = 0; j < P; ++j) {
      FI[(size_t)c * P + j] /= d;
      inv[(size_t)c * P + j] /= d;
    }
    for (int r = 0; r < P; ++r) {
      if (r == c) continue;
      const double f = FI[(size_t)r * P + c];
      for (int j = 0; j < P; ++j) {
        FI[(size_t)r * P + j] -= f * FI[(size_t)c * P + j];
        inv[(size_t)r * P + j] -= f * inv[(size_t)c * P + j];
      }
    }
  }
  for (int k = 0; k < P; ++k) sd[k] = std::sqrt(inv[(size_t)k * P + k]);
}

// ---- non-Gaussian likelihoods (GroupedLaplace)

std::vector<double> GroupedModel::LaplaceCovPars(const double* cov_pars) const {
  const int K = re_->K();
  std::vector<double> cp;
  if (cov_pars != nullptr) cp.assign(cov_pars, cov_pars + K);
  else if (!last_cov_pars_.empty()) cp = last_cov_pars_;
  else Fatal("Covariance parameters have not been estimated or correctly set ");
  for (double v : cp)
    if (!(v > 0.)) Fatal("covariance parameters must be > 0");
  return cp;
}

void GroupedModel::SetInitAuxPars(const double* aux) {
  if (aux_pars_.empty() || aux == nullptr) return;
  if (!(aux[0] > 0.)) Fatal("init_aux_pars must be > 0");
  aux_pars_[0] = aux[0];
  init_aux_pars_[0] = aux[0];
  aux_pars_set_ = true;
}

void GroupedModel::GetInitAuxPars(double* aux) const {
  for (size_t k = 0; k < init_aux_pars_.size(); ++k) aux[k] = init_aux_pars_[k];
}

EvalResult GroupedModel::EvalLaplace(const double* sigma2, bool want_grad, GroupedLaplace::Start start,
                                     bool fatal_on_nan, double* grad_f) {
  if (!y_set_) Fatal("response variable y has not been set");
  UseDevice();
  const bool with_aux = !aux_pars_.empty() && estimate_aux_pars;
  const double aux = aux_pars_.empty() ? 1. : aux_pars_[0];
  GroupedLaplaceResult r = lap_->Eval(sigma2, aux, iter, iterative(), want_grad, with_aux, grad_f, start);
  last_cg_its_ = r.cg_its;
  last_lanczos_ = r.lanczos_steps;
  if (r.nan && fatal_on_nan)
    Fatal("NaN or Inf occurred in the mode finding algorithm for the Laplace approximation");
  EvalResult res;
  res.nll = r.nll;
  res.sigma2 = 1.;
  res.grad = r.grad;
  last_nll_ = res.nll;
  return res;
}

namespace {

// EvalLLforLBFGSpp for the Laplace model: x = log(sigma_1^2 .. sigma_K^2 [, shape]). Every likelihood evaluation
// continues from the previous mode (mode_initialized_, likelihoods.h:1985-1991) and computes the gradient only when the
// caller asks for or announces it; a gradient-only call at the point just evaluated uses that evaluation's mode as it
// stands (eval_likelihood = false, optim_utils.h:314-330), as LatentObjective (optim.cpp) does.
class GroupedLaplaceObjective : public LbfgsObjective {
 public:
  // p > 0: x = [log sigma^2 (K), beta (p, on the scaled covariates), log shape]; every evaluation writes the offset
  // F + X beta on the device first (UpdateFixedEffects) and the coefficient gradient is X^T grad_F (CalcGradPars)
  GroupedLaplaceObjective(GroupedModel* m, int K, bool with_aux, int p = 0) : m_(m), K_(K), p_(p), with_aux_(with_aux) {}
  double Eval(const std::vector<double>& x, std::vector<double>& grad, bool eval_ll, bool calc_grad,
              bool hint_grad) override {
    if (eval_ll || !(has_grad_ && x == x_)) {
      std::vector<double> s2(K_);
      for (int k = 0; k < K_; ++k) s2[k] = std::exp(x[k]);
      if (with_aux_) {
        const double aux = std::exp(x[K_ + p_]);
        m_->SetAuxPars(&aux);
      }
      if (p_ > 0) m_->CoefWriteOffset(x.data() + K_);
      const bool grad_only = !eval_ll && has_x_ && x == x_;
      EvalResult r = m_->EvalLaplace(s2.data(), calc_grad || hint_grad,
                                     grad_only ? GroupedLaplace::Start::kKeep : GroupedLaplace::Start::kWarm,
                                     /*fatal_on_nan=*/false);
      has_x_ = true;
      bool bad = !std::isfinite(r.nll);
      if (p_ > 0 && (calc_grad || hint_grad) && (int)r.grad.size() >= K_) {   // [cov, beta, aux]
        std::vector<double> gb(p_);
        m_->CoefGradient(gb.data());
        r.grad.insert(r.grad.begin() + K_, gb.begin(), gb.end());
      }
      for (double g : r.grad) bad = bad || !std::isfinite(g);
      if (bad) m_->ResetLaplaceModeToPrevious();   // EvalLLforLBFGSpp, optim_utils.h:349-360
      x_ = x;
      nll_ = r.nll;
      has_grad_ = calc_grad || hint_grad;
      if (has_grad_) {
        grad_ = r.grad;
        grad_.resize(x.size(), std::numeric_limits<double>::quiet_NaN());
      }
    }
    if (calc_grad) grad = grad_;
    return nll_;
  }
  double MaxLearningRate(const std::vector<double>& x, const std::vector<double>& drt, double max_log_change) override {
    if (p_ == 0) return LbfgsObjective::MaxLearningRate(x, drt, max_log_change);
    double max_abs = 0.;   // MaximalLearningRateCovAuxPars over the covariance and auxiliary entries
    for (size_t i = 0; i < drt.size(); ++i)
      if ((int)i < K_ || (int)i >= K_ + p_) max_abs = std::max(max_abs, std::fabs(drt[i]));
    const double max_lr = max_log_change / max_abs;
    const double max_lr_beta = m_->CoefMaxLearningRate(x.data() + K_, drt.data() + K_);
    return max_lr_beta < max_lr ? max_lr_beta : max_lr;
  }

 private:
  GroupedModel* m_;
  int K_, p_;
  bool with_aux_;
  std::vector<double> x_, grad_;
  double nll_ = 0.;
  bool has_grad_ = false, has_x_ = false;
};

}  // namespace

void GroupedModel::OptimCovParLaplace(const double* y, const double* fixed_effects, bool with_coef) {
  if (y == nullptr && y_raw_.empty()) Fatal("response variable y has not been set");
  const std::vector<double> yraw(y != nullptr ? y : y_raw_.data(), (y != nullptr ? y : y_raw_.data()) + n_);
  beta_.clear();   // no coefficients until this fit has estimated them
  if (!with_coef) coef_.reset();
  SetResponseAndOffset(yraw.data(), fixed_effects);
  const int K = re_->K();
  const int p = with_coef ? coef_->p() : 0;
  num_iter_ = 0;
  // FindInitCovPar for non-Gaussian data (re_model_template.h:4440-4451): marginal variance 1 / num_comps each
  std::vector<double> s2(K, 1. / K);
  if (cov_pars_initialized_) s2 = cov_pars_orig_;
  else init_used_ = s2;
  const bool with_aux = !aux_pars_.empty() && estimate_aux_pars;
  const double* orig_fixed_effects = fixed_effects;
  if (fixed_effects != nullptr) fit_offset_.assign(fixed_effects, fixed_effects + n_);
  else fit_offset_.clear();
  // initial coefficients (re_model_template.h:1108-1153): 0, the intercept from FindInitialIntercept with the total
  // variance of the initial covariance parameters; the shape below is found with the offset F + X beta_init
  std::vector<double> beta_scaled, off_init;
  if (with_coef) {
    double tot_var = 0.;
    for (double v : s2) tot_var += v;
    beta_scaled = coef_->Init(lik_, yraw.data(), fixed_effects, tot_var);
    off_init.resize(n_);
    coef_->LinearPredictor(beta_scaled.data(), fixed_effects, off_init.data());   // only the intercept is non-zero
    fixed_effects = off_init.data();
  }
  if (with_aux && !aux_pars_set_ && lik_ == kLikNegBinomial) {
    // FindInitialAuxPars, negative_binomial (likelihoods.h:1091-1116, 1147-1156): method of moments on y e^-F,
    // r = avg^2 / (var - avg), or 100 avg^2 where the data show no over-dispersion
    double avg = 0., sum_sq = 0.;
    for (int i = 0; i < n_; ++i) {
      const double v = fixed_effects != nullptr ? yraw[i] / std::exp(fixed_effects[i]) : yraw[i];
      avg += v;
      sum_sq += v * v;
    }
    avg /= n_;
    const double avg_sq = avg * avg;
    const double sample_var = std::max((sum_sq - n_ * avg_sq) / (n_ - 1), 1e-6);
    aux_pars_[0] = sample_var <= avg ? 100 * avg_sq : avg_sq / (sample_var - avg);
    aux_pars_set_ = true;
  }
  if (with_aux && !aux_pars_set_) {
    // FindInitialAuxPars, gamma (likelihoods.h:1116-1145): approximate MLE of the shape ignoring the random
    // effects, s = log(mean y e^-F) - mean(log y - F), k = (3 - s + sqrt((s - 3)^2 + 24 s)) / (12 s)
    double log_avg = 0., avg_log = 0.;
    for (int i = 0; i < n_; ++i) {
      const double f = fixed_effects != nullptr ? fixed_effects[i] : 0.;
      log_avg += fixed_effects != nullptr ? yraw[i] / std::exp(f) : yraw[i];
      avg_log += fixed_effects != nullptr ? std::log(yraw[i]) - f : std::log(yraw[i]);
    }
    log_avg = std::log(log_avg / n_);
    avg_log /= n_;
    const double sv = log_avg - avg_log;
    aux_pars_[0] = (3. - sv + std::sqrt((sv - 3.) * (sv - 3.) + 24. * sv)) / (12. * sv);
    aux_pars_set_ = true;
  }
  if (optim_.max_iterations <= 0) {
    num_it_ = 0;
    cov_pars_orig_ = s2;
    cov_pars_initialized_ = true;
    last_cov_pars_ = cov_pars_orig_;
    if (with_coef) {
      beta_ = coef_->ToOriginal(beta_scaled);
      RefreshCoefOffset();
    }
    return;
  }
  if (isettings_.optimizer == "gradient_descent") {
    if (with_coef)
      Fatal("optimizer_cov = 'gradient_descent' together with linear regression covariates is not supported for "
            "likelihood '%s' with grouped random effects by gpboost_amd (use 'lbfgs')", likelihood_.c_str());
    GradientDescentLaplace(s2, with_aux);
    return;
  }
  std::vector<double> x(K);
  for (int k = 0; k < K; ++k) x[k] = std::log(s2[k]);
  x.insert(x.end(), beta_scaled.begin(), beta_scaled.end());
  if (with_aux) x.push_back(std::log(aux_pars_[0]));
  double fx = 0.;
  lap_->ClearModePrevious();
  if (with_coef) {
    coef_->SetF(orig_fixed_effects);
    lap_->KeepDeviceGradF(true);
  }
  GroupedLaplaceObjective obj(this, K, with_aux, p);
  try {
    num_it_ = lbfgs_minimize(obj, x, fx, optim_);
  } catch (...) {
    lap_->KeepDeviceGradF(false);
    throw;
  }
  lap_->KeepDeviceGradF(false);
  for (double v : x)
    if (std::isnan(v) || std::isinf(v))
      Fatal("NaN or Inf occurred in covariance parameter optimization using 'lbfgs' (the reference's nelder_mead "
            "restart is not supported by gpboost_amd)");
  cov_pars_orig_.assign(K, 0.);
  for (int k = 0; k < K; ++k) cov_pars_orig_[k] = std::exp(x[k]);
  if (with_aux) aux_pars_[0] = std::exp(x[K + p]);
  if (with_coef) {   // TransformBackCoef (:1604-1612); the device offset already holds F + X beta at the optimum
    beta_ = coef_->ToOriginal(std::vector<double>(x.begin() + K, x.begin() + K + p));
    RefreshCoefOffset();
  }
  cov_pars_initialized_ = true;
  last_nll_ = fx;
  last_cov_pars_ = cov_pars_orig_;
}

void GroupedModel::GradientDescentLaplace(const std::vector<double>& start, bool with_aux) {
  // OptimLinRegrCoefCovPar's loop without profiling (re_model_template.h:1290-1549), as REModelAMD runs it for the GP
  // Laplace models (optim.cpp): the variances and the auxiliary parameter on the log scale with their own learning
  // rates (AvoidTooLargeLearningRatesCovAuxPars :7539-7560), separate Armijo conditions for both blocks
  // (UpdateCovAuxPars :7850-7990), Nesterov momentum over all of them (ApplyMomentumStep), the Laplace mode continued
  // across evaluations and put back to its previous value after a rejected trial.
  const int nc = re_->K(), na = with_aux ? 1 : 0, P = nc + na;
  std::vector<double> pars = start;
  if (with_aux) pars.push_back(aux_pars_[0]);
  const double kMaxLog = std::log(100.);   // MAX_GRADIENT_UPDATE_LOG_SCALE_
  double lr_cov = isettings_.lr < 0. ? 0.1 : isettings_.lr, lr_aux = lr_cov;   // SetInitialValueLRCov :7505-7521
  const bool nest = isettings_.nesterov;
  if (nest && isettings_.schedule != 0) Fatal("NesterovSchedule: version = %d is not supported ", isettings_.schedule);
  auto sched = [&](int it, double acc) { return it < isettings_.momentum_offset ? 0. : acc; };
  auto eval_nll = [&](const std::vector<double>& v) {
    if (with_aux) SetAuxPars(&v[nc]);
    return EvalLaplace(v.data(), false, GroupedLaplace::Start::kWarm, /*fatal_on_nan=*/false).nll;
  };
  lap_->ClearModePrevious();
  double nll = eval_nll(pars);
  if (!std::isfinite(nll)) Fatal("NaN or Inf occurred in initial approximate negative marginal log-likelihood");
  std::vector<double> after = pars, after_lag1 = pars;
  num_it_ = isettings_.max_iter;
  for (int it = 0; it < isettings_.max_iter; ++it) {
    num_iter_ = it;
    const double nll_lag1 = nll;
    const std::vector<double> pars_lag1 = pars;
    if (with_aux) SetAuxPars(&pars[nc]);
    std::vector<double> g = EvalLaplace(pars.data(), true, GroupedLaplace::Start::kKeep, false).grad;   // at the mode
    if ((int)g.size() < P) Fatal("internal error: the Laplace gradient has %d entries", (int)g.size());
    g.resize(P);
    double mc = 0., ma = 0.;
    for (int k = 0; k < nc; ++k) mc = std::max(mc, std::fabs(g[k]));
    for (int k = nc; k < P; ++k) ma = std::max(ma, std::fabs(g[k]));
    if (mc > 0. && lr_cov > kMaxLog / mc) lr_cov = kMaxLog / mc;
    if (na && ma > 0. && lr_aux > kMaxLog / ma) lr_aux = kMaxLog / ma;
    double dd_c = 0., dd_a = 0., md_c = 0., md_a = 0.;
    for (int k = 0; k < nc; ++k) dd_c -= g[k] * g[k];
    for (int k = nc; k < P; ++k) dd_a -= g[k] * g[k];
    if (nest) {
      for (int k = 0; k < nc; ++k) md_c += g[k] * (std::log(pars[k]) - std::log(after[k]));
      for (int k = nc; k < P; ++k) md_a += g[k] * (std::log(pars[k]) - std::log(after[k]));
    }
    double lc = lr_cov, la = lr_aux, acc = isettings_.acc_rate;
    bool halving = false;
    std::vector<double> np(P);
    for (int ih = 0; ih < 30; ++ih) {   // MAX_NUMBER_LR_SHRINKAGE_STEPS_DEFAULT_
      for (int k = 0; k < P; ++k) np[k] = std::exp(std::log(pars[k]) - (k < nc ? lc : la) * g[k]);
      const double mu = nest ? sched(it, acc) : 0.;
      if (nest) {
        after = np;
        for (int k = 0; k < P; ++k) np[k] = std::exp((mu + 1.) * std::log(after[k]) - mu * std::log(after_lag1[k]));
      }
      nll = eval_nll(np);
      bool ok = nll <= nll_lag1 + 1e-4 * lc * dd_c + 1e-4 * mu * md_c;
      if (na) ok = ok && nll <= nll_lag1 + 1e-4 * la * dd_a + 1e-4 * mu * md_a;
      if (ok) break;
      halving = true;
      lc *= 0.5;
      la *= 0.5;
      acc *= 0.5;
      lap_->ResetModeToPrevious();
    }
    if (halving) {   // permanently decreased for gradient descent (:7978-7979)
      lr_cov = lc;
      lr_aux = la;
    }
    if (nest) after_lag1 = after;
    pars = np;
    bool bad = !std::isfinite(nll);
    for (double v : pars) bad = bad || !std::isfinite(v);
    if (bad) Fatal("NaN or Inf occurred in covariance parameter optimization using 'gradient_descent'");
    bool conv;
    if (isettings_.crit_params) {
      double dn = 0., ln = 0.;
      for (int k = 0; k < P; ++k) {
        dn += (pars[k] - pars_lag1[k]) * (pars[k] - pars_lag1[k]);
        ln += pars_lag1[k] * pars_lag1[k];
      }
      conv = std::sqrt(dn) <= isettings_.delta * std::sqrt(ln);
    } else {
      conv = (nll_lag1 - nll) <= isettings_.delta * std::max(std::fabs(nll_lag1), 1.);
    }
    if (conv) {
      num_it_ = it + 1;
      break;
    }
  }
  cov_pars_orig_.assign(pars.begin(), pars.begin() + nc);
  if (with_aux) aux_pars_[0] = pars[nc];
  cov_pars_initialized_ = true;
  last_nll_ = nll;
  last_cov_pars_ = cov_pars_orig_;
}

void GroupedModel::CalcGradientF(double* y, const double* fixed_effects, bool calc_cov_factor) {
  if (y == nullptr) Fatal("the output array 'y' is NULL");
  if (!y_set_) Fatal("Response variable data has not been set");
  const int K = re_->K();
  if (last_cov_pars_.empty()) {   // InitializeCovParsIfNotDefined (re_model.cpp:1142-1164)
    last_cov_pars_ = cov_pars_initialized_ ? cov_pars_orig_ : std::vector<double>(K, 1. / K);
  }
  SetResponseAndOffset(nullptr, fixed_effects);   // null: the offset stays as it is, as in Predict
  std::vector<double> g(n_);
  const std::vector<double> cp = last_cov_pars_;
  EvalLaplace(cp.data(), true, calc_cov_factor ? GroupedLaplace::Start::kWarm : GroupedLaplace::Start::kKeep, true,
              g.data());
  std::copy(g.begin(), g.end(), y);
}

void GroupedModel::GetLaplaceInfo(int* dims, int* rowptr, int* col, double* diag, double* vals) {
  if (!laplace()) Fatal("GPB_GetGroupedLaplaceInfo: the model has a Gaussian likelihood");
  UseDevice();
  const GroupedRE::View v = re_->view();
  if (dims != nullptr) {
    dims[0] = v.M;
    dims[1] = v.nnz;
  }
  if (rowptr != nullptr) std::copy(v.rowptr_h->begin(), v.rowptr_h->end(), rowptr);
  if (col != nullptr && v.nnz > 0) {
    HIP_CHECK(hipMemcpy(col, v.d_col, sizeof(int) * v.nnz, hipMemcpyDeviceToHost));
  }
  if (diag != nullptr && vals != nullptr) lap_->GetZtWZ(diag, vals);
}

void GroupedModel::PredictLaplace(const double* y, int n_pred, const char* re_group_data_pred, const double* cov_pars,
                                  bool predict_var, bool predict_response, const double* fixed_effects,
                                  const double* fixed_effects_pred, double* out, const double* slope_data_pred) {
  // PredictLaplaceApproxGroupedRE (likelihoods.h:5696-5953) / ...OnlyOneGroupedRECalculationsOnREScale (:5973-6032):
  // latent mean = sum_k mode_k[level] (0 for a level not in the training data); latent variance = sum_k sigma_k^2
  // [level not seen] + e_p^T A^-1 e_p, e_p the indicator of p's seen levels (the posterior covariance of the
  // random effects is A^-1 at the mode); then the likelihood's response moments
  if (n_pred <= 0) Fatal("num_data_pred must be > 0");
  if (re_group_data_pred == nullptr) Fatal("re_group_data_pred must be provided for grouped random effects");
  const int K = re_->K();
  std::vector<int> idx;
  std::vector<double> wt;
  PredComponents(n_pred, re_group_data_pred, slope_data_pred, idx, wt, nullptr);
  const bool wtd = !wt.empty();
  const std::vector<double> cp = LaplaceCovPars(cov_pars);
  if (y != nullptr || fixed_effects != nullptr) SetResponseAndOffset(y, fixed_effects);
  if (!y_set_) Fatal("Response variable data is not provided and has not been set before");
  EvalLaplace(cp.data(), false, GroupedLaplace::Start::kZero, true);
  std::vector<double> b(re_->M());
  lap_->GetMode(b.data());
  std::vector<double> mu(n_pred, 0.);
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < n_pred; ++i) {
      const int a = idx[(size_t)i * K + k];
      if (a >= 0) mu[i] += wtd ? wt[(size_t)i * K + k] * b[a] : b[a];
    }
  for (int i = 0; i < n_pred; ++i) mu[i] += fixed_effects_pred ? fixed_effects_pred[i] : 0.;
  const bool want_var = predict_var || predict_response;
  if (want_var && iterative())
    Fatal("predict_response needs the predictive variances, which for grouped random effects with "
          "matrix_inversion_method = 'iterative' (the reference's simulation-based estimate) are not supported by "
          "gpboost_amd (use 'cholesky' or predict_response = false)");
  std::vector<double> var(n_pred, 0.);
  if (want_var) {
    lap_->PredVar(n_pred, idx, var.data(), wtd ? wt.data() : nullptr);
    for (int i = 0; i < n_pred; ++i)
      for (int k = 0; k < K; ++k)
        if (idx[(size_t)i * K + k] < 0) var[i] += wtd ? cp[k] * wt[(size_t)i * K + k] * wt[(size_t)i * K + k] : cp[k];
  }
  if (predict_response)
    response_transform(lik_, aux_pars_.empty() ? 1. : aux_pars_[0], 0., iter.delta_conv_mode_finding, stream_, n_pred,
                       mu.data(), var.data(), nullptr);
  std::copy(mu.begin(), mu.end(), out);
  if (predict_var) std::copy(var.begin(), var.end(), out + n_pred);
}

// ---- linear regression coefficients of Laplace models (CoefLayer, coef.h)

void GroupedModel::SetOptimizerCoef(const char* optimizer_coef, bool init_coef_given) {
  optimizer_coef_ = optimizer_coef != nullptr && optimizer_coef[0] != '\0' ? optimizer_coef : "lbfgs";
  init_coef_given_ = init_coef_given;
}

void GroupedModel::RefreshCoefOffset() {
  std::vector<double> off(n_);
  coef_->LinearPredictor(beta_.data(), fit_offset_.empty() ? nullptr : fit_offset_.data(), off.data());
  UseDevice();
  lap_->SetOffset(off.data());
}

void GroupedModel::CoefWriteOffset(const double* beta) { coef_->WriteOffset(beta, lap_->DeviceOffset()); }
void GroupedModel::CoefGradient(double* grad_beta) { coef_->Gradient(lap_->DeviceGradF(), grad_beta); }
double GroupedModel::CoefMaxLearningRate(const double* beta, const double* dir) {
  return coef_->MaxLearningRate(beta, dir);
}

void GroupedModel::OptimLinRegrCoefCovPar(const double* y, const double* X, int p, const double* fixed_effects) {
  if (!laplace() || has_gp())
    Fatal("linear regression covariates with grouped random effects are not supported by gpboost_amd");
  if (optimizer_coef_ != "lbfgs")
    Fatal("optimizer_coef = '%s' is not supported for likelihood '%s' with grouped random effects by gpboost_amd "
          "(supported: lbfgs)", optimizer_coef_.c_str(), likelihood_.c_str());
  if (init_coef_given_)
    Fatal("init_coef is not supported for grouped random effects models by gpboost_amd (the coefficients start at 0, "
          "the intercept at the reference's initial value)");
  if (cov_par_index_given_)
    Fatal("estimate_cov_par_index together with linear regression covariates is not supported for grouped random "
          "effects by gpboost_amd");
  if (p > kCoefMaxCols)
    Fatal("num_covariates = %d is not supported for likelihood '%s' with grouped random effects by gpboost_amd (at "
          "most %d)", p, likelihood_.c_str(), kCoefMaxCols);
  UseDevice();
  beta_.clear();
  coef_.reset(new CoefLayer(n_, p, X, lap_->stream()));
  try {
    OptimCovParLaplace(y, fixed_effects, /*with_coef=*/true);
  } catch (...) {
    beta_.clear();
    coef_.reset();
    throw;
  }
}

void GroupedModel::GetCovariateData(double* out) const {
  if (coef_ == nullptr) Fatal("Model does not have covariates for a linear predictor");
  std::copy(coef_->X_colmajor().begin(), coef_->X_colmajor().end(), out);
}

void GroupedModel::AddLinearPredictor(const double* X_pred, int n_pred, double* mean_add) const {
  if (!has_covariates()) Fatal("Model does not have covariates for a linear predictor");
  for (int j = 0; j < coef_->p(); ++j)
    for (int i = 0; i < n_pred; ++i) mean_add[i] += X_pred[(size_t)j * n_pred + i] * beta_[j];
}

double GroupedModel::EvalGradCoef(const double* cov_pars, const double* aux, const double* coef, const double* y,
                                  const double* X, int p, const double* fixed_effects, double* grad_cov,
                                  double* grad_aux, double* grad_coef) {
  if (!laplace() || has_gp())
    Fatal("GPB_EvalNegLogLikelihoodGradCoef: the model needs grouped random effects with a non-Gaussian likelihood");
  if (cov_pars == nullptr || coef == nullptr || X == nullptr) Fatal("GPB_EvalNegLogLikelihoodGradCoef: NULL argument");
  if (p > kCoefMaxCols)
    Fatal("num_covariates = %d is not supported for likelihood '%s' with grouped random effects by gpboost_amd (at "
          "most %d)", p, likelihood_.c_str(), kCoefMaxCols);
  const int K = re_->K();
  const std::vector<double> cp = LaplaceCovPars(cov_pars);
  UseDevice();
  if (y != nullptr) {   // the response alone: the offset is written on the device below
    for (int i = 0; i < n_; ++i)
      if (std::isnan(y[i]) || std::isinf(y[i])) Fatal("NaN or Inf in response variable / label ");
    y_raw_.assign(y, y + n_);
    lap_->SetY(y_raw_.data());
    y_set_ = true;
  }
  if (!y_set_) Fatal("response variable y has not been set");
  if (aux != nullptr && !aux_pars_.empty()) {
    if (!(aux[0] > 0.)) Fatal("aux_pars must be > 0");
    SetAuxPars(aux);
  }
  CoefLayer layer(n_, p, X, lap_->stream(), /*transform=*/false);
  layer.SetF(fixed_effects);
  EvalResult r;
  try {
    layer.WriteOffset(coef, lap_->DeviceOffset());
    lap_->KeepDeviceGradF(true);
    r = EvalLaplace(cp.data(), true, GroupedLaplace::Start::kZero, true);
    layer.Gradient(lap_->DeviceGradF(), grad_coef);
  } catch (...) {
    lap_->KeepDeviceGradF(false);
    if (has_covariates()) RefreshCoefOffset();
    throw;
  }
  lap_->KeepDeviceGradF(false);
  if (grad_cov != nullptr)
    for (int k = 0; k < K; ++k) grad_cov[k] = r.grad[k];
  if (grad_aux != nullptr && (int)r.grad.size() > K) grad_aux[0] = r.grad[K];
  last_cov_pars_ = cp;
  if (has_covariates()) RefreshCoefOffset();   // the model's own offset again
  return r.nll;
}

void GroupedModel::GetCoef(double* out, bool calc_std_dev) {
  if (!has_covariates()) Fatal("Model does not have covariates for a linear predictor");
  const int p = coef_->p();
  std::copy(beta_.begin(), beta_.end(), out);
  if (!calc_std_dev) return;
  if (iterative())
    Fatal("standard deviations of the regression coefficients (std_err) for matrix_inversion_method = 'iterative' are "
          "not supported by gpboost_amd (use 'cholesky')");
  // CalcStdDevCoefNonGaussian (re_model_template.h:9825-9854): H = Jacobian of grad_beta by central differences with
  // step beta_i eps^(1/3) on the unscaled X, symmetrised; sd = sqrt(diag(H^-1))
  UseDevice();
  const std::vector<double> cp = LaplaceCovPars(nullptr);
  CoefLayer layer(n_, p, coef_->X_colmajor().data(), lap_->stream(), /*transform=*/false);
  layer.SetF(fit_offset_.empty() ? nullptr : fit_offset_.data());
  const double eps3 = std::cbrt(std::numeric_limits<double>::epsilon());
  std::vector<double> H((size_t)p * p), gp(p), gm(p);
  const double nll_fit = last_nll_;   // the evaluations below are not the model's current likelihood
  lap_->KeepDeviceGradF(true);
  try {
    for (int i = 0; i < p; ++i) {
      const double step = beta_[i] * eps3;
      std::vector<double> b = beta_;
      b[i] = beta_[i] + step;
      layer.WriteOffset(b.data(), lap_->DeviceOffset());
      EvalLaplace(cp.data(), true, GroupedLaplace::Start::kWarm, true);
      layer.Gradient(lap_->DeviceGradF(), gp.data());
      b[i] = beta_[i] - step;
      layer.WriteOffset(b.data(), lap_->DeviceOffset());
      EvalLaplace(cp.data(), true, GroupedLaplace::Start::kWarm, true);
      layer.Gradient(lap_->DeviceGradF(), gm.data());
      for (int j = 0; j < p; ++j) H[(size_t)i * p + j] = (gp[j] - gm[j]) / (2. * step);
    }
  } catch (...) {
    lap_->KeepDeviceGradF(false);
    throw;
  }
  lap_->KeepDeviceGradF(false);
  last_nll_ = nll_fit;
  RefreshCoefOffset();
  std::vector<double> S((size_t)p * p), inv((size_t)p * p, 0.);
  for (int i = 0; i < p; ++i)
    for (int j = 0; j < p; ++j) S[(size_t)i * p + j] = 0.5 * (H[(size_t)i * p + j] + H[(size_t)j * p + i]);
  // Hsym.inverse(): Gauss-Jordan with partial pivoting on the small p x p matrix
  for (int i = 0; i < p; ++i) inv[(size_t)i * p + i] = 1.;
  for (int c = 0; c < p; ++c) {
    int piv = c;
    for (int r = c + 1; r < p; ++r)
      if (std::fabs(S[(size_t)r * p + c]) > std::fabs(S[(size_t)piv * p + c])) piv = r;
    const double d = S[(size_t)piv * p + c];
    if (!(d != 0.) || !std::isfinite(d)) Fatal("the numerical Hessian of the regression coefficients is singular");
    for (int j = 0; j < p; ++j) {
      std::swap(S[(size_t)c * p + j], S[(size_t)piv * p + j]);
      std::swap(inv[(size_t)c * p + j], inv[(size_t)piv * p + j]);
    }
    for (int j = 0; j < p; ++j) {
      S[(size_t)c * p + j] /= d;
      inv[(size_t)c * p + j] /= d;
    }
    for (int r = 0; r < p; ++r) {
      if (r == c) continue;
      const double f = S[(size_t)r * p + c];
      for (int j = 0; j < p; ++j) {
        S[(size_t)r * p + j] -= f * S[(size_t)c * p + j];
        inv[(size_t)r * p + j] -= f * inv[(size_t)c * p + j];
      }
    }
  }
  for (int i = 0; i < p; ++i) out[p + i] = std::sqrt(inv[(size_t)i * p + i]);
}

}  // namespace gpb_amd
