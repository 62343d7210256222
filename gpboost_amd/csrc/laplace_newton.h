// The host rules every Laplace driver shares (DenseLaplace, FitcLaplace, VifLaplace, GroupedLaplace and the three
// LatentVecchia evaluations): the constants of the Newton mode finding, one Armijo backtracking line search with
// the reference's convergence rule, and the gamma-shape gradient. Host only, header only.
#pragma once

#include <cmath>

namespace gpb_amd {

constexpr int kMaxItModeNewton = 1000;   // maxit_mode_newton_ (likelihoods.h:12721)
constexpr int kMaxShrinkNewton = 20;     // max_number_lr_shrinkage_steps_newton_ (likelihoods.h:12725)
constexpr double kCArmijo = 1e-4;        // c_armijo_ (likelihoods.h:12737)

struct LineSearchResult {
  double obj_new;   // objective of the last trial evaluated
  double lam;       // its learning rate
  int trials;
  bool terminate;   // the mode finding has converged
  bool nan;         // obj_new is NaN or Inf: the caller reports the failure, terminate is false
};

// One Newton step's backtracking (likelihoods.h:1910-1928) and CheckConvergenceModeFinding (:11820-11870) at
// iteration it, from the objective obj with the slope gdd = grad_dot_direction. trial(lam, ih) builds the trial
// state of shrink step ih at learning rate lam and returns its objective; the last trial is kept when none is
// accepted. The caller swaps its buffers and counts the iteration.
template <class Trial>
LineSearchResult newton_line_search(int it, double obj, double gdd, double delta, int max_shrink, Trial&& trial) {
  LineSearchResult r{obj, 1., 0, false, false};
  double lam = 1.;
  for (int ih = 0; ih < max_shrink; ++ih) {
    r.lam = lam;
    r.obj_new = trial(lam, ih);
    ++r.trials;
    if (r.obj_new < obj + kCArmijo * lam * gdd || std::isnan(r.obj_new) || std::isinf(r.obj_new)) lam *= 0.5;
    else break;
  }
  r.nan = std::isnan(r.obj_new) || std::isinf(r.obj_new);
  if (!r.nan)
    r.terminate = it == 0 ? std::abs(r.obj_new - obj) < delta * std::abs(obj) : (r.obj_new - obj) < delta * std::abs(obj);
  return r;
}

// digamma by the asymptotic expansion after recurrence to x >= 8.5 (Bernardo 1976, Algorithm AS 103; the form the
// reference's GPBoost::digamma uses, DF_utils.cpp:82-123)
inline double digamma_asa103(double x) {
  if (x <= 0.000001) return -0.57721566490153286060 - 1.0 / x + 1.6449340668482264365 * x;
  double value = 0., x2 = x;
  while (x2 < 8.5) {
    value = value - 1.0 / x2;
    x2 = x2 + 1.0;
  }
  double r = 1.0 / x2;
  value = value + std::log(x2) - 0.5 * r;
  r = r * r;
  return value - r * (1.0 / 12.0 - r * (1.0 / 120.0 - r * (1.0 / 252.0 - r * (1.0 / 240.0 - r * (1.0 / 132.0)))));
}

// d nll / d log(shape) of likelihood 'gamma' (likelihoods.h:10508-10524 with the two trace terms, :3379-3411):
// s0 = sum (l + y e^-l), s1 = sum W_i diag((Sigma^-1 + W)^-1)_i, s2 = sum d1_i ((Sigma^-1 + W)^-1 d_mll_d_mode)_i
inline double gamma_shape_grad(double a, int n, double s0, double s1, double s2, double sum_log_y) {
  return a * (s0 - n * (std::log(a) + 1. - digamma_asa103(a)) - sum_log_y) + 0.5 * s1 + s2;
}

}  // namespace gpb_amd
