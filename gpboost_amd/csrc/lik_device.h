// Per-sample log-likelihood, its first derivative, the information (negative second derivative) and
// the information's derivative wrt the location parameter, for the latent (Laplace) likelihoods.
//   gaussian        likelihoods.h :8795, 9263, 9937 (aux = error variance)
//   bernoulli_logit likelihoods.h :8724, 9226, 9896, 10187; sigmoid_stable / softplus DF_utils.h:37-60
//   bernoulli_probit :8708, 9208, 9871, 10171;  poisson :8730, 9230, 9904, 10200
//   gamma           :8740, 9234, 9908, 10228 (aux = shape; log link, the normalizing constant on the host)
//   negative_binomial (grouped random effects only): the nb_* functions at the end, not dispatched by lik_*
// Shared by every Laplace path: sparse Vecchia (sparse_kernels.hip, lowrank_precond.hip), sparse Cholesky
// (sparse_chol.hip), FITC (fitc_laplace.hip), full-scale Vecchia (vif_laplace.hip), dense (dense_laplace.hip) and
// grouped (grouped_laplace.hip), and by the logit response mean of latent_pred.hip. Tested point by point through
// GPB_TestLikPoint / GPB_TestLikPath (lik_test.cpp) against the bounds of tests/lik_cases.py.
#pragma once

#include <hip/hip_runtime.h>

#include "latent_kernels.h"

namespace gpb_amd {

__device__ __forceinline__ double sigmoid_stable(double x) {
  if (x >= 0.) {
    const double e = exp(-x);
    return 1. / (1. + e);
  }
  const double e = exp(x);
  return e / (1. + e);
}
__device__ __forceinline__ double softplus(double x) { return log1p(exp(-fabs(x))) + fmax(x, 0.); }

// DF_utils.h:62-104: normal log-CDF with its tails, inverse Mills ratios phi / Phi and phi / (1 - Phi)
__device__ __forceinline__ double normal_log_pdf(double x) { return -x * x / 2. - 0.91893853320467274178; }
// Left tail: erfc up to u = -x = kProbitSeriesFrom, where erfc(u / sqrt 2) ~ 6e-300 is still a normal number (it is
// a denormal with a few bits left from u ~ 37.6 on, and whether a libm returns, flushes or zeroes those differs);
// past it the asymptotic series Phi(-u) = phi(u) / u (1 - 1/u^2 + 3/u^4 - ... + 10395/u^12), whose first dropped
// term 135135 / u^14 is below 2e-17 there. The threshold is a constant, so host and device take the same branch.
constexpr double kProbitSeriesFrom = 37.;
__device__ __forceinline__ double normal_log_cdf(double x) {
  if (x < 0.) {
    const double u = -x;
    if (u <= kProbitSeriesFrom) return -0.69314718055994530942 + log(erfc(u * 0.70710678118654752440));
    const double u2 = u * u, v = 1. / u2;
    const double series = 1. + v * (-1. + v * (3. + v * (-15. + v * (105. + v * (-945. + v * 10395.)))));
    return -0.5 * u2 - log(u) - 0.5 * log(2. * 3.14159265358979323846) + log(series);
  }
  const double Q = 0.5 * erfc(x * 0.70710678118654752440);
  if (Q == 0.) return 0.;
  return log1p(-Q);
}
__device__ __forceinline__ double mills_phi(double x) { return exp(normal_log_pdf(x) - normal_log_cdf(x)); }
__device__ __forceinline__ double mills_one_minus_phi(double x) { return exp(normal_log_pdf(x) - normal_log_cdf(-x)); }

// log-likelihood without the normalizing constant (the Poisson -log y! is added on the host)
__device__ __forceinline__ double lik_loglik(int lik, double aux, double y, double l) {
  if (lik == kLikGaussian) {
    const double r = y - l;
    return -r * r / 2. / aux - 0.91893853320467274178 - 0.5 * log(aux);   // M_LOGSQRT2PI
  }
  if (lik == kLikBernoulliProbit) return y == 0. ? normal_log_cdf(-l) : normal_log_cdf(l);   // :8708-8715
  if (lik == kLikPoisson) return y * l - exp(l);                                              // :8730-8737
  if (lik == kLikGamma) return -aux * (l + y * exp(-l));                                      // :8740-8748
  // bernoulli_logit: y l - softplus(l) cancels for y = 1, l >> 0; log p and log (1 - p) directly do not
  if (y == 1.) return -softplus(-l);
  if (y == 0.) return -softplus(l);
  return y * l - softplus(l);
}
__device__ __forceinline__ double lik_d1(int lik, double aux, double y, double l) {
  if (lik == kLikGaussian) return (y - l) / aux;
  if (lik == kLikBernoulliProbit) return y == 0. ? -mills_one_minus_phi(l) : mills_phi(l);    // :9208-9215
  if (lik == kLikPoisson) return y - exp(l);                                                  // :9230-9232
  if (lik == kLikGamma) return aux * (y * exp(-l) - 1.);                                      // :9234-9236
  if (y == 1.) return sigmoid_stable(-l);   // 1 - p without the cancellation at l >> 0
  return y - sigmoid_stable(l);
}
// information (negative second derivative), likelihoods.h:9871-9906
__device__ __forceinline__ double lik_info(int lik, double aux, double y, double l) {
  if (lik == kLikGaussian) return 1. / aux;
  if (lik == kLikBernoulliProbit) {
    if (y == 0.) {
      const double r = mills_one_minus_phi(l);
      return -r * (l - r);
    }
    const double r = mills_phi(l);
    return r * (l + r);
  }
  if (lik == kLikPoisson) return exp(l);
  if (lik == kLikGamma) return aux * y * exp(-l);   // :9908-9910
  // p q with q = 1 - p = sigmoid(-l) computed on its own: p (1. - p) loses q's digits for l >> 0 (it is 0 from
  // l = 37 on) and is not even in l
  return sigmoid_stable(l) * sigmoid_stable(-l);
}
// derivative of the information wrt the location parameter, likelihoods.h:10165-10195
__device__ __forceinline__ double lik_dinfo(int lik, double aux, double y, double l) {
  if (lik == kLikGaussian) return 0.;
  if (lik == kLikGamma) return -aux * y * exp(-l);   // :10228-10233
  if (lik == kLikBernoulliProbit) {
    const double x2 = l * l;
    if (y == 0.) {
      const double r = mills_one_minus_phi(l);
      return -r * (1. - x2 + r * (3. * l - 2. * r));
    }
    const double r = mills_phi(l);
    return -r * (x2 - 1. + r * (3. * l + 2. * r));
  }
  if (lik == kLikPoisson) return exp(l);
  const double p = sigmoid_stable(l), q = sigmoid_stable(-l);
  return -p * q * (p - q);
}

// negative_binomial (aux = shape r, log link, mu = e^l; the normalizing constant on the host): likelihoods.h :8750,
// :10241, shape derivatives :10872-10885, explicit shape gradient :10527-10538. Grouped random effects only, so
// these are functions of their own (called by grouped_laplace.hip and the point kernel) and the lik_* dispatchers
// above stay as they are. Everything goes through t = l - log r, p = sigmoid(t) = mu / (mu + r) and q = sigmoid(-t)
// = r / (mu + r), each computed on its own: e^l overflows from l = 709.8 and mu / (mu + r) has no digit of q left
// for l >> log r. log_r = log(r), computed once by the caller.
// log-likelihood: y l - (y + r) log(mu + r) with l - log(mu + r) = -softplus(-t): two terms that do not cancel
__device__ __forceinline__ double nb_loglik(double r, double log_r, double y, double l) {
  const double t = l - log_r;
  return -y * softplus(-t) - r * (log_r + softplus(t));
}
// y - (y + r) p = y q - r p
__device__ __forceinline__ double nb_d1(double r, double log_r, double y, double l) {
  const double t = l - log_r;
  return y * sigmoid_stable(-t) - r * sigmoid_stable(t);
}
__device__ __forceinline__ double nb_info(double r, double log_r, double y, double l) {
  const double t = l - log_r;
  return (y + r) * (sigmoid_stable(t) * sigmoid_stable(-t));
}
__device__ __forceinline__ double nb_dinfo(double r, double log_r, double y, double l) {
  const double t = l - log_r;
  const double p = sigmoid_stable(t), q = sigmoid_stable(-t);
  return -(y + r) * (p * q) * (p - q);
}
// d d1 / dlog r = p q (y - mu), with (y - mu) q = y q - r p (mu q = r p)
__device__ __forceinline__ double nb_dd1_aux(double r, double log_r, double y, double l) {
  const double t = l - log_r;
  const double p = sigmoid_stable(t), q = sigmoid_stable(-t);
  return p * (y * q - r * p);
}
// d info / dlog r as the reference has it, -p q (y (r - mu) - 2 r mu) / (y + r), with q (r - mu) = r (q - p) and
// q mu = r p
__device__ __forceinline__ double nb_dinfo_aux(double r, double log_r, double y, double l) {
  const double t = l - log_r;
  const double p = sigmoid_stable(t), q = sigmoid_stable(-t);
  return -(p * r) * (y * (q - p) - 2. * (r * p)) / (y + r);
}
// log(mu + r) + (y + r) / (mu + r), the per-observation part of the explicit shape gradient
__device__ __forceinline__ double nb_aux_term(double r, double log_r, double y, double l) {
  const double t = l - log_r;
  return log_r + softplus(t) + (y + r) * sigmoid_stable(-t) / r;
}

}  // namespace gpb_amd
