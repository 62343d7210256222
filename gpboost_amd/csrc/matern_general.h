// Matern covariance with a general smoothness nu > 0 (cov_fcts.h:1701-1715 CovarianceMaternGeneralShape): what
// depends on nu alone, computed once per model on the host and passed to the kernels by value. The evaluation
// (cov.h, matern_general) then needs no gamma function on the device.
//
// The evaluation returns the covariance and its range derivative from K_{nu-1} and K_nu, which one Temme / Steed
// evaluation at an order |mu| <= 1/2 and nrec upward recurrence steps give together:
//   nu >= 1/2: nu - 1 = mu + nrec, the pair (K_mu, K_{mu+1}) is stepped up nrec times to (K_{nu-1}, K_nu);
//   nu <  1/2: mu = -nu, and (K_mu, K_{mu+1}) = (K_nu, K_{1-nu}) = (K_nu, K_{nu-1}) as it stands (low).
#pragma once

#include <cmath>

namespace gpb_amd {

struct MaternGeneralPars {
  double nu;
  double mu;           // the order of the Temme / Steed evaluation, |mu| <= 1/2
  double gam_p, gam_m; // Gamma(1 + mu), Gamma(1 - mu)
  double gam1, gam2;   // Temme: (1/Gamma(1 - mu) - 1/Gamma(1 + mu)) / (2 mu), (1/Gamma(1 - mu) + 1/Gamma(1 + mu)) / 2
  double fact;         // pi mu / sin(pi mu)
  double cc;           // 2 / Gamma(nu):  c = var cc (x/2)^nu K_nu(x)
  double cd;           // 1 / Gamma(nu): dc = -var cd x^2 (x/2)^(nu-1) K_{nu-1}(x)
  int nrec;            // upward recurrence steps
  int low;             // nu < 1/2
};

// The largest shape served: the recurrence runs nrec = nu - 1 steps per evaluation and Gamma(nu) must be finite; a
// Matern model this smooth is the Gaussian covariance for every practical purpose.
constexpr double kMaternGeneralMaxShape = 100.;

// Taylor coefficients of 1 / Gamma(1 + z) at 0 (Abramowitz & Stegun 6.1.34, to 20 digits): with them gam1 has no
// cancellation at and near integer nu (mu -> 0), where the quotient form loses every digit.
inline MaternGeneralPars matern_general_pars(double nu) {
  static const double g[31] = {1.0,
                               0.57721566490153286061,
                               -0.65587807152025388108,
                               -0.042002635034095235529,
                               0.1665386113822914895,
                               -0.042197734555544336748,
                               -0.0096219715278769735621,
                               0.0072189432466630995424,
                               -0.0011651675918590651121,
                               -0.00021524167411495097282,
                               0.00012805028238811618615,
                               -0.000020134854780788238656,
                               -1.2504934821426706573e-6,
                               1.1330272319816958824e-6,
                               -2.0563384169776071035e-7,
                               6.1160951044814158179e-9,
                               5.0020076444692229301e-9,
                               -1.1812745704870201446e-9,
                               1.0434267116911005105e-10,
                               7.782263439905071254e-12,
                               -3.6968056186422057082e-12,
                               5.100370287454475979e-13,
                               -2.0583260535665067832e-14,
                               -5.3481225394230179824e-15,
                               1.2267786282382607902e-15,
                               -1.1812593016974587695e-16,
                               1.1866922547516003326e-18,
                               1.4123806553180317816e-18,
                               -2.2987456844353702066e-19,
                               1.7144063219273374334e-20,
                               1.3373517304936931149e-22};
  MaternGeneralPars p{};
  p.nu = nu;
  p.low = nu < 0.5 ? 1 : 0;
  if (p.low) {
    p.nrec = 0;
    p.mu = -nu;
  } else {
    p.nrec = (int)std::floor(nu - 0.5);
    p.mu = nu - 1. - p.nrec;
  }
  const double mu = p.mu, mu2 = mu * mu;
  double even = 0., odd = 0.;   // sum of g_j mu^j over even j, of g_j mu^(j-1) over odd j (Horner in mu^2)
  for (int j = 30; j >= 0; j -= 2) even = even * mu2 + g[j];
  for (int j = 29; j >= 1; j -= 2) odd = odd * mu2 + g[j];
  p.gam2 = even;
  p.gam1 = -odd;
  p.gam_p = 1. / (even + mu * odd);
  p.gam_m = 1. / (even - mu * odd);
  const double pimu = M_PI * mu;
  p.fact = std::fabs(pimu) < 1e-8 ? 1. : pimu / std::sin(pimu);
  p.cd = 1. / std::tgamma(nu);
  p.cc = 2. * p.cd;
  return p;
}

}  // namespace gpb_amd
