// Covariance kernels and their derivatives on the reference's transformed scale,
// shared by host and device code.
//   C(r)       : cov_fcts.h:1681-1745 (CovarianceMaternShape0_5 / 1_5 / 2_5, CovarianceGaussian)
//   dC/dlog phi: cov_fcts.h:1750-1786 (DetermineConstantsForGradient, transf_scale=true)
//                and :2116-2143 (GradientRangeMaternShape*, GradientRangeGaussian)
//   parameters : var = sigma1^2 / sigma2, phi = range transform (cov_fcts.h:438-460)
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.h"
#include "matern_general.h"

namespace gpb_amd {

// kMaternGeneral (any smoothness nu > 0, matern_general below) is served by the kernels that name it; dispatch_cov
// does not reach it, so the other engines refuse it instead of instantiating it everywhere.
enum CovType : int { kMatern05 = 0, kMatern15 = 1, kMatern25 = 2, kGaussian = 3, kMaternGeneral = 4 };

// f(std::integral_constant<int, cov>{}): the host's switch from a runtime covariance type to a template argument
template <typename F>
void dispatch_cov(int cov, F&& f) {
  switch (cov) {
    case kMatern05: f(std::integral_constant<int, kMatern05>{}); break;
    case kMatern15: f(std::integral_constant<int, kMatern15>{}); break;
    case kMatern25: f(std::integral_constant<int, kMatern25>{}); break;
    case kGaussian: f(std::integral_constant<int, kGaussian>{}); break;
    default: Fatal("unsupported covariance type %d", cov);
  }
}

template <int COV>
__host__ __device__ __forceinline__ void cov_dcov(double r, double var, double phi, double& c, double& dc) {
  if constexpr (COV == kMatern05) {
    const double e = exp(-phi * r);
    c = var * e;
    dc = -phi * r * c;
  } else if constexpr (COV == kMatern15) {
    const double x = phi * r;
    const double e = exp(-x);
    c = var * (1. + x) * e;
    dc = -var * x * x * e;
  } else if constexpr (COV == kMatern25) {
    const double x = phi * r;
    const double e = exp(-x);
    c = var * (1. + x + x * x / 3.) * e;
    dc = -var * x * x / 3. * (1. + x) * e;
  } else {
    const double e = exp(-phi * r * r);
    c = var * e;
    dc = -phi * r * r * c;
  }
}

// ---- device forms for the row kernels: the same operation sequences as the ROCm device library's
// sqrt and exp (so the same bits on their common range), minus the range handling these arguments
// never need. sqrt: no denormal rescaling (squared distances are 0 or far above 2^-767; 0 gives 0
// exactly: the rsq seed is taken of max(s, 1e-300) and every refinement uses s itself). exp: the
// argument is <= 0 (no overflow branch); it is clamped at -1075, below which the result is 0 either
// way (2^-1551 after the final ldexp), replacing the underflow compare-and-selects.
__device__ __forceinline__ double sqrt_nonneg(double s) {
  const double y0 = __builtin_amdgcn_rsq(fmax(s, 1e-300));
  double g = s * y0;
  double h = y0 * 0.5;
  const double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  double e = fma(-g, g, s);
  h = fma(h, r, h);
  g = fma(e, h, g);
  e = fma(-g, g, s);
  return fma(e, h, g);
}

// exp's constants that no instruction can take as an inline operand: log2(e), ln 2 (high, low) and the
// polynomial's coefficients. A kernel short of VGPRs passes a copy it holds in scalar registers
// (ExpCoef::scalar()), so they are not re-materialised by 64-bit VALU moves at every evaluation.
struct ExpCoef {
  double log2e = 0x1.71547652b82fep+0, ln2hi = -0x1.62e42fefa39efp-1, ln2lo = -0x1.abc9e3b39803fp-56;
  double c[10] = {0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22, 0x1.71dee623fde64p-19, 0x1.a01997c89e6b0p-16,
                  0x1.a01a014761f6ep-13, 0x1.6c16c1852b7b0p-10, 0x1.1111111122322p-7,  0x1.55555555502a1p-5,
                  0x1.5555555555511p-3,  0x1.000000000000bp-1};
  __device__ __forceinline__ static ExpCoef scalar() {
    ExpCoef k;
    asm volatile("" : "+s"(k.log2e), "+s"(k.ln2hi), "+s"(k.ln2lo));
#pragma unroll
    for (int q = 0; q < 10; ++q) asm volatile("" : "+s"(k.c[q]));
    return k;
  }
};

__device__ __forceinline__ double exp_nonpos(double x, const ExpCoef& k = ExpCoef{}) {
  x = fmax(x, -1075.);
  const double n = __builtin_rint(x * k.log2e);
  double t = fma(k.ln2hi, n, x);
  t = fma(k.ln2lo, n, t);
  double p = fma(k.c[0], t, k.c[1]);
#pragma unroll
  for (int q = 2; q < 10; ++q) p = fma(t, p, k.c[q]);
  p = fma(t, p, 1.);
  p = fma(t, p, 1.);
  return __builtin_amdgcn_ldexp(p, (int)n);
}

// cov_dcov on the distance with the device exp above (identical formulas)
template <int COV>
__device__ __forceinline__ void cov_dcov_r(double r, double var, double phi, double& c, double& dc,
                                           const ExpCoef& k = ExpCoef{}) {
  if constexpr (COV == kMatern05) {
    const double e = exp_nonpos(-phi * r, k);
    c = var * e;
    dc = -phi * r * c;
  } else if constexpr (COV == kMatern15) {
    const double x = phi * r;
    const double e = exp_nonpos(-x, k);
    c = var * (1. + x) * e;
    dc = -var * x * x * e;
  } else if constexpr (COV == kMatern25) {
    const double x = phi * r;
    const double e = exp_nonpos(-x, k);
    c = var * (1. + x + x * x / 3.) * e;
    dc = -var * x * x / 3. * (1. + x) * e;
  } else {
    const double e = exp_nonpos(-phi * r * r, k);
    c = var * e;
    dc = -phi * r * r * c;
  }
}

// ... and on the squared distance: the device sqrt, then the form above
template <int COV>
__device__ __forceinline__ void cov_dcov_sq(double s, double var, double phi, double& c, double& dc,
                                            const ExpCoef& k = ExpCoef{}) {
  cov_dcov_r<COV>(sqrt_nonneg(s), var, phi, c, dc, k);
}

// ---- Matern with a general smoothness (cov_fcts.h:1701-1715, range gradient :2153-2163 with transf_scale = true).
// With x = phi r, phi = sqrt(2 nu) / rho:
//   c  = var 2^(1-nu) / Gamma(nu) x^nu K_nu(x)
//   dc = dc / dlog(phi) = -var 2^(1-nu) / Gamma(nu) x^(nu+1) K_{nu-1}(x)
// (the reference's x^nu (2 nu K_nu - x K_{nu+1}) is the same number, but cancels to nothing for small x). K_mu and
// K_{mu+1} at the order |mu| <= 1/2 of MaternGeneralPars come from Temme's series for x <= 2 (accurate at and near
// mu = 0, where the two-series form cancels) and from Steed's continued fraction CF2 with the factor exp(-x) kept
// apart for x > 2 (Temme 1975; Thompson & Barnett 1987; Numerical Recipes 6.7). The upward recurrence runs on
// kappa_o = (x/2)^o K_o(x), kappa_{o+1} = (x/2)^2 kappa_{o-1} + o kappa_o, which tends to Gamma(o) / 2 for x -> 0:
// nothing overflows for x >= 1e-150 (smaller arguments are evaluated there; x <= 0 gives (var, 0), NaN gives NaN).
// For x > 2 the factor exp(-x) is applied as exp(-x/2) twice, once before the recurrence and once after it: the
// recurrence then grows values of at most (x/2)^nu exp(-x/2) <= 1e157 (nu <= 100), so nothing overflows, and the
// result underflows to 0 only where the covariance itself is below 1e-290 (exp(-x/2) = 0 needs x > 1489). Loops run until every active lane of the wave has converged, with the
// converged lanes predicated; a NaN argument ends them at once.
#if defined(__HIP_DEVICE_COMPILE__)
#define GPB_MG_ANY(b) (__builtin_amdgcn_ballot_w64(b) != 0)
#define GPB_MG_EXPM(x) exp_nonpos(x)
#else
#define GPB_MG_ANY(b) (b)
#define GPB_MG_EXPM(x) exp(x)
#endif
__host__ __device__ inline void matern_general(double x, double var, const MaternGeneralPars& p, double& c, double& dc) {
  constexpr double kEps = 1e-16;
  const double xs = fmax(x, 1e-150);
  const double xh = 0.5 * xs;
  const double mu = p.mu, mu2 = mu * mu;
  const double e = -mu * log(xh);
  const double ee = exp(e);   // (x/2)^-mu
  double k0, k1, E;           // K_mu / E, K_{mu+1} / E with E = 1 (x <= 2) or exp(-x/2)
  if (xs <= 2.) {
    const double d = -log(xh);
    const double fact2 = fabs(e) < 1e-8 ? 1. : sinh(e) / e;
    double ff = p.fact * (p.gam1 * 0.5 * (ee + 1. / ee) + p.gam2 * fact2 * d);
    double sum = ff, pp = 0.5 * ee * p.gam_p, qq = 0.5 * p.gam_m / ee;
    double sum1 = pp, cf = 1.;
    const double d2 = xh * xh;
    bool done = false;
    for (int it = 1; it <= 64 && GPB_MG_ANY(!done); ++it) {
      const double fi = it;
      const double ffn = (fi * ff + pp + qq) / (fi * fi - mu2);
      const double cn = cf * d2 / fi, ppn = pp / (fi - mu), qqn = qq / (fi + mu);
      const double del = cn * ffn, del1 = cn * (ppn - fi * ffn);
      if (!done) {
        ff = ffn; cf = cn; pp = ppn; qq = qqn;
        sum += del;
        sum1 += del1;
        done = !(fabs(del) >= fabs(sum) * kEps);
      }
    }
    k0 = sum;
    k1 = sum1 / xh;
    E = 1.;
  } else {
    double b = 2. * (1. + xs), d = 1. / b, h = d, delh = d, q1 = 0., q2 = 1.;
    const double a1 = 0.25 - mu2;
    double q = a1, cq = a1, a = -a1, s = 1. + q * delh;
    bool done = false;
    for (int it = 2; it <= 500 && GPB_MG_ANY(!done); ++it) {
      const double an = a - 2. * (it - 1);
      const double cn = -an * cq / it;
      const double qnew = (q1 - b * q2) / an;
      const double qn = q + cn * qnew;
      const double bn = b + 2.;
      const double dn = 1. / (bn + an * d);
      const double delhn = (bn * dn - 1.) * delh;
      const double dels = qn * delhn;
      if (!done) {
        a = an; cq = cn; q1 = q2; q2 = qnew; q = qn; b = bn; d = dn; delh = delhn;
        h += delhn;
        s += dels;
        done = !(fabs(dels) >= fabs(s) * kEps);
      }
    }
    h = a1 * h;
    E = GPB_MG_EXPM(-0.5 * xs);
    k0 = sqrt(M_PI / (2. * xs)) / s * E;
    k1 = k0 * (mu + xs + 0.5 - h) / xs;
  }
  double ka, kb;   // kappa_{nu-1}, kappa_nu (both over E)
  if (p.low) {
    kb = k0 * ee;
    ka = k1 * ee / xh;
  } else {
    ka = k0 / ee;
    kb = k1 * xh / ee;
    const double d2 = xh * xh;
    for (int j = 0; j < p.nrec; ++j) {   // the same for every lane
      const double t = fma(d2, ka, (mu + 1. + j) * kb);
      ka = kb;
      kb = t;
    }
  }
  const double cv = var * p.cc * kb * E, dv = -var * p.cd * (xs * ka) * xs * E;
  c = x > 0. ? cv : (x <= 0. ? var : x);   // a NaN argument stays NaN, as in the closed forms
  dc = x > 0. ? dv : (x <= 0. ? 0. : x);
}
#undef GPB_MG_ANY
#undef GPB_MG_EXPM

// What a kernel instantiated for COV carries beside (var, phi): nothing for the closed forms
struct NoShape {};
template <int COV>
using CovShape = std::conditional_t<COV == kMaternGeneral, MaternGeneralPars, NoShape>;

// cov_dcov / cov_dcov_sq with the shape: the closed forms ignore it
template <int COV>
__host__ __device__ __forceinline__ void cov_dcov_s(double r, double var, double phi, const CovShape<COV>& sh, double& c,
                                                    double& dc) {
  if constexpr (COV == kMaternGeneral) matern_general(phi * r, var, sh, c, dc);
  else cov_dcov<COV>(r, var, phi, c, dc);
}
template <int COV>
__device__ __forceinline__ void cov_dcov_sq_s(double s, double var, double phi, const CovShape<COV>& sh, double& c,
                                              double& dc) {
  if constexpr (COV == kMaternGeneral) matern_general(phi * sqrt_nonneg(s), var, sh, c, dc);
  else cov_dcov_sq<COV>(s, var, phi, c, dc);
}

}  // namespace gpb_amd
