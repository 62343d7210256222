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

namespace gpb_amd {

enum CovType : int { kMatern05 = 0, kMatern15 = 1, kMatern25 = 2, kGaussian = 3 };

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

}  // namespace gpb_amd
