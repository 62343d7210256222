// The per-observation kernels shared by the dense, FITC and full-scale Vecchia Laplace drivers (laplace_kernels.h):
// the elementwise product, the Armijo slope and the line-search trial of the drivers that iterate on
// (mode, a = Sigma^-1 mode).
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "laplace_kernels.h"
#include "lik_device.h"
#include "lik_test.h"
#include "reduce.h"

namespace gpb_amd {
namespace {

constexpr int kT = 256;

__global__ void __launch_bounds__(kT) laplace_mul_kernel(int n, const double* __restrict__ a, const double* __restrict__ b,
                                                        double* __restrict__ out) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i < n) out[i] = a[i] * b[i];
}

// Armijo slope: sum_i dir_i (aupd_i - a_i + W_i dir_i), dir = mupd - mode (likelihoods.h:1906-1909, 3166-3169)
__global__ void __launch_bounds__(kT) laplace_gdd_kernel(int n, const double* __restrict__ mode,
                                                        const double* __restrict__ a, const double* __restrict__ mupd,
                                                        const double* __restrict__ aupd, const double* __restrict__ w,
                                                        double* __restrict__ part) {
  __shared__ double red[kT];
  double acc = 0.;
  for (int i = blockIdx.x * kT + threadIdx.x; i < n; i += gridDim.x * kT) {
    const double dir = mupd[i] - mode[i];
    acc += dir * (aupd[i] - a[i] + w[i] * dir);
  }
  const double s = block_tree_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one line-search trial (likelihoods.h:1910-1928, 3171-3190): the new state mixed at learning rate lam (lam = 1:
// the update itself), partials of [a^T mode, sum log p(y | mode + F)]
__global__ void __launch_bounds__(kT) laplace_trial_kernel(int n, int lik, double aux, double lam,
                                                          const double* __restrict__ mode, const double* __restrict__ a,
                                                          const double* __restrict__ mupd, const double* __restrict__ aupd,
                                                          const double* __restrict__ y, const double* __restrict__ off,
                                                          double* __restrict__ mnew, double* __restrict__ anew,
                                                          double* __restrict__ part) {
  __shared__ double red[kT];
  double sq = 0., sl = 0.;
  for (int i = blockIdx.x * kT + threadIdx.x; i < n; i += gridDim.x * kT) {
    double mi, ai;
    if (lam == 1.) {
      mi = mupd[i];
      ai = aupd[i];
    } else {
      ai = (1. - lam) * a[i] + lam * aupd[i];
      mi = (1. - lam) * mode[i] + lam * mupd[i];
    }
    mnew[i] = mi;
    anew[i] = ai;
    sq += ai * mi;
    sl += lik_loglik(lik, aux, y[i], off ? mi + off[i] : mi);
  }
  const double s0 = block_tree_sum(sq, red);
  const double s1 = block_tree_sum(sl, red);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = s0;
    part[2 * blockIdx.x + 1] = s1;
  }
}

}  // namespace

void launch_laplace_mul(int n, const double* a, const double* b, double* out, hipStream_t s) {
  hipLaunchKernelGGL(laplace_mul_kernel, dim3(laplace_grid(n)), dim3(kT), 0, s, n, a, b, out);
  HIP_CHECK(hipGetLastError());
}

void launch_laplace_gdd(int n, const double* mode, const double* a, const double* mupd, const double* aupd,
                        const double* w, double* part, hipStream_t s) {
  hipLaunchKernelGGL(laplace_gdd_kernel, dim3(laplace_blocks(n)), dim3(kT), 0, s, n, mode, a, mupd, aupd, w, part);
  HIP_CHECK(hipGetLastError());
}

void launch_laplace_trial(int n, int lik, double aux, double lam, const double* mode, const double* a,
                          const double* mupd, const double* aupd, const double* y, const double* off, double* mnew,
                          double* anew, double* part, hipStream_t s) {
  hipLaunchKernelGGL(laplace_trial_kernel, dim3(laplace_blocks(n)), dim3(kT), 0, s, n, lik, aux, lam, mode, a, mupd, aupd,
                     y, off, mnew, anew, part);
  HIP_CHECK(hipGetLastError());
}

// ---- test launcher (lik_test.h): the trial of the FITC and dense drivers' objective with its block sums
void test_laplace_trial(int n, int lik, double aux, double lam, const double* mode, const double* a, const double* mupd,
                        const double* aupd, const double* y, const double* off, double* mnew, double* anew, double* part,
                        double* sums, hipStream_t s) {
  launch_laplace_trial(n, lik, aux, lam, mode, a, mupd, aupd, y, off, mnew, anew, part, s);
  launch_sum_blocks(part, laplace_blocks(n), 2, sums, s);
}

}  // namespace gpb_amd
