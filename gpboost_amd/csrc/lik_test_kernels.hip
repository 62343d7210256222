// The point kernels of GPB_TestLikPoint / GPB_TestLikAuxPoint (lik_test.h): the functions of lik_device.h at (y_i,
// loc_i), nothing else.
#include <hip/hip_runtime.h>

#include "common.h"
#include "lik_device.h"
#include "lik_test.h"

namespace gpb_amd {
namespace {

__global__ void __launch_bounds__(256) test_lik_point_kernel(int n, int lik, double aux, const double* __restrict__ y,
                                                             const double* __restrict__ loc, double* __restrict__ ll,
                                                             double* __restrict__ d1, double* __restrict__ info,
                                                             double* __restrict__ dinfo) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  ll[i] = lik_loglik(lik, aux, y[i], loc[i]);
  d1[i] = lik_d1(lik, aux, y[i], loc[i]);
  info[i] = lik_info(lik, aux, y[i], loc[i]);
  dinfo[i] = lik_dinfo(lik, aux, y[i], loc[i]);
}

// negative_binomial: the nb_* functions, log(shape) taken once per thread as the production kernels do
__global__ void __launch_bounds__(256) test_nb_point_kernel(int n, double aux, const double* __restrict__ y,
                                                            const double* __restrict__ loc, double* __restrict__ ll,
                                                            double* __restrict__ d1, double* __restrict__ info,
                                                            double* __restrict__ dinfo) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double log_r = log(aux);
  ll[i] = nb_loglik(aux, log_r, y[i], loc[i]);
  d1[i] = nb_d1(aux, log_r, y[i], loc[i]);
  info[i] = nb_info(aux, log_r, y[i], loc[i]);
  dinfo[i] = nb_dinfo(aux, log_r, y[i], loc[i]);
}

__global__ void __launch_bounds__(256) test_nb_aux_point_kernel(int n, double aux, const double* __restrict__ y,
                                                                const double* __restrict__ loc,
                                                                double* __restrict__ dd1a, double* __restrict__ dinfoa,
                                                                double* __restrict__ term) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double log_r = log(aux);
  dd1a[i] = nb_dd1_aux(aux, log_r, y[i], loc[i]);
  dinfoa[i] = nb_dinfo_aux(aux, log_r, y[i], loc[i]);
  term[i] = nb_aux_term(aux, log_r, y[i], loc[i]);
}

}  // namespace

void launch_test_nb_aux_point(int n, double aux, const double* y, const double* loc, double* dd1a, double* dinfoa,
                              double* term, hipStream_t s) {
  hipLaunchKernelGGL(test_nb_aux_point_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, aux, y, loc, dd1a, dinfoa,
                     term);
  HIP_CHECK(hipGetLastError());
}

void launch_test_lik_point(int n, int lik, double aux, const double* y, const double* loc, double* ll, double* d1,
                           double* info, double* dinfo, hipStream_t s) {
  if (lik == kLikNegBinomial) {
    hipLaunchKernelGGL(test_nb_point_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, aux, y, loc, ll, d1, info, dinfo);
    HIP_CHECK(hipGetLastError());
    return;
  }
  hipLaunchKernelGGL(test_lik_point_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, lik, aux, y, loc, ll, d1, info,
                     dinfo);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gpb_amd
