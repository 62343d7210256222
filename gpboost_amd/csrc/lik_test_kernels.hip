// The point kernel of GPB_TestLikPoint (lik_test.h): the four functions of lik_device.h at (y_i, loc_i), nothing else.
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

}  // namespace

void launch_test_lik_point(int n, int lik, double aux, const double* y, const double* loc, double* ll, double* d1,
                           double* info, double* dinfo, hipStream_t s) {
  hipLaunchKernelGGL(test_lik_point_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, lik, aux, y, loc, ll, d1, info,
                     dinfo);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gpb_amd
