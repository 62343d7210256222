// The per-observation kernels the dense, FITC and full-scale Vecchia Laplace drivers share (laplace_kernels.hip)
// and their grid arithmetic: 256 threads per block, one thread per observation, reductions on at most 1024
// grid-stride blocks whose partials launch_sum_blocks (kernels.h) adds in a fixed order.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

namespace gpb_amd {

inline int laplace_grid(int n) { return std::max(1, (n + 255) / 256); }
inline int laplace_blocks(int n) { return std::min(1024, laplace_grid(n)); }

// out = a o b
void launch_laplace_mul(int n, const double* a, const double* b, double* out, hipStream_t s);
// Armijo slope: part[laplace_blocks(n)] = block partials of sum_i dir_i (aupd_i - a_i + w_i dir_i), dir = mupd - mode
void launch_laplace_gdd(int n, const double* mode, const double* a, const double* mupd, const double* aupd,
                        const double* w, double* part, hipStream_t s);
// One line-search trial at learning rate lam: (mnew, anew) = (1 - lam) (mode, a) + lam (mupd, aupd) (lam = 1: the
// update itself); part[2 laplace_blocks(n)] = block partials of [anew^T mnew, sum log p(y | mnew + off)]
void launch_laplace_trial(int n, int lik, double aux, double lam, const double* mode, const double* a,
                          const double* mupd, const double* aupd, const double* y, const double* off, double* mnew,
                          double* anew, double* part, hipStream_t s);

}  // namespace gpb_amd
