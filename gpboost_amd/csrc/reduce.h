// Fixed-order sums inside a wave and a 256-thread block (HIP only), shared by the dense, FITC and full-scale
// Vecchia kernels. The forms below add in different orders, so they give different bits: a kernel keeps the
// form it has.
#pragma once

#include <hip/hip_runtime.h>

namespace gpb_amd {

// sum over the 64 lanes of a wave by the xor butterfly, in every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum of the wave-uniform values of the 4 waves of a block, (w0 + w1) + (w2 + w3), in every thread; red: 4 doubles
__device__ __forceinline__ double block4_sum(double v, double* red) {
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return s;
}

// sum of per-thread values over a block: wave_sum, then block4_sum; red: 4 doubles
__device__ __forceinline__ double block_wave_sum(double v, double* red) { return block4_sum(wave_sum(v), red); }

// sum of per-thread values over a block by the halving tree through LDS, in every thread; red: 256 doubles
__device__ __forceinline__ double block_tree_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

}  // namespace gpb_amd
