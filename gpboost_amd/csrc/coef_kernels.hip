// Passes over the scaled covariate matrix X (row-major n x p, p <= 31) of a Laplace model with linear regression
// coefficients in the L-BFGS vector (coef.h): the offset F + X beta, the gradient X^T grad_F and the four sums of
// MaximalLearningRateCoef (re_model_template.h:4952-4981). Each reads X once (8 n p bytes) and is bandwidth-bound.
//
// Access pattern: a row of X is p doubles, p no power of two, so a thread per row reading its own row would touch
// addresses 8 p bytes apart. Instead a block copies a tile of kCoefRows consecutive rows, which is one contiguous
// run of rows * p doubles, into LDS with consecutive threads on consecutive doubles (fully coalesced; the tile
// starts at a multiple of 256 p doubles, so every wave's 512-byte run is 512-byte aligned), and then every thread
// reads its own row from LDS. The LDS row stride is p | 1 doubles: with an odd stride the 32 lanes of a half-wave
// reading one column of 32 consecutive rows hit 32 distinct 8-byte bank pairs (bank = (byte / 4) mod 64 for
// ds_read_b64), so the row reads are conflict-free for every p.
//
// Reductions: a thread sums its rows over the block's tiles in ascending tile order, the block sums its threads by
// wave_sum and block4_sum (reduce.h), and one wave per output adds the block partials in block order. The block
// count is coef_blocks(n), a function of n alone; no atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>

#include <vector>

#include "coef.h"
#include "common.h"
#include "reduce.h"
#include "wave_ops.h"

namespace gpb_amd {

namespace {

__device__ __forceinline__ int coef_stride(int p) { return p | 1; }

// Tile t (rows t * kCoefRows ..) of X into xs[row][col] with row stride p | 1; returns the rows of the tile.
__device__ __forceinline__ int load_tile(int n, int p, const double* __restrict__ X, int t, double* xs) {
  const int r0 = t * kCoefRows;
  const int rows = min(kCoefRows, n - r0);
  const int cnt = rows * p, st = coef_stride(p);
  const double* src = X + (size_t)r0 * p;
  // (row, column) of element e = threadIdx.x + k * kCoefRows, advanced without a division per element
  const int dr = kCoefRows / p, dc = kCoefRows - dr * p;
  int r = threadIdx.x / p, c = threadIdx.x - r * p;
  for (int e = threadIdx.x; e < cnt; e += kCoefRows) {
    xs[r * st + c] = src[e];
    r += dr;
    c += dc;
    if (c >= p) {
      c -= p;
      ++r;
    }
  }
  return rows;
}

__global__ void __launch_bounds__(kCoefRows) coef_offset_kernel(int n, int p, const double* __restrict__ X,
                                                                const double* __restrict__ beta,
                                                                const double* __restrict__ F,
                                                                double* __restrict__ eta0) {
  extern __shared__ double xs[];
  __shared__ double b[kCovMaxCols];
  if ((int)threadIdx.x < p) b[threadIdx.x] = beta[threadIdx.x];
  const int tiles = (n + kCoefRows - 1) / kCoefRows, st = coef_stride(p);
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    __syncthreads();   // b written; the previous tile read
    const int rows = load_tile(n, p, X, t, xs);
    __syncthreads();
    const int r = threadIdx.x;
    if (r < rows) {
      const size_t i = (size_t)t * kCoefRows + r;
      double v = F != nullptr ? F[i] : 0.;
      for (int j = 0; j < p; ++j) v = fma(xs[r * st + j], b[j], v);
      eta0[i] = v;
    }
  }
}

// partial[block][j] = sum over the block's rows of X_ij gF_i
__global__ void __launch_bounds__(kCoefRows) coef_grad_kernel(int n, int p, const double* __restrict__ X,
                                                              const double* __restrict__ gF,
                                                              double* __restrict__ partial) {
  extern __shared__ double xs[];
  __shared__ double red[4];
  const int tiles = (n + kCoefRows - 1) / kCoefRows, st = coef_stride(p);
  double acc[kCoefMaxCols];
#pragma unroll
  for (int j = 0; j < kCoefMaxCols; ++j) acc[j] = 0.;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    __syncthreads();
    const int rows = load_tile(n, p, X, t, xs);
    __syncthreads();
    const int r = threadIdx.x;
    if (r < rows) {
      const double g = gF[(size_t)t * kCoefRows + r];
#pragma unroll
      for (int j = 0; j < kCoefMaxCols; ++j)
        if (j < p) acc[j] = fma(xs[r * st + j], g, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < kCoefMaxCols; ++j) {
    if (j < p) {   // p is uniform over the block: every thread takes part in the barriers of block4_sum
      const double s = block_wave_sum(acc[j], red);
      if (threadIdx.x == 0) partial[(size_t)blockIdx.x * p + j] = s;
    }
  }
}

// partial[block][0..3] = sums over the block's rows of a, c, a^2, a c with a = (X dir)_i, c = (X beta)_i
__global__ void __launch_bounds__(kCoefRows) coef_moments_kernel(int n, int p, const double* __restrict__ X,
                                                                 const double* __restrict__ beta,
                                                                 const double* __restrict__ dir,
                                                                 double* __restrict__ partial) {
  extern __shared__ double xs[];
  __shared__ double b[kCovMaxCols], d[kCovMaxCols];
  __shared__ double red[4];
  if ((int)threadIdx.x < p) {
    b[threadIdx.x] = beta[threadIdx.x];
    d[threadIdx.x] = dir[threadIdx.x];
  }
  const int tiles = (n + kCoefRows - 1) / kCoefRows, st = coef_stride(p);
  double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    __syncthreads();
    const int rows = load_tile(n, p, X, t, xs);
    __syncthreads();
    const int r = threadIdx.x;
    if (r < rows) {
      double a = 0., c = 0.;
      for (int j = 0; j < p; ++j) {
        const double x = xs[r * st + j];
        a = fma(x, d[j], a);
        c = fma(x, b[j], c);
      }
      s0 += a;
      s1 += c;
      s2 = fma(a, a, s2);
      s3 = fma(a, c, s3);
    }
  }
  __syncthreads();   // a block without tiles still wrote b, d
  s0 = block_wave_sum(s0, red);
  s1 = block_wave_sum(s1, red);
  s2 = block_wave_sum(s2, red);
  s3 = block_wave_sum(s3, red);
  if (threadIdx.x == 0) {
    double* o = partial + (size_t)blockIdx.x * 4;
    o[0] = s0;
    o[1] = s1;
    o[2] = s2;
    o[3] = s3;
  }
}

// out[j] = sum_b partial[b][j], blocks in ascending order: one wave per output; 64 partials at a time are loaded by
// the 64 lanes (independent loads in flight together) and added in lane order from scalar registers, so the order
// of the additions is the plain loop's and the latency of one load is paid per 64 blocks, not per block
__global__ void __launch_bounds__(64) coef_finish_kernel(const double* __restrict__ partial, int nblocks, int width,
                                                         double* __restrict__ out) {
  const int j = blockIdx.x, lane = threadIdx.x;
  double s = 0.;
  for (int b0 = 0; b0 < nblocks; b0 += 64) {
    const int b = b0 + lane;
    const double v = b < nblocks ? partial[(size_t)b * width + j] : 0.;
    const int cnt = min(64, nblocks - b0);
#pragma unroll
    for (int k = 0; k < 64; ++k)
      if (k < cnt) s += readlane_f64(v, k);
  }
  if (lane == 0) out[j] = s;
}

size_t tile_bytes(int p) { return sizeof(double) * (size_t)kCoefRows * (size_t)(p | 1); }

void check_dims(int n, int p) {
  if (n < 1) Fatal("coefficient kernels: n = %d must be >= 1", n);
  if (p < 1 || p > kCoefMaxCols) Fatal("number of covariates = %d outside [1, %d]", p, kCoefMaxCols);
}

}  // namespace

int coef_blocks(int n) {
  const int tiles = (n + kCoefRows - 1) / kCoefRows;
  return tiles < kCoefMaxBlocks ? (tiles > 0 ? tiles : 1) : kCoefMaxBlocks;
}

size_t coef_partial_len(int n, int p) { return (size_t)coef_blocks(n) * (size_t)(p > 4 ? p : 4); }

void launch_coef_offset(int n, int p, const double* X, const double* beta, const double* F, double* eta0,
                        hipStream_t s) {
  check_dims(n, p);
  hipLaunchKernelGGL(coef_offset_kernel, dim3(coef_blocks(n)), dim3(kCoefRows), tile_bytes(p), s, n, p, X, beta, F,
                     eta0);
  HIP_CHECK(hipGetLastError());
}

void launch_coef_grad(int n, int p, const double* X, const double* gF, double* partial, double* g, hipStream_t s) {
  check_dims(n, p);
  const int nb = coef_blocks(n);
  hipLaunchKernelGGL(coef_grad_kernel, dim3(nb), dim3(kCoefRows), tile_bytes(p), s, n, p, X, gF, partial);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(coef_finish_kernel, dim3(p), dim3(64), 0, s, partial, nb, p, g);
  HIP_CHECK(hipGetLastError());
}

void launch_coef_step_moments(int n, int p, const double* X, const double* beta, const double* dir, double* partial,
                              double* mom, hipStream_t s) {
  check_dims(n, p);
  const int nb = coef_blocks(n);
  hipLaunchKernelGGL(coef_moments_kernel, dim3(nb), dim3(kCoefRows), tile_bytes(p), s, n, p, X, beta, dir, partial);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(coef_finish_kernel, dim3(4), dim3(64), 0, s, partial, nb, 4, mom);
  HIP_CHECK(hipGetLastError());
}

void test_coef_ops(int n, int p, const double* X, const double* beta, const double* dir, const double* F,
                   const double* gF, double* eta0, double* g, double* mom) {
  check_dims(n, p);
  if (X == nullptr) Fatal("GPB_TestCoefOps: X is NULL");
  if ((eta0 != nullptr || mom != nullptr) && beta == nullptr) Fatal("GPB_TestCoefOps: beta is NULL");
  if (mom != nullptr && dir == nullptr) Fatal("GPB_TestCoefOps: dir is NULL");
  if (g != nullptr && gF == nullptr) Fatal("GPB_TestCoefOps: gF is NULL");
  hipStream_t s = nullptr;
  const size_t np = (size_t)n * p;
  DevBuf<double> dX(np), dv(2 * kCovMaxCols), dF(n), dgF(n), dout(n), dpart(coef_partial_len(n, p)),
      dsmall(kCovMaxCols + 4);
  HIP_CHECK(hipMemcpyAsync(dX.get(), X, sizeof(double) * np, hipMemcpyHostToDevice, s));
  if (beta != nullptr) HIP_CHECK(hipMemcpyAsync(dv.get(), beta, sizeof(double) * p, hipMemcpyHostToDevice, s));
  if (dir != nullptr)
    HIP_CHECK(hipMemcpyAsync(dv.get() + kCovMaxCols, dir, sizeof(double) * p, hipMemcpyHostToDevice, s));
  if (F != nullptr) HIP_CHECK(hipMemcpyAsync(dF.get(), F, sizeof(double) * n, hipMemcpyHostToDevice, s));
  if (gF != nullptr) HIP_CHECK(hipMemcpyAsync(dgF.get(), gF, sizeof(double) * n, hipMemcpyHostToDevice, s));
  if (eta0 != nullptr) {
    launch_coef_offset(n, p, dX.get(), dv.get(), F != nullptr ? dF.get() : nullptr, dout.get(), s);
    HIP_CHECK(hipMemcpyAsync(eta0, dout.get(), sizeof(double) * n, hipMemcpyDeviceToHost, s));
  }
  if (g != nullptr) {
    launch_coef_grad(n, p, dX.get(), dgF.get(), dpart.get(), dsmall.get(), s);
    HIP_CHECK(hipMemcpyAsync(g, dsmall.get(), sizeof(double) * p, hipMemcpyDeviceToHost, s));
  }
  if (mom != nullptr) {
    launch_coef_step_moments(n, p, dX.get(), dv.get(), dv.get() + kCovMaxCols, dpart.get(), dsmall.get() + kCovMaxCols,
                             s);
    HIP_CHECK(hipMemcpyAsync(mom, dsmall.get() + kCovMaxCols, sizeof(double) * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace gpb_amd
