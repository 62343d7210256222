// Gram matrix [X | y]^T Psi^-1 [X | y] of the linear regression covariates (generalised least squares)
// under the two Woodbury-form covariances, gp_approx = "fitc" and "full_scale_vecchia".
//
// Reference: CalcXTPsiInvX, fitc / full_scale_vecchia branches with matrix_inversion_method = "cholesky"
// (re_model_template.h:6078-6117), ProfileOutCoef (:2427-2445), UpdateCoefGLS (:9125-9132). With
// Psi = K_nm K_mm,s^-1 K_mn + R and the Woodbury matrix M = K_mm,s + K_mn R^-1 K_nm = L_M L_M^T,
//   Z^T Psi^-1 Z = Z^T R^-1 Z - S^T S,   S = L_M^-1 K_mn R^-1 Z.
// FITC: R = diag(d). Full-scale Vecchia: R^-1 = B^T D^-1 B, so with U = B Z and BK = B K_nm the same two
// products appear with (BK, 1 / D, U) in place of (K_mn, 1 / d, Z).
//
// The one O(n m c) step is the primitive below: T = A diag(w) U (m x c) and G0 = U^T diag(w) U (c x c) in one
// pass over the n points, A the m x n matrix whose point i holds its m entries contiguously (K_mn / BK).
//   grid (ranges, ceil(m / 64)): workgroup (r, b) takes points [512 r, 512 (r + 1)) and rows [64 b, 64 b + 64)
//   of A, 16 rows per wave. Per step of 64 points the workgroup stages U and diag(w) U (zero past c columns
//   and past the range) in LDS; every wave loads its 16 x 64 block of A straight into MFMA A operands (lane l:
//   row l & 15, point 4 q + (l >> 4)) and runs 16 v_mfma_f64_16x16x4 per 16 columns of U. The workgroups with
//   b = 0 also form G0, one 16 x 16 tile of it per wave, from the two staged arrays.
//   Every range writes its own partial (no atomics); the second kernel adds an entry's partials in a fixed
//   order (four strided sums over the ranges ascending, combined pairwise), so equal inputs give equal bits
//   whatever the grid's scheduling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "covariates.h"
#include "dense.h"

namespace gpb_amd {

namespace {

typedef double wts_double4 __attribute__((ext_vector_type(4)));

constexpr int kWtsRange = 512;   // points per partial
constexpr int kWtsStep = 64;     // points staged in LDS at a time
constexpr int kWtsRows = 64;     // rows of A per workgroup (16 per wave)
// LDS row stride in doubles: 48 = 16 mod 32, so the two 16-lane groups of a half wave (points k, k + 1) read
// disjoint banks with ds_read_b64
constexpr int kWtsLd = 48;
static_assert(kCovMaxCols == 32, "the staging below indexes 32 columns");
static_assert(kWtsRange % kWtsStep == 0, "a range is a whole number of steps");

__global__ void __launch_bounds__(256) weighted_tall_skinny_kernel(int m, int n, int c, const double* __restrict__ A,
                                                                   int ldm, const double* __restrict__ w,
                                                                   const double* __restrict__ U,
                                                                   double* __restrict__ Tpart,
                                                                   double* __restrict__ Gpart) {
  __shared__ double us[kWtsStep][kWtsLd];    // U
  __shared__ double wus[kWtsStep][kWtsLd];   // diag(w) U
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int range = blockIdx.x;
  const int i0 = range * kWtsRange, i1 = min(n, i0 + kWtsRange);
  const int row = blockIdx.y * kWtsRows + wave * 16 + (lane & 15);   // this lane's row of the A operand
  const bool row_ok = row < m;
  const bool wide = c > 16;
  const int ga = (wave >> 1) * 16, gb = (wave & 1) * 16;   // this wave's tile of G0
  const bool gtile = blockIdx.y == 0 && ga < c && gb < c;
  wts_double4 t0 = {0., 0., 0., 0.}, t1 = {0., 0., 0., 0.}, g = {0., 0., 0., 0.};
  // this lane's A operands of one step: A[row][s0 + 4 q + (lane >> 4)], q = 0..15 (0 past the range / past row m)
  auto load_a = [&](int s0, double* a) {
#pragma unroll
    for (int q = 0; q < kWtsStep / 4; ++q) {
      const int i = s0 + 4 * q + (lane >> 4);
      a[q] = (row_ok && i < i1) ? A[(size_t)i * ldm + row] : 0.;
    }
  };
  double a[kWtsStep / 4], an[kWtsStep / 4];
  load_a(i0, a);
  for (int s0 = i0; s0 < i1; s0 += kWtsStep) {
    for (int e = tid; e < kWtsStep * kCovMaxCols; e += 256) {
      const int r = e >> 5, col = e & 31;
      const int i = s0 + r;
      double u = 0., wu = 0.;
      if (i < i1 && col < c) {
        u = U[(size_t)i * c + col];
        wu = w[i] * u;
      }
      us[r][col] = u;
      wus[r][col] = wu;
    }
    load_a(s0 + kWtsStep, an);   // the next step's operands are in flight while this step's MFMAs run
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kWtsStep / 4; ++q) {
      const int k = 4 * q + (lane >> 4);
      t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], wus[k][lane & 15], t0, 0, 0, 0);
      if (wide) t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], wus[k][16 + (lane & 15)], t1, 0, 0, 0);
      if (gtile) g = __builtin_amdgcn_mfma_f64_16x16x4f64(us[k][ga + (lane & 15)], wus[k][gb + (lane & 15)], g, 0, 0, 0);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kWtsStep / 4; ++q) a[q] = an[q];
  }
  // f64 MFMA C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
  const int j = lane & 15;
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    const int rr = (lane >> 4) + 4 * rg;
    const int r = blockIdx.y * kWtsRows + wave * 16 + rr;
    if (r < m && j < c) Tpart[((size_t)range * c + j) * ldm + r] = t0[rg];
    if (wide && r < m && 16 + j < c) Tpart[((size_t)range * c + 16 + j) * ldm + r] = t1[rg];
    if (gtile && ga + rr < c && gb + j < c) Gpart[(size_t)range * c * c + (size_t)(ga + rr) * c + gb + j] = g[rg];
  }
}

// out[e] = sum over the nr range partials part[z * stride + e], in a fixed order: four strided sums (z = q, q + 4,
// ... ascending, q = 0..3; eight loads in flight each) combined as (s0 + s1) + (s2 + s3)
__device__ __forceinline__ double sum_partials(const double* __restrict__ part, size_t stride, int nr, int q,
                                               double* red) {
  double s = 0.;
  int z = q;
  for (; z + 28 < nr; z += 32) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = part[(size_t)(z + 4 * k) * stride];
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  for (; z < nr; z += 4) s += part[(size_t)z * stride];
  red[threadIdx.x] = s;
  __syncthreads();
  const int el = threadIdx.x & 63;
  return (red[el] + red[64 + el]) + (red[128 + el] + red[192 + el]);
}

// T[e] = sum_z Tpart[z][e] over the ldm x c entries (rows >= m: 0) and G0[pair(a <= b)] = sum_z Gpart[z][a c + b].
// A workgroup takes 64 consecutive entries, four threads each (sum_partials).
__global__ void __launch_bounds__(256) weighted_tall_skinny_reduce_kernel(int m, int c, int ldm, int nr,
                                                                          const double* __restrict__ Tpart,
                                                                          const double* __restrict__ Gpart,
                                                                          double* __restrict__ T,
                                                                          double* __restrict__ G0) {
  __shared__ double red[256];
  const int el = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int nt = c * ldm;
  const int tblocks = nt / 64;   // ldm is a multiple of 64
  if ((int)blockIdx.x < tblocks) {
    const int e = blockIdx.x * 64 + el;
    const bool live = e % ldm < m;
    const double s = sum_partials(Tpart + e, (size_t)nt, live ? nr : 0, q, red);
    if (q == 0) T[e] = s;
    return;
  }
  const int pr = (blockIdx.x - tblocks) * 64 + el;
  const bool live = pr < c * (c + 1) / 2;
  int a = 0, rem = live ? pr : 0;
  while (a < c && rem >= c - a) { rem -= c - a; ++a; }   // pair index -> (a, a + rem)
  const int b = a + rem;
  const double s = sum_partials(Gpart + (size_t)a * c + b, (size_t)c * c, live ? nr : 0, q, red);
  if (q == 0 && live) G0[pr] = s;
}

__global__ void __launch_bounds__(256) reciprocal_kernel(int n, const double* __restrict__ d, double* __restrict__ w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) w[i] = 1. / d[i];
}

// one thread per (point, column), the row form of vecchia_gram_kernel's first phase
__global__ void __launch_bounds__(256) vecchia_bz_kernel(int n, int nn, int c, const int* __restrict__ nbr,
                                                         const double* __restrict__ Bv, const double* __restrict__ Z,
                                                         double* __restrict__ U) {
  const size_t it = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= (size_t)n * c) return;
  const int i = (int)(it / c), col = (int)(it - (size_t)i * c);
  const int k = i < nn ? i : nn;
  double v = Z[it];
  for (int e = 0; e < k; ++e) v = fma(Bv[(size_t)i * nn + e], Z[(size_t)nbr[(size_t)i * nn + e] * c + col], v);
  U[it] = v;
}

}  // namespace

int weighted_tall_skinny_ranges(int n) { return n > 0 ? (n + kWtsRange - 1) / kWtsRange : 1; }

void launch_weighted_tall_skinny(int m, int n, int c, const double* A, int ldm, const double* w, const double* U,
                                 double* Tpart, double* Gpart, double* T, double* G0, hipStream_t s) {
  if (c < 1 || c > kCovMaxCols) Fatal("number of covariates + 1 = %d outside [1, %d]", c, kCovMaxCols);
  if (m < 1 || n < 1 || ldm < m) Fatal("weighted tall-skinny product: bad extents m = %d, n = %d, ldm = %d", m, n, ldm);
  const int nr = weighted_tall_skinny_ranges(n);
  hipLaunchKernelGGL(weighted_tall_skinny_kernel, dim3(nr, (m + kWtsRows - 1) / kWtsRows), dim3(256), 0, s, m, n, c, A,
                     ldm, w, U, Tpart, Gpart);
  HIP_CHECK(hipGetLastError());
  if (ldm % 64 != 0) Fatal("weighted tall-skinny product: ldm = %d is not a multiple of 64", ldm);
  const int rblocks = c * ldm / 64 + (c * (c + 1) / 2 + 63) / 64;
  hipLaunchKernelGGL(weighted_tall_skinny_reduce_kernel, dim3(rblocks), dim3(256), 0, s, m, c, ldm, nr, Tpart, Gpart, T,
                     G0);
  HIP_CHECK(hipGetLastError());
}

void launch_vecchia_bz(int n, int nn, int c, const int* nbr, const double* Bv, const double* Z, double* U,
                       hipStream_t s) {
  const size_t items = (size_t)n * c;
  hipLaunchKernelGGL(vecchia_bz_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, n, nn, c, nbr, Bv, Z, U);
  HIP_CHECK(hipGetLastError());
}

void lowrank_gram(hipStream_t s, int m, int n, int c, int ldm, const double* A, const double* dvec, const double* U,
                  const double* Li, LowrankGramWork& ws, double* G_host) {
  const int nr = weighted_tall_skinny_ranges(n);
  const int npairs = c * (c + 1) / 2;
  ws.w.alloc(n);
  ws.Tpart.alloc((size_t)nr * kCovMaxCols * ldm);
  ws.Gpart.alloc((size_t)nr * kCovMaxCols * kCovMaxCols);
  ws.T.alloc((size_t)kCovMaxCols * ldm);
  ws.S.alloc((size_t)kCovMaxCols * ldm);
  ws.G0.alloc(kCovMaxCols * (kCovMaxCols + 1) / 2);
  hipLaunchKernelGGL(reciprocal_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, dvec, ws.w.get());
  HIP_CHECK(hipGetLastError());
  launch_weighted_tall_skinny(m, n, c, A, ldm, ws.w.get(), U, ws.Tpart.get(), ws.Gpart.get(), ws.T.get(), ws.G0.get(), s);
  // S = Li T (Li lower triangular: the structural zeros are skipped)
  gemm_f64(s, m, c, m, 1., Li, ldm, 0, ws.T.get(), ldm, 0, 0., ws.S.get(), ldm, 0, 1, 0, 0);
  std::vector<double> hS((size_t)c * ldm), hG0(npairs);
  HIP_CHECK(hipMemcpyAsync(hS.data(), ws.S.get(), sizeof(double) * hS.size(), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(hG0.data(), ws.G0.get(), sizeof(double) * npairs, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  int pr = 0;
  for (int a = 0; a < c; ++a)
    for (int b = a; b < c; ++b, ++pr) {
      double ss = 0.;
      for (int j = 0; j < m; ++j) ss += hS[(size_t)a * ldm + j] * hS[(size_t)b * ldm + j];
      G_host[(size_t)a * c + b] = G_host[(size_t)b * c + a] = hG0[pr] - ss;
    }
}

void test_weighted_tall_skinny(int m, int n, int c, const double* A, long a_len, const double* w, const double* U,
                               double* T_out, double* G0_out) {
  if (m < 1 || n < 1) Fatal("GPB_TestWeightedTallSkinny: m = %d and n = %d must be positive", m, n);
  if (c < 1 || c > kCovMaxCols) Fatal("GPB_TestWeightedTallSkinny: c = %d outside [1, %d]", c, kCovMaxCols);
  if (A == nullptr || w == nullptr || U == nullptr || T_out == nullptr || G0_out == nullptr)
    Fatal("GPB_TestWeightedTallSkinny: NULL array");
  const int ldm = (m + 63) / 64 * 64;
  if (a_len != (long)ldm * n) Fatal("GPB_TestWeightedTallSkinny: a_len = %ld, expected round_up(m, 64) * n = %ld", a_len, (long)ldm * n);
  const int nr = weighted_tall_skinny_ranges(n);
  const int npairs = c * (c + 1) / 2;
  DevBuf<double> dA((size_t)a_len), dw(n), dU((size_t)n * c), Tpart((size_t)nr * c * ldm), Gpart((size_t)nr * c * c),
      T((size_t)c * ldm), G0(npairs);
  hipStream_t s = nullptr;
  HIP_CHECK(hipMemcpyAsync(dA.get(), A, sizeof(double) * a_len, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(dw.get(), w, sizeof(double) * n, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(dU.get(), U, sizeof(double) * n * c, hipMemcpyHostToDevice, s));
  launch_weighted_tall_skinny(m, n, c, dA.get(), ldm, dw.get(), dU.get(), Tpart.get(), Gpart.get(), T.get(), G0.get(), s);
  std::vector<double> hT((size_t)c * ldm), hG(npairs);
  HIP_CHECK(hipMemcpyAsync(hT.data(), T.get(), sizeof(double) * hT.size(), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(hG.data(), G0.get(), sizeof(double) * npairs, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < c; ++j) T_out[(size_t)i * c + j] = hT[(size_t)j * ldm + i];
  const std::vector<double> G = unpack_gram(hG.data(), c);
  std::copy(G.begin(), G.end(), G0_out);
}

}  // namespace gpb_amd
