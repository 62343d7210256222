// The core of the two wide Vecchia row kernels (64 < num_neighbors <= kRowsWideMaxM, gfx950, wave64):
// vecchia_rows_wide.hip (likelihood and gradient rows) and vecchia_fisher_rows_wide.hip (Fisher rows), and of their
// wave-per-row forms for the general-shape Matern covariance and m <= 64 (vecchia_rows_bessel.hip,
// vecchia_fisher_rows_bessel.hip: NW = 1 and NT = 64 below, one LDS slice per wave). Included by these four files
// only. One 256-thread workgroup (four waves) owns a Vecchia row with k = min(i, m) neighbours; with
// KP = k rounded up to a multiple of 16 (rows >= k are identity padding with zero right-hand sides, which leaves
// every solution unchanged) the between-neighbour matrix lives in ONE square LDS array A (KP x KP, odd row stride
// S = MP + 1, MP = m rounded up to 16): C_rc in the lower triangle (r > c), dC_rc / dlog(phi) in the upper one
// (A[c][r]). The kernels' own stage 1 fills the coordinates nbx and the diagonal of A; from here come
//
//  - wide_pairs (stage 2): the KP (KP - 1) / 2 pair covariances are evaluated once, split evenly over the 256
//    threads (rows h and KP - 1 - h together hold KP - 1 pairs, so the pairs form a KP / 2 x (KP - 1) rectangle),
//    and both values are stored. No second matrix and no second exp pass;
//  - wide_chol (stage 3): blocked right-looking Cholesky of the lower triangle in place, 16-column panels. Per
//    panel: every wave loads the 16 x 16 diagonal block (lane & 15 = block row, 16 registers), factors it by a
//    column sweep whose broadcasts are 16-lane shuffles, and solves X L_bb^T = P for the panel rows below with the
//    same shuffles (thread = row, 16 registers; the four waves hold the same L_bb, so no barrier separates factor
//    and solve); then the trailing update A_IJ -= P_I P_J^T runs as 16 x 16 tiles of four v_mfma_f64_16x16x4 each,
//    the tiles I >= J dealt round-robin to the four waves. Diagonal tiles store only their lower half: the upper
//    triangle keeps dC. Two barriers per panel. DIV chooses how a pivot is applied, everywhere in this file:
//    false multiplies by 1 / L_jj (and diag_out receives the reciprocals), true divides by L_jj (diag_out receives
//    L_jj): one rounding fewer in every entry, which the Fisher rows' cancelling sums (var - a.c - a.a) show.
//    BORDER carries a right-hand side through the factorization as row KP of the matrix, kept in the vector zb: in
//    every panel the thread after the last panel row solves the border's 16 entries against L_bb with the panel
//    rows, and after the panel barrier thread jj updates zb[jj] -= sum_s zb[j0 + s] L[jj][j0 + s] (16 terms, fixed
//    order) beside the MFMA tiles. When the last panel is done zb = L^-1 (what zb held);
//  - wide_forward / wide_backward: L z = rhs and L^T x = z for NR right-hand sides together on ONE wave: lane l
//    holds entries l and l + 64 of each, column sweeps with one wave shuffle per column and right-hand side, one
//    load of L and of the pivot per column for all of them, no barrier inside;
//  - wide_launch, wave_rows_launch: the host side (LDS check, grid = resident capacity, launch).
// Every loop's trip count is uniform over the workgroup or the wave; where the work per lane differs, the lanes are
// predicated instead. Every sum has a fixed order and there is no atomic. A failed pivot has no path of its own:
// sqrt of a negative pivot is NaN, which spreads to everything after it.
//
// LDS per workgroup: MP S + 9 MP doubles: 141312 bytes at m = 128, 81408 at m = 96, 57600 at m = 80; sized by the
// model's m and checked against the device's per-workgroup limit, which bounds the largest m. After A come the
// coordinates (3 MP) and six vectors of MP: c, dc, y_nbr, a, v, 1 / L_kk in the rows kernel; dc, zb, a, L_kk and the
// two halves of t in the Fisher kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "cov.h"
#include "kernels.h"

namespace gpb_amd {

constexpr int kDMax = 3;
constexpr int kWideThreads = 256;
constexpr int kPanel = 16;   // panel width = MFMA tile edge
typedef double double4_t __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int wide_mp(int m) { return (m + kPanel - 1) & ~(kPanel - 1); }
// A (MP x S) | coordinates (MP x 3) | the kernel's six vectors (6 MP)
__host__ __device__ constexpr size_t wide_lds_doubles(int m) {
  return (size_t)wide_mp(m) * (wide_mp(m) + 1) + (size_t)(kDMax + 6) * wide_mp(m);
}

// x / L_jj: by the pivot itself (DIV) or by its stored reciprocal
template <bool DIV>
__device__ __forceinline__ double wide_unscale(double x, double pv) {
  if constexpr (DIV) return x / pv;
  else return x * pv;
}

// The barrier between the stages of a row: of the workgroup that owns it (NW waves), or, where ONE wave owns the row
// (NW = 1, vecchia_rows_bessel.hip), of that wave alone: its LDS accesses complete in program order, so all that
// is needed is that the compiler keeps them there.
template <int NW>
__device__ __forceinline__ void wide_sync() {
  if constexpr (NW == 1) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

// pairs: e -> (h, q); q < h: (row h, column q), else (row KP - 1 - h, column q - h). NT threads share them (tid is
// the thread's index among them); sh is the covariance's shape (empty for the closed forms)
template <int COV, int NT = kWideThreads>
__device__ __forceinline__ void wide_pairs(double* A, int S, const double* nbx, int KP, int k, double var, double phi,
                                           int tid, const CovShape<COV>& sh = {}) {
  const int npairs = (KP / 2) * (KP - 1);
  for (int e0 = 0; e0 < npairs; e0 += NT) {   // workgroup-uniform trip count; the last trip is partial
    const int e = min(e0 + tid, npairs - 1);
    const int h = e / (KP - 1), q = e - h * (KP - 1);
    const int r = q < h ? h : KP - 1 - h;
    const int c = q < h ? q : q - h;
    double s = 0.;
#pragma unroll
    for (int qq = 0; qq < kDMax; ++qq) {
      const double t = nbx[r * kDMax + qq] - nbx[c * kDMax + qq];
      s += t * t;
    }
    double cc, dc;
    cov_dcov_sq_s<COV>(s, var, phi, sh, cc, dc);
    const bool valid = r < k;   // c < r
    if (e0 + tid < npairs) {
      A[r * S + c] = valid ? cc : 0.;
      A[c * S + r] = valid ? dc : 0.;
    }
  }
}

// Called by the whole workgroup after a barrier; ends with one. diag_out[j] = L_jj (DIV) or 1 / L_jj. NW: the waves
// that share the row (tid over all of them; NW = 1: the row's wave takes every trailing tile itself).
template <bool DIV, bool BORDER, int NW = kWideThreads / 64>
__device__ __forceinline__ void wide_chol(double* A, int S, int KP, double* diag_out, double* zb, int tid, int lane,
                                          int wave) {
  const int lr = lane & 15, lq = lane >> 4;
  const int NB = KP / kPanel;
  for (int p = 0; p < NB; ++p) {
    const int j0 = p * kPanel;
    double row[kPanel], pv[kPanel];   // block row lr (entries c > lr hold dC and are never used); the pivots
#pragma unroll
    for (int c = 0; c < kPanel; ++c) row[c] = A[(j0 + lr) * S + j0 + c];
#pragma unroll
    for (int j = 0; j < kPanel; ++j) {
      const double l = sqrt(__shfl(row[j], j, kPanel));
      if constexpr (DIV) pv[j] = l;
      else pv[j] = 1. / l;
      const double lik = wide_unscale<DIV>(row[j], pv[j]);   // L[lr][j] for lr > j
      row[j] = lr == j ? l : lik;
#pragma unroll
      for (int jj = j + 1; jj < kPanel; ++jj) row[jj] = fma(-lik, __shfl(lik, jj, kPanel), row[jj]);   // lr >= jj
    }
    // panel rows below the block, and the border row (t == KP): x L_bb^T = P, thread = row (threads past the last
    // of them redo the last panel row and store nothing)
    const int t = j0 + kPanel + tid;
    double* px = A + min(t, KP - 1) * S + j0;
    if constexpr (BORDER) px = t == KP ? zb + j0 : px;
    double x[kPanel];
#pragma unroll
    for (int c = 0; c < kPanel; ++c) x[c] = px[c];
#pragma unroll
    for (int j = 0; j < kPanel; ++j) {
      double s = x[j];
#pragma unroll
      for (int q = 0; q < j; ++q) s = fma(-x[q], __shfl(row[q], j, kPanel), s);   // L[j][q] from lane j
      x[j] = wide_unscale<DIV>(s, pv[j]);
    }
    if (BORDER ? t <= KP : t < KP) {
#pragma unroll
      for (int c = 0; c < kPanel; ++c) px[c] = x[c];
    }
    wide_sync<NW>();   // the panel is final; every wave has read the diagonal block
    if (tid < kPanel) {
#pragma unroll
      for (int c = 0; c < kPanel; ++c) {
        if (c <= lr) A[(j0 + lr) * S + j0 + c] = row[c];
        if (c == lr) diag_out[j0 + c] = pv[c];
      }
    }
    if constexpr (BORDER) {   // column t of the border against panel row t (both final since the barrier)
      if (t < KP) {
        double s = zb[t];
#pragma unroll
        for (int c = 0; c < kPanel; ++c) s = fma(-zb[j0 + c], A[t * S + j0 + c], s);
        zb[t] = s;
      }
    }
    // trailing update, tiles I >= J > p round-robin over the waves. MFMA operands: a = P_I[lr][4 s + lq],
    // b = P_J[lr][4 s + lq]; result entry rg of a lane is row lq + 4 rg, column lr of the tile
    int cnt = 0;
    for (int I = p + 1; I < NB; ++I) {
      for (int J = p + 1; J <= I; ++J, ++cnt) {
        if ((cnt & (NW - 1)) != wave) continue;
        const double* pa = A + (I * kPanel + lr) * S + j0 + lq;
        const double* pb = A + (J * kPanel + lr) * S + j0 + lq;
        double4_t u = {0., 0., 0., 0.};
#pragma unroll
        for (int s4 = 0; s4 < kPanel; s4 += 4) u = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[s4], pb[s4], u, 0, 0, 0);
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int ii = I * kPanel + lq + 4 * rg, jj = J * kPanel + lr;
          if (jj <= ii) A[ii * S + jj] -= u[rg];
        }
      }
    }
    wide_sync<NW>();
  }
}

// L z = rhs on one wave, in place: x0[r] and x1[r] are entries lane and lane + 64 of right-hand side r (zeros where
// the entry is >= KP, which stay zeros); dg is what wide_chol<DIV, ...> stored
template <int NR, bool DIV>
__device__ __forceinline__ void wide_forward(const double* A, int S, int KP, const double* dg, int lane,
                                             double (&x0)[NR], double (&x1)[NR]) {
  const int t0 = lane, t1 = lane + 64;
  const bool h0 = t0 < KP, h1 = t1 < KP;
  const int K0 = min(KP, 64);
  for (int c = 0; c < K0; ++c) {
    const double pv = dg[c];
    double xk[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) xk[r] = wide_unscale<DIV>(__shfl(x0[r], c), pv);
    const double l0 = (h0 && t0 > c) ? A[t0 * S + c] : 0.;
    const double l1 = h1 ? A[t1 * S + c] : 0.;
#pragma unroll
    for (int r = 0; r < NR; ++r) x0[r] = t0 == c ? xk[r] : fma(-l0, xk[r], x0[r]);
#pragma unroll
    for (int r = 0; r < NR; ++r) x1[r] = fma(-l1, xk[r], x1[r]);
  }
  for (int c = 64; c < KP; ++c) {
    const double pv = dg[c];
    double xk[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) xk[r] = wide_unscale<DIV>(__shfl(x1[r], c - 64), pv);
    const double l1 = (h1 && t1 > c) ? A[t1 * S + c] : 0.;
#pragma unroll
    for (int r = 0; r < NR; ++r) x1[r] = t1 == c ? xk[r] : fma(-l1, xk[r], x1[r]);
  }
}

// L^T x = z, the same way (row c of L is contiguous)
template <int NR, bool DIV>
__device__ __forceinline__ void wide_backward(const double* A, int S, int KP, const double* dg, int lane,
                                              double (&x0)[NR], double (&x1)[NR]) {
  const int t0 = lane, t1 = lane + 64;
  const int K0 = min(KP, 64);
  for (int c = KP - 1; c >= 64; --c) {
    const double pv = dg[c];
    double xk[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) xk[r] = wide_unscale<DIV>(__shfl(x1[r], c - 64), pv);
    const double l1 = t1 < c ? A[c * S + t1] : 0.;
    const double l0 = A[c * S + t0];
#pragma unroll
    for (int r = 0; r < NR; ++r) x1[r] = t1 == c ? xk[r] : fma(-l1, xk[r], x1[r]);
#pragma unroll
    for (int r = 0; r < NR; ++r) x0[r] = fma(-l0, xk[r], x0[r]);
  }
  for (int c = K0 - 1; c >= 0; --c) {
    const double pv = dg[c];
    double xk[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) xk[r] = wide_unscale<DIV>(__shfl(x0[r], c), pv);
    const double l0 = t0 < c ? A[c * S + t0] : 0.;
#pragma unroll
    for (int r = 0; r < NR; ++r) x0[r] = t0 == c ? xk[r] : fma(-l0, xk[r], x0[r]);
  }
}

// Host side: checks the LDS a model with m neighbours needs against the device's limit, launches kern over `rows`
// Vecchia rows and returns the grid. The grid is the resident capacity (at most kRowsWideMaxBlocks), so every
// workgroup strides over an equal share of the rows in one round. tag names the kernel in the
// GPBOOST_AMD_ROWS_PROF line, lds_for completes the LDS error message.
template <typename Args>
int wide_launch(void (*kern)(Args), const Args& a, int m, int rows, const char* tag, const char* lds_for,
                hipStream_t s) {
  int dev = 0, cus = 0, lds_max = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  HIP_CHECK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  const size_t bytes = wide_lds_doubles(m) * sizeof(double);
  if (bytes > (size_t)lds_max)
    Fatal("num_neighbors = %d needs %zu bytes of LDS per workgroup%s, this device has %d", m, bytes, lds_for, lds_max);
  if (bytes > 64 * 1024)   // above the default dynamic-LDS limit
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)bytes));
  int per_cu = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kWideThreads, bytes));
  const int blocks = std::min({rows, std::max(per_cu, 1) * std::max(cus, 1), kRowsWideMaxBlocks});
  static const bool info = std::getenv("GPBOOST_AMD_ROWS_PROF") != nullptr;
  if (info)
    std::fprintf(stderr, "[%s] m=%d grid=%d workgroups/CU=%d LDS bytes/workgroup=%zu\n", tag, m, blocks, per_cu, bytes);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWideThreads), bytes, s, a);
  HIP_CHECK(hipGetLastError());
  return blocks;
}

// Host side of the wave-per-row kernels (m <= 64, one wave's LDS slice is wide_lds_doubles(m)): kern4 / kern2 / kern1
// are the instances with four, two and one independent waves per workgroup; four are taken where the device's
// per-workgroup LDS limit allows, else two or one. The grid is the resident capacity; returns it.
template <typename Args>
int wave_rows_launch(void (*kern4)(Args), void (*kern2)(Args), void (*kern1)(Args), const Args& a, int m, int rows,
                     const char* tag, hipStream_t s) {
  int dev = 0, cus = 0, lds_max = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  HIP_CHECK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  const size_t wave_bytes = wide_lds_doubles(m) * sizeof(double);
  if (wave_bytes > (size_t)lds_max)
    Fatal("num_neighbors = %d needs %zu bytes of LDS per wave, this device has %d", m, wave_bytes, lds_max);
  const int nw = 4 * wave_bytes <= (size_t)lds_max ? 4 : (2 * wave_bytes <= (size_t)lds_max ? 2 : 1);
  void (*kern)(Args) = nw == 4 ? kern4 : (nw == 2 ? kern2 : kern1);
  const size_t bytes = nw * wave_bytes;
  if (bytes > 64 * 1024)   // above the default dynamic-LDS limit
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)bytes));
  int per_cu = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * nw, bytes));
  const int blocks = std::min({(rows + nw - 1) / nw, std::max(per_cu, 1) * std::max(cus, 1), kRowsWideMaxBlocks});
  static const bool info = std::getenv("GPBOOST_AMD_ROWS_PROF") != nullptr;
  if (info)
    std::fprintf(stderr, "[%s] m=%d grid=%d waves/workgroup=%d workgroups/CU=%d LDS bytes/workgroup=%zu\n", tag, m,
                 blocks, nw, per_cu, bytes);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(64 * nw), bytes, s, a);
  HIP_CHECK(hipGetLastError());
  return blocks;
}

}  // namespace gpb_amd
