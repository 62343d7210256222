// Kernels of LowRankPrecond (lowrank_precond.h): pivoted Cholesky of the exact covariance, the k x k
// Gram matrix with its Cholesky factor and inverse in one workgroup, and the tall-skinny products of
// the Woodbury application.
#include "lowrank_precond.h"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

#include "cov.h"
#include "latent_kernels.h"
#include "lik_device.h"

namespace gpb_amd {

namespace {

constexpr int kPB = 256;          // threads of the row kernels
constexpr int kMaxPart = 1024;    // row ranges (= partial sums) of the split-n products: four workgroups per CU
constexpr int kLdsBytes = 49152;  // row chunk of a split-n product staged in LDS
constexpr int kStateHead = 4;     // state: [0] stop, [1] rank, [2] weight / Gram flags, [3] unused, [4 + m] pivot of step m
constexpr int kMaxRank = 256;

// ---------------------------------------------------------------- pivoted Cholesky
__global__ void __launch_bounds__(kPB) pc_init_kernel(int n, double var, const int* start, int* pi, double* diag,
                                                      int* state, int nstate) {
  const int i = blockIdx.x * kPB + threadIdx.x;
  if (i < n) {
    pi[i] = start[i];
    diag[i] = var;   // the diagonal of Sigma is the marginal variance (CG_utils.h:453-458)
  }
  if (i < nstate) state[i] = 0;
}

// Step m: column m of L for the positions j > m of the permutation and their diagonal update
// (CG_utils.h:466-481), then this workgroup's share of err = sum |diag| and of the next pivot search
// (first maximum in position order, :461, 482).
template <int COV>
__global__ void __launch_bounds__(kPB) pc_update_kernel(const double* __restrict__ X, int d, int n, double var,
                                                        double phi, int m, int kpad, const int* __restrict__ pi,
                                                        double* diag, double* L, const int* __restrict__ state,
                                                        double* red_sum, double* red_max, int* red_pos) {
  if (state[0]) return;   // stopped early: the remaining steps are no-ops
  extern __shared__ double lds[];
  double* Lp = lds;                                   // kpad: row pi(m) of the columns before m
  __shared__ double s_sum[kPB], s_max[kPB];
  __shared__ int s_pos[kPB];
  const int tid = threadIdx.x;
  const int p = pi[m];
  const double dp = diag[p];   // before this step's updates (row p itself is not updated)
  const double sq = sqrt(dp);
  for (int a = tid; a < m; a += kPB) Lp[a] = L[(size_t)p * kpad + a];
  __syncthreads();
  const int j = m + 1 + blockIdx.x * kPB + tid;
  double vsum = 0., vmax = -DBL_MAX;
  int vpos = INT_MAX;
  if (j < n) {
    const int r = pi[j];
    double s = 0.;
    for (int q = 0; q < d; ++q) {
      const double df = X[(size_t)r * d + q] - X[(size_t)p * d + q];
      s = fma(df, df, s);
    }
    double c, dc;
    cov_dcov_sq<COV>(s, var, phi, c, dc);
    double* Lr = L + (size_t)r * kpad;
    double dot = 0.;
    for (int a = 0; a < m; ++a) dot = fma(Lr[a], Lp[a], dot);
    double l = c - dot;
    if (!(fabs(l) < kPivCholDropTol)) {   // small entries: not stored, not divided, still subtracted (:476-480)
      l /= sq;
      Lr[m] = l;
    }
    const double dn = diag[r] - l * l;
    diag[r] = dn;
    vsum = fabs(dn);
    vmax = dn;
    vpos = j;
  }
  if (blockIdx.x == 0 && tid == 0) L[(size_t)p * kpad + m] = sq;   // :485
  s_sum[tid] = vsum;
  s_max[tid] = vmax;
  s_pos[tid] = vpos;
  __syncthreads();
  for (int off = kPB / 2; off > 0; off >>= 1) {
    if (tid < off) {
      s_sum[tid] += s_sum[tid + off];
      const double o = s_max[tid + off];
      const int op = s_pos[tid + off];
      if (o > s_max[tid] || (o == s_max[tid] && op < s_pos[tid])) {
        s_max[tid] = o;
        s_pos[tid] = op;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    red_sum[blockIdx.x] = s_sum[0];
    red_max[blockIdx.x] = s_max[0];
    red_pos[blockIdx.x] = s_pos[0];
  }
}

// End of step m (one workgroup): err and the next pivot from the nb partial results, the loop test
// m + 1 < k && err > tol (:460), and the swap of the permutation (:463-465).
__global__ void __launch_bounds__(kPB) pc_finish_kernel(int nb, int m, int k, double tol, const double* red_sum,
                                                        const double* red_max, const int* red_pos, int* pi,
                                                        int* state) {
  if (state[0]) return;
  __shared__ double s_sum[kPB], s_max[kPB];
  __shared__ int s_pos[kPB];
  const int tid = threadIdx.x;
  double vsum = 0., vmax = -DBL_MAX;
  int vpos = INT_MAX;
  for (int b = tid; b < nb; b += kPB) {   // positions ascend with b: ties keep the lower position
    vsum += red_sum[b];
    if (red_max[b] > vmax || (red_max[b] == vmax && red_pos[b] < vpos)) {
      vmax = red_max[b];
      vpos = red_pos[b];
    }
  }
  s_sum[tid] = vsum;
  s_max[tid] = vmax;
  s_pos[tid] = vpos;
  __syncthreads();
  for (int off = kPB / 2; off > 0; off >>= 1) {
    if (tid < off) {
      s_sum[tid] += s_sum[tid + off];
      const double o = s_max[tid + off];
      const int op = s_pos[tid + off];
      if (o > s_max[tid] || (o == s_max[tid] && op < s_pos[tid])) {
        s_max[tid] = o;
        s_pos[tid] = op;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    state[kStateHead + m] = pi[m];
    state[1] = m + 1;
    const double err = s_sum[0];
    const int i = s_pos[0];
    if (!(m + 1 < k && err > tol) || i == INT_MAX) {
      state[0] = 1;
    } else {
      const int old = pi[m + 1];
      pi[m + 1] = pi[i];
      pi[i] = old;
    }
  }
}

// ---------------------------------------------------------------- split-n products
// part[b][a * nc + c] = sum over the rows of range b of A[i, a] * w[i] * Bm[i, c] (a < k, c < nc; w nullable).
// A: leading dimension lda, Bm: ldb. The rows of a range pass through LDS in chunks; a thread owns the
// output entries idx = tid, tid + kPB, ... and adds chunk after chunk in row order.
__global__ void __launch_bounds__(kPB) tn_partial_kernel(int n, int rows_per_range, int chunk, const double* __restrict__ A,
                                                         int lda, int k, const double* __restrict__ w,
                                                         const double* __restrict__ Bm, int ldb, int nc, double* part,
                                                         int* flags) {
  extern __shared__ double lds[];
  double* As = lds;                       // chunk x k
  double* Bs = lds + (size_t)chunk * k;   // chunk x nc (scaled by w)
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * rows_per_range, r1 = min(n, r0 + rows_per_range);
  double* out = part + (size_t)blockIdx.x * k * nc;
  const int cnt = k * nc;
  int bad = 0;
  bool first = true;
  for (int c0 = r0; c0 < r1 || first; c0 += chunk) {
    const int rows = max(0, min(chunk, r1 - c0));
    __syncthreads();
    for (int e = tid; e < rows * k; e += kPB) As[e] = A[(size_t)(c0 + e / k) * lda + e % k];
    for (int e = tid; e < rows * nc; e += kPB) {
      const int r = e / nc;
      const double wi = w ? w[c0 + r] : 1.;
      if (flags != nullptr && e % nc == 0) {
        if (wi > 1e10) bad |= 1;
        if (!(wi > 0.) || isinf(wi)) bad |= 2;
      }
      Bs[e] = wi * Bm[(size_t)(c0 + r) * ldb + e % nc];
    }
    __syncthreads();
    for (int idx = tid; idx < cnt; idx += kPB) {
      const int a = idx / nc, c = idx % nc;
      double acc = first ? 0. : out[idx];
      for (int r = 0; r < rows; ++r) acc = fma(As[r * k + a], Bs[r * nc + c], acc);
      out[idx] = acc;
    }
    first = false;
  }
  if (flags != nullptr && bad) atomicOr(flags, bad);
}

// out[idx] = (eye && row == col) + sum_b part[b][idx]: 16 outputs x 16 groups per workgroup; group g adds the
// partials g, g + 16, ... in ascending order, then the 16 group sums are added in group order (a fixed order)
__global__ void __launch_bounds__(kPB) tn_reduce_kernel(int nb, int cnt, int nc, int eye, const double* __restrict__ part,
                                                        double* out) {
  __shared__ double sh[16][17];
  const int ox = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int idx = blockIdx.x * 16 + ox;
  double s = 0.;
  if (idx < cnt)
    for (int b = g; b < nb; b += 16) s += part[(size_t)b * cnt + idx];
  sh[g][ox] = s;
  __syncthreads();
  if (g == 0 && idx < cnt) {
    double tot = 0.;
    for (int q = 0; q < 16; ++q) tot += sh[q][ox];
    out[idx] = (eye && idx / nc == idx % nc) ? tot + 1. : tot;
  }
}

// One workgroup: G (k x k row-major, lower triangle) -> its Cholesky factor E in place, log|G| = 2 sum
// log E_jj, Ei = E^-1 and M = Ei^T Ei = G^-1. Global memory throughout (k x k may exceed LDS); the
// workgroup barrier orders the steps.
__global__ void __launch_bounds__(1024) kk_factor_kernel(int k, double* G, double* Ei, double* M, double* out,
                                                         int* flags) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int j = 0; j < k; ++j) {
    __syncthreads();
    if (tid == 0) {
      const double dj = G[(size_t)j * k + j];
      if (!(dj > 0.)) atomicOr(flags, 4);
      G[(size_t)j * k + j] = sqrt(dj);
    }
    __syncthreads();
    const double ej = G[(size_t)j * k + j];
    for (int i = j + 1 + tid; i < k; i += nt) G[(size_t)i * k + j] /= ej;
    __syncthreads();
    const int cnt = k - j - 1;
    for (int idx = tid; idx < cnt * cnt; idx += nt) {
      const int i = j + 1 + idx / cnt, c = j + 1 + idx % cnt;
      if (c <= i) G[(size_t)i * k + c] -= G[(size_t)i * k + j] * G[(size_t)c * k + j];
    }
  }
  __syncthreads();
  if (tid == 0) {
    double ld = 0.;
    for (int j = 0; j < k; ++j) ld += log(G[(size_t)j * k + j]);
    out[0] = 2. * ld;
  }
  for (int c = tid; c < k; c += nt) {   // column c of E^-1 by forward substitution
    for (int i = 0; i < c; ++i) Ei[(size_t)i * k + c] = 0.;
    Ei[(size_t)c * k + c] = 1. / G[(size_t)c * k + c];
    for (int i = c + 1; i < k; ++i) {
      double s = 0.;
      for (int j = c; j < i; ++j) s = fma(G[(size_t)i * k + j], Ei[(size_t)j * k + c], s);
      Ei[(size_t)i * k + c] = -s / G[(size_t)i * k + i];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < k * k; idx += nt) {
    const int a = idx / k, b = idx % k;
    double s = 0.;
    for (int i = max(a, b); i < k; ++i) s = fma(Ei[(size_t)i * k + a], Ei[(size_t)i * k + b], s);
    M[idx] = s;
  }
}

// T = M S (k x k times k x t)
__global__ void __launch_bounds__(kPB) kk_apply_kernel(int k, int t, const double* __restrict__ M,
                                                       const double* __restrict__ S, double* T) {
  const int idx = blockIdx.x * kPB + threadIdx.x;
  if (idx >= k * t) return;
  const int a = idx / t, c = idx % t;
  double s = 0.;
  for (int b = 0; b < k; ++b) s = fma(M[(size_t)a * k + b], S[(size_t)b * t + c], s);
  T[idx] = s;
}

// out[i, c] = d0[i] R[i, c] + sgn d1[i] sum_a L[i, a] T[a, c]; `rows_wg` rows per workgroup with their L rows in
// LDS, and T too when t_lds (it fits the LDS budget)
__global__ void __launch_bounds__(kPB) combine_kernel(int n, int t, int k, int kpad, int rows_wg, int t_lds,
                                                      const double* __restrict__ L, const double* __restrict__ T,
                                                      const double* __restrict__ R, const double* __restrict__ d0,
                                                      const double* __restrict__ d1, double sgn, double* out) {
  extern __shared__ double lds[];   // rows_wg x k (+ k x t)
  double* Ts = lds + (size_t)rows_wg * k;
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * rows_wg;
  const int rows = min(rows_wg, n - r0);
  for (int e = tid; e < rows * k; e += kPB) lds[e] = L[(size_t)(r0 + e / k) * kpad + e % k];
  if (t_lds)
    for (int e = tid; e < k * t; e += kPB) Ts[e] = T[e];
  __syncthreads();
  const double* Tv = t_lds ? Ts : T;
  for (int idx = tid; idx < rows * t; idx += kPB) {
    const int r = idx / t, c = idx % t, i = r0 + r;
    double s = 0.;
    for (int a = 0; a < k; ++a) s = fma(lds[r * k + a], Tv[(size_t)a * t + c], s);
    const size_t o = (size_t)i * t + c;
    const double base = R ? (d0 ? d0[i] * R[o] : R[o]) : 0.;
    out[o] = base + sgn * (d1 ? d1[i] * s : s);
  }
}

__global__ void __launch_bounds__(kPB) rowdiag_kernel(int n, int k, int kpad, const double* __restrict__ L,
                                                      const double* __restrict__ M, double* diag) {
  const int i = blockIdx.x * kPB + threadIdx.x;
  if (i >= n) return;
  const double* Li = L + (size_t)i * kpad;
  double s = 0.;
  for (int a = 0; a < k; ++a) {
    const double la = Li[a];
    if (la == 0.) continue;
    double q = 0.;
    for (int b = 0; b < k; ++b) q = fma(M[(size_t)a * k + b], Li[b], q);
    s = fma(la, q, s);
  }
  diag[i] = s;
}

// ---------------------------------------------------------------- elementwise / column sums
constexpr int kCdRows = 4;   // 64 columns x 4 rows per workgroup pass
__global__ void __launch_bounds__(kPB) wcoldots_partial_kernel(int n, int t, const double* __restrict__ A,
                                                               const double* __restrict__ w,
                                                               const double* __restrict__ B, double* partials) {
  __shared__ double sh[kPB];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cx;
  double acc = 0.;
  if (c < t)
    for (int i = blockIdx.x * kCdRows + ry; i < n; i += gridDim.x * kCdRows) {
      const size_t o = (size_t)i * t + c;
      acc += w ? A[o] * w[i] * B[o] : A[o] * B[o];
    }
  sh[threadIdx.x] = acc;
  __syncthreads();
  if (ry == 0 && c < t) partials[(size_t)blockIdx.x * t + c] = ((sh[cx] + sh[64 + cx]) + sh[128 + cx]) + sh[192 + cx];
}

__global__ void __launch_bounds__(64) wcoldots_final_kernel(int nb, int t, const double* __restrict__ partials, double* out) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= t) return;
  double s = 0.;
  for (int b = 0; b < nb; ++b) s += partials[(size_t)b * t + c];
  out[c] = s;
}

__global__ void __launch_bounds__(kPB) row_scale_kernel(size_t cnt, int t, const double* __restrict__ d, int inv,
                                                        const double* X, double* Y) {
  const size_t e = (size_t)blockIdx.x * kPB + threadIdx.x;
  if (e >= cnt) return;
  const double di = d[e / t];
  Y[e] = inv ? X[e] / di : di * X[e];
}

__global__ void __launch_bounds__(kPB) add_winv_kernel(size_t cnt, int t, const double* __restrict__ w,
                                                       const double* __restrict__ H, double* V) {
  const size_t e = (size_t)blockIdx.x * kPB + threadIdx.x;
  if (e >= cnt) return;
  V[e] += H[e] / w[e / t];
}

__global__ void __launch_bounds__(kPB) rsqrt_vec_kernel(int n, const double* __restrict__ x, double* y) {
  const int i = blockIdx.x * kPB + threadIdx.x;
  if (i < n) y[i] = 1. / sqrt(x[i]);
}

__global__ void __launch_bounds__(kPB) lik_dinfo_kernel(int n, int lik, double aux, const double* __restrict__ y,
                                                        const double* __restrict__ loc, const double* __restrict__ offset,
                                                        double* dW) {
  const int i = blockIdx.x * kPB + threadIdx.x;
  if (i < n) dW[i] = lik_dinfo(lik, aux, y ? y[i] : 0., offset ? loc[i] + offset[i] : loc[i]);
}

// One wave per row; no FMA contraction: pass 2 recomputes the products of pass 1 bit-identically (for
// t = 1 the centred values are then exactly 0 -> c = 1, CalcOptimalCVectorized CG_utils.cpp:1026-1041).
__global__ void __launch_bounds__(kPB) lowrank_mode_deriv_kernel(int n, int t, const double* __restrict__ dW,
                                                                 const double* __restrict__ W,
                                                                 const double* __restrict__ rowdiag,
                                                                 const double* __restrict__ WIU,
                                                                 const double* __restrict__ WIPZ, double* dmll) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (kPB / 64) + (threadIdx.x >> 6);
  if (i >= n) return;
  const double dWi = dW[i];
  double s1 = 0., sP = 0.;
  for (int c = lane; c < t; c += 64) {
    const size_t o = (size_t)i * t + c;
    s1 += -(WIU[o] * dWi * WIPZ[o]);
    sP += -(WIPZ[o] * dWi * WIPZ[o]);
  }
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_xor(s1, off, 64);
    sP += __shfl_xor(sP, off, 64);
  }
  const double tr1 = s1 / t, trP = sP / t;
  double cv = 0., vv = 0.;
  for (int c = lane; c < t; c += 64) {
    const size_t o = (size_t)i * t + c;
    const double z1 = -(WIU[o] * dWi * WIPZ[o]) - tr1;
    const double zP = -(WIPZ[o] * dWi * WIPZ[o]) - trP;
    cv += z1 * zP;
    vv += zP * zP;
  }
  for (int off = 32; off > 0; off >>= 1) {
    cv += __shfl_xor(cv, off, 64);
    vv += __shfl_xor(vv, off, 64);
  }
  cv /= t;
  vv /= t;
  const double copt = (vv == 0.) ? 1. : cv / vv;
  const double a = dWi / W[i];           // tr(W^-1 dW / db_i)
  const double kk = rowdiag[i] * dWi;    // tr(L (I_k + L^T W L)^-1 L^T dW / db_i)
  if (lane == 0) dmll[i] = 0.5 * (tr1 + a + copt * (kk - a) - copt * trP);
}

int grid_of(size_t cnt) { return (int)((cnt + kPB - 1) / kPB); }

void launch_tn_reduce(int nb, int cnt, int nc, int eye, const double* part, double* out, hipStream_t s) {
  hipLaunchKernelGGL(tn_reduce_kernel, dim3((cnt + 15) / 16), dim3(kPB), 0, s, nb, cnt, nc, eye, part, out);
  HIP_CHECK(hipGetLastError());
}

template <int COV>
void pc_update(const double* X, int d, int n, double var, double phi, int m, int kpad, const int* pi, double* diag,
               double* L, const int* state, double* rs, double* rm, int* rp, int nb, hipStream_t s) {
  hipLaunchKernelGGL(pc_update_kernel<COV>, dim3(nb), dim3(kPB), sizeof(double) * kpad, s, X, d, n, var, phi, m, kpad,
                     pi, diag, L, state, rs, rm, rp);
}

}  // namespace

// ---------------------------------------------------------------- host restatement
int pivoted_cholesky_host(int cov_type, const double* X, int n, int d, double var, double phi, int k, double tol,
                          double* L, int* piv) {
  k = std::min(k, n);
  std::fill(L, L + (size_t)n * k, 0.);
  std::vector<double> diag(n, var);
  std::vector<int> pi(n);
  for (int h = 0; h < n; ++h) pi[h] = h;
  auto cov = [&](int a, int b) {
    double s = 0.;
    for (int q = 0; q < d; ++q) {
      const double df = X[(size_t)a * d + q] - X[(size_t)b * d + q];
      s += df * df;
    }
    double c, dc;
    const double r = std::sqrt(s);
    switch (cov_type) {
      case kMatern05: cov_dcov<kMatern05>(r, var, phi, c, dc); break;
      case kMatern15: cov_dcov<kMatern15>(r, var, phi, c, dc); break;
      case kMatern25: cov_dcov<kMatern25>(r, var, phi, c, dc); break;
      default: cov_dcov<kGaussian>(r, var, phi, c, dc); break;
    }
    return c;
  };
  int m = 0;
  double err = var * n;
  while (m == 0 || (m < k && err > tol)) {
    int i = m;   // first maximum of the remaining diagonal in position order
    for (int h = m + 1; h < n; ++h)
      if (diag[pi[h]] > diag[pi[i]]) i = h;
    std::swap(pi[m], pi[i]);
    const int p = pi[m];
    if (m + 1 < n) {
      const double sq = std::sqrt(diag[p]);
      err = 0.;
      for (int j = m + 1; j < n; ++j) {
        const int r = pi[j];
        double l = cov(r, p);
        double dot = 0.;
        for (int a = 0; a < m; ++a) dot += L[(size_t)r * k + a] * L[(size_t)p * k + a];
        l -= dot;
        if (!(std::fabs(l) < kPivCholDropTol)) {
          l /= sq;
          L[(size_t)r * k + m] = l;
        }
        diag[r] -= l * l;
        err += std::fabs(diag[r]);
      }
    }
    L[(size_t)p * k + m] = std::sqrt(diag[p]);
    if (piv) piv[m] = p;
    ++m;
  }
  return m;
}

// ---------------------------------------------------------------- LowRankPrecond
LowRankPrecond::LowRankPrecond(int n, int k, hipStream_t s) : n_(n), k_(k), kpad_((k + 7) / 8 * 8), s_(s) {
  if (k < 1 || k > n) Fatal("LowRankPrecond: rank %d outside [1, %d]", k, n);
  if (k > kMaxRank)
    Fatal("'fitc_piv_chol_preconditioner_rank' = %d: ranks above %d are not supported by gpboost_amd", k, kMaxRank);
  L_.alloc((size_t)n * kpad_);
  diag_.alloc(n);
  pi_.alloc(n);
  state_.alloc(kStateHead + k);
  const int nb = (n + kPB - 1) / kPB;
  red_val_.alloc((size_t)2 * nb);
  red_pos_.alloc(nb);
  G_.alloc((size_t)k * k);
  M_.alloc((size_t)k * k);
  S_.alloc((size_t)k * k);   // E^-1 during SetWeights; L^T (w .* Q) during Project (grown there)
  out_.alloc(4);
  HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_state_), sizeof(int) * (kStateHead + k), hipHostMallocDefault));
  HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_out_), sizeof(double) * 4, hipHostMallocDefault));
}

LowRankPrecond::~LowRankPrecond() {
  if (h_state_) (void)hipHostFree(h_state_);
  if (h_out_) (void)hipHostFree(h_out_);
}

void LowRankPrecond::Factorize(int cov_type, const double* X, int d, double var, double phi, const int* start) {
  const int n = n_, k = k_;
  HIP_CHECK(hipMemsetAsync(L_.get(), 0, sizeof(double) * (size_t)n * kpad_, s_));
  const int nstate = kStateHead + k;
  hipLaunchKernelGGL(pc_init_kernel, dim3(grid_of(std::max(n, nstate))), dim3(kPB), 0, s_, n, var, start, pi_.get(),
                     diag_.get(), state_.get(), nstate);
  HIP_CHECK(hipGetLastError());
  const int nb0 = (n + kPB - 1) / kPB;
  double* rs = red_val_.get();
  double* rm = red_val_.get() + nb0;
  for (int m = 0; m < k; ++m) {
    const int nb = std::max(1, (n - m - 1 + kPB - 1) / kPB);   // <= nb0
    switch (cov_type) {
      case kMatern05:
        pc_update<kMatern05>(X, d, n, var, phi, m, kpad_, pi_.get(), diag_.get(), L_.get(), state_.get(), rs, rm,
                             red_pos_.get(), nb, s_);
        break;
      case kMatern15:
        pc_update<kMatern15>(X, d, n, var, phi, m, kpad_, pi_.get(), diag_.get(), L_.get(), state_.get(), rs, rm,
                             red_pos_.get(), nb, s_);
        break;
      case kMatern25:
        pc_update<kMatern25>(X, d, n, var, phi, m, kpad_, pi_.get(), diag_.get(), L_.get(), state_.get(), rs, rm,
                             red_pos_.get(), nb, s_);
        break;
      case kGaussian:
        pc_update<kGaussian>(X, d, n, var, phi, m, kpad_, pi_.get(), diag_.get(), L_.get(), state_.get(), rs, rm,
                             red_pos_.get(), nb, s_);
        break;
      default: Fatal("pivoted Cholesky: covariance type %d is not supported", cov_type);
    }
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pc_finish_kernel, dim3(1), dim3(kPB), 0, s_, nb, m, k, kPivCholStopTol, rs, rm, red_pos_.get(),
                       pi_.get(), state_.get());
    HIP_CHECK(hipGetLastError());
  }
}

int LowRankPrecond::Rank(std::vector<int>* piv) {
  HIP_CHECK(hipMemcpyAsync(h_state_, state_.get(), sizeof(int) * (kStateHead + k_), hipMemcpyDeviceToHost, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
  const int rank = h_state_[1];
  if (piv) piv->assign(h_state_ + kStateHead, h_state_ + kStateHead + rank);
  return rank;
}

namespace {
// rows per range and LDS chunk of a split-n product with k + nc doubles per row and k * nc outputs
void split_plan(int n, int k, int nc, int* ranges, int* rows_per_range, int* chunk) {
  *chunk = std::max(1, std::min(kLdsBytes / (int)(sizeof(double) * (k + nc)), 128));
  const long out = (long)k * nc;
  const int max_ranges = (int)std::max(8L, std::min((long)kMaxPart, (4L << 20) / out));
  int r = std::min(max_ranges, (n + *chunk - 1) / *chunk);
  r = std::max(r, 1);
  *rows_per_range = (n + r - 1) / r;
  *ranges = (n + *rows_per_range - 1) / *rows_per_range;
}
}  // namespace

void LowRankPrecond::SetWeights(const double* w) {
  w_ = w;
  const int k = k_;
  int ranges, rpr, chunk;
  split_plan(n_, k, k, &ranges, &rpr, &chunk);
  const size_t need = (size_t)ranges * k * k;
  if (part_.size() < need) part_.alloc(need);
  HIP_CHECK(hipMemsetAsync(state_.get() + 2, 0, sizeof(int), s_));
  hipLaunchKernelGGL(tn_partial_kernel, dim3(ranges), dim3(kPB), sizeof(double) * (size_t)chunk * 2 * k, s_, n_, rpr,
                     chunk, L_.get(), kpad_, k, w, L_.get(), kpad_, k, part_.get(), state_.get() + 2);
  HIP_CHECK(hipGetLastError());
  launch_tn_reduce(ranges, k * k, k, 1, part_.get(), G_.get(), s_);
  if (S_.size() < (size_t)k * k) S_.alloc((size_t)k * k);
  hipLaunchKernelGGL(kk_factor_kernel, dim3(1), dim3(1024), 0, s_, k, G_.get(), S_.get(), M_.get(), out_.get(),
                     state_.get() + 2);
  HIP_CHECK(hipGetLastError());
}

double LowRankPrecond::LogDetG(int* flags) {
  HIP_CHECK(hipMemcpyAsync(h_state_, state_.get(), sizeof(int) * kStateHead, hipMemcpyDeviceToHost, s_));
  HIP_CHECK(hipMemcpyAsync(h_out_, out_.get(), sizeof(double), hipMemcpyDeviceToHost, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
  if (flags) *flags = h_state_[2];
  return h_out_[0];
}

void LowRankPrecond::Project(const double* Q, int t) {
  if (w_ == nullptr) Fatal("LowRankPrecond: SetWeights must precede an application");
  const int k = k_;
  int ranges, rpr, chunk;
  split_plan(n_, k, t, &ranges, &rpr, &chunk);
  const size_t need = (size_t)ranges * k * t;
  if (part_.size() < need) part_.alloc(need);
  if (S_.size() < (size_t)k * std::max(t, k)) S_.alloc((size_t)k * std::max(t, k));
  if (T_.size() < (size_t)k * t) T_.alloc((size_t)k * t);
  hipLaunchKernelGGL(tn_partial_kernel, dim3(ranges), dim3(kPB), sizeof(double) * (size_t)chunk * (k + t), s_, n_, rpr,
                     chunk, L_.get(), kpad_, k, w_, Q, t, t, part_.get(), (int*)nullptr);
  HIP_CHECK(hipGetLastError());
  launch_tn_reduce(ranges, k * t, t, 0, part_.get(), S_.get(), s_);
  hipLaunchKernelGGL(kk_apply_kernel, dim3(grid_of((size_t)k * t)), dim3(kPB), 0, s_, k, t, M_.get(), S_.get(), T_.get());
  HIP_CHECK(hipGetLastError());
}

void LowRankPrecond::Combine(const double* R, const double* d0, const double* d1, double sgn, const double* Q,
                             const double* Tin, double* out, int t) {
  if (Q != nullptr) Project(Q, t);
  const double* T = Q != nullptr ? T_.get() : Tin;
  // rows per workgroup: about one (row, column) pair per thread pass for narrow blocks, 32 rows for wide ones,
  // within the LDS budget; T joins them in LDS when both fit
  const int budget = kLdsBytes / (int)sizeof(double);
  int rows_wg = std::max(8, std::min(64, t >= 32 ? 32 : kPB / t));
  rows_wg = std::max(1, std::min(rows_wg, budget / k_));
  const int t_lds = (size_t)rows_wg * k_ + (size_t)k_ * t <= (size_t)budget ? 1 : 0;
  const size_t lds = sizeof(double) * ((size_t)rows_wg * k_ + (t_lds ? (size_t)k_ * t : 0));
  hipLaunchKernelGGL(combine_kernel, dim3((n_ + rows_wg - 1) / rows_wg), dim3(kPB), lds, s_, n_, t, k_, kpad_, rows_wg,
                     t_lds, L_.get(), T, R, d0, d1, sgn, out);
  HIP_CHECK(hipGetLastError());
}

void LowRankPrecond::Apply(const double* R, double* Z, int t) { Combine(R, w_, w_, -1., R, nullptr, Z, t); }

void LowRankPrecond::RowDiag(double* diag) {
  hipLaunchKernelGGL(rowdiag_kernel, dim3(grid_of(n_)), dim3(kPB), 0, s_, n_, k_, kpad_, L_.get(), M_.get(), diag);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------- launchers
void launch_weighted_coldots(int n, int t, const double* A, const double* w, const double* B, double* partials,
                             double* out, hipStream_t s) {
  const int nb = std::max(1, std::min(512, (n + kCdRows - 1) / kCdRows));
  const int gy = (t + 63) / 64;
  hipLaunchKernelGGL(wcoldots_partial_kernel, dim3(nb, gy), dim3(kPB), 0, s, n, t, A, w, B, partials);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(wcoldots_final_kernel, dim3(gy), dim3(64), 0, s, nb, t, partials, out);
  HIP_CHECK(hipGetLastError());
}

void launch_row_scale(int n, int t, const double* d, bool inv, const double* X, double* Y, hipStream_t s) {
  const size_t cnt = (size_t)n * t;
  hipLaunchKernelGGL(row_scale_kernel, dim3(grid_of(cnt)), dim3(kPB), 0, s, cnt, t, d, inv ? 1 : 0, X, Y);
  HIP_CHECK(hipGetLastError());
}

void launch_add_winv(int n, int t, const double* w, const double* H, double* V, hipStream_t s) {
  const size_t cnt = (size_t)n * t;
  hipLaunchKernelGGL(add_winv_kernel, dim3(grid_of(cnt)), dim3(kPB), 0, s, cnt, t, w, H, V);
  HIP_CHECK(hipGetLastError());
}

void launch_rsqrt_vec(int n, const double* x, double* y, hipStream_t s) {
  hipLaunchKernelGGL(rsqrt_vec_kernel, dim3(grid_of(n)), dim3(kPB), 0, s, n, x, y);
  HIP_CHECK(hipGetLastError());
}

void launch_lowrank_mode_deriv(int n, int t, const double* dW, const double* W, const double* rowdiag, const double* WIU,
                               const double* WIPZ, double* dmll, hipStream_t s) {
  const int rows = kPB / 64;
  hipLaunchKernelGGL(lowrank_mode_deriv_kernel, dim3((n + rows - 1) / rows), dim3(kPB), 0, s, n, t, dW, W, rowdiag, WIU,
                     WIPZ, dmll);
  HIP_CHECK(hipGetLastError());
}

void launch_lik_dinfo(int n, int lik, double aux, const double* y, const double* loc, const double* offset, double* dW,
                      hipStream_t s) {
  hipLaunchKernelGGL(lik_dinfo_kernel, dim3(grid_of(n)), dim3(kPB), 0, s, n, lik, aux, y, loc, offset, dW);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gpb_amd
