// GroupedLaplace: kernels and host driver (grouped_laplace.h).
#include "grouped_laplace.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <utility>

#include "grouped_test.h"
#include "lik_device.h"
#include "lik_test.h"
#include "slq_host.h"
#include "wave_ops.h"

namespace gpb_amd {

namespace {

constexpr int kMaxBlocks = 1024;      // blocks of an observation pass (grid-stride; fixed by n -> fixed sum order)
constexpr int kShortLen = 32;         // destinations of at most this many observations: one thread each
constexpr int kChunkLen = 512;        // chunk of a longer list: one wave, 8 observations per lane
constexpr int kRed = 128;             // scalar slots
// slots of the general shape gradient (negative_binomial); 0 .. 63 are the evaluation's and the gamma gradient's
constexpr int kRedAuxSum = 64;        // sum_i log(mu_i + r) + (y_i + r) / (mu_i + r)
constexpr int kRedAuxTrace = 65;      // cholesky: sum_i (dW / dlog r)_i q_i
constexpr int kRedAuxImp = 72;        // K: v_k^T (Z^T dd1 / dlog r)_k
constexpr int kRedAuxDinv = 80;       // K, iterative: sum over effect k of diag(Z^T dW/dlog r Z) / D

struct EffArgs {   // per-effect constants, by value
  int K;
  int cum[kGlpMaxK + 1];
  double sigi[kGlpMaxK];   // 1 / sigma_k^2
};

__device__ __forceinline__ int effect_of(const EffArgs& a, int r) {
  int k = 0;
  while (k + 1 < a.K && r >= a.cum[k + 1]) ++k;
  return k;
}

// sum over the 256 threads of a block, in every thread (fixed order)
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = lane_group_sum<64>(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return r;
}

// Observation pass: eta_i = F_i + sum_k b[lev_k(i)] (K gathers), the log-likelihood summed per block, and
// (DERIV) d1, W and, when asked, dW / deta from the same read of y. WT (random slopes): eta_i = F_i + sum_k
// zw[k n + i] b[lev_k(i)], one more coalesced read per gather.
template <bool DERIV, bool WT>
__global__ void __launch_bounds__(256) glp_obs_kernel(int n, int K, const int* __restrict__ glev,
                                                      const double* __restrict__ zw, const double* __restrict__ y, const double* __restrict__ F,
                                                      const double* __restrict__ b, int lik, double aux,
                                                      double* __restrict__ d1, double* __restrict__ W,
                                                      double* __restrict__ dW, double* __restrict__ partial) {
  __shared__ double sh[4];
  double ll = 0.;
  if (lik == kLikNegBinomial) {   // kernel-uniform: the nb_* functions with log(shape) taken once per thread
    const double log_r = log(aux);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
      double eta = F != nullptr ? F[i] : 0.;
      for (int k = 0; k < K; ++k)
        eta += WT ? zw[(size_t)k * n + i] * b[glev[(size_t)k * n + i]] : b[glev[(size_t)k * n + i]];
      const double yi = y[i];
      ll += nb_loglik(aux, log_r, yi, eta);
      if (DERIV) {
        d1[i] = nb_d1(aux, log_r, yi, eta);
        W[i] = nb_info(aux, log_r, yi, eta);
        if (dW != nullptr) dW[i] = nb_dinfo(aux, log_r, yi, eta);
      }
    }
  } else {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
      double eta = F != nullptr ? F[i] : 0.;
      for (int k = 0; k < K; ++k)
        eta += WT ? zw[(size_t)k * n + i] * b[glev[(size_t)k * n + i]] : b[glev[(size_t)k * n + i]];
      const double yi = y[i];
      ll += lik_loglik(lik, aux, yi, eta);
      if (DERIV) {
        d1[i] = lik_d1(lik, aux, yi, eta);
        W[i] = lik_info(lik, aux, yi, eta);
        if (dW != nullptr) dW[i] = lik_dinfo(lik, aux, yi, eta);
      }
    }
  }
  ll = block_sum(ll, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = ll;
}

// negative_binomial, at the converged mode: the shape derivatives dd1 / dlog r and dW / dlog r per observation and
// per block the sum of log(mu_i + r) + (y_i + r) / (mu_i + r) (the explicit shape gradient, likelihoods.h:10527-10538);
// grid, stride and block sum as glp_obs_kernel, finished by glp_finish_kernel
template <bool WT>
__global__ void __launch_bounds__(256) glp_nb_aux_kernel(int n, int K, const int* __restrict__ glev,
                                                         const double* __restrict__ zw, const double* __restrict__ y, const double* __restrict__ F,
                                                         const double* __restrict__ b, double aux,
                                                         double* __restrict__ dd1a, double* __restrict__ dWa,
                                                         double* __restrict__ partial) {
  __shared__ double sh[4];
  const double log_r = log(aux);
  double acc = 0.;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    double eta = F != nullptr ? F[i] : 0.;
    for (int k = 0; k < K; ++k)
      eta += WT ? zw[(size_t)k * n + i] * b[glev[(size_t)k * n + i]] : b[glev[(size_t)k * n + i]];
    const double yi = y[i];
    dd1a[i] = nb_dd1_aux(aux, log_r, yi, eta);
    dWa[i] = nb_dinfo_aux(aux, log_r, yi, eta);
    acc += nb_aux_term(aux, log_r, yi, eta);
  }
  acc = block_sum(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// out[c] = sum_j partial[c nb + j], one block per column
__global__ void __launch_bounds__(256) glp_finish_kernel(int nb, const double* __restrict__ partial,
                                                         double* __restrict__ out) {
  __shared__ double sh[4];
  double s = 0.;
  for (int j = threadIdx.x; j < nb; j += 256) s += partial[(size_t)blockIdx.x * nb + j];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// Segmented sums, short destinations: out[d] = sum of w over d's observations, in list order. WT (random slopes):
// entry e of the lists carries the precomputed value sw[e] of Z (z_a[i] for Z^T v, z_a[i] z_b[i] for a destination
// of Z^T W Z), streamed beside obs[e].
template <bool WT>
__global__ void __launch_bounds__(256) glp_seg_short_kernel(int ndst, const int* __restrict__ ptr,
                                                            const int* __restrict__ obs, const double* __restrict__ sw,
                                                            const double* __restrict__ w, double* __restrict__ out) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= ndst) return;
  const int e0 = ptr[d], e1 = ptr[d + 1];
  if (e1 - e0 > kShortLen) return;   // chunked
  double s = 0.;
  for (int e = e0; e < e1; ++e) s += WT ? sw[e] * w[obs[e]] : w[obs[e]];
  out[d] = s;
}

// long destinations, stage 1: one wave per chunk
template <bool WT>
__global__ void __launch_bounds__(256) glp_seg_chunk_kernel(int nchunks, const int* __restrict__ c0,
                                                            const int* __restrict__ c1, const int* __restrict__ obs,
                                                            const double* __restrict__ sw, const double* __restrict__ w,
                                                            double* __restrict__ P) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nchunks) return;   // wave-uniform
  const int lane = threadIdx.x & 63;
  double s = 0.;
  const int e1 = c1[q];
  for (int e = c0[q] + lane; e < e1; e += 64) s += WT ? sw[e] * w[obs[e]] : w[obs[e]];
  s = lane_group_sum<64>(s);
  if (lane == 0) P[q] = s;
}

// stage 2: the chunk partials of a destination in chunk order
__global__ void __launch_bounds__(256) glp_seg_long_kernel(int nlong, const int* __restrict__ dst,
                                                           const int* __restrict__ cptr, const double* __restrict__ P,
                                                           double* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nlong) return;
  double s = 0.;
  for (int q = cptr[j]; q < cptr[j + 1]; ++q) s += P[q];
  out[dst[j]] = s;
}

enum VecOp : int {
  kVecDiag = 0,   // out = sigi + x                  (diag(A) from diag(Z^T W Z))
  kVecRhs,        // out = x - sigi y                (Z^T d1 - Sigma^-1 b)
  kVecDiv,        // out = x / y
  kVecAxpy,       // out = x + alpha y
  kVecInvSqrt,    // out = sqrt(1 / x)
};
template <int OP>
__global__ void __launch_bounds__(256) glp_vec_kernel(int M, EffArgs a, double alpha, const double* __restrict__ x,
                                                      const double* __restrict__ y, double* __restrict__ out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= M) return;
  if (OP == kVecDiag) out[r] = a.sigi[effect_of(a, r)] + x[r];
  if (OP == kVecRhs) out[r] = x[r] - a.sigi[effect_of(a, r)] * y[r];
  if (OP == kVecDiv) out[r] = x[r] / y[r];
  if (OP == kVecAxpy) out[r] = x[r] + alpha * y[r];
  if (OP == kVecInvSqrt) out[r] = sqrt(1. / x[r]);
}

// out[k] = sum over the rows of effect k of x y (MODE 1: of log x, 2: of 1 / x, 3: of x / y); one block per effect
template <int MODE>
__global__ void __launch_bounds__(256) glp_effect_dots_kernel(EffArgs a, const double* __restrict__ x,
                                                              const double* __restrict__ y, double* __restrict__ out) {
  __shared__ double sh[4];
  const int k = blockIdx.x;
  double s = 0.;
  for (int r = a.cum[k] + threadIdx.x; r < a.cum[k + 1]; r += 256)
    s += MODE == 1 ? log(x[r]) : MODE == 2 ? 1. / x[r] : MODE == 3 ? x[r] / y[r] : x[r] * y[r];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) out[k] = s;
}

// q_ij = sum_k A^-1[lev_j(i), lev_k(i)] (K^2 gathers from the dense inverse; K == 1: 1 / D), q_i = sum_j q_ij;
// written: dwq_i = dW_i q_i / 2 and per block the sums of W_i q_ij (column j); AUX: also the sums of Wa_i q_i
// (column K: the determinant term of a shape whose dW / dlog shape is not W). WT (random slopes): q_ij =
// z_j(i) sum_k z_k(i) A^-1[lev_j(i), lev_k(i)] (K == 1: z^2 / D), z from the K x n table zw.
template <bool AUX, bool WT>
__global__ void __launch_bounds__(256) glp_q_kernel(int n, int K, const int* __restrict__ glev,
                                                    const double* __restrict__ zw,
                                                    const double* __restrict__ Ainv, int ld,
                                                    const double* __restrict__ D, const double* __restrict__ W,
                                                    const double* __restrict__ dW, const double* __restrict__ Wa,
                                                    double* __restrict__ dwq, double* __restrict__ partial) {
  __shared__ double sh[4];
  double tra = 0.;
  double tr[kGlpMaxK];
#pragma unroll
  for (int j = 0; j < kGlpMaxK; ++j) tr[j] = 0.;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    int g[kGlpMaxK];
#pragma unroll
    for (int k = 0; k < kGlpMaxK; ++k) g[k] = k < K ? glev[(size_t)k * n + i] : 0;
    double z[kGlpMaxK];
    if (WT) {
#pragma unroll
      for (int k = 0; k < kGlpMaxK; ++k) z[k] = k < K ? zw[(size_t)k * n + i] : 0.;
    }
    const double wi = W[i];
    double qi = 0.;
#pragma unroll
    for (int j = 0; j < kGlpMaxK; ++j) {
      if (j < K) {
        double qj = 0.;
        if (Ainv == nullptr) {
          qj = WT ? z[0] * z[0] / D[g[0]] : 1. / D[g[0]];
        } else if (WT) {
#pragma unroll
          for (int k = 0; k < kGlpMaxK; ++k)
            if (k < K) qj += z[k] * Ainv[(size_t)g[k] * ld + g[j]];
          qj *= z[j];
        } else {
          for (int k = 0; k < K; ++k) qj += Ainv[(size_t)g[k] * ld + g[j]];
        }
        qi += qj;
        tr[j] += wi * qj;
      }
    }
    dwq[i] = 0.5 * dW[i] * qi;
    if (AUX) tra += Wa[i] * qi;
  }
#pragma unroll
  for (int j = 0; j < kGlpMaxK; ++j) {
    if (j < K) {   // block-uniform
      const double s = block_sum(tr[j], sh);
      if (threadIdx.x == 0) partial[(size_t)j * gridDim.x + blockIdx.x] = s;
    }
  }
  if (AUX) {
    const double s = block_sum(tra, sh);
    if (threadIdx.x == 0) partial[(size_t)K * gridDim.x + blockIdx.x] = s;
  }
}

// iterative: dwq_i = dW_i mean_c[(Z U)_ic (Z V)_ic] / 2 from the M x t blocks U = A^-1 z and V = P^-1 z (row-major:
// K gathered rows of t doubles per observation; no n x t matrix is formed). WT: row k enters with z_k(i).
template <bool WT>
__global__ void __launch_bounds__(256) glp_row_trace_kernel(int n, int K, int t, const int* __restrict__ glev,
                                                            const double* __restrict__ zw, const double* __restrict__ U, const double* __restrict__ V,
                                                            const double* __restrict__ dW, double* __restrict__ dwq) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  size_t g[kGlpMaxK];
#pragma unroll
  for (int k = 0; k < kGlpMaxK; ++k) g[k] = k < K ? (size_t)glev[(size_t)k * n + i] * t : 0;
  double z[kGlpMaxK];
  if (WT) {
#pragma unroll
    for (int k = 0; k < kGlpMaxK; ++k) z[k] = k < K ? zw[(size_t)k * n + i] : 0.;
  }
  double acc = 0.;
  for (int c = 0; c < t; ++c) {
    double a = 0., p = 0.;
#pragma unroll
    for (int k = 0; k < kGlpMaxK; ++k) {
      if (k < K) {
        a += WT ? z[k] * U[g[k] + c] : U[g[k] + c];
        p += WT ? z[k] * V[g[k] + c] : V[g[k] + c];
      }
    }
    acc += a * p;
  }
  dwq[i] = 0.5 * dW[i] * (acc / t);
}

// gradient wrt the fixed effects: -d1_i + dW_i q_i / 2 - W_i (Z v)_i
template <bool WT>
__global__ void __launch_bounds__(256) glp_grad_f_kernel(int n, int K, const int* __restrict__ glev,
                                                         const double* __restrict__ zw, const double* __restrict__ d1, const double* __restrict__ dwq,
                                                         const double* __restrict__ W, const double* __restrict__ v,
                                                         double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double zv = 0.;
  for (int k = 0; k < K; ++k)
    zv += WT ? zw[(size_t)k * n + i] * v[glev[(size_t)k * n + i]] : v[glev[(size_t)k * n + i]];
  out[i] = -d1[i] + dwq[i] - W[i] * zv;
}

inline int blocks_of(int count) { return (count + 255) / 256; }
// blocks of an observation pass (nb_)
inline int obs_blocks(int n) { return std::max(1, std::min(blocks_of(n), kMaxBlocks)); }

// Launches of the observation kernels: zw null runs the unweighted instantiation (models without random slopes),
// else the weighted one on the K x n table of Z's values.
void launch_glp_obs(int nb, bool deriv, const double* zw, int n, int K, const int* glev, const double* y,
                    const double* F, const double* b, int lik, double aux, double* d1, double* W, double* dW,
                    double* partial, hipStream_t s) {
  if (zw != nullptr) {
    if (deriv) glp_obs_kernel<true, true><<<nb, 256, 0, s>>>(n, K, glev, zw, y, F, b, lik, aux, d1, W, dW, partial);
    else glp_obs_kernel<false, true><<<nb, 256, 0, s>>>(n, K, glev, zw, y, F, b, lik, aux, nullptr, nullptr, nullptr, partial);
  } else {
    if (deriv) glp_obs_kernel<true, false><<<nb, 256, 0, s>>>(n, K, glev, zw, y, F, b, lik, aux, d1, W, dW, partial);
    else glp_obs_kernel<false, false><<<nb, 256, 0, s>>>(n, K, glev, zw, y, F, b, lik, aux, nullptr, nullptr, nullptr, partial);
  }
}
void launch_glp_nb_aux(int nb, const double* zw, int n, int K, const int* glev, const double* y, const double* F,
                       const double* b, double aux, double* dd1a, double* dWa, double* partial, hipStream_t s) {
  if (zw != nullptr) glp_nb_aux_kernel<true><<<nb, 256, 0, s>>>(n, K, glev, zw, y, F, b, aux, dd1a, dWa, partial);
  else glp_nb_aux_kernel<false><<<nb, 256, 0, s>>>(n, K, glev, zw, y, F, b, aux, dd1a, dWa, partial);
}
void launch_glp_q(int nb, bool aux, const double* zw, int n, int K, const int* glev, const double* Ainv, int ld,
                  const double* D, const double* W, const double* dW, const double* Wa, double* dwq, double* partial,
                  hipStream_t s) {
  if (zw != nullptr) {
    if (aux) glp_q_kernel<true, true><<<nb, 256, 0, s>>>(n, K, glev, zw, Ainv, ld, D, W, dW, Wa, dwq, partial);
    else glp_q_kernel<false, true><<<nb, 256, 0, s>>>(n, K, glev, zw, Ainv, ld, D, W, dW, nullptr, dwq, partial);
  } else {
    if (aux) glp_q_kernel<true, false><<<nb, 256, 0, s>>>(n, K, glev, zw, Ainv, ld, D, W, dW, Wa, dwq, partial);
    else glp_q_kernel<false, false><<<nb, 256, 0, s>>>(n, K, glev, zw, Ainv, ld, D, W, dW, nullptr, dwq, partial);
  }
}
void launch_glp_row_trace(const double* zw, int n, int K, int t, const int* glev, const double* U, const double* V,
                          const double* dW, double* dwq, hipStream_t s) {
  if (zw != nullptr) glp_row_trace_kernel<true><<<blocks_of(n), 256, 0, s>>>(n, K, t, glev, zw, U, V, dW, dwq);
  else glp_row_trace_kernel<false><<<blocks_of(n), 256, 0, s>>>(n, K, t, glev, zw, U, V, dW, dwq);
}
void launch_glp_grad_f(const double* zw, int n, int K, const int* glev, const double* d1, const double* dwq,
                       const double* W, const double* v, double* out, hipStream_t s) {
  if (zw != nullptr) glp_grad_f_kernel<true><<<blocks_of(n), 256, 0, s>>>(n, K, glev, zw, d1, dwq, W, v, out);
  else glp_grad_f_kernel<false><<<blocks_of(n), 256, 0, s>>>(n, K, glev, zw, d1, dwq, W, v, out);
}

}  // namespace

GroupedLaplace::GroupedLaplace(GroupedRE* re, const std::vector<std::vector<int>>& levels, int lik,
                               const std::vector<const double*>& weights)
    : re_(re), v_(re->view()), lik_(lik), s_(v_.s) {
  const int n = v_.n, K = v_.K, M = v_.M;
  if (!weights.empty() && (int)weights.size() != K) Fatal("grouped random effects: one weight array per effect");
  for (const double* w : weights) wt_ = wt_ || w != nullptr;
  if (wt_ != re->weighted()) Fatal("internal error: the weights of GroupedLaplace and GroupedRE differ");
  auto zw = [&](int k, int i) { return weights[k] != nullptr ? weights[k][i] : 1.; };
  if (K > kGlpMaxK)
    Fatal("non-Gaussian likelihoods with grouped random effects: at most %d grouping variables are supported by "
          "gpboost_amd", kGlpMaxK);
  const std::vector<int>& cum = *v_.cum;
  nb_ = obs_blocks(n);
  std::vector<int> glev((size_t)K * n);
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < n; ++i) glev[(size_t)k * n + i] = cum[k] + levels[k][i];
  // inverted index: the M levels (observations ascending), then the CSR slots of Z^T Z. The CSR holds the
  // distinct (row, column) pairs in ascending order, so slot e is the e-th distinct key of the sorted pairs.
  const int ND = M + v_.nnz;
  std::vector<int> ptr(ND + 1, 0), obs;
  obs.reserve((size_t)n * K * K);
  // weighted: Z's value of every list entry, z_k[i] for the M levels as destinations of Z^T v (w1) and z_k[i]^2 /
  // z_a[i] z_b[i] for the destinations of Z^T W Z (w2)
  std::vector<double> w1, w2;
  std::vector<int> blk(wt_ ? M : 0);
  for (int k = 0; wt_ && k < K; ++k)
    for (int r = cum[k]; r < cum[k + 1]; ++r) blk[r] = k;
  {
    std::vector<int> cnt(M, 0);
    for (size_t e = 0; e < glev.size(); ++e) ++cnt[glev[e]];
    for (int r = 0; r < M; ++r) ptr[r + 1] = ptr[r] + cnt[r];
    obs.resize((size_t)n * K);
    std::vector<int> fill(ptr.begin(), ptr.begin() + M);
    if (wt_) {
      w1.resize((size_t)n * K);
      w2.reserve((size_t)n * K * K);
      w2.resize((size_t)n * K);
    }
    for (int k = 0; k < K; ++k)
      for (int i = 0; i < n; ++i) {
        const int e = fill[glev[(size_t)k * n + i]]++;
        obs[e] = i;
        if (wt_) {
          w1[e] = zw(k, i);
          w2[e] = w1[e] * w1[e];
        }
      }
  }
  if (K > 1) {
    std::vector<std::pair<int64_t, int>> pairs;
    pairs.reserve((size_t)n * K * (K - 1));
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < K; ++k)
        for (int l = 0; l < K; ++l)
          if (k != l)
            pairs.emplace_back((int64_t)glev[(size_t)k * n + i] * M + glev[(size_t)l * n + i], i);
    std::sort(pairs.begin(), pairs.end());
    int slot = 0;
    for (size_t a = 0; a < pairs.size();) {
      size_t b = a;
      const int pr = (int)(pairs[a].first / M), pc = (int)(pairs[a].first % M);
      while (b < pairs.size() && pairs[b].first == pairs[a].first) {
        if (wt_) w2.push_back(zw(blk[pr], pairs[b].second) * zw(blk[pc], pairs[b].second));
        obs.push_back(pairs[b++].second);
      }
      if (slot >= v_.nnz) Fatal("internal error: the inverted index does not match the CSR of Z^T Z");
      ptr[M + slot + 1] = (int)obs.size();
      ++slot;
      a = b;
    }
    if (slot != v_.nnz) Fatal("internal error: the inverted index does not match the CSR of Z^T Z");
  }
  std::vector<int> c0, c1, long_dst, long_cptr(1, 0);
  for (int d = 0; d < ND; ++d) {
    if (d == M) {
      n_long_diag_ = (int)long_dst.size();
      n_chunks_diag_ = (int)c0.size();
    }
    if (ptr[d + 1] - ptr[d] <= kShortLen) continue;
    for (int e = ptr[d]; e < ptr[d + 1]; e += kChunkLen) {
      c0.push_back(e);
      c1.push_back(std::min(e + kChunkLen, ptr[d + 1]));
    }
    long_dst.push_back(d);
    long_cptr.push_back((int)c0.size());
  }
  if (ND == M) {
    n_long_diag_ = (int)long_dst.size();
    n_chunks_diag_ = (int)c0.size();
  }
  n_long_ = (int)long_dst.size();
  n_chunks_ = (int)c0.size();
  auto upload = [&](DevBuf<int>& dst, const std::vector<int>& src) {
    dst.alloc(std::max<size_t>(src.size(), 1));
    if (!src.empty())
      HIP_CHECK(hipMemcpyAsync(dst.get(), src.data(), sizeof(int) * src.size(), hipMemcpyHostToDevice, s_));
  };
  upload(d_glev_, glev);
  upload(d_seg_ptr_, ptr);
  upload(d_seg_obs_, obs);
  upload(d_c0_, c0);
  upload(d_c1_, c1);
  upload(d_long_dst_, long_dst);
  upload(d_long_cptr_, long_cptr);
  if (wt_) {
    std::vector<double> tab((size_t)K * n);
    for (int k = 0; k < K; ++k)
      for (int i = 0; i < n; ++i) tab[(size_t)k * n + i] = zw(k, i);
    auto upload_d = [&](DevBuf<double>& dst, const std::vector<double>& src) {
      dst.alloc(std::max<size_t>(src.size(), 1));
      HIP_CHECK(hipMemcpyAsync(dst.get(), src.data(), sizeof(double) * src.size(), hipMemcpyHostToDevice, s_));
    };
    upload_d(d_zw_, tab);
    upload_d(d_seg_w1_, w1);
    upload_d(d_seg_w2_, w2);
    HIP_CHECK(hipStreamSynchronize(s_));   // tab goes out of scope
  }
  d_chunk_P_.alloc(std::max(n_chunks_, 1));
  for (auto* b : {&d_y_, &d_d1_, &d_W_, &d_dW_, &d_dwq_}) b->alloc(n);
  for (auto* b : {&d_mode_, &d_mode_new_, &d_mode_prev_, &d_upd_, &d_rhs_, &d_ztd1_, &d_D_, &d_dmll_, &d_vS_, &d_dis_})
    b->alloc(M);
  d_ztwz_.alloc(ND);
  d_partial_.alloc((size_t)kMaxBlocks * (kGlpMaxK + 1));   // K columns of glp_q_kernel and its shape column
  if (lik_ == kLikNegBinomial) {
    d_dd1a_.alloc(n);
    d_dWa_.alloc(n);
    d_zta_.alloc(M);
  }
  d_red_.alloc(kRed);
  HIP_CHECK(hipMemsetAsync(d_mode_.get(), 0, sizeof(double) * M, s_));
  HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_red_), kRed * sizeof(double), hipHostMallocDefault));
  for (auto& e : ev_) HIP_CHECK(hipEventCreate(&e));
  HIP_CHECK(hipStreamSynchronize(s_));   // the host vectors go out of scope
}

GroupedLaplace::~GroupedLaplace() {
  if (h_red_) (void)hipHostFree(h_red_);
  for (auto& e : ev_)
    if (e) (void)hipEventDestroy(e);
}

void GroupedLaplace::SetY(const double* y) {
  const int n = v_.n;
  // CheckY (likelihoods.h:637-737), CalculateLogNormalizingConstant (:8290-8310)
  lognorm_ = 0.;
  sum_log_y_ = 0.;
  if (lik_ == kLikBernoulliLogit || lik_ == kLikBernoulliProbit) {
    for (int i = 0; i < n; ++i)
      if (y[i] != 0. && y[i] != 1.)
        Fatal("The response variable ('y') needs to be 0 or 1 for likelihood = '%s' ",
              lik_ == kLikBernoulliLogit ? "bernoulli_logit" : "bernoulli_probit");
  } else if (lik_ == kLikGamma) {
    for (int i = 0; i < n; ++i) {
      if (y[i] <= 0.)
        Fatal(" Must have y > 0 for the response variable ('y') for likelihood = 'gamma', found %g ", y[i]);
      sum_log_y_ += std::log(y[i]);
    }
  } else if (lik_ == kLikPoisson) {
    for (int i = 0; i < n; ++i) {
      if (y[i] < 0.) Fatal(" Must have y >= 0 for the response variable ('y') for likelihood = 'poisson', found %g ", y[i]);
      double ip;
      if (std::modf(y[i], &ip) != 0.)
        Fatal("Found non-integer response variable ('y'). Response variable can only be integer valued for likelihood = "
              "'poisson' ");
      for (int k = 2; k <= (int)y[i]; ++k) lognorm_ -= std::log((double)k);
    }
  } else if (lik_ == kLikNegBinomial) {   // the checks of poisson (:655-667)
    for (int i = 0; i < n; ++i) {
      if (y[i] < 0.)
        Fatal(" Must have y >= 0 for the response variable ('y') for likelihood = 'negative_binomial', found %g ", y[i]);
      double ip;
      if (std::modf(y[i], &ip) != 0.)
        Fatal("Found non-integer response variable ('y'). Response variable can only be integer valued for likelihood = "
              "'negative_binomial' ");
    }
    std::vector<double> sorted(y, y + n);
    std::sort(sorted.begin(), sorted.end());
    y_vals_.clear();
    y_cnt_.clear();
    for (int i = 0; i < n; ++i) {
      if (y_vals_.empty() || sorted[i] != y_vals_.back()) {
        y_vals_.push_back(sorted[i]);
        y_cnt_.push_back(0.);
      }
      y_cnt_.back() += 1.;
    }
    lognorm_ = -SumOverY([](double x) { return std::lgamma(x); }, 1.);   // -sum log y_i! (:8308)
  }
  HIP_CHECK(hipMemcpyAsync(d_y_.get(), y, sizeof(double) * n, hipMemcpyHostToDevice, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
  y_set_ = true;
}

void GroupedLaplace::SetOffset(const double* offset) {
  has_off_ = offset != nullptr;
  if (!has_off_) return;
  d_off_.alloc(v_.n);
  HIP_CHECK(hipMemcpyAsync(d_off_.get(), offset, sizeof(double) * v_.n, hipMemcpyHostToDevice, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
}

double* GroupedLaplace::DeviceOffset() {
  d_off_.alloc(v_.n);
  has_off_ = true;
  return d_off_.get();
}

double GroupedLaplace::LogLikConst(double aux) const {
  if (lik_ == kLikPoisson) return lognorm_;
  if (lik_ == kLikGamma)   // likelihoods.h:8181-8191
    return (aux - 1.) * sum_log_y_ + v_.n * (aux * std::log(aux) - std::lgamma(aux));
  if (lik_ == kLikNegBinomial)   // LogNormalizingConstantNegBin (:8448-8463)
    return SumOverY([](double x) { return std::lgamma(x); }, aux) + lognorm_ +
           v_.n * (aux * std::log(aux) - std::lgamma(aux));
  return 0.;
}

double GroupedLaplace::SumOverY(double (*f)(double), double r) const {
  double s = 0.;
  for (size_t k = 0; k < y_vals_.size(); ++k) s += y_cnt_[k] * f(y_vals_[k] + r);
  return s;
}

void GroupedLaplace::Assemble(const double* w, double* out, bool diag_only) {
  const int ndst = diag_only ? v_.M : v_.M + v_.nnz;
  const int nchunks = diag_only ? n_chunks_diag_ : n_chunks_;
  const int nlong = diag_only ? n_long_diag_ : n_long_;
  if (wt_) {   // diag_only: Z^T w (Z's values), else the destinations of Z^T diag(w) Z (their products)
    const double* sw = diag_only ? d_seg_w1_.get() : d_seg_w2_.get();
    glp_seg_short_kernel<true><<<blocks_of(ndst), 256, 0, s_>>>(ndst, d_seg_ptr_.get(), d_seg_obs_.get(), sw, w, out);
    if (nchunks > 0)
      glp_seg_chunk_kernel<true><<<(nchunks + 3) / 4, 256, 0, s_>>>(nchunks, d_c0_.get(), d_c1_.get(),
                                                                    d_seg_obs_.get(), sw, w, d_chunk_P_.get());
  } else {
    glp_seg_short_kernel<false><<<blocks_of(ndst), 256, 0, s_>>>(ndst, d_seg_ptr_.get(), d_seg_obs_.get(), nullptr, w,
                                                                 out);
    if (nchunks > 0)
      glp_seg_chunk_kernel<false><<<(nchunks + 3) / 4, 256, 0, s_>>>(nchunks, d_c0_.get(), d_c1_.get(),
                                                                     d_seg_obs_.get(), nullptr, w, d_chunk_P_.get());
  }
  if (nchunks > 0) {
    glp_seg_long_kernel<<<blocks_of(nlong), 256, 0, s_>>>(nlong, d_long_dst_.get(), d_long_cptr_.get(),
                                                          d_chunk_P_.get(), out);
  }
  HIP_CHECK(hipGetLastError());
}

namespace {
EffArgs make_eff(const GroupedRE::View& v, const double* sigma2) {
  EffArgs a{};
  a.K = v.K;
  for (int k = 0; k <= v.K; ++k) a.cum[k] = (*v.cum)[k];
  for (int k = 0; k < v.K; ++k) a.sigi[k] = 1. / sigma2[k];
  return a;
}
}  // namespace

double GroupedLaplace::Objective(const double* mode, double aux, const double* sigi) {
  const int n = v_.n, K = v_.K;
  launch_glp_obs(nb_, false, d_zw_.get(), n, K, d_glev_.get(), d_y_.get(), has_off_ ? d_off_.get() : nullptr, mode,
                 lik_, aux, nullptr, nullptr, nullptr, d_partial_.get(), s_);
  glp_finish_kernel<<<1, 256, 0, s_>>>(nb_, d_partial_.get(), d_red_.get());
  EffArgs a{};
  a.K = K;
  for (int k = 0; k <= K; ++k) a.cum[k] = (*v_.cum)[k];
  glp_effect_dots_kernel<0><<<K, 256, 0, s_>>>(a, mode, mode, d_red_.get() + 1);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h_red_, d_red_.get(), sizeof(double) * (1 + K), hipMemcpyDeviceToHost, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
  double quad = 0.;
  for (int k = 0; k < K; ++k) quad += sigi[k] * h_red_[1 + k];
  return h_red_[0] + LogLikConst(aux) - 0.5 * quad;
}

void GroupedLaplace::Deriv(const double* mode, double aux, bool want_dw) {
  launch_glp_obs(nb_, true, d_zw_.get(), v_.n, v_.K, d_glev_.get(), d_y_.get(), has_off_ ? d_off_.get() : nullptr,
                 mode, lik_, aux, d_d1_.get(), d_W_.get(), want_dw ? d_dW_.get() : nullptr, d_partial_.get(), s_);
  HIP_CHECK(hipGetLastError());
}

GroupedLaplaceResult GroupedLaplace::Eval(const double* sigma2, double aux, const IterativeConfig& cfg, bool iterative,
                                          bool want_grad, bool want_aux_grad, double* grad_f, Start start) {
  const double delta_conv = cfg.delta_conv_mode_finding;
  constexpr double kCgDeltaConvPred = 1e-3;   // cg_delta_conv_pred_ (re_model_template.h:5370)
  if (!y_set_) Fatal("response variable y has not been set");
  const int n = v_.n, K = v_.K, M = v_.M;
  const std::vector<int>& cum = *v_.cum;
  for (int k = 0; k < K; ++k)
    if (!(sigma2[k] > 0.)) Fatal("covariance parameters must be > 0");
  if (lik_ == kLikGamma && !(aux > 0.)) Fatal("the shape parameter of the gamma likelihood must be > 0");
  if (lik_ == kLikNegBinomial && !(aux > 0.))
    Fatal("the shape parameter of the negative_binomial likelihood must be > 0");
  const bool nb_aux = lik_ == kLikNegBinomial && want_aux_grad;   // the general shape gradient
  if (iterative && K < 2) Fatal("iterative methods need several grouped random effects");
  if (K > 1 && !iterative) re_->CheckDenseSize();
  const EffArgs ea = make_eff(v_, sigma2);
  GroupedLaplaceResult res;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  auto fail = [&]() {
    res.nan = true;
    res.nll = nan;
    evaluated_ = false;
    return res;
  };

  if (start == Start::kZero) {
    HIP_CHECK(hipMemsetAsync(d_mode_.get(), 0, sizeof(double) * M, s_));
  } else if (start == Start::kWarm) {
    HIP_CHECK(hipMemcpyAsync(d_mode_prev_.get(), d_mode_.get(), sizeof(double) * M, hipMemcpyDeviceToDevice, s_));
    mode_prev_valid_ = true;
  }
  // diag(A), the weighted off-diagonal values and (K >= 2) the dense factor at the current mode's W
  static const bool timing = std::getenv("GPBOOST_AMD_TIMING") != nullptr;   // HIP events around the last steps
  auto factor = [&]() -> bool {
    if (timing) HIP_CHECK(hipEventRecord(ev_[0], s_));
    Assemble(d_W_.get(), d_ztwz_.get(), false);
    if (timing) HIP_CHECK(hipEventRecord(ev_[1], s_));
    glp_vec_kernel<kVecDiag><<<blocks_of(M), 256, 0, s_>>>(M, ea, 0., d_ztwz_.get(), nullptr, d_D_.get());
    HIP_CHECK(hipGetLastError());
    if (iterative) {   // the SSOR preconditioner's D^-1/2 and the weighted operator of GroupedRE's PCG
      glp_vec_kernel<kVecInvSqrt><<<blocks_of(M), 256, 0, s_>>>(M, ea, 0., d_D_.get(), nullptr, d_dis_.get());
      HIP_CHECK(hipGetLastError());
      re_->SetOperator(d_ztwz_.get() + M, d_ztwz_.get(), d_D_.get(), d_dis_.get());
      return true;
    }
    if (K > 1) return re_->DenseFactorOf(d_D_.get(), d_ztwz_.get() + M);
    return true;
  };
  struct OperatorGuard {   // GroupedRE's own Z^T Z back when the evaluation ends
    GroupedRE* re;
    ~OperatorGuard() { re->SetOperator(nullptr, nullptr, nullptr, nullptr); }
  } guard{re_};
  // warm (iterative): out holds the initial guess
  auto solve = [&](const double* rhs, double* out, bool warm, double delta) -> int {
    if (iterative) return re_->SolveVec(rhs, out, cfg.cg_max_num_it, delta, warm);
    if (K > 1) {
      re_->DenseSolve(rhs, out);
    } else {
      glp_vec_kernel<kVecDiv><<<blocks_of(M), 256, 0, s_>>>(M, ea, 0., rhs, d_D_.get(), out);
      HIP_CHECK(hipGetLastError());
    }
    return 0;
  };

  // ---- mode finding (likelihoods.h:1995-2088 / 2224-2274)
  double mll = Objective(d_mode_.get(), aux, ea.sigi);
  const int newton_its = start == Start::kKeep ? 0 : kMaxItModeNewton;
  for (int it = 0; it < newton_its; ++it) {
    if (timing) HIP_CHECK(hipEventRecord(ev_[2], s_));
    Deriv(d_mode_.get(), aux, false);
    Assemble(d_d1_.get(), d_ztd1_.get(), true);
    glp_vec_kernel<kVecRhs><<<blocks_of(M), 256, 0, s_>>>(M, ea, 0., d_ztd1_.get(), d_mode_.get(), d_rhs_.get());
    if (!factor()) return fail();
    const int its = solve(d_rhs_.get(), d_upd_.get(), it > 0, cfg.cg_delta_conv);
    if (it == 0) res.cg_its = its;
    glp_effect_dots_kernel<0><<<K, 256, 0, s_>>>(ea, d_upd_.get(), d_rhs_.get(), d_red_.get() + 16);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h_red_ + 16, d_red_.get() + 16, sizeof(double) * K, hipMemcpyDeviceToHost, s_));
    HIP_CHECK(hipStreamSynchronize(s_));
    double gdd = 0.;   // grad_dot_direction (rhs = gradient of the objective)
    for (int k = 0; k < K; ++k) gdd += h_red_[16 + k];
    const LineSearchResult ls = newton_line_search(it, mll, gdd, delta_conv, kMaxShrinkNewton, [&](double lr, int) {
      glp_vec_kernel<kVecAxpy><<<blocks_of(M), 256, 0, s_>>>(M, ea, lr, d_mode_.get(), d_upd_.get(), d_mode_new_.get());
      return Objective(d_mode_new_.get(), aux, ea.sigi);
    });
    std::swap(d_mode_, d_mode_new_);
    if (timing) HIP_CHECK(hipEventRecord(ev_[3], s_));
    res.newton_its = it + 1;
    if (ls.nan) return fail();
    mll = ls.obj_new;
    if (ls.terminate) break;
  }
  // ---- derivatives, information and factor at the mode; the determinant (:2089-2193 / 2275-2289)
  Deriv(d_mode_.get(), aux, want_grad);
  glp_finish_kernel<<<1, 256, 0, s_>>>(nb_, d_partial_.get(), d_red_.get() + 32);   // ll at the mode (aux gradient)
  if (!factor()) return fail();
  double logdet = 0.;
  if (iterative) {   // SLQ of log|P^-1 A| + log|P|, log|P| = sum log D (:2155-2169)
    logdet = re_->SlqLogdet(cfg, &res.lanczos_steps);
    glp_effect_dots_kernel<1><<<K, 256, 0, s_>>>(ea, d_D_.get(), nullptr, d_red_.get() + 33);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h_red_ + 32, d_red_.get() + 32, sizeof(double) * (1 + K), hipMemcpyDeviceToHost, s_));
    HIP_CHECK(hipStreamSynchronize(s_));
    for (int k = 0; k < K; ++k) logdet += h_red_[33 + k];
  } else if (K > 1) {
    logdet = re_->dense_logdet();
    HIP_CHECK(hipMemcpyAsync(h_red_ + 32, d_red_.get() + 32, sizeof(double), hipMemcpyDeviceToHost, s_));
  } else {
    glp_effect_dots_kernel<1><<<1, 256, 0, s_>>>(ea, d_D_.get(), nullptr, d_red_.get() + 33);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h_red_ + 32, d_red_.get() + 32, sizeof(double) * 2, hipMemcpyDeviceToHost, s_));
  }
  HIP_CHECK(hipStreamSynchronize(s_));
  if (K == 1) logdet = h_red_[33];
  if (!std::isfinite(logdet)) return fail();
  const double ll_mode = h_red_[32];
  double sum_log_sigi = 0.;
  for (int k = 0; k < K; ++k) sum_log_sigi += (cum[k + 1] - cum[k]) * std::log(ea.sigi[k]);
  res.nll = -(mll - 0.5 * logdet + 0.5 * sum_log_sigi);
  if (timing && newton_its > 0 && res.newton_its > 0) {
    HIP_CHECK(hipEventElapsedTime(&res.ms_assembly, ev_[0], ev_[1]));
    HIP_CHECK(hipEventElapsedTime(&res.ms_newton_step, ev_[2], ev_[3]));
    std::fprintf(stderr, "[grouped laplace] %d Newton steps, %d CG its in the first, %d Lanczos steps; last weighted "
                 "assembly %.3f ms, last Newton step %.3f ms\n", res.newton_its, res.cg_its, res.lanczos_steps,
                 res.ms_assembly, res.ms_newton_step);
  }
  if (!std::isfinite(res.nll)) return fail();
  evaluated_ = true;
  if (!want_grad) return res;

  // ---- gradient (:3634-3740 / 3791-3853)
  if (nb_aux) {   // dd1/dlog r, dW/dlog r and the explicit sum at the mode (:10872-10885, 10527-10538)
    launch_glp_nb_aux(nb_, d_zw_.get(), n, K, d_glev_.get(), d_y_.get(), has_off_ ? d_off_.get() : nullptr,
                      d_mode_.get(), aux, d_dd1a_.get(), d_dWa_.get(), d_partial_.get(), s_);
    glp_finish_kernel<<<1, 256, 0, s_>>>(nb_, d_partial_.get(), d_red_.get() + kRedAuxSum);
    HIP_CHECK(hipGetLastError());
  }
  std::vector<double> tr_iter(K, 0.);
  double aux_det = 0.;   // iterative: d log|A| / dlog shape
  if (iterative) {
    const int t = cfg.num_rand_vec_trace;
    glp_effect_dots_kernel<2><<<K, 256, 0, s_>>>(ea, d_D_.get(), nullptr, d_red_.get() + 40);
    glp_effect_dots_kernel<3><<<K, 256, 0, s_>>>(ea, d_ztwz_.get(), d_D_.get(), d_red_.get() + 48);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h_red_ + 40, d_red_.get() + 40, sizeof(double) * 16, hipMemcpyDeviceToHost, s_));
    HIP_CHECK(hipStreamSynchronize(s_));
    std::vector<double> sum_Dinv(h_red_ + 40, h_red_ + 40 + K);
    double tr_dinv_w = 0.;   // tr(D^-1 diag(Z^T W Z))
    for (int k = 0; k < K; ++k) tr_dinv_w += h_red_[48 + k];
    // m_j + tr(A^-1 dSigma^-1/dlog sigma_j^2) = tr(A^-1 I_j Z^T W Z) (:3565-3582)
    re_->StochTraces(sigma2, sum_Dinv.data(), t, tr_iter.data());
    const double* U = re_->slq_solution();
    const double* PI = re_->probes_pinv();
    const double* DI = re_->probes_dinv_upper();
    launch_glp_row_trace(d_zw_.get(), n, K, t, d_glev_.get(), U, PI, d_dW_.get(), d_dwq_.get(), s_);
    HIP_CHECK(hipGetLastError());
    if (lik_ == kLikGamma && want_aux_grad) {
      // dW/dlog shape = W: tr(A^-1 Z^T W Z) by the probes, its SSOR control variate with the lower triangle of
      // Z^T W Z (:3607-3625)
      const size_t mt = (size_t)M * t;
      d_blkA_.alloc(mt);
      d_blkB_.alloc(mt);
      std::vector<double> z1(t), zP(t), tmp(t);
      re_->ApplyOffDiagPlus(PI, d_blkA_.get(), t);
      re_->ColDots(U, d_blkA_.get(), t, z1.data());
      re_->ApplyLower(d_ztwz_.get(), DI, d_blkB_.get(), t);
      re_->ColDots(PI, d_blkB_.get(), t, zP.data());
      re_->ColDots(DI, d_blkB_.get(), t, tmp.data());
      double tr1 = 0., trP = 0.;
      for (int c = 0; c < t; ++c) {
        zP[c] = 2. * zP[c] - tmp[c];
        tr1 += z1[c];
        trP += zP[c];
      }
      tr1 /= t;
      trP /= t;
      aux_det = tr1 + optimal_c(z1.data(), zP.data(), t, tr1, trP) * (tr_dinv_w - trP);
    }
    if (nb_aux) {
      // the same estimate with Z^T diag(dW/dlog r) Z in the place of Z^T W Z (:3607-3625): assembled beside d_ztwz_
      // and made the operator of the two products, on the same probes
      const size_t mt = (size_t)M * t;
      d_blkA_.alloc(mt);
      d_blkB_.alloc(mt);
      d_ztdwz_.alloc(M + v_.nnz);
      Assemble(d_dWa_.get(), d_ztdwz_.get(), false);
      glp_effect_dots_kernel<3><<<K, 256, 0, s_>>>(ea, d_ztdwz_.get(), d_D_.get(), d_red_.get() + kRedAuxDinv);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(h_red_ + kRedAuxDinv, d_red_.get() + kRedAuxDinv, sizeof(double) * K,
                               hipMemcpyDeviceToHost, s_));
      std::vector<double> z1(t), zP(t), tmp(t);
      re_->SetOperator(d_ztdwz_.get() + M, d_ztdwz_.get(), d_D_.get(), d_dis_.get());
      re_->ApplyOffDiagPlus(PI, d_blkA_.get(), t);
      re_->ColDots(U, d_blkA_.get(), t, z1.data());   // synchronizes
      re_->ApplyLower(d_ztdwz_.get(), DI, d_blkB_.get(), t);
      re_->ColDots(PI, d_blkB_.get(), t, zP.data());
      re_->ColDots(DI, d_blkB_.get(), t, tmp.data());
      re_->SetOperator(d_ztwz_.get() + M, d_ztwz_.get(), d_D_.get(), d_dis_.get());   // A again, for the solve below
      double tr_dinv_dw = 0.;   // tr(D^-1 diag(Z^T dW/dlog r Z))
      for (int k = 0; k < K; ++k) tr_dinv_dw += h_red_[kRedAuxDinv + k];
      double tr1 = 0., trP = 0.;
      for (int c = 0; c < t; ++c) {
        zP[c] = 2. * zP[c] - tmp[c];
        tr1 += z1[c];
        trP += zP[c];
      }
      tr1 /= t;
      trP /= t;
      aux_det = tr1 + optimal_c(z1.data(), zP.data(), t, tr1, trP) * (tr_dinv_dw - trP);
    }
  } else {
    const double* Ainv = K > 1 ? re_->DenseInverse() : nullptr;
    if (nb_aux) {   // one more fused partial: sum_i (dW/dlog r)_i q_i
      launch_glp_q(nb_, true, d_zw_.get(), n, K, d_glev_.get(), Ainv, re_->dense_ld(), d_D_.get(), d_W_.get(),
                   d_dW_.get(), d_dWa_.get(), d_dwq_.get(), d_partial_.get(), s_);
      glp_finish_kernel<<<1, 256, 0, s_>>>(nb_, d_partial_.get() + (size_t)K * nb_, d_red_.get() + kRedAuxTrace);
    } else {
      launch_glp_q(nb_, false, d_zw_.get(), n, K, d_glev_.get(), Ainv, re_->dense_ld(), d_D_.get(), d_W_.get(),
                   d_dW_.get(), nullptr, d_dwq_.get(), d_partial_.get(), s_);
    }
    glp_finish_kernel<<<K, 256, 0, s_>>>(nb_, d_partial_.get(), d_red_.get());   // sum_i W_i q_ij
    HIP_CHECK(hipGetLastError());
  }
  Assemble(d_dwq_.get(), d_dmll_.get(), true);                                 // d_mll_d_mode
  solve(d_dmll_.get(), d_vS_.get(), false, kCgDeltaConvPred);                  // v = A^-1 d_mll_d_mode
  Assemble(d_d1_.get(), d_ztd1_.get(), true);
  glp_effect_dots_kernel<0><<<K, 256, 0, s_>>>(ea, d_vS_.get(), d_ztd1_.get(), d_red_.get() + kGlpMaxK);
  glp_effect_dots_kernel<0><<<K, 256, 0, s_>>>(ea, d_mode_.get(), d_mode_.get(), d_red_.get() + 2 * kGlpMaxK);
  HIP_CHECK(hipGetLastError());
  if (nb_aux) {   // the implicit term v^T Z^T (dd1/dlog r) (:3628, 3737, 3848)
    Assemble(d_dd1a_.get(), d_zta_.get(), true);
    glp_effect_dots_kernel<0><<<K, 256, 0, s_>>>(ea, d_vS_.get(), d_zta_.get(), d_red_.get() + kRedAuxImp);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(h_red_ + kRedAuxSum, d_red_.get() + kRedAuxSum, sizeof(double) * (kRedAuxImp + K - kRedAuxSum),
                             hipMemcpyDeviceToHost, s_));
  }
  if (grad_f != nullptr || keep_gradf_) {
    d_gradf_.alloc(n);
    launch_glp_grad_f(d_zw_.get(), n, K, d_glev_.get(), d_d1_.get(), d_dwq_.get(), d_W_.get(), d_vS_.get(),
                      d_gradf_.get(), s_);
    HIP_CHECK(hipGetLastError());
    if (grad_f != nullptr)
      HIP_CHECK(hipMemcpyAsync(grad_f, d_gradf_.get(), sizeof(double) * n, hipMemcpyDeviceToHost, s_));
  }
  HIP_CHECK(hipMemcpyAsync(h_red_, d_red_.get(), sizeof(double) * 3 * kGlpMaxK, hipMemcpyDeviceToHost, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
  double tr_all = 0., imp_all = 0.;
  for (int j = 0; j < K; ++j) {
    const double tr = iterative ? tr_iter[j] : h_red_[j], imp = h_red_[kGlpMaxK + j], bb = h_red_[2 * kGlpMaxK + j];
    res.grad.push_back(-0.5 * bb * ea.sigi[j] + 0.5 * tr + imp);
    tr_all += tr;
    imp_all += imp;
  }
  if (lik_ == kLikGamma && want_aux_grad) {
    // shape on the log scale (:3720-3739, 10508-10524): -dll/dlog a = -ll - a n (log a + 1 - digamma(a)) - a sum log y
    // with ll = -a sum (eta + y e^-eta); dW/dlog a = W and dd1/dlog a = d1
    const double neg = -ll_mode - aux * (n * (std::log(aux) + 1. - digamma_asa103(aux)) + sum_log_y_);
    res.grad.push_back(neg + 0.5 * (iterative ? aux_det : tr_all) + imp_all);
  }
  if (nb_aux) {
    // shape on the log scale (:10527-10538): -dll/dlog r = r sum_i [-digamma(y_i + r) + log(mu_i + r) + (y_i + r) /
    // (mu_i + r)] + n r (digamma(r) - log r - 1), the digamma sum from the table of distinct responses
    const double neg = aux * (h_red_[kRedAuxSum] - SumOverY(digamma_asa103, aux)) +
                       n * aux * (digamma_asa103(aux) - std::log(aux) - 1.);
    double imp_aux = 0.;
    for (int j = 0; j < K; ++j) imp_aux += h_red_[kRedAuxImp + j];
    res.grad.push_back(neg + 0.5 * (iterative ? aux_det : h_red_[kRedAuxTrace]) + imp_aux);
  }
  for (double g : res.grad)
    if (!std::isfinite(g)) res.nan = true;
  return res;
}

void GroupedLaplace::ResetModeToPrevious() {
  if (!mode_prev_valid_) return;
  HIP_CHECK(hipMemcpyAsync(d_mode_.get(), d_mode_prev_.get(), sizeof(double) * v_.M, hipMemcpyDeviceToDevice, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
}

void GroupedLaplace::GetMode(double* b) {
  HIP_CHECK(hipMemcpyAsync(b, d_mode_.get(), sizeof(double) * v_.M, hipMemcpyDeviceToHost, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
}

void GroupedLaplace::PredVar(int np, const std::vector<int>& idx, double* out, const double* wt) {
  if (!evaluated_) Fatal("predictive variances need an evaluation of the Laplace approximation first");
  re_->PredCov(np, idx, false, out, v_.K == 1 ? d_D_.get() : nullptr, wt);
}

void GroupedLaplace::GetZtWZ(double* diag, double* vals) {
  if (!evaluated_) Fatal("Z^T W Z is available after an evaluation of the Laplace approximation");
  HIP_CHECK(hipMemcpyAsync(diag, d_ztwz_.get(), sizeof(double) * v_.M, hipMemcpyDeviceToHost, s_));
  if (v_.nnz > 0)
    HIP_CHECK(hipMemcpyAsync(vals, d_ztwz_.get() + v_.M, sizeof(double) * v_.nnz, hipMemcpyDeviceToHost, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
}

// ---- test launchers (lik_test.h): the launches of Objective / Deriv on nb_ blocks, then the finish of Objective
int test_glp_blocks(int n) { return obs_blocks(n); }

void test_glp_obs(int n, int K, const int* glev, const double* y, const double* F, const double* b, int lik, double aux,
                  bool deriv, double* d1, double* W, double* dW, double* partial, double* ll, hipStream_t s) {
  const int nb = obs_blocks(n);
  launch_glp_obs(nb, deriv, nullptr, n, K, glev, y, F, b, lik, aux, d1, W, dW, partial, s);
  glp_finish_kernel<<<1, 256, 0, s>>>(nb, partial, ll);
  HIP_CHECK(hipGetLastError());
}

void test_glp_nb_aux(int n, int K, const int* glev, const double* y, const double* F, const double* b, double aux,
                     double* dd1a, double* dWa, double* partial, double* sum, hipStream_t s) {
  const int nb = obs_blocks(n);
  launch_glp_nb_aux(nb, nullptr, n, K, glev, y, F, b, aux, dd1a, dWa, partial, s);
  glp_finish_kernel<<<1, 256, 0, s>>>(nb, partial, sum);
  HIP_CHECK(hipGetLastError());
}

// ---- test launchers (grouped_test.h): the gradient's launches of Eval with its grids
void test_glp_q(int n, int K, const int* glev, const double* zw, const double* Ainv, int ld, const double* D,
                const double* W, const double* dW, const double* Wa, bool aux, double* dwq, double* partial, double* out,
                hipStream_t s) {
  const int nb = obs_blocks(n);
  launch_glp_q(nb, aux, zw, n, K, glev, Ainv, ld, D, W, dW, Wa, dwq, partial, s);
  if (aux) glp_finish_kernel<<<1, 256, 0, s>>>(nb, partial + (size_t)K * nb, out + K);
  glp_finish_kernel<<<K, 256, 0, s>>>(nb, partial, out);
  HIP_CHECK(hipGetLastError());
}

void test_glp_row_trace(int n, int K, int t, const int* glev, const double* zw, const double* U, const double* V,
                        const double* dW, double* dwq, hipStream_t s) {
  launch_glp_row_trace(zw, n, K, t, glev, U, V, dW, dwq, s);
  HIP_CHECK(hipGetLastError());
}

void test_glp_grad_f(int n, int K, const int* glev, const double* zw, const double* d1, const double* dwq,
                     const double* W, const double* v, double* out, hipStream_t s) {
  launch_glp_grad_f(zw, n, K, glev, d1, dwq, W, v, out, s);
  HIP_CHECK(hipGetLastError());
}

void test_glp_vec(int form, const GroupedRE::View& v, const double* sigma2, double alpha, const double* x,
                  const double* y, double* out, hipStream_t s) {
  const EffArgs ea = make_eff(v, sigma2);
  const int M = v.M;
  switch (form) {
    case kVecDiag: glp_vec_kernel<kVecDiag><<<blocks_of(M), 256, 0, s>>>(M, ea, alpha, x, y, out); break;
    case kVecRhs: glp_vec_kernel<kVecRhs><<<blocks_of(M), 256, 0, s>>>(M, ea, alpha, x, y, out); break;
    case kVecDiv: glp_vec_kernel<kVecDiv><<<blocks_of(M), 256, 0, s>>>(M, ea, alpha, x, y, out); break;
    case kVecAxpy: glp_vec_kernel<kVecAxpy><<<blocks_of(M), 256, 0, s>>>(M, ea, alpha, x, y, out); break;
    case kVecInvSqrt: glp_vec_kernel<kVecInvSqrt><<<blocks_of(M), 256, 0, s>>>(M, ea, alpha, x, y, out); break;
    default: Fatal("test_glp_vec: unknown form %d", form);
  }
  HIP_CHECK(hipGetLastError());
}

void test_glp_effect_dots(int mode, const GroupedRE::View& v, const double* sigma2, const double* x, const double* y,
                          double* out, hipStream_t s) {
  const EffArgs ea = make_eff(v, sigma2);
  const int K = v.K;
  switch (mode) {
    case 0: glp_effect_dots_kernel<0><<<K, 256, 0, s>>>(ea, x, y, out); break;
    case 1: glp_effect_dots_kernel<1><<<K, 256, 0, s>>>(ea, x, y, out); break;
    case 2: glp_effect_dots_kernel<2><<<K, 256, 0, s>>>(ea, x, y, out); break;
    case 3: glp_effect_dots_kernel<3><<<K, 256, 0, s>>>(ea, x, y, out); break;
    default: Fatal("test_glp_effect_dots: unknown mode %d", mode);
  }
  HIP_CHECK(hipGetLastError());
}

// the friend of GroupedLaplace and GroupedRE: its GroupedLaplace half lives here, beside the private members it reads
void GroupedTestAccess::Assemble(GroupedLaplace& g, const double* w, double* out, bool diag_only) {
  g.Assemble(w, out, diag_only);
}
const int* GroupedTestAccess::Glev(const GroupedLaplace& g) { return g.d_glev_.get(); }
const double* GroupedTestAccess::Zw(const GroupedLaplace& g) { return g.d_zw_.get(); }
void GroupedTestAccess::SegCounts(const GroupedLaplace& g, int out[4]) {
  out[0] = g.n_long_diag_;
  out[1] = g.n_chunks_diag_;
  out[2] = g.n_long_;
  out[3] = g.n_chunks_;
}

}  // namespace gpb_amd
