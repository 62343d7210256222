// Batched dense likelihood of many small clusters (dense_batch.h): one wave per cluster, everything in LDS.
//
// Lane t owns row t of its cluster (n <= 64 rows, lanes t >= n idle). Per cluster:
//   1. Psi = var corr + I, lower triangle, row-major with an odd row stride S = nmax | 1: lanes reading one
//      column (addresses S doubles apart) fall on 32 distinct 8-byte bank pairs, lanes reading one row are
//      contiguous; a common address is a broadcast.
//   2. right-looking Cholesky in place, one column per step; a pivot that is not positive and finite ends the
//      cluster: info = 1, NaN sums, NaN u.
//   3. logdet = 2 sum log L_kk, z = L^-1 y and u = L^-T z by column sweeps; lane t keeps entry t in a register
//      and the pivot entry is a wave broadcast; q = sum z_k^2 in index order.
//   4. want_grad: W = L^-1 (lane t solves column t; the upper triangle holds zeros, so every loop is
//      wave-uniform), then with P = Psi^-1 = W^T W lane i adds over all j
//        P_ij C_ij, P_ij dC_ij (the traces) and u_i u_j C_ij, u_i u_j dC_ij (the quadratic forms),
//      C_ij and dC_ij recomputed by cov_dcov<COV>; the 64 partials of each are added in lane order by lane 0.
// Every sum has a fixed order, there is no atomic, and a cluster's outputs depend on nothing but its data, the
// parameters and nmax: results do not depend on the grid or the schedule.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "cov.h"
#include "dense_batch.h"
#include "kernels.h"

namespace gpb_amd {

namespace {

constexpr int kLanes = 64;

// doubles ahead of the matrices: u (64), four partial arrays (4 x 64), the coordinates (nmax x 3)
__host__ __device__ inline int batch_head_doubles(int nmax) { return kLanes + 4 * kLanes + nmax * 3; }

template <int COV>
__global__ void __launch_bounds__(kLanes) dense_batch_kernel(DenseBatchArgs a) {
  extern __shared__ double lds[];
  const int c = blockIdx.x, t = threadIdx.x;
  const int p0 = a.ptr[c], n = a.ptr[c + 1] - p0, d = a.d;
  const int S = a.nmax | 1;
  double* us = lds;
  double* red = us + kLanes;
  double* xs = red + 4 * kLanes;
  double* A = lds + batch_head_doubles(a.nmax);
  double* W = A + a.nmax * S;   // want_grad only
  const bool row = t < n;
  const int tc = row ? t : 0;   // a valid row for the reads of idle lanes

  for (int e = t; e < n * d; e += kLanes) xs[e] = a.X[(size_t)p0 * d + e];
  double yi = row ? a.Y[p0 + t] : 0.;
  __syncthreads();

  // 1. Psi, lower triangle
  for (int e = t; e < n * n; e += kLanes) {
    const int i = e / n, j = e - i * n;
    if (j > i) continue;
    double s = 0.;
    for (int q = 0; q < d; ++q) {
      const double df = xs[i * d + q] - xs[j * d + q];
      s += df * df;
    }
    double cc, dc;
    cov_dcov<COV>(sqrt(s), a.var, a.phi, cc, dc);
    A[i * S + j] = i == j ? cc + 1. : cc;
  }
  __syncthreads();

  // 2. Cholesky
  double logsum = 0.;
  bool bad = false;
  for (int k = 0; k < n; ++k) {
    const double p = A[k * S + k];
    if (!(p > 0.) || !(p < __builtin_inf())) {   // the same for every lane
      bad = true;
      break;
    }
    const double l = sqrt(p);
    logsum += log(l);
    double lik = 0.;
    if (row && t > k) {
      lik = A[t * S + k] / l;
      A[t * S + k] = lik;
    }
    __syncthreads();   // column k is final; every lane has read the pivot
    if (t == k) A[k * S + k] = l;
    if (row && t > k)
      for (int j = k + 1; j <= t; ++j) A[t * S + j] -= lik * A[j * S + k];
    __syncthreads();
  }
  if (bad) {
    const double nan = __builtin_nan("");
    if (t < kVecchiaSums) a.sums[(size_t)c * kVecchiaSums + t] = nan;
    if (t == 0) a.info[c] = 1;
    if (a.u != nullptr && row) a.u[p0 + t] = nan;
    return;
  }

  // 3. z = L^-1 y, q = z'z, u = L^-T z
  double qq = 0.;
  for (int k = 0; k < n; ++k) {
    const double zk = __shfl(yi, k, kLanes) / A[k * S + k];
    qq += zk * zk;
    if (t == k) yi = zk;
    else if (row && t > k) yi -= A[t * S + k] * zk;
  }
  for (int k = n - 1; k >= 0; --k) {
    const double uk = __shfl(yi, k, kLanes) / A[k * S + k];
    if (t == k) yi = uk;
    else if (t < k) yi -= A[k * S + t] * uk;
  }
  if (a.u != nullptr && row) a.u[p0 + t] = yi;

  double tv = 0., tp = 0., qv = 0., qp = 0.;
  if (a.want_grad) {
    us[t] = row ? yi : 0.;
    // 4. W = L^-1: column tc by lane t (idle lanes recompute column 0 and store nothing)
    for (int e = t; e < n * S; e += kLanes) W[e] = 0.;
    __syncthreads();
    if (row) W[t * S + t] = 1. / A[t * S + t];
    __syncthreads();
    for (int i = 1; i < n; ++i) {
      double s = 0.;
      for (int k = 0; k < i; ++k) s += A[i * S + k] * W[k * S + tc];
      if (row && t < i) W[i * S + t] = -s / A[i * S + i];
      // lane t reads its own column only: no barrier between the rows
    }
    __syncthreads();
    const double ui = us[tc];
    for (int j = 0; j < n; ++j) {
      double s = 0.;
      for (int q = 0; q < d; ++q) {
        const double df = xs[tc * d + q] - xs[j * d + q];
        s += df * df;
      }
      double cc, dc;
      cov_dcov<COV>(sqrt(s), a.var, a.phi, cc, dc);
      double P = 0.;
      for (int k = j; k < n; ++k) P += W[k * S + tc] * W[k * S + j];   // W[k][tc] = 0 for k < tc
      const double uu = ui * us[j];
      tv += P * cc;
      tp += P * dc;
      qv += uu * cc;
      qp += uu * dc;
    }
    red[t] = row ? tv : 0.;
    red[kLanes + t] = row ? tp : 0.;
    red[2 * kLanes + t] = row ? qv : 0.;
    red[3 * kLanes + t] = row ? qp : 0.;
    __syncthreads();
    if (t == 0) {
      tv = tp = qv = qp = 0.;
      for (int k = 0; k < n; ++k) {
        tv += red[k];
        tp += red[kLanes + k];
        qv += red[2 * kLanes + k];
        qp += red[3 * kLanes + k];
      }
    }
  }
  if (t == 0) {
    double* o = a.sums + (size_t)c * kVecchiaSums;
    o[0] = 2. * logsum;
    o[1] = qq;
    o[2] = -0.5 * qv;
    o[3] = -0.5 * qp;
    o[4] = tv;
    o[5] = tp;
    a.info[c] = 0;
  }
}

}  // namespace

size_t dense_batch_lds_bytes(int nmax, int want_grad) {
  const size_t S = (size_t)(nmax | 1);
  return sizeof(double) * (batch_head_doubles(nmax) + (size_t)nmax * S * (want_grad ? 2 : 1));
}

void launch_dense_batch(int cov_type, const DenseBatchArgs& a, hipStream_t s) {
  if (a.C <= 0) return;
  if (a.d < 1 || a.d > 3) Fatal("dense_batch: d = %d not supported (1..3)", a.d);
  if (a.nmax < 1 || a.nmax > kBatchMaxN) Fatal("dense_batch: largest cluster %d outside 1..%d", a.nmax, kBatchMaxN);
  const size_t bytes = dense_batch_lds_bytes(a.nmax, a.want_grad);
  dispatch_cov(cov_type, [&](auto cov) {
    constexpr int COV = decltype(cov)::value;
    if (bytes > 64 * 1024)   // above the default dynamic-LDS limit (the model's device may differ between calls)
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_batch_kernel<COV>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)dense_batch_lds_bytes(kBatchMaxN, 1)));
    hipLaunchKernelGGL(dense_batch_kernel<COV>, dim3(a.C), dim3(kLanes), bytes, s, a);
  });
  HIP_CHECK(hipGetLastError());
}

DenseBatch::DenseBatch(int d, const std::vector<double>& X, const std::vector<int>& ptr, hipStream_t stream)
    : d_(d), C_((int)ptr.size() - 1), N_(ptr.empty() ? 0 : ptr.back()), nmax_(0), stream_(stream) {
  if (C_ < 1 || ptr[0] != 0) Fatal("dense_batch: invalid cluster offsets");
  for (int c = 0; c < C_; ++c) {
    const int nc = ptr[c + 1] - ptr[c];
    if (nc < 1 || nc > kBatchMaxN) Fatal("dense_batch: cluster of %d points (1..%d)", nc, kBatchMaxN);
    nmax_ = std::max(nmax_, nc);
  }
  if (X.size() != (size_t)N_ * d) Fatal("dense_batch: coordinates do not match the offsets");
  X_.alloc(X.size());
  y_.alloc(N_);
  ptr_.alloc(ptr.size());
  sums_.alloc((size_t)C_ * kVecchiaSums);
  info_.alloc(C_);
  out_.alloc(8);
  HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_out_), 8 * sizeof(double), hipHostMallocDefault));
  HIP_CHECK(hipMemcpyAsync(X_.get(), X.data(), sizeof(double) * X.size(), hipMemcpyHostToDevice, stream_));
  HIP_CHECK(hipMemcpyAsync(ptr_.get(), ptr.data(), sizeof(int) * ptr.size(), hipMemcpyHostToDevice, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
}

DenseBatch::~DenseBatch() {
  if (h_out_) (void)hipHostFree(h_out_);
}

void DenseBatch::SetY(const double* y) {
  HIP_CHECK(hipMemcpyAsync(y_.get(), y, sizeof(double) * N_, hipMemcpyHostToDevice, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
}

void DenseBatch::Eval(int cov_type, double var, double phi, bool want_grad, double* sums6) {
  DenseBatchArgs a{};
  a.X = X_.get();
  a.Y = y_.get();
  a.ptr = ptr_.get();
  a.C = C_;
  a.d = d_;
  a.nmax = nmax_;
  a.var = var;
  a.phi = phi;
  a.want_grad = want_grad ? 1 : 0;
  a.sums = sums_.get();
  a.u = nullptr;
  a.info = info_.get();
  launch_dense_batch(cov_type, a, stream_);
  launch_sum_blocks(sums_.get(), C_, kVecchiaSums, out_.get(), stream_);
  HIP_CHECK(hipMemcpyAsync(h_out_, out_.get(), sizeof(double) * kVecchiaSums, hipMemcpyDeviceToHost, stream_));
  HIP_CHECK(hipStreamSynchronize(stream_));
  if (std::isnan(h_out_[0])) {   // a flagged cluster writes NaN sums: tell it from NaN data
    std::vector<int> info(C_);
    HIP_CHECK(hipMemcpy(info.data(), info_.get(), sizeof(int) * C_, hipMemcpyDeviceToHost));
    for (int v : info)
      if (v != 0) Fatal("the covariance matrix is not positive definite (Cholesky failed)");
  }
  for (int q = 0; q < kVecchiaSums; ++q) sums6[q] = h_out_[q];
}

void test_dense_batch(int cov_type, int C, int d, const int32_t* ptr, int64_t ptr_len, const double* X, int64_t x_len,
                      const double* y, int64_t y_len, double var, double phi, int want_grad, double* sums,
                      int64_t sums_len, double* u, int64_t u_len, int32_t* info, int64_t info_len) {
  if (C < 1 || d < 1 || d > 3) Fatal("test_dense_batch: C = %d, d = %d", C, d);
  if (ptr == nullptr || X == nullptr || y == nullptr || sums == nullptr || info == nullptr)
    Fatal("test_dense_batch: NULL argument");
  if (ptr_len != (int64_t)C + 1 || ptr[0] != 0) Fatal("test_dense_batch: ptr needs C + 1 entries starting at 0");
  int nmax = 0;
  for (int c = 0; c < C; ++c) {
    const int64_t nc = (int64_t)ptr[c + 1] - ptr[c];
    if (nc < 1 || nc > kBatchMaxN) Fatal("test_dense_batch: cluster %d has %lld points (1..%d)", c, (long long)nc, kBatchMaxN);
    nmax = std::max(nmax, (int)nc);
  }
  const int64_t N = ptr[C];
  if (x_len != N * d || y_len != N) Fatal("test_dense_batch: X / y do not match ptr");
  if (sums_len != (int64_t)C * kVecchiaSums || info_len != C || (u != nullptr && u_len != N))
    Fatal("test_dense_batch: output extents do not match");
  if (!(var > 0.) || !(phi > 0.)) Fatal("test_dense_batch: var and phi must be > 0");
  DevBuf<double> dX(x_len), dy(N), dsums(sums_len), du(N);
  DevBuf<int> dptr(ptr_len), dinfo(C);
  HIP_CHECK(hipMemcpy(dX.get(), X, sizeof(double) * x_len, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dy.get(), y, sizeof(double) * N, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dptr.get(), ptr, sizeof(int) * ptr_len, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemset(dsums.get(), 0xff, sizeof(double) * sums_len));
  HIP_CHECK(hipMemset(du.get(), 0xff, sizeof(double) * N));
  HIP_CHECK(hipMemset(dinfo.get(), 0xff, sizeof(int) * C));
  DenseBatchArgs a{};
  a.X = dX.get();
  a.Y = dy.get();
  a.ptr = dptr.get();
  a.C = C;
  a.d = d;
  a.nmax = nmax;
  a.var = var;
  a.phi = phi;
  a.want_grad = want_grad ? 1 : 0;
  a.sums = dsums.get();
  a.u = u != nullptr ? du.get() : nullptr;
  a.info = dinfo.get();
  launch_dense_batch(cov_type, a, nullptr);
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(sums, dsums.get(), sizeof(double) * sums_len, hipMemcpyDeviceToHost));
  if (u != nullptr) HIP_CHECK(hipMemcpy(u, du.get(), sizeof(double) * N, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(info, dinfo.get(), sizeof(int) * C, hipMemcpyDeviceToHost));
}

}  // namespace gpb_amd
