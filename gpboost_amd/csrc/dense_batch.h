// Batched dense Gaussian-process likelihood for many small independent realisations (cluster_ids):
// every cluster of n_c <= kBatchMaxN points is built, factored and differentiated by one wave entirely in
// LDS, all clusters in one launch (dense_batch.hip). The per-cluster sums have the layout of
// DenseSolver::Eval and are added over the clusters in a fixed order (launch_sum_blocks).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "common.h"

namespace gpb_amd {

constexpr int kBatchMaxN = 64;   // the largest cluster of the batched kernel (one lane per row)

struct DenseBatchArgs {
  const double* X;   // coordinates of all clusters, cluster-major, row-major N x d
  const double* Y;   // response in the same order (N)
  const int* ptr;    // C + 1 offsets: cluster c holds rows [ptr[c], ptr[c + 1]), 1 .. nmax of them
  int C;
  int d;             // 1 .. 3
  int nmax;          // the largest cluster (<= kBatchMaxN); sizes the LDS
  double var, phi;
  int want_grad;
  double* sums;      // C x 6: [logdet, q, s1_var, s1_range, s2_var, s2_range] per cluster (NaN: info set)
  double* u;         // nullable, N: Psi_c^-1 y_c
  int* info;         // C: 1 when a pivot of the cluster was not positive and finite, else 0
};

// dynamic LDS bytes of one workgroup (one cluster)
size_t dense_batch_lds_bytes(int nmax, int want_grad);
void launch_dense_batch(int cov_type, const DenseBatchArgs& a, hipStream_t s);

// The small clusters of one model: device copies of their coordinates and response, one kernel launch and one
// fixed-order sum per evaluation.
class DenseBatch {
 public:
  // X: host row-major N x d (cluster-major), ptr: C + 1 offsets
  DenseBatch(int d, const std::vector<double>& X, const std::vector<int>& ptr, hipStream_t stream);
  ~DenseBatch();
  int num_points() const { return N_; }
  int num_clusters() const { return C_; }
  void SetY(const double* y);   // host, N (cluster-major)
  // sums6 as DenseSolver::Eval; fails like the dense path when a cluster is not positive definite
  void Eval(int cov_type, double var, double phi, bool want_grad, double* sums6);

 private:
  int d_, C_, N_, nmax_;
  hipStream_t stream_;
  DevBuf<double> X_, y_, sums_, out_;
  DevBuf<int> ptr_, info_;
  double* h_out_ = nullptr;   // pinned
};

// GPB_TestDenseBatch (include/gpboost_amd.h): the kernel on caller-given clusters; every extent is checked on the
// host before the launch. sums: C x 6, u: N (nullable), info: C.
void test_dense_batch(int cov_type, int C, int d, const int32_t* ptr, int64_t ptr_len, const double* X, int64_t x_len,
                      const double* y, int64_t y_len, double var, double phi, int want_grad, double* sums,
                      int64_t sums_len, double* u, int64_t u_len, int32_t* info, int64_t info_len);

}  // namespace gpb_amd
