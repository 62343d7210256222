// Host bookkeeping of independent GP realisations (cluster_ids): the row partition of the observations and the
// scatter of per-cluster predictions back to the caller's order. Plain C++ (no device code), header-only.
#pragma once

#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace gpb_amd {

// SetUpGPIds (re_model_template.h:6211-6243): clusters in order of first appearance, observations in their
// order within a cluster.
struct ClusterPartition {
  std::vector<int32_t> ids;   // the id of cluster c
  std::vector<int> ptr;       // C + 1 offsets into rows
  std::vector<int> rows;      // observation indices, cluster-major
  int num_clusters() const { return (int)ids.size(); }
  int size(int c) const { return ptr[c + 1] - ptr[c]; }
  // the cluster of an id, or -1
  int find(int32_t id) const {
    auto it = index.find(id);
    return it == index.end() ? -1 : it->second;
  }
  std::unordered_map<int32_t, int> index;
};

inline ClusterPartition partition_clusters(const int32_t* cluster_ids, int n) {
  ClusterPartition p;
  std::vector<int> of(n > 0 ? n : 0), count;
  for (int i = 0; i < n; ++i) {
    auto it = p.index.find(cluster_ids[i]);
    if (it == p.index.end()) {
      it = p.index.emplace(cluster_ids[i], (int)p.ids.size()).first;
      p.ids.push_back(cluster_ids[i]);
      count.push_back(0);
    }
    of[i] = it->second;
    ++count[it->second];
  }
  const int C = (int)p.ids.size();
  p.ptr.assign(C + 1, 0);
  for (int c = 0; c < C; ++c) p.ptr[c + 1] = p.ptr[c] + count[c];
  p.rows.resize(n > 0 ? n : 0);
  std::vector<int> fill(p.ptr.begin(), p.ptr.end() - 1);
  for (int i = 0; i < n; ++i) p.rows[fill[of[i]]++] = i;
  return p;
}

// v (original order, n) -> cluster-major order
inline std::vector<double> gather_rows(const ClusterPartition& p, const double* v) {
  std::vector<double> out(p.rows.size());
  for (size_t k = 0; k < p.rows.size(); ++k) out[k] = v[p.rows[k]];
  return out;
}

// One cluster's predictions into the caller's output: out = [mean (n_pred) | variances (n_pred) or the
// column-major n_pred x n_pred covariance]; idx: the caller's positions of the cluster's k prediction points;
// mean (k), var (k, when want_var), cov (column-major k x k, when want_cov). Blocks between clusters stay as
// the caller initialised them (zero).
inline void scatter_cluster_prediction(int n_pred, const std::vector<int>& idx, const double* mean, const double* var,
                                       const double* cov, bool want_var, bool want_cov, double* out) {
  const size_t k = idx.size();
  for (size_t a = 0; a < k; ++a) out[idx[a]] = mean[a];
  if (want_cov) {
    for (size_t b = 0; b < k; ++b)
      for (size_t a = 0; a < k; ++a)
        out[(size_t)n_pred + (size_t)idx[b] * n_pred + idx[a]] = cov[b * k + a];
  } else if (want_var) {
    for (size_t a = 0; a < k; ++a) out[(size_t)n_pred + idx[a]] = var[a];
  }
}

}  // namespace gpb_amd
