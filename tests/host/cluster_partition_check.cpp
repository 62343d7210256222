// Stand-alone host check of csrc/cluster_partition.h (no GPU, no HIP): the row partition by cluster id and the
// scatter of per-cluster predictions. Built and run by tests/test_cluster_partition_host.py; for a sanitizer run
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Igpboost_amd/csrc \
//       tests/host/cluster_partition_check.cpp -o cluster_partition_check && ./cluster_partition_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "cluster_partition.h"

using namespace gpb_amd;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static void check_partition(const std::vector<int32_t>& ids) {
  const int n = (int)ids.size();
  const ClusterPartition p = partition_clusters(ids.data(), n);
  const int C = p.num_clusters();
  CHECK((int)p.ptr.size() == C + 1 && p.ptr[0] == 0 && p.ptr[C] == n && (int)p.rows.size() == n);
  std::vector<int> seen(n, 0);
  int first_prev = -1;
  for (int c = 0; c < C; ++c) {
    CHECK(p.size(c) >= 1);
    CHECK(p.find(p.ids[c]) == c);
    CHECK(p.rows[p.ptr[c]] > first_prev);   // clusters in order of first appearance
    first_prev = p.rows[p.ptr[c]];
    for (int k = p.ptr[c]; k < p.ptr[c + 1]; ++k) {
      const int i = p.rows[k];
      CHECK(i >= 0 && i < n && ids[i] == p.ids[c] && !seen[i]);
      seen[i] = 1;
      if (k > p.ptr[c]) CHECK(p.rows[k - 1] < i);   // observations keep their order
    }
  }
  std::vector<double> v(n);
  for (int i = 0; i < n; ++i) v[i] = 10. * i;
  const std::vector<double> g = gather_rows(p, v.data());
  for (int k = 0; k < n; ++k) CHECK(g[k] == 10. * p.rows[k]);
}

static void check_scatter(const std::vector<int32_t>& ids, bool want_var, bool want_cov) {
  const int n = (int)ids.size();
  const ClusterPartition p = partition_clusters(ids.data(), n);
  const size_t extra = want_cov ? (size_t)n * n : (want_var ? (size_t)n : 0);
  std::vector<double> out(n + extra, 0.);
  for (int c = 0; c < p.num_clusters(); ++c) {
    const std::vector<int> idx(p.rows.begin() + p.ptr[c], p.rows.begin() + p.ptr[c + 1]);
    const size_t k = idx.size();
    std::vector<double> res(k + (want_cov ? k * k : (want_var ? k : 0)));
    for (size_t a = 0; a < k; ++a) res[a] = 1. + idx[a];
    if (want_cov)
      for (size_t b = 0; b < k; ++b)
        for (size_t a = 0; a < k; ++a) res[k + b * k + a] = 1000. * (1 + idx[b]) + (1 + idx[a]);
    else if (want_var)
      for (size_t a = 0; a < k; ++a) res[k + a] = -1. - idx[a];
    scatter_cluster_prediction(n, idx, res.data(), res.data() + k, res.data() + k, want_var, want_cov, out.data());
  }
  for (int i = 0; i < n; ++i) CHECK(out[i] == 1. + i);
  if (want_cov) {
    for (int b = 0; b < n; ++b)
      for (int a = 0; a < n; ++a) {
        const double want = ids[a] == ids[b] ? 1000. * (1 + b) + (1 + a) : 0.;   // blocks between clusters stay 0
        CHECK(out[(size_t)n + (size_t)b * n + a] == want);
      }
  } else if (want_var) {
    for (int i = 0; i < n; ++i) CHECK(out[n + i] == -1. - i);
  }
}

int main() {
  check_partition({});
  check_partition({4});
  check_partition({7, 3, 7, 7, 3, 9});
  check_partition({-1, 2147483647, -2147483647 - 1, -1});
  std::mt19937 rng(1);
  for (int rep = 0; rep < 50; ++rep) {
    const int n = 1 + (int)(rng() % 300), C = 1 + (int)(rng() % 40);
    std::vector<int32_t> ids(n);
    for (auto& v : ids) v = (int32_t)(rng() % C) * 7 - 50;
    check_partition(ids);
    if (n <= 120) {
      check_scatter(ids, false, false);
      check_scatter(ids, true, false);
      check_scatter(ids, true, true);
    }
  }
  std::puts("cluster_partition_check ok");
  return 0;
}
