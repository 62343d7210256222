// REModelAMD: independent realisations of the process (cluster_ids with more than one distinct value).
//
// Equal ids are one realisation, different ids independent realisations that share the covariance parameters
// (re_model_template.h: SetUpGPIds :6211-6243, one set of components per cluster). y' Psi^-1 y, log|Psi| and every
// quadratic and trace term of the gradient are sums over the clusters, so the six sums of every cluster are added
// and combine_partials runs once over all n (sigma^2 is profiled over all n). Clusters of at most kBatchMaxN points
// go to the batched kernel in one launch (dense_batch.hip); every other cluster has an engine, a single-cluster
// REModelAMD on its rows. Under the Vecchia approximation a cluster of at most min(kBatchMaxN, m + 1) points is
// exact (every row conditions on all earlier ones) and goes to the batched kernel too.
// GPBOOST_AMD_NO_CLUSTER_BATCH=1 (read at construction) gives every cluster an engine (A/B timing, tests).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>

#include "cov.h"
#include "kernels.h"
#include "re_model.h"

namespace gpb_amd {

void REModelAMD::RefuseClusters(const char* option) const {
  if (clustered())
    Fatal("%s with several clusters (cluster_ids) is not supported by gpboost_amd", option);
}

void REModelAMD::GetClusterInfo(int32_t* out) const {
  int batched = 0;
  for (int e : cl_engine_of_) batched += e < 0 ? 1 : 0;
  out[0] = clustered() ? cl_.num_clusters() : 1;
  out[1] = batched;
  out[2] = (int32_t)cl_engines_.size();
}

// The engine of cluster c: this model's configuration on the cluster's rows. A Vecchia model's cluster of one
// point has no neighbours: its engine is the dense one (the same likelihood).
std::unique_ptr<REModelAMD> REModelAMD::ClusterEngine(int c, std::mt19937* order_rng) const {
  const int d = cfg_.d, nc = cl_.size(c);
  ModelConfig sc = cfg_in_;
  sc.n = nc;
  if (vecchia_ && nc < 2) sc.gp_approx = "none";
  std::vector<double> xc((size_t)nc * d);   // column-major nc x d
  for (int i = 0; i < nc; ++i)
    for (int q = 0; q < d; ++q) xc[(size_t)q * nc + i] = coords_[(size_t)cl_.rows[cl_.ptr[c] + i] * d + q];
  return std::unique_ptr<REModelAMD>(new REModelAMD(sc, xc.data(), nullptr, order_rng));
}

void REModelAMD::SetUpClusters(const int32_t* cluster_ids) {
  const int n = cfg_.n, d = cfg_.d;
  cl_ = partition_clusters(cluster_ids, n);
  const int C = cl_.num_clusters();
  if (vecchia_ && cfg_.num_neighbors < 1) Fatal("num_neighbors must be >= 1");
  const char* e = std::getenv("GPBOOST_AMD_NO_CLUSTER_BATCH");
  const bool no_batch = e != nullptr && e[0] != '\0' && e[0] != '0';
  const int batch_max = vecchia_ ? std::min(kBatchMaxN, cfg_.num_neighbors + 1) : kBatchMaxN;
  // vecchia_ordering "random": every cluster is shuffled from the model's generator in cluster order; a batched
  // cluster draws its shuffle too (and needs no order), so the engines' orders do not depend on the routing
  std::mt19937 order_rng((std::mt19937::result_type)cfg_.seed);
  const bool shuffle = vecchia_ && cfg_.vecchia_ordering == "random";
  cl_engine_of_.assign(C, -1);
  std::vector<double> bx;
  std::vector<int> bptr(1, 0);
  for (int c = 0; c < C; ++c) {
    const int nc = cl_.size(c);
    if (!no_batch && nc <= batch_max) {
      for (int i = 0; i < nc; ++i) {
        const int o = cl_.rows[cl_.ptr[c] + i];
        cl_batch_rows_.push_back(o);
        for (int q = 0; q < d; ++q) bx.push_back(coords_[(size_t)o * d + q]);
      }
      bptr.push_back((int)cl_batch_rows_.size());
      if (shuffle) {
        std::vector<int> dummy(nc);
        std::iota(dummy.begin(), dummy.end(), 0);
        std::shuffle(dummy.begin(), dummy.end(), order_rng);
      }
    } else {
      cl_engine_of_[c] = (int)cl_engines_.size();
      cl_engines_.push_back(ClusterEngine(c, &order_rng));
    }
  }
  if (bptr.size() > 1) cl_batch_.reset(new DenseBatch(d, bx, bptr, stream_));
}

void REModelAMD::SetYClusters(const double* y) {
  const int n = cfg_.n;
  cl_y_.assign(y, y + n);
  if (cl_batch_) {
    std::vector<double> yb(cl_batch_rows_.size());
    for (size_t k = 0; k < yb.size(); ++k) yb[k] = y[cl_batch_rows_[k]];
    cl_batch_->SetY(yb.data());
  }
  std::vector<double> yc;
  for (int c = 0; c < cl_.num_clusters(); ++c) {
    if (cl_engine_of_[c] < 0) continue;
    yc.resize(cl_.size(c));
    for (int i = 0; i < cl_.size(c); ++i) yc[i] = y[cl_.rows[cl_.ptr[c] + i]];
    cl_engines_[cl_engine_of_[c]]->SetY(yc.data());
  }
  y_set_ = true;
}

void REModelAMD::RawSums(const double* trafo, bool want_grad, double* sums) {
  UseDevice();
  EnsureStructure();
  if (vecchia_) EvalVecchia(trafo, sums);
  else EvalExactGaussian(trafo, want_grad, sums);
}

void REModelAMD::EvalClusters(const double* trafo, bool want_grad, double* sums) {
  std::fill(sums, sums + kVecchiaSums, 0.);
  double s[kVecchiaSums];
  events_pending_ = false;
  if (cl_batch_) {
    cl_batch_->Eval(cfg_.cov_type, trafo[1], trafo[2], want_grad, s);
    for (int q = 0; q < kVecchiaSums; ++q) sums[q] += s[q];
  }
  for (auto& eng : cl_engines_) {   // cluster order
    eng->RawSums(trafo, want_grad, s);
    for (int q = 0; q < kVecchiaSums; ++q) sums[q] += s[q];
  }
}

void REModelAMD::PredictClusters(const double* y, int n_pred, const double* coords_pred,
                                 const int32_t* cluster_ids_pred, const double* cov_pars, bool predict_cov_mat,
                                 bool predict_var, bool predict_response, double* out, const double* mean_add) {
  if (!clustered()) Fatal("PredictClusters: the model has one cluster");
  if (n_pred <= 0) Fatal("num_data_pred must be > 0");
  if (coords_pred == nullptr) Fatal("gp_coords_data_pred must be provided");
  if (cluster_ids_pred == nullptr)
    Fatal("cluster_ids_pred (cluster_ids_data_pred) must be provided for predictions of a model with several clusters");
  UseDevice();
  if (y != nullptr) SetY(y);
  if (!y_set_) Fatal("response variable y has not been set (pass y or evaluate the likelihood first)");
  double cp[3];
  if (cov_pars != nullptr) std::copy(cov_pars, cov_pars + 3, cp);
  else if ((int)last_cov_pars_.size() == 3) std::copy(last_cov_pars_.begin(), last_cov_pars_.end(), cp);
  else Fatal("cov_pars must be provided (no previous evaluation)");
  double trafo[3];
  TransformCovPars(cp, trafo);
  const int d = cfg_.d;
  const bool want_cov = predict_cov_mat, want_var = predict_var && !predict_cov_mat;
  const size_t extra = want_cov ? (size_t)n_pred * n_pred : (want_var ? (size_t)n_pred : 0);
  std::fill(out, out + n_pred + extra, 0.);   // covariances between clusters are 0
  const ClusterPartition pp = partition_clusters(cluster_ids_pred, n_pred);
  std::vector<double> xk, res, madd, yc;
  for (int g = 0; g < pp.num_clusters(); ++g) {
    const std::vector<int> idx(pp.rows.begin() + pp.ptr[g], pp.rows.begin() + pp.ptr[g + 1]);
    const int k = (int)idx.size();
    const int c = cl_.find(pp.ids[g]);
    res.assign((size_t)k + (want_cov ? (size_t)k * k : (want_var ? (size_t)k : 0)), 0.);
    if (c < 0) {
      // an id without training data: mean 0 (or the offset) and the prior covariance sigma1^2 corr, plus the nugget
      // for the response (re_model_template.h:3350-3384)
      const double nug = predict_response ? cp[0] : 0.;
      for (int a = 0; a < k; ++a) res[a] = mean_add != nullptr ? mean_add[idx[a]] : 0.;
      if (want_var)
        for (int a = 0; a < k; ++a) res[k + a] = cp[1] + nug;
      if (want_cov)
        dispatch_cov(cfg_.cov_type, [&](auto cov) {
          constexpr int COV = decltype(cov)::value;
          for (int b = 0; b < k; ++b)
            for (int a = 0; a < k; ++a) {
              double s = 0.;
              for (int q = 0; q < d; ++q) {
                const double df = coords_pred[(size_t)q * n_pred + idx[a]] - coords_pred[(size_t)q * n_pred + idx[b]];
                s += df * df;
              }
              double cc, dc;
              cov_dcov<COV>(std::sqrt(s), cp[1], trafo[2], cc, dc);
              res[(size_t)k + (size_t)b * k + a] = a == b ? cp[1] + nug : cc;
            }
        });
    } else {
      xk.resize((size_t)k * d);   // column-major k x d
      for (int a = 0; a < k; ++a)
        for (int q = 0; q < d; ++q) xk[(size_t)q * k + a] = coords_pred[(size_t)q * n_pred + idx[a]];
      const double* ma = nullptr;
      if (mean_add != nullptr) {
        madd.resize(k);
        for (int a = 0; a < k; ++a) madd[a] = mean_add[idx[a]];
        ma = madd.data();
      }
      // the cluster's engine, or one built for this call (a batched cluster; prediction is not the hot path)
      std::unique_ptr<REModelAMD> tmp;
      REModelAMD* eng = nullptr;
      const double* ye = nullptr;
      if (cl_engine_of_[c] >= 0) {
        eng = cl_engines_[cl_engine_of_[c]].get();
      } else {
        tmp = ClusterEngine(c, nullptr);
        eng = tmp.get();
        yc.resize(cl_.size(c));
        for (int i = 0; i < cl_.size(c); ++i) yc[i] = cl_y_[cl_.rows[cl_.ptr[c] + i]];
        ye = yc.data();
      }
      if (eng->vecchia_) eng->SetPredictionData(vecchia_pred_type_.c_str(), num_neighbors_pred_, nsim_var_pred_);
      eng->Predict(ye, k, xk.data(), cp, predict_cov_mat, predict_var, predict_response, res.data(), ma);
    }
    scatter_cluster_prediction(n_pred, idx, res.data(), res.data() + k, res.data() + k, want_var, want_cov, out);
  }
}

}  // namespace gpb_amd
