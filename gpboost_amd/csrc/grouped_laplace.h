// GroupedLaplace: Laplace-approximated marginal likelihood of K grouped (crossed or nested) random effects
// under a non-Gaussian likelihood (bernoulli_logit, bernoulli_probit, poisson, gamma, negative_binomial) on one GPU.
//
// Model: b ~ N(0, Sigma), Sigma = diag(sigma_k^2 I_{m_k}); eta = F + Z b; y_i ~ p(. | eta_i). With
// A = Sigma^-1 + Z^T W Z (W = the information at the mode, changing with every Newton step) the reference's
//   FindModePostRandEffCalcMLLGroupedRE                                  likelihoods.h:1975-2194 (K >= 2)
//   FindModePostRandEffCalcMLLOnlyOneGroupedRECalculationsOnREScale      :2206-2293              (K == 1)
//   CalcGradNegMargLikelihoodLaplaceApproxGroupedRE, Cholesky branch     :3634-3740
//   CalcGradNegMargLikelihoodLaplaceApproxOnlyOneGroupedRE...            :3761-3854
// become
//   mode:  Newton steps A delta = Z^T d1 - Sigma^-1 b with Armijo halving (newton_line_search, laplace_newton.h) on
//          the objective ll(eta) - b^T Sigma^-1 b / 2, stopped on its relative change;
//   nll  = -(objective - log|A| / 2 + sum log diag(Sigma^-1) / 2);
//   grad (wrt log sigma_j^2) = -b_j^T b_j / (2 sigma_j^2) + sum_i W_i q_ij / 2 + v_j^T (Z^T d1)_j, where
//          q_ij = sum_k A^-1[lev_j(i), lev_k(i)], q_i = sum_j q_ij = diag(Z A^-1 Z^T)_i,
//          v = A^-1 Z^T (dW/deta . q) / 2 (the derivative of the log-determinant through the mode);
//          sum_i W_i q_ij = sum (A^-1 . I_j Z^T W Z), the reference's explicit trace, taken per observation;
//   grad (wrt log shape, gamma) = dnll/dlog a + sum_i W_i q_i / 2 + v^T Z^T d1 (dW/dlog a = W, dd1/dlog a = d1);
//   grad (wrt log shape, negative_binomial) = dnll/dlog r + sum_i (dW/dlog r)_i q_i / 2 + v^T Z^T (dd1/dlog r), the
//          general form (:3602-3625, 3723-3739, 3830-3850): glp_nb_aux_kernel writes the two per-observation
//          derivatives at the mode and sums log(mu_i + r) + (y_i + r) / (mu_i + r); the sum over i of
//          digamma(y_i + r) (and lgamma(y_i + r) of the normalising constant) comes from a table of the distinct
//          responses on the host; iterative: the trace by the probes with Z^T diag(dW/dlog r) Z as the operator;
//   grad (wrt F)_i = -d1_i + dW_i q_i / 2 - W_i (Z v)_i.
// K == 1: A is diagonal and every solve a division; K >= 2 with matrix_inversion_method = "cholesky": A dense in
// HBM, refactored at every Newton step on GroupedRE's MFMA POTRF / TRTRI path; K >= 2 with "iterative" (the
// default there): GroupedRE's SSOR-PCG, SLQ and stochastic traces on the weighted operator (GroupedRE::SetOperator),
// q_i estimated by mean_t[(Z A^-1 z)_i (Z P^-1 z)_i] over the probes z ~ N(0, P). The structure of Z^T Z (CSR,
// chunk plans, PCG work space, probes, dense factor buffers) is GroupedRE's.
//
// Z^T W Z and Z^T v are segmented sums over an inverted index built once on the host: the observations of
// every destination (the M levels, then the CSR slots of the level pairs) in ascending order. Destinations of
// at most 32 observations are summed by one thread each; longer lists (the levels of an effect with few
// levels) are cut into chunks of 512 summed by one wave each, and the chunk partials are added in chunk order.
// No floating-point atomics: equal inputs give equal bits.
//
// Random slopes (Z[i, lev_k(i)] = z_k[i] instead of 1): every formula above holds for any Z. The kernels have a
// second, WEIGHTED instantiation: the per-observation gathers multiply by z_k[i] read from a K x n table, and the
// segmented sums multiply each list entry by its precomputed value of Z (z_a[i], or z_a[i] z_b[i] for a destination
// of Z^T W Z), stored beside the observation index: one streamed double per entry, where two gathers from the
// table would move two 64-byte sectors. Models without slopes run the unweighted instantiation, unchanged.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"
#include "grouped.h"

namespace gpb_amd {

constexpr int kGlpMaxK = 8;

struct GroupedLaplaceResult {
  double nll = 0.;
  std::vector<double> grad;   // d/dlog sigma_k^2 (K), then (gamma / negative_binomial, if requested) d/dlog shape
  int newton_its = 0, cg_its = 0, lanczos_steps = 0;   // cg_its: the first Newton step's PCG (num_cg_steps_last_)
  bool nan = false;           // NaN / Inf in the mode finding or A not positive definite: nll = NaN
  float ms_assembly = 0.f, ms_newton_step = 0.f;   // GPBOOST_AMD_TIMING: last weighted assembly / Newton step (HIP events)
};

class GroupedLaplace {
 public:
  // where the Newton iterations begin (as LatentSolverBase::ModeStart, latent.h)
  enum class Start { kZero, kWarm, kKeep };
  // weights: as GroupedRE's (the same arrays; empty or all null: no random slopes, the unweighted kernels run)
  GroupedLaplace(GroupedRE* re, const std::vector<std::vector<int>>& levels, int lik,
                 const std::vector<const double*>& weights = {});
  ~GroupedLaplace();
  GroupedLaplace(const GroupedLaplace&) = delete;
  GroupedLaplace& operator=(const GroupedLaplace&) = delete;

  void SetY(const double* y);              // host, n
  void SetOffset(const double* offset);    // host, n; null: none
  // Device form of SetOffset: the offset buffer (n doubles on stream()) for the caller to fill before Eval; the
  // model has an offset from this call on, until SetOffset(nullptr).
  double* DeviceOffset();
  // Device access to the gradient wrt the fixed effects: with keep, every Eval with want_grad leaves it in
  // DeviceGradF() (n doubles, valid after Eval returns) whether or not a host grad_f is given.
  void KeepDeviceGradF(bool keep) { keep_gradf_ = keep; }
  const double* DeviceGradF() const { return d_gradf_.get(); }
  hipStream_t stream() const { return s_; }
  // sigma2: the K variances. grad_f (host n, nullable; needs want_grad): gradient wrt the fixed effects.
  // iterative (K >= 2; likelihoods.h:2019-2048, 2094-2180, 3467-3633): the Newton systems by SSOR-PCG (the first
  // solve of an evaluation from zero, later ones from the previous update), log|A| by SLQ on probes from N(0, P),
  // the traces stochastic with the SSOR control variate, diag(Z A^-1 Z^T) dW by the row-wise probe products, and
  // A^-1 d_mll_d_mode by one more PCG at cg_delta_conv_pred = 1e-3 (re_model_template.h:5370)
  GroupedLaplaceResult Eval(const double* sigma2, double aux, const IterativeConfig& cfg, bool iterative, bool want_grad,
                            bool want_aux_grad, double* grad_f, Start start);
  void ResetModeToPrevious();
  void ClearModePrevious() { mode_prev_valid_ = false; }
  void GetMode(double* b);                 // host, M (effect-major)
  // e_p^T A^-1 e_p on the factor of the last evaluation (idx: np x K global level indices, -1: unseen; wt nullable,
  // np x K: Z's values of the prediction points, the entries of e_p)
  void PredVar(int np, const std::vector<int>& idx, double* out, const double* wt = nullptr);
  // test hook: the diagonal (M) and the off-diagonal CSR values (nnz) of Z^T W Z of the last evaluation
  void GetZtWZ(double* diag, double* vals);
  // test hook (grouped_test.cpp): Assemble on a caller's w, the level table and the segment counts
  friend struct GroupedTestAccess;

 private:
  void Assemble(const double* w, double* out, bool diag_only);
  double Objective(const double* mode, double aux, const double* sigi);   // ll + const - b^T Sigma^-1 b / 2
  void Deriv(const double* mode, double aux, bool want_dw);
  double LogLikConst(double aux) const;

  GroupedRE* re_;
  GroupedRE::View v_;
  int lik_;
  hipStream_t s_;
  int nb_ = 1;   // blocks of the observation passes
  DevBuf<int> d_glev_;   // K x n global level indices
  // random slopes (wt_): Z's values as the K x n table of the per-observation gathers (eta, q, the probe rows,
  // grad_F) and per entry of the inverted index (d_seg_w1_: z_k[i] over the M level lists, for Z^T v; d_seg_w2_:
  // z_k[i]^2 over them and z_a[i] z_b[i] over the pair lists, for Z^T W Z). Null without slopes.
  bool wt_ = false;
  DevBuf<double> d_zw_, d_seg_w1_, d_seg_w2_;
  // inverted index: destination -> observations
  DevBuf<int> d_seg_ptr_, d_seg_obs_, d_c0_, d_c1_, d_long_dst_, d_long_cptr_;
  int n_chunks_ = 0, n_chunks_diag_ = 0, n_long_ = 0, n_long_diag_ = 0;
  DevBuf<double> d_chunk_P_;
  DevBuf<double> d_y_, d_off_, d_d1_, d_W_, d_dW_, d_dwq_, d_gradf_;
  DevBuf<double> d_mode_, d_mode_new_, d_mode_prev_, d_upd_, d_rhs_, d_ztd1_, d_ztwz_, d_D_, d_dmll_, d_vS_;
  DevBuf<double> d_partial_, d_red_, d_dis_, d_blkA_, d_blkB_;
  double* h_red_ = nullptr;   // pinned
  bool has_off_ = false, keep_gradf_ = false, y_set_ = false, mode_prev_valid_ = false, evaluated_ = false;
  double lognorm_ = 0., sum_log_y_ = 0.;
  // negative_binomial: the distinct responses ascending with their multiplicities (SetY), so that the sums over
  // i of lgamma(y_i + r) and digamma(y_i + r) cost O(distinct values) per evaluation and have one order; the
  // per-observation shape derivatives dd1 / dlog r and dW / dlog r at the mode, Z^T of the former, and (iterative)
  // Z^T diag(dW / dlog r) Z in the layout of d_ztwz_
  std::vector<double> y_vals_, y_cnt_;
  double SumOverY(double (*f)(double), double r) const;   // sum_v c_v f(v + r), ascending v
  DevBuf<double> d_dd1a_, d_dWa_, d_zta_, d_ztdwz_;
  hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
};

}  // namespace gpb_amd
