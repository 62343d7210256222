// LowRankPrecond: low-rank-plus-diagonal preconditioner P = Dg + L L^T of the latent-Vecchia CG on
// W^-1 + Sigma (cg_preconditioner_type = "pivoted_cholesky": Dg = W^-1, L = the pivoted Cholesky
// factor of the exact covariance Sigma; a later "fitc" preconditioner only brings another factor and
// diagonal).
//
// Reference replaced:
//   PivotedCholsekyFactorizationSigma                         CG_utils.h:438-488
//   the P^-1 products of CGVecchiaLaplaceSigmaPlusWinvVec /
//   CGTridiagVecchiaLaplaceSigmaPlusWinv                      CG_utils.cpp:276-282, 382-392
//   I_k + L^T W L and its Cholesky factor                     likelihoods.h:11986-11989, 12099-12103
//   the P^(1/2) draws, W^-1 P^-1 Z, the diagonal of
//   L (I_k + L^T W L)^-1 L^T                                  likelihoods.h:12093-12098, 12251-12261, 12288-12293
//
// Layout: L is row-major n x kpad (kpad = the rank rounded up to 8), so a row's earlier entries are
// contiguous for the L[j, :m] . L[p, :m] dot of the factorisation and for the tall-skinny products.
// Blocks of t vectors are row-major n x t like the rest of LatentVecchia. All reductions are two-stage
// sums in a fixed order (no floating-point atomics): equal inputs give equal bits.
//
// With G = I_k + L^T Dg^-1 L = E E^T and M = G^-1 (k x k, one workgroup):
//   P^-1 R   = Dg^-1 R - Dg^-1 L M L^T Dg^-1 R          (Woodbury)
//   log|P|   = log|G| + sum log Dg
//   P^(1/2)  : L e2 + Dg^(1/2) e1 ~ N(0, P)
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"

namespace gpb_amd {

constexpr double kPivCholStopTol = 1e-6;     // PIV_CHOL_STOP_TOL (re_model_template.h:8470-8476)
constexpr double kPivCholDropTol = 1e-12;    // entries below are not stored (CG_utils.h:476)

// Host restatement of PivotedCholsekyFactorizationSigma on points X (row-major n x d, in the order the
// permutation starts from), covariance cov_type (cov.h) with marginal variance var and range transform
// phi. L: row-major n x k (zero beyond the reached rank); piv: the pivot rows taken, in order. Returns
// the reached rank. The device factorisation follows the same rules; this form is the one tests check
// against an independent restatement without a GPU.
int pivoted_cholesky_host(int cov_type, const double* X, int n, int d, double var, double phi, int k, double tol,
                          double* L, int* piv);

class LowRankPrecond {
 public:
  LowRankPrecond(int n, int k, hipStream_t s);

  int n() const { return n_; }
  int k() const { return k_; }
  int kpad() const { return kpad_; }
  const double* L() const { return L_.get(); }

  // Pivoted Cholesky of the exact covariance of the points X (device, row-major n x d, storage order).
  // start (device, n): the storage row at position h of the initial permutation (the Vecchia order).
  // One update launch and one single-workgroup reduction per step, chained on the stream; the early
  // stop is a device flag that turns the later steps into no-ops (no host read-back in the loop).
  void Factorize(int cov_type, const double* X, int d, double var, double phi, const int* start);
  // Reached rank and pivots (storage rows) of the last Factorize; synchronises the stream.
  int Rank(std::vector<int>* piv = nullptr);

  // G = I + L^T diag(w) L, E = chol(G), M = G^-1, log|G|; w = Dg^-1 (device, n). flags() afterwards:
  // bit 0: some w > 1e10 (likelihoods.h:11977), bit 1: some w <= 0 or not finite, bit 2: G not positive definite.
  void SetWeights(const double* w);
  // log|G| and the flags of the last SetWeights; synchronises the stream.
  double LogDetG(int* flags);

  // Z = P^-1 R = w .* (R - L M L^T (w .* R)), t columns
  void Apply(const double* R, double* Z, int t);
  // out = d0 .* R + sgn * d1 .* (L T), T = M L^T (w .* Q) (Q nullable: T = Tin, k x t row-major device);
  // d0 / d1 nullable (= 1). The building block of Apply, of the P^(1/2) draws (Q null, T = e2, d0 =
  // Dg^(1/2)) and of W^-1 P^-1 Z = Z - L M L^T W Z (Q = Z, sgn = -1).
  void Combine(const double* R, const double* d0, const double* d1, double sgn, const double* Q, const double* Tin,
               double* out, int t);
  // diag[i] = L_i M L_i^T: the diagonal of L (I_k + L^T W L)^-1 L^T
  void RowDiag(double* diag);

 private:
  void Project(const double* Q, int t);   // T_ = M L^T (w .* Q)
  int n_, k_, kpad_;
  hipStream_t s_;
  DevBuf<double> L_, diag_, part_, G_, M_, S_, T_, out_;   // S_: E^-1 (SetWeights), L^T (w .* Q) (Project)
  DevBuf<int> pi_, state_;
  DevBuf<double> red_val_;
  DevBuf<int> red_pos_;
  const double* w_ = nullptr;
  int* h_state_ = nullptr;   // pinned read-back
  double* h_out_ = nullptr;
 public:
  ~LowRankPrecond();
  LowRankPrecond(const LowRankPrecond&) = delete;
  LowRankPrecond& operator=(const LowRankPrecond&) = delete;
};

// out[c] = sum_i A[i,c] * w[i] * B[i,c] (w nullable), c < t; deterministic two-stage sum through
// partials (>= 512 * t doubles)
void launch_weighted_coldots(int n, int t, const double* A, const double* w, const double* B, double* partials,
                             double* out, hipStream_t s);
// Y[i,c] = d[i] * X[i,c] (inv: X[i,c] / d[i]); Y may alias X
void launch_row_scale(int n, int t, const double* d, bool inv, const double* X, double* Y, hipStream_t s);
// V[i,c] += H[i,c] / w[i]
void launch_add_winv(int n, int t, const double* w, const double* H, double* V, hipStream_t s);
// y = 1 / sqrt(x)
void launch_rsqrt_vec(int n, const double* x, double* y, hipStream_t s);

// Row-wise stochastic d log|Sigma W + I| / d mode for P = W^-1 + L L^T (likelihoods.h:12276-12300) with
// per-row control variates: dmll[i] = 0.5 (tr1_i + a_i + c_i (k_i - a_i) - c_i trP_i), a_i = dW_i / W_i,
// k_i = rowdiag_i dW_i, tr1 / trP the row means of -WIU dW WIPZ and -WIPZ dW WIPZ over the t probes
// (WIU = W^-1 (W^-1 + Sigma)^-1 Z, WIPZ = W^-1 P^-1 Z). dW (device, n) = the derivative of the
// information wrt the location parameter.
void launch_lowrank_mode_deriv(int n, int t, const double* dW, const double* W, const double* rowdiag, const double* WIU,
                               const double* WIPZ, double* dmll, hipStream_t s);
// dW[i] = d information_i / d location_i of likelihood lik at loc (+ offset)
void launch_lik_dinfo(int n, int lik, double aux, const double* y, const double* loc, const double* offset, double* dW,
                      hipStream_t s);

}  // namespace gpb_amd
