// Full-scale Vecchia approximation ("VIF", gp_approx = "full_scale_vecchia" / "vif") for the Gaussian
// likelihood: the reference's predictive-process-plus-Vecchia-residual covariance
//   Psi = K_nm K_mm,s^-1 K_mn + B^-1 D B^-T
// on the transformed scale (nugget 1 in the residual part), where B (unit lower, the Vecchia neighbours
// of each point in the model order) and D come from the RESIDUAL covariances
//   C_res(a, b) = k(a, b) + [a == b] - V_a . V_b,   V = L^-1 K_mn,  L = chol(K_mm,s)
// among each point and its neighbours, and K_mm,s = K_mm with its diagonal times (1 + 1e-6).
//
// Reference path replaced:
//   ordering + inducing points  re_model_template.h:348-357 (shuffle with rng_, then CreateREComponentsFITC_FSA
//                               on the shuffled coordinates with the same generator)
//   neighbours                  Vecchia_utils.cpp:732-1058 (Euclidean kNN among earlier points; the GPU search)
//   Sigma components            re_model_template.h:7341-7378 (CalcSigmaComps)
//   residual factor + gradient  Vecchia_utils.cpp:1388-1617 (CalcCovFactorGradientVecchia, full_scale_vecchia)
//   Woodbury factor             re_model_template.h:8770-8880 (CalcCovFactorFITC_FSA, cholesky)
//   y_aux, log det              re_model_template.h:8898-8935, 2698-2714
//   gradient                    re_model_template.h:1985-2232 (CalcGradPars_FITC_FSA_GaussLikelihood_Cluster_i)
// The reference runs these with Eigen sparse products, cuBLAS / cuSPARSE offloads (cuda_kernel.cu:613-941).
// This build: one wave per row for the residual factor with the neighbour set's Gram blocks V_S^T [V P_0
// P_1]_S on the fp64 MFMA (operands loaded straight from the m x n matrices; sets of up to 32 points, the
// reference's default 30 neighbours; larger sets: a 256-thread LDS-staged register-tile form), the small
// Cholesky and solves in LDS / registers of that wave; sparse B / B^T products over contiguous m-vectors
// (one wave per point; B^T vectors from the factor values gathered into column order); every m x n /
// m x m product on the fp64 MFMA GEMM (split-K for the m x m Woodbury Gram).
// A row whose residual matrix is not positive definite gets D_i = NaN (VifRowsLaunch below), so the sums are NaN.
//
// HBM layout: every m x n matrix column-major with leading dimension ldm = round_up(m, 64) (point i's m
// entries contiguous), the B / D factor and its derivatives as n x nn value rows beside the neighbour lists.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "common.h"
#include "fitc.h"

namespace gpb_amd {

// ---- host launch code of the row-factor, product and vector kernels (vif_kernels.hip): the one way these kernels
// are launched, by VifSolver and by the test entries (vif_test.cpp) alike.

// One launch of the residual row factor for the rows i0 .. n_total - 1 (device pointers; vif_kernels.hip states the
// formulas). form 0: the production dispatch (the MFMA Gram form for nn <= 31, else the LDS-staged form), 1: the
// MFMA form (nn <= 31), 2: the LDS-staged form. Limits: nn <= 48 with derivatives, <= 64 without.
// Non-positive-definite contract: a row whose residual matrix C has a pivot that is not > 0 or not finite gets
// D_i = NaN (in both forms; its B / dB / dD entries are unspecified); every other row is unaffected, and the
// evaluation's sums (log D) become NaN.
struct VifRowsLaunch {
  const double* X = nullptr;     // n_total x d
  const int* nbr = nullptr;      // (n_total - i0) x nn, row i - i0 holds min(i, nn) indices < i
  int n_total = 0, d = 0, nn = 0, m = 0, ldm = 0, i0 = 0;
  const double* V = nullptr;     // m x n_total (ldm)
  const double* P0 = nullptr;    // with grad
  const double* P1 = nullptr;
  int cov_type = 0;
  double var = 0., phi = 0., nugget = 1., cjit = 1.;
  bool grad = false;
  int form = 0;
  const int* ord = nullptr;      // nullable: the n_total - i0 rows in processing order (vif_morton_order)
  double* Bv = nullptr;          // (n_total - i0) x nn
  double* D = nullptr;           // n_total - i0
  double* dBv0 = nullptr;
  double* dBv1 = nullptr;
  double* dD0 = nullptr;
  double* dD1 = nullptr;
};
void vif_launch_rows(const VifRowsLaunch& L, hipStream_t s);
constexpr int kVifMaxNn = 64, kVifMaxNnGrad = 48, kVifMaxNnMfma = 31;

// the points along a Morton curve of their (first two) coordinates (X host row-major n x d)
std::vector<int> vif_morton_order(const double* X, int n, int d);
// B^T lists of the n x nn neighbour lists: for every column j the rows i (ascending) that hold j, with the slot
// i nn + r of the value; returns the number of entries
int vif_transpose_lists(int n, int nn, const int* nbr, std::vector<int>& tptr, std::vector<int>& trow,
                        std::vector<int>& tslot);

// the graph of the sparse products (device pointers); ord nullable
struct VifGraph {
  int n = 0, nn = 0, m = 0, ldm = 0;
  const int* nbr = nullptr;
  const int* tptr = nullptr;
  const int* trow = nullptr;
  const int* ord = nullptr;
};
// out[:, i] = self in[:, i] + sum_r coef[i nn + r] in[:, nbr[i nn + r]], div: then times 1 / D_i; out_div
// (nullable): the same columns times 1 / D_i (D is read only with div or out_div)
void vif_launch_brow(hipStream_t s, const VifGraph& g, const double* in, const double* coef, const double* D,
                     double self, bool div, double* out, double* out_div);
// out[:, j] = self in[:, j] + sum over column j's entries t of coefT[t] in[:, trow[t]]
void vif_launch_bcol(hipStream_t s, const VifGraph& g, const double* in, const double* coefT, double self, double* out);
// out_i = (self x_i + sum_r coef[i nn + r] x[nbr[i nn + r]]) (/ D_i with D)
void vif_launch_bvec(hipStream_t s, const VifGraph& g, const double* x, const double* coef, const double* D,
                     double self, double* out);
void vif_launch_btvec(hipStream_t s, const VifGraph& g, const double* x, const double* coefT, double self, double* out);
void vif_launch_gather(hipStream_t s, int nnz, const int* tslot, const double* coef, double* coefT);
// out (m) = M x for the m x n matrix M (ldm); part: (n + 63) / 64 x ldm doubles
void vif_launch_gemv(hipStream_t s, int n, int m, int ldm, const double* M, const double* x, double* part, double* out);
// out_i = M[:, i] . w (w != nullptr) or M[:, i] . M2[:, i], i < cols
void vif_launch_coldot(hipStream_t s, int cols, int m, int ldm, const double* M, const double* w, const double* M2,
                       double* out);
// z_i = (e_i - dD_i u_i) / D_i
void vif_launch_zvec(hipStream_t s, int n, const double* dD, const double* u, const double* e, const double* D,
                     double* z);
// Sums over i < n of up to 8 elementwise terms; op 0: a (b) (c) (nullable factors), 1: log a, 2: a (b) / c,
// 3: a b^2 / c^2, 4: a b / c^2. part: min(512, blocks) x nt doubles; out: nt sums.
struct VifTerms {
  const double* a[8];
  const double* b[8];
  const double* c[8];
  int op[8];
};
void vif_launch_sum(hipStream_t s, int n, int nt, const VifTerms& T, double* part, double* out);
// dK_mn / dlog(phi) (m x n, ldm) for the points X (n x d) and the inducing points Z (m x d)
void vif_launch_dkmn(hipStream_t s, int cov_type, const double* X, const double* Z, int n, int m, int d, int ldm,
                     double var, double phi, double* dK);

class VifSolver {
 public:
  // d_X: device row-major n x d coordinates in the model order; Z: host row-major m x d inducing points;
  // nbr: host n x nn neighbour lists (row i holds its min(i, nn) neighbours, the rest -1).
  VifSolver(int n, int d, const double* d_X, const std::vector<double>& Z, const std::vector<int>& nbr, int nn,
            hipStream_t stream);
  ~VifSolver();
  const std::vector<double>& inducing_points() const { return F_->inducing_points(); }
  // sums = [logdet, q, s1_var, s1_range, s2_var, s2_range] (combine_partials): s1_k = -1/2 y_aux^T dPsi_k
  // y_aux, s2_k = tr(Psi^-1 dPsi_k) with the reference's dPsi_k (un-jittered dK_mm, B_grad, D_grad). A
  // non-positive-definite factor gives NaN sums. kernel_ms[0] = factor part, [1] = whole evaluation.
  void Eval(int cov_type, double var, double phi, const double* d_y, bool want_grad, double* sums, double* kernel_ms);
  // D (n) and B's values (n x nn, 0 past a row's neighbours) of the last evaluation (host); nullable: their
  // derivatives with respect to log var and log phi of the last evaluation with the gradient
  void GetFactor(double* D, double* Bv, double* dD0 = nullptr, double* dD1 = nullptr, double* dBv0 = nullptr,
                 double* dBv1 = nullptr) const;
  // The residual factor with its derivatives at (var, phi): the likelihood-independent part of an evaluation with
  // the gradient (the GEMM chain that makes V and P_k, then the rows), then GetFactor
  void Factor(int cov_type, double var, double phi, double* D, double* Bv, double* dD0, double* dD1, double* dBv0,
              double* dBv1);
  // Predictions for the Gaussian likelihood (CalcPredVecchiaObservedFirstOrder, full_scale_vecchia branches,
  // Vecchia_utils.cpp:1686-1707, 1826-1840, 1872-1873, 1901-1980) at (var, phi) on the transformed scale,
  // nugget 1 included: Xp host row-major np x d prediction points (after the n observed points); nbr host
  // np x mp neighbour indices (< n: observed points; >= n: earlier prediction points, cond_all). mean (np);
  // pvar (np, nullable); pcov (np x np column-major, nullable). Runs Eval(want_grad = false) first.
  void Predict(int cov_type, double var, double phi, const double* d_y, const double* Xp, int np, const int* nbr,
               int mp, bool cond_all, double* mean, double* pvar, double* pcov);
  // G = Z^T Psi^-1 Z (host, c x c row-major) for the device matrix d_Z (n x c row-major, model order) on the
  // transformed scale (DenseSolver::Gram's contract): G0 - S^T S with U = B Z, T = BK diag(1 / D) U, G0 = U^T
  // diag(1 / D) U, S = L_M^-1 T (lowrank_gram.hip). Runs Prepare(grad) and keeps its results for the next
  // Eval(want_grad == grad) at the same (cov_type, var, phi), which then reruns only its response-dependent part.
  // A non-positive-definite factor gives a NaN G. gram_ms (nullable): device ms of Prepare and of the whole call.
  void Gram(int cov_type, double var, double phi, bool grad, const double* d_Z, int c, double* G_host,
            double* gram_ms = nullptr);

 private:
  friend class VifLaplace;   // the Laplace approximation for non-Gaussian likelihoods (vif_laplace.h)
  // the likelihood-independent part of an evaluation: the low-rank part (K_mn, K_mm,s, L, V), with grad the
  // derivative blocks (dK, A, P_0, P_1), the residual factor (+ column-order values) and the Woodbury
  // matrix M = K_mm,s + BK^T D^-1 BK factored in place (F_->W_ = L_M, Wi_ = L_M^-1, WiT_); red[0] = log det
  // K_mm,s, red[1] = log det M; M_copy (nullable, ldm x ldm): M before its factorization
  void Prepare(int cov_type, double var, double phi, bool grad, double* red, double* M_copy = nullptr);
  void Rows(int cov_type, double var, double phi, bool grad);
  VifGraph graph() const;
  // Prepare's results are in place for (kept_cov_, kept_var_, kept_phi_, kept_grad_) with their sums in red_: set
  // by Gram, used once by the next Eval, cleared by Prepare (every other entry overwrites the buffers through it)
  bool kept_ = false, kept_grad_ = false;
  int kept_cov_ = 0;
  double kept_var_ = 0., kept_phi_ = 0.;
  DevBuf<double> gram_U_;   // B Z (n x kCovMaxCols)
  LowrankGramWork gram_ws_;
  // the prediction points' residual rows (Xp host np x d after the n observed points, nbr host np x mp):
  // KP = K_mp (m x np), Va = [V | L^-1 K_mp], Bvp (np x mp), Dp (np), dnb the neighbour lists on the device
  void PredRows(int cov_type, double var, double phi, const double* Xp, int np, const int* nbr, int mp,
                DevBuf<double>& KP, DevBuf<double>& Va, DevBuf<double>& Bvp, DevBuf<double>& Dp, DevBuf<int>& dnb);
  // mo_p = sum over observed neighbours of B(p, j) r_j, Qt[:, p] = sum of B(p, j) M[:, j] (M m x n; Qt m x np)
  void PredBpo(int np, int mp, const int* dnb, const double* Bvp, const double* r, const double* M, double* mo,
               double* Qt);
  // out_i = M[:, i] . w (w != nullptr) or M[:, i] . M2[:, i] for `cols` columns
  void ColDotN(const double* M, const double* w, const double* M2, int cols, double* out);
  // out = B in (self = 1) or dB in (self = 0) over m-vector columns; div: then times D^-1; out_div
  // (nullable): the same columns times D^-1 as a second output
  void BRow(const double* in, const double* coef, double self, bool div, double* out, double* out_div = nullptr);
  // out = B^T in (self = 1) or dB^T in (self = 0) over m-vector columns
  void BCol(const double* in, const double* coefT, double self, double* out);   // coefT: values in column order
  void BVec(const double* x, const double* coef, double self, double* out);
  // out = B^T x (self = 1) or dB^T x (self = 0), coefT: the factor's values in column order (BvT_ ...)
  void BtVec(const double* x, const double* coefT, double self, double* out);
  void Gemv(const double* M, const double* x, double* out);   // out (m) = M x, M m x n
  void ColDot(const double* M, const double* w, const double* M2, double* out);   // out_i = M_i . (w | M2_i)

  std::unique_ptr<FitcSolver> F_;
  int n_, d_, m_, ldm_, nn_;
  bool latent_ = false;   // residual rows of the latent form (no nugget; JITTER_MULT_VECCHIA on the neighbour diagonal)
  hipStream_t s_;
  const double* d_X_;
  DevBuf<int> nbr_, tptr_, trow_, tslot_;
  DevBuf<int> ord_;   // the points in spatial (Morton) order: processing order of the row / B-product kernels
  DevBuf<double> dK_, P0_, P1_, BK_;                 // m x n (ldm)
  DevBuf<double> Bv_, dBv0_, dBv1_;                   // n x nn
  DevBuf<double> BvT_, dBvT0_, dBvT1_;                // the same values in column (B^T) order
  int nnz_ = 0;
  DevBuf<double> D_, dD0_, dD1_;                      // n
  DevBuf<double> vec_;                                // n-vectors (scratch)
  DevBuf<double> mvec_;                               // m-vectors (scratch)
  DevBuf<double> part_, red_;
  double* h_red_ = nullptr;
  size_t lds_bytes_ = 0;
  hipEvent_t ev_[3] = {nullptr, nullptr, nullptr};
};

}  // namespace gpb_amd
