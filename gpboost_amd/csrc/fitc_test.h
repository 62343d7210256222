// Test entries of the FITC kernels and the k-means inducing-point search (GPB_TestFitc*, include/gpboost_amd.h;
// fitc_test.cpp). Host arrays in and out; every extent and index is checked on the host before any device call; the
// kernels run through the launch functions of fitc.h, the ones FitcSolver and fitc_inducing_points use.
#pragma once

#include <cstdint>

namespace gpb_amd {

// op of GPB_TestFitcVector. Matrices that the device holds as m x n (ld ldm) are host arrays n x m row-major, the
// m x m ones m x m row-major (row k = the device's column k); outputs of that kind come back with their padding
// (n x ldm, m x ldm).
enum FitcVecOp : int {
  kFitcKmn = 0,      // arrays X (n d), Z (m d); outs Kmn (n ldm)
  kFitcKmm,          // arrays Z; outs Kmm, Ks, dK (m ldm each)
  kFitcDkmn,         // arrays X, Z; outs dKmn (n ldm)
  kFitcDiag,         // arrays V, Kmn (n m); extra = dvar; outs d (n), Kd (n ldm), sum log d (1)
  kFitcDy,           // arrays d, y (n); outs Dy (n)
  kFitcWsum,         // arrays P (chunks m m), Ks (m m); ints [chunks]; outs W (m ldm)
  kFitcGemv,         // arrays M (n m), x (n); outs out (m)
  kFitcSymv,         // arrays S (m m), x (m); outs out (m)
  kFitcLowerT,       // arrays L (m m); outs LT (m ldm)
  kFitcCholSolve,    // arrays Li, LiT (m m), x (m); outs out (m)
  kFitcYaux,         // arrays Kmn (n m), w (m), y, Dy, d (n); outs yaux (n), y^T yaux (1)
  kFitcGrad,         // arrays X, Z, Kmn, A, Gt, Mr (n m), a (m), d, yaux (n); extra = delta; outs sums (4), parts (4 nb4)
  kFitcMmTerms,      // arrays Kinv, Winv, Kmm, dK (m m), a (m); outs sums (6)
  kFitcColdot,       // arrays M (n m), v (m, nullable: squares); outs out (n)
  kFitcPredCorr,     // n = training points; ints [np, pi_0, oj_0, pi_1, ...]; arrays P (np m), Kmn (n m), d (n),
                     // Maux (np m); extra = sii; outs Maux (np ldm), corr (max(npairs, 1))
  kFitcFfDiagGrad,   // arrays A, dK, M (n m); extra = base; outs dd (n)
  kFitcFfRecip,      // arrays x (n); outs y (n)
  kFitcFfRowscale,   // m = t columns; arrays s (n), X (n t column-major), Yin (nullable); extra = alpha; ints [alias]:
                     // 1 = Y is Yin's own buffer; outs Y (n t)
  kFitcFfDot,        // n = count; arrays a, b (n); outs sum (1)
  kNumFitcVecOps
};

void test_fitc_vector(int op, int n, int m, int d, int cov_type, double var, double phi, double extra, double pad_fill,
                      const double* const* arrays, const int64_t* lens, int n_arrays, const int32_t* ints,
                      int64_t ints_len, double* const* outs, const int64_t* out_lens, int n_outs, int* guard);

// op of GPB_TestFitcKmeans
enum FitcKmeansOp : int {
  kFitcKmAssign = 0,   // X, mu; ints_out: the cluster of every point (n)
  kFitcKmMeans,        // X, mu (the old means), cluster_in (n), scan; mu_out (k d); member-list path: ints_out = cnt,
                       // off (nbk k each), tot (k), base (k + 1), list (n)
  kFitcKmCmp,          // mu, mu_a, mu_b (k d each); ints_out: the two flags
  kFitcKmLloyd,        // X, mu (seeds), scan, max_it; mu_out, its
  kNumFitcKmeansOps
};

void test_fitc_kmeans(int op, int n, int k, int d, const double* X, int64_t x_len, const double* mu, const double* mu_a,
                      const double* mu_b, int64_t mu_len, const int32_t* cluster_in, int64_t cluster_len, int scan,
                      int max_it, double* mu_out, int32_t* ints_out, int64_t ints_len, int* its, int* guard);

// stage of GPB_TestFitcStages: a FitcSolver on X (n x d), Z (m x d) and y runs the stage, then its buffers are
// copied out as they stand
enum FitcStage : int {
  kFitcStFactor = 0,      // Factor(var, phi)
  kFitcStEval,            // Eval(var, phi) with the gradient
  kFitcStGramEval,        // Gram(var, phi) then Eval(var, phi): the kept_ hand-over
  kFitcStGramOtherEval,   // Gram(var2, phi2) then Eval(var, phi): the hand-over must not happen
  kFitcStPredict,         // Predict(var, phi) at Xp (np x d) with match (np) and want_var, want_cov
  kNumFitcStages
};
// outs[k] (nullable; out_lens[k] entries) in this order, matrices with their padding (n x ldm, m x ldm):
enum FitcStageOut : int {
  kFsKmn = 0, kFsKmm, kFsKs, kFsDKmm, kFsLi, kFsLiT, kFsKinv, kFsV, kFsD, kFsKd, kFsW, kFsWi, kFsWiT, kFsDy, kFsU, kFsWvec,
  kFsYaux, kFsA, kFsAvec, kFsWinv, kFsSums /* 6 */, kFsMean /* np */, kFsVar /* np */, kFsCov /* np x np */, kNumFitcStageOuts
};
void test_fitc_stages(int stage, int n, int m, int d, int cov_type, double var, double phi, double var2, double phi2,
                      const double* X, const double* Z, const double* y, int np, const double* Xp, const int32_t* match,
                      double* const* outs, const int64_t* out_lens, int n_outs);

}  // namespace gpb_amd
