// Linear regression covariates (GLS, re_model_template.h:9125-9132) and training-data random-effect
// predictions (PredictTrainingDataRandomEffects) for the Gaussian likelihood: device launchers
// (covariate_kernels.hip) and host helpers (covariates.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "common.h"

namespace gpb_amd {

constexpr int kCovMaxCols = 32;   // covariates + the response column

// Blocks used by launch_vecchia_gram (its `partial` needs blocks * c (c + 1) / 2 doubles).
int vecchia_gram_blocks(int n);
// out[pair(a, b), a <= b, row-major upper triangle] = sum_i D^-1_i (B Z)_ia (B Z)_ib for the n x c
// row-major matrix Z (Vecchia order); B, D^-1 from the row kernel's factor mode.
void launch_vecchia_gram(int n, int m, int c, const int* nbr, const double* B, const double* Dinv, const double* Z,
                         double* partial, double* out, hipStream_t s);
// yaux = B^T D^-1 B y (= Psi^-1 y) and diag = diag(B^T D^-1 B); u: n scratch. tptr / trow / tslot:
// the transposed neighbour lists (rows ascending).
void launch_vecchia_psi_inv_diag(int n, int m, const int* nbr, const int* tptr, const int* trow, const int* tslot,
                                 const double* B, const double* Dinv, const double* y, double* u, double* yaux,
                                 double* diag, hipStream_t s);

// ---- Woodbury-form covariances (gp_approx = "fitc", "full_scale_vecchia"; lowrank_gram.hip)
// Row ranges (one partial each) that launch_weighted_tall_skinny splits n points into.
int weighted_tall_skinny_ranges(int n);
// One pass over the n points: T = A diag(w) U (m x c, column-major, leading dimension ldm; rows m..ldm-1
// zero) and G0 = U^T diag(w) U (packed upper triangle, as launch_vecchia_gram returns it).
// A: m x n column-major with leading dimension ldm (point i's m entries contiguous); w: n weights;
// U: n x c row-major, c <= kCovMaxCols. Tpart: ranges * c * ldm doubles, Gpart: ranges * c * c doubles of
// scratch (one partial per range, summed in a fixed order: equal inputs give equal bits).
void launch_weighted_tall_skinny(int m, int n, int c, const double* A, int ldm, const double* w, const double* U,
                                 double* Tpart, double* Gpart, double* T, double* G0, hipStream_t s);
// U = B Z for the n x c row-major Z: U_i = Z_i + sum_r Bv[i nn + r] Z[nbr[i nn + r]] over row i's min(i, nn)
// neighbours (B unit lower triangular, its off-diagonal values in Bv).
void launch_vecchia_bz(int n, int nn, int c, const int* nbr, const double* Bv, const double* Z, double* U,
                       hipStream_t s);

// Device scratch of lowrank_gram (allocated on first use, kept by the solver)
struct LowrankGramWork {
  DevBuf<double> w, Tpart, Gpart, T, S, G0;
};
// Z^T Psi^-1 Z (host, c x c row-major) of a low-rank-plus-residual covariance by the Woodbury identity:
//   G = U^T diag(1 / dvec) U - S^T S,  S = Li (A diag(1 / dvec) U),
// Li (m x m lower, leading dimension ldm) the inverse Cholesky factor of the Woodbury matrix. FITC: A = K_mn,
// dvec = d, U = Z; full-scale Vecchia: A = B K_nm, dvec = D, U = B Z. The c x c subtraction runs on the
// host in a fixed order.
void lowrank_gram(hipStream_t s, int m, int n, int c, int ldm, const double* A, const double* dvec, const double* U,
                  const double* Li, LowrankGramWork& ws, double* G_host);

// Test entry (GPB_TestWeightedTallSkinny): host arrays in and out, the default stream, synchronised. A: a_len =
// round_up(m, 64) * n doubles; T_out: m x c row-major; G0_out: c x c row-major (both triangles).
void test_weighted_tall_skinny(int m, int n, int c, const double* A, long a_len, const double* w, const double* U,
                               double* T_out, double* G0_out);

// Host: unpack the packed upper triangle of a c x c Gram matrix into a full row-major matrix.
std::vector<double> unpack_gram(const double* packed, int c);
// Host: beta = G_XX^-1 G_Xy by Cholesky (Eigen's llt().solve, re_model_template.h:9131), where
// G is the full (p + 1) x (p + 1) Gram of [X | y]. Fails on a non-positive-definite G_XX.
std::vector<double> gls_coef(const std::vector<double>& G, int p);
// Host: sqrt(diag((G_XX / sigma2)^-1)) (CalcStdDevCoef, re_model_template.h:9797-9814).
std::vector<double> gls_coef_std_dev(const std::vector<double>& G, int p, double sigma2);

}  // namespace gpb_amd
