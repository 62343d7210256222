// Test entries of the Laplace likelihood functions (lik_device.h) and of the per-sample kernels that call them
// (GPB_TestLikPoint / GPB_TestLikPath, include/gpboost_amd.h; lik_test.cpp). Host arrays in and out; every extent
// and index is checked on the host before any device call. The production kernels sit in anonymous namespaces, so
// each .hip file ends in small test_* launchers (below) with exactly the grid and block arithmetic of its
// production caller; no kernel body is copied. The fitc and dense paths share one trial kernel and one launcher.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gpb_amd {

// path / kernel of GPB_TestLikPath
enum LikPath : int { kLikPathGrouped = 0, kLikPathVif, kLikPathFitc, kLikPathDense, kLikPathVecchia, kNumLikPaths };
enum LikKernel : int {
  kLikKernelPrep = 0,   // grouped: glp_obs_kernel<true>; vif / fitc / dense: *_prep_kernel; vecchia: newton_prep_kernel
  kLikKernelTrial,      // grouped: glp_obs_kernel<false>; vif: vl_trial_kernel; fitc / dense: laplace_trial_kernel
  kLikKernelFinal,      // fitc: fl_final_kernel; dense: dl_dmll_kernel; grouped (lik 5 only): glp_nb_aux_kernel
  kNumLikKernels
};
constexpr int kLikPathMaxVecs = 4, kLikPathMaxOuts = 5, kLikPathMaxOpts = 4, kLikPathMaxScalars = 3;

struct LikPathTest {
  int path, kernel, n, lik;
  double aux;
  const double* y;
  const double* mode;
  const double* offset;
  const double* const* vecs;
  int n_vecs;
  const int32_t* idx;
  int64_t idx_len;
  const double* arr0;
  const double* arr1;
  int64_t arr_len;
  const double* mats;
  int64_t mats_len;
  double lam;
  const int32_t* opts;
  int n_opts;
  double* const* outs;
  int n_outs;
  double* scalars;
  int n_scalars;
};

// the point kernel of lik_test_kernels.hip: the four device functions and nothing else
void launch_test_lik_point(int n, int lik, double aux, const double* y, const double* loc, double* ll, double* d1,
                           double* info, double* dinfo, hipStream_t s);

// negative_binomial (lik 5): the three shape functions nb_dd1_aux, nb_dinfo_aux and nb_aux_term
void launch_test_nb_aux_point(int n, double aux, const double* y, const double* loc, double* dd1a, double* dinfoa,
                              double* term, hipStream_t s);

// lik 5: dinfo_lowrank stays NaN (the low-rank preconditioner belongs to the GP drivers, which do not have it)
void test_lik_point(int lik, double aux, int n, const double* y, const double* loc, double* ll, double* d1, double* info,
                    double* dinfo, double* dinfo_lowrank, int* guard);
// GPB_TestLikAuxPoint: the derivatives of d1 and of the information wrt the log of the auxiliary parameter and the
// per-observation term of the explicit shape gradient; likelihoods with the general shape gradient only (lik 5)
void test_lik_aux_point(int lik, double aux, int n, const double* y, const double* loc, double* dd1_aux,
                        double* dinfo_aux, double* aux_term, int* guard);
void test_lik_path(const LikPathTest& t, int* guard);

// ---- launchers at the end of the production files (device pointers)
// grouped_laplace.hip: glp_obs_kernel<deriv> on the constructor's nb_ blocks, then glp_finish_kernel -> *ll.
// partial: test_glp_blocks(n) doubles
int test_glp_blocks(int n);
void test_glp_obs(int n, int K, const int* glev, const double* y, const double* F, const double* b, int lik, double aux,
                  bool deriv, double* d1, double* W, double* dW, double* partial, double* ll, hipStream_t s);
// glp_nb_aux_kernel on the same blocks, then glp_finish_kernel -> *sum
void test_glp_nb_aux(int n, int K, const int* glev, const double* y, const double* F, const double* b, double aux,
                     double* dd1a, double* dWa, double* partial, double* sum, hipStream_t s);
// vif_laplace.hip: part (nullable for prep) holds test_vl_blocks(n) doubles; the partials are summed into *sum
int test_vl_blocks(int n);
void test_vl_prep(int n, int lik, double aux, const double* y, const double* off, const double* mode, double* d1,
                  double* W, double* dW, double* rhs, double* part, double* sum, hipStream_t s);
void test_vl_trial(int n, int lik, double aux, const double* y, const double* off, const double* mode, const double* upd,
                   double lam, int first, int cap, double* trial, double* part, double* sum, hipStream_t s);
// laplace_kernels.hip: the trial of the fitc and dense paths; part holds 2 laplace_blocks(n) doubles, sums: 2
void test_laplace_trial(int n, int lik, double aux, double lam, const double* mode, const double* a, const double* mupd,
                        const double* aupd, const double* y, const double* off, double* mnew, double* anew, double* part,
                        double* sums, hipStream_t s);
// fitc_laplace.hip: part holds 3 laplace_blocks(n) doubles; sums: 3 doubles
void test_fl_prep(int n, int lik, double aux, const double* y, const double* off, const double* mode, const double* dvec,
                  int w_update, double* d1, double* w, double* wdw, double* DW, double* rhs, hipStream_t s);
void test_fl_final(int n, int lik, double aux, const double* y, const double* off, const double* mode, const double* dvec,
                   double* d1, double* w, double* DW, double* dpwi, double* part, double* sums, hipStream_t s);
// dense_laplace.hip: C, S: n x n column-major with leading dimension ld
void test_dl_prep(int n, int lik, double aux, const double* y, const double* off, const double* mode, double* d1,
                  double* w, double* ws, double* rhs, hipStream_t s);
void test_dl_dmll(const double* C, const double* S, int n, int ld, int lik, double aux, const double* y, const double* off,
                  const double* mode, double* dmll, double* dg, hipStream_t s);

}  // namespace gpb_amd
