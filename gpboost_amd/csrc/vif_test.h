// Test entries of the full-scale Vecchia row factor, sparse products and vector kernels (GPB_TestVif*,
// include/gpboost_amd.h; vif_test.cpp). Host arrays in and out; every extent and index is checked on the host
// before any device call; the kernels run through the launch functions of vif.h, the ones VifSolver uses.
#pragma once

#include <cstdint>

namespace gpb_amd {

// op of GPB_TestVifApply
enum VifApplyOp : int { kVifBRow = 0, kVifBCol = 1, kVifBVec = 2, kVifBtVec = 3, kNumVifApplyOps };
// op of GPB_TestVifVector
enum VifVecOp : int {
  kVifGemv = 0,     // arrays = M (n x m), x (n); out (m)
  kVifColDotW,      // arrays = M (n x m), w (m); out (n)
  kVifColDotM,      // arrays = M, M2 (n x m); out (n)
  kVifZvec,         // arrays = dD, u, e, D (n each); out (n)
  kVifSum,          // arrays = a_0, b_0, c_0, a_1, ... (n each, b / c nullable), sum_ops (nt); out (nt)
  kVifDkmn,         // arrays = X (n x d), Z (m x d); out (n x ldm)
  kNumVifVecOps
};

struct VifRowsTest {
  int n_total, d, i0, nn, m;
  const double* X;
  const int32_t* nbr;
  const double* V;
  const double* P0;
  const double* P1;
  int cov_type;
  double var, phi, nugget, cjit;
  int grad, form, order;
  double pad_fill;
  double* D;
  double* Bv;
  double* dD0;
  double* dD1;
  double* dBv0;
  double* dBv1;
};
// lengths: x_len = n_total d, nbr_len = rows nn, mat_len = n_total m, rows_len = rows = n_total - i0
void test_vif_rows(const VifRowsTest& t, int64_t x_len, int64_t nbr_len, int64_t mat_len, int64_t rows_len,
                   int* guard);

void test_vif_apply(int op, int n, int nn, int m, const int32_t* nbr, int64_t nbr_len, const double* coef,
                    int64_t coef_len, const double* D, const double* in, int64_t in_len, double self, int div,
                    int want_div, const double* X, int d, int order, double pad_fill, double* out, double* out2,
                    int64_t out_len, int* guard);

void test_vif_vector(int op, int n, int m, int d, int cov_type, double var, double phi, double pad_fill,
                     const double* const* arrays, const int64_t* lens, int n_arrays, const int32_t* sum_ops, int nt,
                     double* out, int64_t out_len, int* guard);

}  // namespace gpb_amd
