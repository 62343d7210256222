// Test entries of the grouped random-effects engine (GPB_TestGrouped*, include/gpboost_amd.h; grouped_test.cpp):
// the launchers of grouped_kernels.hip, GroupedRE::Precond / SolveVec and the segmented sums and per-observation
// gradient kernels of grouped_laplace.hip, on host arrays. Every extent and index is checked on the host before
// any device call; the kernels run through the production launch functions (the kernels of grouped_laplace.hip
// sit in an anonymous namespace, so that file ends in test_glp_* launchers with the grid arithmetic of Eval).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "grouped.h"
#include "grouped_laplace.h"

namespace gpb_amd {

// op of GPB_TestGroupedApply
enum GroupedApplyOp : int {
  kGreApply = 0,     // Out0 = (diag(dg) + offdiag) In
  kGreApplyLower,    // Out0 = (diag(dg) + lower offdiag) In
  kGreLdsMult,       // Out0 = (L D^-1/2) In
  kGreSsor,          // Out0 = X = (L D^-1/2)^-1 In, Out1 = Z = (L D^-1/2)^-T X
  kGreUpper,         // Out0 = D^-1 (upper triangle incl. the diagonal) In
  kGrePrecond,       // GroupedRE::Precond after SetOperator: Out0 = its scratch X, Out1 = Z
  kNumGroupedApplyOps
};
// op of GPB_TestGroupedSmall
enum GroupedSmallOp : int { kGreZty = 0, kGreDiag, kGreSingle, kGreResidual, kNumGroupedSmallOps };
// op of GPB_TestGroupedDense
enum GroupedDenseOp : int { kGreDenseBuild = 0, kGreInvDiag, kGrePredE, kGrePredVar, kGreFisherCols, kNumGroupedDenseOps };
// op of GPB_TestGroupedLaplaceOps
enum GroupedLaplaceOp : int { kGlpAssemble = 0, kGlpQ, kGlpRowTrace, kGlpGradF, kGlpVec, kGlpEffectDots, kNumGroupedLaplaceOps };

constexpr int kGroupedInfoStats = 14;
constexpr int kGroupedMaxArrays = 8;

struct GroupedTestAccess;   // friend of GroupedRE and GroupedLaplace

// the handle of GPB_TestGroupedCreate: a GroupedRE on a stream of its own and, on first use, a GroupedLaplace on it
struct GroupedTest {
  // weights (nullable): K x n values of Z, has_weight (K): 0 = effect k has none (all ones, a null array to the
  // engine). With weights every op runs the weighted kernels; the prediction ops take wt (np K) as one more input.
  GroupedTest(int n, int K, const int32_t* levels, const double* weights = nullptr, const int32_t* has_weight = nullptr);
  ~GroupedTest();
  GroupedTest(const GroupedTest&) = delete;
  GroupedTest& operator=(const GroupedTest&) = delete;

  // stats, ints and dbls as GPB_TestGroupedInfo documents them; ints / dbls nullable together
  void Info(int t, int64_t* stats, int64_t stats_len, int32_t* ints, int64_t ints_len, double* dbls, int64_t dbls_len);
  void Apply(int op, int t, const double* val, const double* dg, const double* dis, const double* In, double* Out0,
             double* Out1, int64_t block_len, int* guard);
  void Small(int op, const double* const* in, const int64_t* in_len, int n_in, double* const* out,
             const int64_t* out_len, int n_out, int* guard);
  void Dense(int op, int ld, int np, const int32_t* idx, const double* const* in, const int64_t* in_len, int n_in,
             double* const* out, const int64_t* out_len, int n_out, int* guard);
  void Solve(const double* val, const double* cnt, const double* D, const double* dis, const double* rhs, int warm,
             const double* u0, int pmax, double delta, double* u, int* its, int* guard);
  void LaplaceOps(int op, int sub, int t, int ld, double alpha, const double* const* in, const int64_t* in_len, int n_in,
                  double* const* out, const int64_t* out_len, int n_out, int* guard);

 private:
  GroupedLaplace& Laplace();
  int n_, K_;
  std::vector<std::vector<int>> levels_;
  std::vector<std::vector<double>> weights_;
  std::vector<const double*> wptr_;   // empty: unweighted
  hipStream_t s_ = nullptr;
  std::unique_ptr<GroupedRE> re_;
  std::unique_ptr<GroupedLaplace> glp_;
};

// ---- launchers at the end of grouped_laplace.hip (device pointers)
// glp_q_kernel<aux> on the constructor's block count, then glp_finish_kernel as Eval runs it: out[0 .. K) = the
// sums of W_i q_ij, (aux) out[K] = the sum of Wa_i q_i. partial: (K + 1) test_glp_blocks(n) doubles
// zw: the K x n table of Z's values (null: the unweighted instantiation)
void test_glp_q(int n, int K, const int* glev, const double* zw, const double* Ainv, int ld, const double* D,
                const double* W, const double* dW, const double* Wa, bool aux, double* dwq, double* partial, double* out,
                hipStream_t s);
void test_glp_row_trace(int n, int K, int t, const int* glev, const double* zw, const double* U, const double* V,
                        const double* dW, double* dwq, hipStream_t s);
void test_glp_grad_f(int n, int K, const int* glev, const double* zw, const double* d1, const double* dwq,
                     const double* W, const double* v, double* out, hipStream_t s);
// form: VecOp of grouped_laplace.hip (0 sigi + x, 1 x - sigi y, 2 x / y, 3 x + alpha y, 4 sqrt(1 / x)); sigma2: host, K
void test_glp_vec(int form, const GroupedRE::View& v, const double* sigma2, double alpha, const double* x,
                  const double* y, double* out, hipStream_t s);
// mode 0: sum x y, 1: sum log x, 2: sum 1 / x, 3: sum x / y, per effect
void test_glp_effect_dots(int mode, const GroupedRE::View& v, const double* sigma2, const double* x, const double* y,
                          double* out, hipStream_t s);

struct GroupedTestAccess {
  // GroupedLaplace (defined in grouped_laplace.hip)
  static void Assemble(GroupedLaplace& g, const double* w, double* out, bool diag_only);
  static const int* Glev(const GroupedLaplace& g);
  static const double* Zw(const GroupedLaplace& g);   // null without weights
  static void SegCounts(const GroupedLaplace& g, int out[4]);   // long levels, their chunks, all long, all chunks
  // GroupedRE (defined in grouped_test.cpp)
  static GroupedOp Op(GroupedRE& re, int t);
  static void PlanQ(GroupedRE& re, int tc, std::vector<int>& lower_q, std::vector<int>& upper_q);
  static void Precond(GroupedRE& re, const double* R, double* Z, double* S, int t);
  static const std::vector<int>& Cum(const GroupedRE& re);
  static const int* ObsPtr(const GroupedRE& re);
  static const int* Obs(const GroupedRE& re);
  static const double* ObsW(const GroupedRE& re);   // null without weights
  static const int* DevCum(const GroupedRE& re);
  static const int* Split(const GroupedRE& re);
  static const double* Val(const GroupedRE& re);
  static const double* Cnt(const GroupedRE& re);
};

}  // namespace gpb_amd
