// Test entries of the latent-Vecchia operator layer (GPB_TestLatentOps*, include/gpboost_amd.h; latent_test.cpp).
#pragma once

#include <cstdint>
#include <memory>

#include "latent.h"

namespace gpb_amd {

// op of GPB_TestLatentOpsApply
enum LatentTestOp : int { kLatentOpB = 0, kLatentOpBt = 1, kLatentOpA = 2, kLatentOpPrecond = 3 };
// form of op 0 (launch_b_apply); 0 = the production dispatch
enum LatentBForm : int {
  kBFormEll = 1,       // t = 1: b_apply1e (ELL, the default)
  kBFormGroups,        // t = 1: b_apply1m (m <= 32)
  kBFormOld,           // t = 1: b_apply1 (one row per 32-lane group)
  kBFormWave16,        // t >= 2: b_apply_wave<16> (m <= 64, the default)
  kBFormWave32,        // t >= 2: b_apply_wave<32>
  kBFormCh0,           // t >= 2: b_apply_kernel<0, false>
  kBFormCh16,          //         <16, false>
  kBFormCh0Pers,       //         <0, true>, grid capped at 8 blocks
  kBFormCh16Pers,      //         <16, true>
  kBFormTiled,         // t >= 2, unit = 1: apply_tile_kernel<false>
  kNumBForms
};
// form of op 1 (launch_bt_apply); 0 = the production dispatch
enum LatentBtForm : int {
  kBtFormPaired = 1,   // t = 1: bt_apply1p (the default)
  kBtFormE2,           // t = 1: bt_apply1sE<2, 4>
  kBtFormE4,           //        bt_apply1sE<4, 2>
  kBtFormS2,           //        bt_apply1s2
  kBtFormShfl,         //        bt_apply1s<false>
  kBtFormE1,           //        bt_apply1s<true>
  kBtFormGroups,       //        bt_apply1m + long-row waves
  kBtFormOld,          //        bt_apply1
  kBtFormWave16,       // t >= 2: bt_apply_wave<16> (the default)
  kBtFormWave32,
  kBtFormCh0,          // t >= 2: bt_apply_kernel<0, false> (use_alt_vals: the tslot gather form)
  kBtFormCh16,
  kBtFormCh0Pers,
  kBtFormCh16Pers,
  kBtFormTiled,        // t >= 2, unit = 1, no pre: apply_tile_kernel<true>
  kNumBtForms
};

// op of GPB_TestLatentOpsVector
enum LatentVecOp : int {
  kVecColdots = 0,   // out[q t + c] = sum_i A_q[i, c] B_q[i, c], q < np; blocks = A_0, B_0, A_1, B_1, ...
  kVecCgUpdate,      // U += a .* H, R -= a .* V, rr[c] = sum_i R[i, c]^2; blocks = H, V, U, R; sv0 = a
  kVecHUpdate,       // H = Z + b .* H; blocks = Z, H; sv0 = b
  kVecAlpha,         // a = rz / hv (0 where act = 0); sv0 = rz, sv1 = hv; small_out = a, hist
  kVecBeta,          // b = rz_new / rz, rz = rz_new (b = 0, rz kept where act = 0); sv0 = rz_new, sv1 = rz; small_out = b, hist, rz
  kVecAxpby,         // Z = alpha X + beta Y; blocks = X, Y
  kVecCapMode,       // the Newton step's change capped at log(100) per entry; blocks = mode, mnew
  kVecPack,          // dst[i, ib + c] = src[i, ia + c], c < np; blocks = src, dst
  kNumVecOps
};
void test_latent_vector(int op, int n, int t, int np, int ia, int ib, double alpha, double beta,
                        const double* const* blocks, const double* sv0, const double* sv1, const int* act,
                        double* out0, double* out1, double* small_out, int* guard);

// n >= 1, 1 <= m, d >= 1, nbr_len = n m, x_len = n d, 0 <= nbr[i m + r] < i and distinct for r < min(i, m)
void test_latent_check_graph(const char* fn, int n, int m, const int* nbr, int64_t nbr_len, int d, const double* X,
                             int64_t x_len);
// opts (nullable, 9 entries): {relabel, dense_rows, head_rows, tail_merge, seg_form, tail_order, tail_form, tail_w,
// no_graph}, an entry < 0 = the environment's / the default
LatentOptions test_latent_options(const char* fn, const int64_t* opts, int n);

// A LatentVecchia on a stream of its own with its own device copy of the coordinates.
class TestLatentOps {
 public:
  TestLatentOps(int n, int m, const int* nbr, int d, const double* X, const LatentOptions& opt);
  ~TestLatentOps();
  LatentVecchia& lv() { return *lv_; }
  int n() const { return n_; }
  int m() const { return m_; }

 private:
  int n_, m_;
  hipStream_t s_ = nullptr;
  DevBuf<double> X_;
  std::unique_ptr<LatentVecchia> lv_;
};

}  // namespace gpb_amd
