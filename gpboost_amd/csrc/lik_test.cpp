// Test entries of the likelihood layer (GPB_TestLikPoint / GPB_TestLikPath, include/gpboost_amd.h): the four
// functions of lik_device.h point by point, and the per-sample kernels of the grouped, full-scale Vecchia, FITC,
// dense and sparse Vecchia Laplace paths on host arrays, through launchers with the production grids (lik_test.h).
// Every extent and index is checked on the host before any device call; outputs and scratch sit between guard
// bands and start as NaN, so a write out of range or an entry left unwritten is seen without a fault.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "common.h"
#include "grouped_laplace.h"
#include "kernels.h"
#include "laplace_kernels.h"
#include "latent_kernels.h"
#include "lik_test.h"
#include "lowrank_precond.h"

namespace gpb_amd {

namespace {
constexpr size_t kGuard = 64;            // guard doubles on both sides of an output block
constexpr int kMaxN = 1 << 22;
constexpr int kMaxDenseN = 2048;         // dl_dmll_kernel reads two n x n matrices

// a device block of `len` doubles between guard bands, NaN (or `init`) before the launch
struct Guarded {
  DevBuf<double> buf;
  size_t len = 0;
  double* p() const { return buf.get() + kGuard; }
  void make(size_t n, const double* init = nullptr) {
    len = n;
    buf.alloc(n + 2 * kGuard);
    std::vector<double> h(n + 2 * kGuard, std::numeric_limits<double>::quiet_NaN());
    if (init) std::memcpy(h.data() + kGuard, init, sizeof(double) * n);
    HIP_CHECK(hipMemcpy(buf.get(), h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  }
  // copies the payload to out (nullable); returns whether a guard word changed
  bool fetch(double* out) const {
    std::vector<double> h(len + 2 * kGuard);
    HIP_CHECK(hipMemcpy(h.data(), buf.get(), sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    bool touched = false;
    for (size_t k = 0; k < kGuard; ++k)
      if (!std::isnan(h[k]) || !std::isnan(h[kGuard + len + k])) touched = true;
    if (out) std::memcpy(out, h.data() + kGuard, sizeof(double) * len);
    return touched;
  }
};

void upload(DevBuf<double>& dst, const double* src, size_t len) {
  dst.alloc(std::max<size_t>(len, 1));
  if (len) HIP_CHECK(hipMemcpy(dst.get(), src, sizeof(double) * len, hipMemcpyHostToDevice));
}

void upload_int(DevBuf<int>& dst, const int32_t* src, size_t len) {
  dst.alloc(std::max<size_t>(len, 1));
  if (len) HIP_CHECK(hipMemcpy(dst.get(), src, sizeof(int) * len, hipMemcpyHostToDevice));
}

// path_name: null where negative_binomial (grouped random effects only) is available
void check_lik(const char* fn, int lik, double aux, int n, int n_max, const char* path_name = nullptr) {
  if (lik < kLikGaussian || lik > kLikNegBinomial) Fatal("%s: unknown likelihood %d", fn, lik);
  if (lik == kLikNegBinomial && path_name != nullptr)
    Fatal("%s: likelihood %d (negative_binomial) is not available on path %s", fn, lik, path_name);
  if (!(aux > 0.) || !std::isfinite(aux)) Fatal("%s: aux must be finite and > 0", fn);
  if (n < 1 || n >= n_max) Fatal("%s: n = %d is not in 1..%d", fn, n, n_max - 1);
}

// what a (path, kernel) pair takes: vecs (nullable ones flagged), opts, outs (which opt asks for it, -1: always)
struct Shape {
  int n_vecs;
  bool vec_nullable[kLikPathMaxVecs];
  int n_opts;
  int n_outs;
  int out_opt[kLikPathMaxOuts];
  int n_scalars;     // -1: opts[2] (0 or 1)
  bool valid;
};

Shape shape_of(int path, int kernel) {
  const Shape none{0, {}, 0, 0, {}, 0, false};
  switch (path) {
    case kLikPathGrouped:   // opts = {K, want_dW}
      if (kernel == kLikKernelPrep) return {0, {}, 2, 3, {-1, -1, 1}, 1, true};
      if (kernel == kLikKernelTrial) return {0, {}, 2, 0, {}, 1, true};
      return {0, {}, 1, 2, {-1, -1}, 1, true};   // negative_binomial's shape pass: opts = {K}, outs = {dd1a, dWa}
    case kLikPathVif:
      if (kernel == kLikKernelPrep) return {0, {}, 3, 4, {-1, -1, 0, 1}, -1, true};   // opts = {want_dW, want_rhs, want_count}
      if (kernel == kLikKernelTrial) return {1, {false}, 2, 1, {-1}, 1, true};         // vecs = {upd}; opts = {first, cap}
      return none;
    case kLikPathFitc:
      if (kernel == kLikKernelPrep)   // vecs = {dvec, stored W}; opts = {w_update, want_rhs}
        return {2, {false, true}, 2, 5, {-1, -1, -1, -1, 1}, 0, true};
      if (kernel == kLikKernelTrial) return {3, {false, false, false}, 0, 2, {-1, -1}, 2, true};   // vecs = {a, mupd, aupd}
      return {1, {false}, 0, 4, {-1, -1, -1, -1}, 3, true};                                          // vecs = {dvec}
    case kLikPathDense:
      if (kernel == kLikKernelPrep) return {0, {}, 1, 4, {-1, -1, -1, 0}, 0, true};   // opts = {want_rhs}
      if (kernel == kLikKernelTrial) return {3, {false, false, false}, 0, 2, {-1, -1}, 2, true};
      return {0, {}, 2, 2, {-1, 1}, 0, true};                                          // opts = {ld, want_dg}
    default:   // sparse Vecchia: vecs = {Dinv, stored W}; opts = {W_update, want_rhs, want_dw, want_sdw}
      if (kernel == kLikKernelPrep) return {2, {false, true}, 4, 5, {-1, -1, 1, 2, 3}, 0, true};
      return none;
  }
}
}  // namespace

void test_lik_point(int lik, double aux, int n, const double* y, const double* loc, double* ll, double* d1, double* info,
                    double* dinfo, double* dinfo_lowrank, int* guard) {
  const char* fn = "GPB_TestLikPoint";
  check_lik(fn, lik, aux, n, kMaxN);
  if (y == nullptr || loc == nullptr || ll == nullptr || d1 == nullptr || info == nullptr || dinfo == nullptr ||
      dinfo_lowrank == nullptr || guard == nullptr)
    Fatal("%s: an argument is NULL", fn);
  DevBuf<double> dy, dl;
  upload(dy, y, n);
  upload(dl, loc, n);
  Guarded g[5];
  for (Guarded& b : g) b.make(n);
  hipStream_t s = nullptr;
  launch_test_lik_point(n, lik, aux, dy.get(), dl.get(), g[0].p(), g[1].p(), g[2].p(), g[3].p(), s);
  if (lik != kLikNegBinomial) launch_lik_dinfo(n, lik, aux, dy.get(), dl.get(), nullptr, g[4].p(), s);
  HIP_CHECK(hipDeviceSynchronize());
  double* out[5] = {ll, d1, info, dinfo, dinfo_lowrank};
  bool touched = false;
  for (int k = 0; k < 5; ++k) touched = g[k].fetch(out[k]) || touched;
  *guard = touched ? 1 : 0;
}

void test_lik_aux_point(int lik, double aux, int n, const double* y, const double* loc, double* dd1_aux,
                        double* dinfo_aux, double* aux_term, int* guard) {
  const char* fn = "GPB_TestLikAuxPoint";
  check_lik(fn, lik, aux, n, kMaxN);
  if (lik != kLikNegBinomial) Fatal("%s: likelihood %d has no general shape derivatives (5, negative_binomial, has)", fn, lik);
  if (y == nullptr || loc == nullptr || dd1_aux == nullptr || dinfo_aux == nullptr || aux_term == nullptr ||
      guard == nullptr)
    Fatal("%s: an argument is NULL", fn);
  DevBuf<double> dy, dl;
  upload(dy, y, n);
  upload(dl, loc, n);
  Guarded g[3];
  for (Guarded& b : g) b.make(n);
  hipStream_t s = nullptr;
  launch_test_nb_aux_point(n, aux, dy.get(), dl.get(), g[0].p(), g[1].p(), g[2].p(), s);
  HIP_CHECK(hipDeviceSynchronize());
  double* out[3] = {dd1_aux, dinfo_aux, aux_term};
  bool touched = false;
  for (int k = 0; k < 3; ++k) touched = g[k].fetch(out[k]) || touched;
  *guard = touched ? 1 : 0;
}

void test_lik_path(const LikPathTest& t, int* guard) {
  const char* fn = "GPB_TestLikPath";
  // ---- everything that can be refused is refused before the first device call
  if (t.path < 0 || t.path >= kNumLikPaths || t.kernel < 0 || t.kernel >= kNumLikKernels)
    Fatal("%s: unknown path %d / kernel %d", fn, t.path, t.kernel);
  const Shape sh = shape_of(t.path, t.kernel);
  if (!sh.valid) Fatal("%s: path %d has no kernel %d", fn, t.path, t.kernel);
  const bool dmll = t.path == kLikPathDense && t.kernel == kLikKernelFinal;
  static const char* const kPathNames[kNumLikPaths] = {"grouped", "vif", "fitc", "dense", "vecchia"};
  check_lik(fn, t.lik, t.aux, t.n, dmll ? kMaxDenseN + 1 : kMaxN,
            t.path == kLikPathGrouped ? nullptr : kPathNames[t.path]);
  const int n = t.n;
  if (t.y == nullptr || guard == nullptr) Fatal("%s: y or guard_flag is NULL", fn);
  const bool grouped = t.path == kLikPathGrouped, vecchia = t.path == kLikPathVecchia;
  if (grouped && t.kernel == kLikKernelFinal && t.lik != kLikNegBinomial)
    Fatal("%s: path %d has no kernel %d for likelihood %d (the shape pass is negative_binomial's)", fn, t.path, t.kernel,
          t.lik);
  if (grouped ? t.mode != nullptr : t.mode == nullptr)
    Fatal("%s: mode is %s", fn, grouped ? "not NULL (the grouped path takes b and glev)" : "NULL");
  if (t.n_vecs != sh.n_vecs || t.n_opts != sh.n_opts || t.n_outs != sh.n_outs)
    Fatal("%s: path %d, kernel %d takes %d vectors, %d options and %d outputs, not %d, %d and %d", fn, t.path, t.kernel,
          sh.n_vecs, sh.n_opts, sh.n_outs, t.n_vecs, t.n_opts, t.n_outs);
  if ((sh.n_vecs > 0 && t.vecs == nullptr) || (sh.n_opts > 0 && t.opts == nullptr) || (sh.n_outs > 0 && t.outs == nullptr))
    Fatal("%s: vecs, opts or outs is NULL", fn);
  for (int k = 0; k < sh.n_vecs; ++k)
    if (t.vecs[k] == nullptr && !sh.vec_nullable[k]) Fatal("%s: vecs[%d] is NULL", fn, k);
  int opt[kLikPathMaxOpts] = {0};
  for (int k = 0; k < sh.n_opts; ++k) opt[k] = t.opts[k];
  const int flag0 = grouped || dmll ? 1 : 0;   // opts[0] is K / ld there, a flag elsewhere
  for (int k = flag0; k < sh.n_opts; ++k)
    if (opt[k] != 0 && opt[k] != 1) Fatal("%s: opts[%d] = %d is not 0 or 1", fn, k, opt[k]);
  for (int k = 0; k < sh.n_outs; ++k) {
    const bool want = sh.out_opt[k] < 0 || opt[sh.out_opt[k]] != 0;
    if (want != (t.outs[k] != nullptr))
      Fatal("%s: outs[%d] is %s", fn, k, want ? "NULL" : "given although its option is off");
  }
  const int n_scalars = sh.n_scalars < 0 ? opt[2] : sh.n_scalars;
  if (t.n_scalars != n_scalars || (n_scalars > 0 && t.scalars == nullptr))
    Fatal("%s: path %d, kernel %d writes %d scalars, not %d", fn, t.path, t.kernel, n_scalars, t.n_scalars);
  if (!std::isfinite(t.lam) || t.lam <= 0. || t.lam > 1.) Fatal("%s: lam is not in (0, 1]", fn);
  if (!grouped && !vecchia && (t.idx != nullptr || t.arr0 != nullptr || t.arr1 != nullptr || t.idx_len != 0 || t.arr_len != 0))
    Fatal("%s: path %d takes no idx / arr0 / arr1", fn, t.path);
  if (!dmll && (t.mats != nullptr || t.mats_len != 0)) Fatal("%s: only the dense dmll kernel takes mats", fn);
  int K = 0, ld = 0;
  bool has_obs = false;
  if (grouped) {
    K = opt[0];
    if (K < 1 || K > kGlpMaxK) Fatal("%s: K = %d is not in 1..%d", fn, K, kGlpMaxK);
    if (t.idx == nullptr || t.arr0 == nullptr || t.arr1 != nullptr) Fatal("%s: the grouped path takes glev and b (arr1 NULL)", fn);
    if (t.idx_len != (int64_t)K * n || t.arr_len < 1 || t.arr_len > kMaxN)
      Fatal("%s: glev holds %lld entries (K n = %lld), b %lld", fn, (long long)t.idx_len, (long long)K * n,
            (long long)t.arr_len);
    for (int64_t k = 0; k < t.idx_len; ++k)
      if (t.idx[k] < 0 || t.idx[k] >= t.arr_len)
        Fatal("%s: glev[%lld] = %d is not in 0..%lld", fn, (long long)k, t.idx[k], (long long)t.arr_len - 1);
  }
  if (vecchia) {
    has_obs = t.idx != nullptr;
    if (!has_obs && (t.arr0 != nullptr || t.arr1 != nullptr || t.idx_len != 0 || t.arr_len != 0))
      Fatal("%s: observation arrays without the ObsMap pointer", fn);
    if (has_obs) {
      if (t.idx_len != (int64_t)n + 1 || t.arr0 == nullptr || t.arr_len < 0 || t.arr_len > kMaxN)
        Fatal("%s: ObsMap ptr holds %lld entries (n + 1 = %d), %lld observations", fn, (long long)t.idx_len, n + 1,
              (long long)t.arr_len);
      if (t.idx[0] != 0 || t.idx[n] != t.arr_len) Fatal("%s: ObsMap ptr does not run from 0 to the observation count", fn);
      for (int i = 0; i < n; ++i)
        if (t.idx[i + 1] < t.idx[i]) Fatal("%s: ObsMap ptr decreases at row %d", fn, i);
    }
    if (opt[0] == 0 && t.vecs[1] == nullptr) Fatal("%s: W_update = 0 needs the stored W (vecs[1])", fn);
    if (opt[3] && !opt[2]) Fatal("%s: sdw is written only with dw", fn);
  }
  if (t.path == kLikPathFitc && t.kernel == kLikKernelPrep && opt[0] == 0 && t.vecs[1] == nullptr)
    Fatal("%s: w_update = 0 needs the stored W (vecs[1])", fn);
  if (dmll) {
    ld = opt[0];
    if (ld < n || ld > 2 * kMaxDenseN) Fatal("%s: ld = %d, n = %d", fn, ld, n);
    if (t.mats == nullptr || t.mats_len != 2 * (int64_t)ld * n)
      Fatal("%s: mats holds %lld entries, C and S take 2 ld n = %lld", fn, (long long)t.mats_len, 2 * (long long)ld * n);
  }

  // ---- device blocks
  DevBuf<double> dy, dmode, doff, dv[kLikPathMaxVecs], darr0, darr1, dmats;
  DevBuf<int> didx;
  upload(dy, t.y, n);
  if (t.mode) upload(dmode, t.mode, n);
  if (t.offset) upload(doff, t.offset, n);
  for (int k = 0; k < sh.n_vecs; ++k)
    if (t.vecs[k]) upload(dv[k], t.vecs[k], n);
  if (t.idx) upload_int(didx, t.idx, (size_t)t.idx_len);
  if (t.arr0) upload(darr0, t.arr0, (size_t)t.arr_len);
  if (t.arr1) upload(darr1, t.arr1, (size_t)t.arr_len);
  if (t.mats) upload(dmats, t.mats, (size_t)t.mats_len);
  const double* off = t.offset ? doff.get() : nullptr;
  Guarded go[kLikPathMaxOuts], gpart, gsum;
  double* o[kLikPathMaxOuts] = {nullptr};
  for (int k = 0; k < sh.n_outs; ++k)
    if (t.outs[k]) {
      go[k].make(n);
      o[k] = go[k].p();
    }
  gsum.make(kLikPathMaxScalars);
  hipStream_t s = nullptr;
  switch (t.path) {
    case kLikPathGrouped:
      gpart.make(test_glp_blocks(n));
      if (t.kernel == kLikKernelFinal) {
        test_glp_nb_aux(n, K, didx.get(), dy.get(), off, darr0.get(), t.aux, o[0], o[1], gpart.p(), gsum.p(), s);
        break;
      }
      test_glp_obs(n, K, didx.get(), dy.get(), off, darr0.get(), t.lik, t.aux, t.kernel == kLikKernelPrep, o[0], o[1], o[2],
                   gpart.p(), gsum.p(), s);
      break;
    case kLikPathVif:
      if (t.kernel == kLikKernelPrep) {
        if (opt[2]) {
          gpart.make(test_vl_blocks(n));
            }
        test_vl_prep(n, t.lik, t.aux, dy.get(), off, dmode.get(), o[0], o[1], o[2], o[3], opt[2] ? gpart.p() : nullptr,
                     gsum.p(), s);
      } else {
        gpart.make(test_vl_blocks(n));
          test_vl_trial(n, t.lik, t.aux, dy.get(), off, dmode.get(), dv[0].get(), t.lam, opt[0], opt[1], o[0], gpart.p(),
                      gsum.p(), s);
      }
      break;
    case kLikPathFitc:
      if (t.kernel == kLikKernelPrep) {
        // the stored W is what the kernel reads with w_update = 0 and must leave as it is
        if (t.vecs[1]) {
          go[1].make(n, t.vecs[1]);
          o[1] = go[1].p();
        }
        test_fl_prep(n, t.lik, t.aux, dy.get(), off, dmode.get(), dv[0].get(), opt[0], o[0], o[1], o[2], o[3], o[4], s);
      } else if (t.kernel == kLikKernelTrial) {
        gpart.make((size_t)2 * laplace_blocks(n));
        test_laplace_trial(n, t.lik, t.aux, t.lam, dmode.get(), dv[0].get(), dv[1].get(), dv[2].get(), dy.get(), off, o[0], o[1],
                      gpart.p(), gsum.p(), s);
      } else {
        gpart.make((size_t)3 * laplace_blocks(n));
        test_fl_final(n, t.lik, t.aux, dy.get(), off, dmode.get(), dv[0].get(), o[0], o[1], o[2], o[3], gpart.p(), gsum.p(),
                      s);
      }
      break;
    case kLikPathDense:
      if (t.kernel == kLikKernelPrep) {
        test_dl_prep(n, t.lik, t.aux, dy.get(), off, dmode.get(), o[0], o[1], o[2], o[3], s);
      } else if (t.kernel == kLikKernelTrial) {
        gpart.make((size_t)2 * laplace_blocks(n));
        test_laplace_trial(n, t.lik, t.aux, t.lam, dmode.get(), dv[0].get(), dv[1].get(), dv[2].get(), dy.get(), off, o[0], o[1],
                      gpart.p(), gsum.p(), s);
      } else {
        test_dl_dmll(dmats.get(), dmats.get() + (size_t)ld * n, n, ld, t.lik, t.aux, dy.get(), off, dmode.get(), o[0], o[1],
                     s);
      }
      break;
    default: {
      if (t.vecs[1]) {
        go[1].make(n, t.vecs[1]);
        o[1] = go[1].p();
      }
      NewtonPrepArgs a{};
      a.n = n; a.lik = t.lik; a.aux = t.aux;
      a.y = dy.get(); a.loc = dmode.get(); a.offset = off; a.mode = dmode.get(); a.Dinv = dv[0].get();
      a.d1 = o[0]; a.W = o[1]; a.W_update = opt[0];
      a.rhs = o[2]; a.dw = o[3]; a.sdw = o[4];
      if (has_obs) {
        a.obs.ptr = didx.get();
        a.obs.y = darr0.get();
        a.obs.offset = t.arr1 ? darr1.get() : nullptr;
      }
      launch_newton_prep(a, s);
    }
  }
  HIP_CHECK(hipDeviceSynchronize());
  bool touched = false;
  for (int k = 0; k < sh.n_outs; ++k)
    if (go[k].len) touched = go[k].fetch(t.outs[k]) || touched;
  if (gpart.len) touched = gpart.fetch(nullptr) || touched;
  double sc[kLikPathMaxScalars];
  touched = gsum.fetch(sc) || touched;
  for (int k = 0; k < kLikPathMaxScalars; ++k) {
    if (k < n_scalars) t.scalars[k] = sc[k];
    else if (!std::isnan(sc[k])) touched = true;   // a scalar nobody asked for was written
  }
  *guard = touched ? 1 : 0;
}

}  // namespace gpb_amd
