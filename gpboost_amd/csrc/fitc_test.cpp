// Test entries of the FITC kernels (GPB_TestFitc*, include/gpboost_amd.h): every column, m x m and k-means kernel of
// fitc_kernels.hip and fitc_fisher.hip on host arrays through the launch functions of fitc.h (the ones FitcSolver
// and fitc_inducing_points call). Every extent and index is checked on the host before any device call; outputs
// and scratch sit between guard bands and start as NaN (integers: a negative fill), so a write out of range or an
// entry left unwritten is seen without a fault; the ld-m padding of every input column holds the caller's fill value.
// GPB_TestFitcStages builds a FitcSolver, runs one stage and copies its buffers out (FitcTestAccess, a friend).
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "common.h"
#include "fitc.h"
#include "fitc_test.h"
#include "kernels.h"

namespace gpb_amd {

namespace {
constexpr size_t kGuard = 64;   // guard words on both sides of an output block
constexpr int kMaxM = 4096;
constexpr int kMaxN = 1 << 22;
constexpr int32_t kIntFill = -0x5a5a5a5b;

int round_ldm(int m) { return (m + 63) / 64 * 64; }

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

struct GuardedInt {
  DevBuf<int> buf;
  size_t len = 0;
  int* p() const { return buf.get() + kGuard; }
  void make(size_t n) {
    len = n;
    buf.alloc(n + 2 * kGuard);
    std::vector<int> h(n + 2 * kGuard, kIntFill);
    HIP_CHECK(hipMemcpy(buf.get(), h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice));
  }
  bool fetch(int32_t* out) const {
    std::vector<int> h(len + 2 * kGuard);
    HIP_CHECK(hipMemcpy(h.data(), buf.get(), sizeof(int) * h.size(), hipMemcpyDeviceToHost));
    bool touched = false;
    for (size_t k = 0; k < kGuard; ++k)
      if (h[k] != kIntFill || h[kGuard + len + k] != kIntFill) touched = true;
    if (out) std::memcpy(out, h.data() + kGuard, sizeof(int) * len);
    return touched;
  }
};

// `rows` host rows of m doubles -> a padded host image, row r at r ldm, everything else the fill
std::vector<double> padded(const double* src, size_t rows, int m, int ldm, double fill, size_t total) {
  std::vector<double> h(total, fill);
  for (size_t r = 0; r < rows; ++r) std::memcpy(&h[r * ldm], src + r * m, sizeof(double) * m);
  return h;
}

void upload_vec(DevBuf<double>& dst, const std::vector<double>& h) {
  dst.alloc(std::max<size_t>(h.size(), 1));
  if (!h.empty()) HIP_CHECK(hipMemcpy(dst.get(), h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
}

void upload_padded(DevBuf<double>& dst, const double* src, size_t rows, int m, int ldm, double fill) {
  upload_vec(dst, padded(src, rows, m, ldm, fill, rows * ldm));
}

void upload(DevBuf<double>& dst, const double* src, size_t len) {
  dst.alloc(std::max<size_t>(len, 1));
  if (len) HIP_CHECK(hipMemcpy(dst.get(), src, sizeof(double) * len, hipMemcpyHostToDevice));
}

void upload_int(DevBuf<int>& dst, const int* src, size_t len) {
  dst.alloc(std::max<size_t>(len, 1));
  if (len) HIP_CHECK(hipMemcpy(dst.get(), src, sizeof(int) * len, hipMemcpyHostToDevice));
}

void check_finite(const char* fn, const char* what, const double* x, int64_t len) {
  for (int64_t k = 0; k < len; ++k)
    if (!std::isfinite(x[k])) Fatal("%s: %s[%lld] is not finite", fn, what, (long long)k);
}

void check_cov(const char* fn, int d, int cov_type, double var, double phi) {
  if (d < 1 || d > 3) Fatal("%s: d = %d is not in 1..3", fn, d);
  if (cov_type < 0 || cov_type > 3) Fatal("%s: cov_type = %d", fn, cov_type);
  if (!(var > 0.) || !(phi > 0.) || !std::isfinite(var) || !std::isfinite(phi))
    Fatal("%s: var and phi must be finite and > 0", fn);
}
}  // namespace

void test_fitc_vector(int op, int n, int m, int d, int cov_type, double var, double phi, double extra, double pad_fill,
                      const double* const* arrays, const int64_t* lens, int n_arrays, const int32_t* ints,
                      int64_t ints_len, double* const* outs, const int64_t* out_lens, int n_outs, int* guard) {
  const char* fn = "GPB_TestFitcVector";
  // ---- everything that can be refused is refused before the first device call
  if (op < 0 || op >= kNumFitcVecOps) Fatal("%s: unknown op %d", fn, op);
  if (n < 1 || n >= kMaxN) Fatal("%s: n = %d is not in 1..%d", fn, n, kMaxN - 1);
  if (m < 1 || m > kMaxM) Fatal("%s: m = %d is not in 1..%d", fn, m, kMaxM);
  if (arrays == nullptr || lens == nullptr || outs == nullptr || out_lens == nullptr || guard == nullptr)
    Fatal("%s: arrays, lens, outs, out_lens or guard_flag is NULL", fn);
  if (ints_len < 0 || (ints_len > 0 && ints == nullptr)) Fatal("%s: ints is NULL with ints_len = %lld", fn, (long long)ints_len);
  const int ldm = round_ldm(m);
  const int64_t nm = (int64_t)n * m, mm = (int64_t)m * m, nl = (int64_t)n * ldm, ml = (int64_t)m * ldm;
  const int nb4 = (n + 3) / 4;
  constexpr int kMaxArr = 9, kMaxOut = 3;
  int need = 0, nout = 0, need_ints = 0;
  int64_t want[kMaxArr] = {0}, wout[kMaxOut] = {0};
  bool nullable[kMaxArr] = {false};
  int chunks = 0, np = 0, npairs = 0, alias = 0;
  const bool uses_cov = op == kFitcKmn || op == kFitcKmm || op == kFitcDkmn || op == kFitcGrad;
  if (uses_cov) check_cov(fn, d, cov_type, var, phi);
  if (!std::isfinite(extra)) Fatal("%s: extra is not finite", fn);
  switch (op) {
    case kFitcKmn:
    case kFitcDkmn: need = 2; want[0] = (int64_t)n * d; want[1] = (int64_t)m * d; nout = 1; wout[0] = nl; break;
    case kFitcKmm: need = 1; want[0] = (int64_t)m * d; nout = 3; wout[0] = wout[1] = wout[2] = ml; break;
    case kFitcDiag: need = 2; want[0] = want[1] = nm; nout = 3; wout[0] = n; wout[1] = nl; wout[2] = 1; break;
    case kFitcDy: need = 2; want[0] = want[1] = n; nout = 1; wout[0] = n; break;
    case kFitcWsum:
      need_ints = 1;
      if (ints_len != 1 || ints[0] < 1 || ints[0] > 64) Fatal("%s: op %d takes ints = [chunks], chunks in 1..64", fn, op);
      chunks = ints[0];
      need = 2; want[0] = chunks * mm; want[1] = mm; nout = 1; wout[0] = ml;
      break;
    case kFitcGemv: need = 2; want[0] = nm; want[1] = n; nout = 1; wout[0] = m; break;
    case kFitcSymv: need = 2; want[0] = mm; want[1] = m; nout = 1; wout[0] = m; break;
    case kFitcLowerT: need = 1; want[0] = mm; nout = 1; wout[0] = ml; break;
    case kFitcCholSolve: need = 3; want[0] = want[1] = mm; want[2] = m; nout = 1; wout[0] = m; break;
    case kFitcYaux: need = 5; want[0] = nm; want[1] = m; want[2] = want[3] = want[4] = n; nout = 2; wout[0] = n; wout[1] = 1; break;
    case kFitcGrad:
      need = 9; want[0] = (int64_t)n * d; want[1] = (int64_t)m * d; want[2] = want[3] = want[4] = want[5] = nm;
      want[6] = m; want[7] = want[8] = n; nout = 2; wout[0] = 4; wout[1] = (int64_t)4 * nb4;
      break;
    case kFitcMmTerms: need = 5; want[0] = want[1] = want[2] = want[3] = mm; want[4] = m; nout = 1; wout[0] = 6; break;
    case kFitcColdot: need = 2; want[0] = nm; want[1] = m; nullable[1] = true; nout = 1; wout[0] = n; break;
    case kFitcPredCorr: {
      need_ints = 1;
      if (ints_len < 1 || ints_len % 2 != 1) Fatal("%s: op %d takes ints = [np, pi_0, oj_0, ...]", fn, op);
      np = ints[0];
      npairs = (int)((ints_len - 1) / 2);
      if (np < 1 || np >= kMaxN) Fatal("%s: np = %d", fn, np);
      if (npairs > np) Fatal("%s: %d pairs for %d prediction points", fn, npairs, np);
      std::vector<char> seen(np, 0);
      for (int q = 0; q < npairs; ++q) {
        const int pi = ints[1 + 2 * q], oj = ints[2 + 2 * q];
        if (pi < 0 || pi >= np || oj < 0 || oj >= n)
          Fatal("%s: pair %d = (%d, %d) is out of range (np = %d, n = %d)", fn, q, pi, oj, np, n);
        if (seen[pi]) Fatal("%s: prediction point %d is paired twice", fn, pi);
        seen[pi] = 1;
      }
      need = 4; want[0] = (int64_t)np * m; want[1] = nm; want[2] = n; want[3] = (int64_t)np * m;
      nout = 2; wout[0] = (int64_t)np * ldm; wout[1] = std::max(npairs, 1);
      break;
    }
    case kFitcFfDiagGrad: need = 3; want[0] = want[1] = want[2] = nm; nout = 1; wout[0] = n; break;
    case kFitcFfRecip: need = 1; want[0] = n; nout = 1; wout[0] = n; break;
    case kFitcFfRowscale:
      need_ints = 1;
      if (ints_len != 1 || (ints[0] != 0 && ints[0] != 1)) Fatal("%s: op %d takes ints = [alias], 0 or 1", fn, op);
      alias = ints[0];
      need = 3; want[0] = n; want[1] = want[2] = nm; nullable[2] = true; nout = 1; wout[0] = nm;
      break;
    default: need = 2; want[0] = want[1] = n; nout = 1; wout[0] = 1;   // kFitcFfDot
  }
  if (!need_ints && ints_len != 0) Fatal("%s: op %d takes no ints", fn, op);
  if (n_arrays != need) Fatal("%s: op %d takes %d arrays, not %d", fn, op, need, n_arrays);
  if (n_outs != nout) Fatal("%s: op %d writes %d outputs, not %d", fn, op, nout, n_outs);
  for (int k = 0; k < need; ++k) {
    if (arrays[k] == nullptr) {
      if (!nullable[k]) Fatal("%s: arrays[%d] is NULL", fn, k);
      if (lens[k] != 0) Fatal("%s: arrays[%d] is NULL with lens = %lld", fn, k, (long long)lens[k]);
    } else if (lens[k] != want[k]) {
      Fatal("%s: arrays[%d] holds %lld entries, not %lld", fn, k, (long long)lens[k], (long long)want[k]);
    }
  }
  for (int k = 0; k < nout; ++k) {
    if (outs[k] == nullptr) Fatal("%s: outs[%d] is NULL", fn, k);
    if (out_lens[k] != wout[k])
      Fatal("%s: outs[%d] holds %lld entries, op %d writes %lld", fn, k, (long long)out_lens[k], op, (long long)wout[k]);
  }
  if (uses_cov) {
    if (op != kFitcKmm) check_finite(fn, "X", arrays[0], want[0]);
    check_finite(fn, "Z", arrays[op == kFitcKmm ? 0 : 1], (int64_t)m * d);
  }
  if (alias && arrays[2] == nullptr) Fatal("%s: alias = 1 needs Yin", fn);

  // ---- device blocks
  DevBuf<double> in[kMaxArr];
  DevBuf<int> dints;
  Guarded go[kMaxOut], gpart, gtmp;
  const double* A[kMaxArr];
  for (int k = 0; k < nout; ++k)
    if (!(op == kFitcPredCorr && k == 0) && !(op == kFitcFfRowscale && alias)) go[k].make((size_t)wout[k]);
  // arrays of n x m (columns of ldm) or m x m shape are padded; the rest go up as they are
  auto is_nm = [&](int k) {
    switch (op) {
      case kFitcDiag: case kFitcFfDiagGrad: return true;
      case kFitcGemv: case kFitcYaux: case kFitcColdot: return k == 0;
      case kFitcGrad: return k >= 2 && k <= 5;
      case kFitcPredCorr: return k == 1;
      default: return false;
    }
  };
  auto is_mm = [&](int k) {
    switch (op) {
      case kFitcSymv: case kFitcLowerT: return k == 0;
      case kFitcWsum: return k == 1;
      case kFitcCholSolve: return k < 2;
      case kFitcMmTerms: return k < 4;
      default: return false;
    }
  };
  for (int k = 0; k < need; ++k) {
    A[k] = nullptr;
    if (arrays[k] == nullptr) continue;
    if (op == kFitcPredCorr && k == 0) upload_padded(in[k], arrays[k], np, m, ldm, pad_fill);
    else if (op == kFitcPredCorr && k == 3) continue;   // Maux: the in-place output below
    else if (op == kFitcWsum && k == 0) {
      // the split-K partials: chunk z at z ldm ldm, as gemm_f64_splitk leaves them
      std::vector<double> h((size_t)chunks * ldm * ldm, pad_fill);
      for (int z = 0; z < chunks; ++z)
        for (int r = 0; r < m; ++r)
          std::memcpy(&h[((size_t)z * ldm + r) * ldm], arrays[0] + ((size_t)z * m + r) * m, sizeof(double) * m);
      upload_vec(in[k], h);
    } else if (op == kFitcFfRowscale && k == 2 && alias) continue;   // Yin: the in-place output below
    else if (is_nm(k)) upload_padded(in[k], arrays[k], n, m, ldm, pad_fill);
    else if (is_mm(k)) upload_padded(in[k], arrays[k], m, m, ldm, pad_fill);
    else upload(in[k], arrays[k], (size_t)want[k]);
    A[k] = in[k].get();
  }
  hipStream_t s = nullptr;
  switch (op) {
    case kFitcKmn: fitc_kmn(s, cov_type, A[0], A[1], n, m, d, ldm, var, phi, go[0].p()); break;
    case kFitcDkmn: fitc_ff_dkmn(s, cov_type, A[0], A[1], n, m, d, ldm, var, phi, go[0].p()); break;
    case kFitcKmm: fitc_kmm(s, cov_type, A[0], m, d, ldm, var, phi, go[0].p(), go[1].p(), go[2].p()); break;
    case kFitcDiag:
      gpart.make(nb4);
      fitc_diag(s, A[0], A[1], n, m, ldm, extra, go[0].p(), go[1].p(), gpart.p(), go[2].p());
      break;
    case kFitcDy: fitc_dy(s, A[0], A[1], n, go[0].p()); break;
    case kFitcWsum: fitc_wsum(s, A[0], chunks, (long)ldm * ldm, m, ldm, A[1], go[0].p()); break;
    case kFitcGemv:
      gpart.make((size_t)((n + 63) / 64) * ldm);
      fitc_gemv(s, A[0], A[1], n, m, ldm, gpart.p(), go[0].p());
      break;
    case kFitcSymv: fitc_symv(s, A[0], A[1], m, ldm, go[0].p()); break;
    case kFitcLowerT: fitc_lower_t(s, A[0], m, ldm, go[0].p()); break;
    case kFitcCholSolve:
      gtmp.make(m);
      fitc_chol_solve(s, A[0], A[1], A[2], m, ldm, gtmp.p(), go[0].p());
      break;
    case kFitcYaux:
      gpart.make(nb4);
      fitc_yaux(s, A[0], A[1], A[2], A[3], A[4], n, m, ldm, go[0].p(), gpart.p(), go[1].p());
      break;
    case kFitcGrad:
      fitc_grad_parts(s, cov_type, A[0], A[1], n, m, d, ldm, var, phi, extra, A[2], A[3], A[4], A[5], A[6], A[7], A[8],
                      go[1].p());
      launch_sum_blocks(go[1].p(), nb4, 4, go[0].p(), s);
      break;
    case kFitcMmTerms:
      gpart.make((size_t)6 * ((m + 3) / 4));
      fitc_mm_terms(s, A[0], A[1], A[2], A[3], A[4], m, ldm, gpart.p(), go[0].p());
      break;
    case kFitcColdot: fitc_coldot(s, A[0], A[1], n, m, ldm, go[0].p()); break;
    case kFitcPredCorr: {
      const std::vector<double> h = padded(arrays[3], np, m, ldm, pad_fill, (size_t)np * ldm);
      go[0].make(h.size(), h.data());
      upload_int(dints, ints + 1, (size_t)2 * npairs);
      fitc_pred_corr(s, dints.get(), npairs, A[0], A[1], A[2], m, ldm, extra, go[0].p(), go[1].p());
      break;
    }
    case kFitcFfDiagGrad: fitc_ff_diag_grad(s, A[0], A[1], A[2], n, m, ldm, extra, go[0].p()); break;
    case kFitcFfRecip: fitc_ff_recip(s, n, A[0], go[0].p()); break;
    case kFitcFfRowscale:
      if (alias) {
        go[0].make((size_t)nm, arrays[2]);
        fitc_ff_rowscale(s, n, m, A[0], A[1], extra, go[0].p(), go[0].p());
      } else {
        fitc_ff_rowscale(s, n, m, A[0], A[1], extra, A[2], go[0].p());
      }
      break;
    default:
      gpart.make(kFitcDotBlocks);
      fitc_ff_dot(s, (size_t)n, A[0], A[1], gpart.p(), go[0].p());
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  bool touched = false;
  for (int k = 0; k < nout; ++k) touched = go[k].fetch(outs[k]) || touched;
  if (gpart.len) touched = gpart.fetch(nullptr) || touched;
  if (gtmp.len) touched = gtmp.fetch(nullptr) || touched;
  *guard = touched ? 1 : 0;
}

void test_fitc_kmeans(int op, int n, int k, int d, const double* X, int64_t x_len, const double* mu, const double* mu_a,
                      const double* mu_b, int64_t mu_len, const int32_t* cluster_in, int64_t cluster_len, int scan,
                      int max_it, double* mu_out, int32_t* ints_out, int64_t ints_len, int* its, int* guard) {
  const char* fn = "GPB_TestFitcKmeans";
  if (op < 0 || op >= kNumFitcKmeansOps) Fatal("%s: unknown op %d", fn, op);
  if (n < 1 || n >= kMaxN) Fatal("%s: n = %d is not in 1..%d", fn, n, kMaxN - 1);
  if (k < 1 || k > kMaxM) Fatal("%s: k = %d is not in 1..%d", fn, k, kMaxM);
  if (k > n) Fatal("%s: k = %d clusters for n = %d points", fn, k, n);
  if (d < 1 || d > 3) Fatal("%s: d = %d is not in 1..3", fn, d);
  if (scan != 0 && scan != 1) Fatal("%s: scan = %d", fn, scan);
  if (mu == nullptr || guard == nullptr) Fatal("%s: mu or guard_flag is NULL", fn);
  const int64_t kd = (int64_t)k * d;
  if (mu_len != kd) Fatal("%s: the means hold %lld entries, k d = %lld", fn, (long long)mu_len, (long long)kd);
  check_finite(fn, "mu", mu, kd);
  const bool needs_x = op != kFitcKmCmp;
  if (needs_x) {
    if (X == nullptr || x_len != (int64_t)n * d)
      Fatal("%s: X holds %lld entries, n d = %lld", fn, (long long)(X ? x_len : 0), (long long)n * d);
    check_finite(fn, "X", X, x_len);
  }
  const int nbk = (n + 255) / 256;
  int64_t want_ints = 0;
  switch (op) {
    case kFitcKmAssign: want_ints = n; break;
    case kFitcKmMeans:
      if (cluster_in == nullptr || cluster_len != n) Fatal("%s: op 1 takes cluster_in with n entries", fn);
      for (int i = 0; i < n; ++i)
        if (cluster_in[i] < 0 || cluster_in[i] >= k) Fatal("%s: cluster_in[%d] = %d is not in 0..%d", fn, i, cluster_in[i], k - 1);
      want_ints = scan ? 0 : (int64_t)2 * nbk * k + k + (k + 1) + n;
      if (mu_out == nullptr) Fatal("%s: mu_out is NULL", fn);
      break;
    case kFitcKmCmp:
      if (mu_a == nullptr || mu_b == nullptr) Fatal("%s: op 2 takes mu_a and mu_b", fn);
      want_ints = 2;
      break;
    default:
      if (max_it < 1 || max_it > 1000) Fatal("%s: max_it = %d is not in 1..1000", fn, max_it);
      if (mu_out == nullptr || its == nullptr) Fatal("%s: mu_out or its is NULL", fn);
  }
  if (ints_len != want_ints || (want_ints > 0 && ints_out == nullptr))
    Fatal("%s: ints_out holds %lld entries, op %d writes %lld", fn, (long long)ints_len, op, (long long)want_ints);

  hipStream_t s = nullptr;
  bool touched = false;
  if (op == kFitcKmLloyd) {
    std::vector<double> Z(mu, mu + kd);
    *its = fitc_kmeans_lloyd(s, X, n, d, k, Z.data(), scan != 0, max_it);
    std::memcpy(mu_out, Z.data(), sizeof(double) * kd);
    *guard = 0;
    return;
  }
  DevBuf<double> dX, dmu, da, db;
  DevBuf<int> dcl;
  if (needs_x) upload(dX, X, (size_t)x_len);
  upload(dmu, mu, (size_t)kd);
  if (op == kFitcKmAssign) {
    GuardedInt gc;
    gc.make(n);
    fitc_kmeans_assign(s, dX.get(), dmu.get(), n, k, d, gc.p());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    touched = gc.fetch(ints_out);
  } else if (op == kFitcKmMeans) {
    upload_int(dcl, cluster_in, n);
    Guarded gm;
    gm.make((size_t)kd);
    GuardedInt gcnt, goff, gtot, gbase, glist;
    KmeansWork w{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (!scan) {
      gcnt.make((size_t)nbk * k);
      goff.make((size_t)nbk * k);
      gtot.make(k);
      gbase.make((size_t)k + 1);
      glist.make(n);
      w = KmeansWork{gcnt.p(), goff.p(), gtot.p(), gbase.p(), glist.p()};
    }
    fitc_kmeans_means(s, scan != 0, dX.get(), dcl.get(), n, k, d, dmu.get(), gm.p(), w);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    touched = gm.fetch(mu_out);
    if (!scan) {
      int32_t* o = ints_out;
      touched = gcnt.fetch(o) || touched;
      o += (size_t)nbk * k;
      touched = goff.fetch(o) || touched;
      o += (size_t)nbk * k;
      touched = gtot.fetch(o) || touched;
      o += k;
      touched = gbase.fetch(o) || touched;
      o += k + 1;
      touched = glist.fetch(o) || touched;
    }
  } else {
    upload(da, mu_a, (size_t)kd);
    upload(db, mu_b, (size_t)kd);
    GuardedInt gf;
    gf.make(2);
    fitc_kmeans_cmp(s, dmu.get(), da.get(), db.get(), (int)kd, gf.p());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    touched = gf.fetch(ints_out);
  }
  *guard = touched ? 1 : 0;
}

// the way into FitcSolver's private stage and buffers (friend, fitc.h)
struct FitcTestAccess {
  static void Factor(FitcSolver& f, int cov, double var, double phi, const double* d_y) {
    f.Factor(cov, var, phi, d_y, f.red_.get());
    HIP_CHECK(hipStreamSynchronize(f.stream_));
  }
  // the device buffer of an output and its length (matrices with their padding); nullptr: not a buffer
  static const double* Buffer(const FitcSolver& f, int k, size_t* len) {
    const size_t n = f.n_, ldm = f.ldm_, m = f.m_, mn = ldm * n, mm = ldm * m;
    const double* vec = f.vec_.get();
    switch (k) {
      case kFsKmn: *len = mn; return f.Kmn_.get();
      case kFsKmm: *len = mm; return f.Kmm_.get();
      case kFsKs: *len = mm; return f.Ks_.get();
      case kFsDKmm: *len = mm; return f.dKmm_.get();
      case kFsLi: *len = mm; return f.Li_.get();
      case kFsLiT: *len = mm; return f.LiT_.get();
      case kFsKinv: *len = mm; return f.Kinv_.get();
      case kFsV: *len = mn; return f.V_.get();
      case kFsD: *len = n; return vec;
      case kFsKd: *len = mn; return f.Kd_.get();
      case kFsW: *len = mm; return f.W_.get();
      case kFsWi: *len = mm; return f.Wi_.get();
      case kFsWiT: *len = mm; return f.WiT_.get();
      case kFsDy: *len = n; return vec + n;
      case kFsYaux: *len = n; return vec + 2 * n;
      case kFsU: *len = m; return vec + 3 * n;
      case kFsWvec: *len = m; return vec + 3 * n + ldm;
      case kFsAvec: *len = m; return vec + 3 * n + 2 * ldm;
      case kFsA: *len = mn; return f.A_.get();
      case kFsWinv: *len = mm; return f.Winv_.get();
      default: return nullptr;
    }
  }
};

void test_fitc_stages(int stage, int n, int m, int d, int cov_type, double var, double phi, double var2, double phi2,
                      const double* X, const double* Z, const double* y, int np, const double* Xp, const int32_t* match,
                      double* const* outs, const int64_t* out_lens, int n_outs) {
  const char* fn = "GPB_TestFitcStages";
  if (stage < 0 || stage >= kNumFitcStages) Fatal("%s: unknown stage %d", fn, stage);
  if (n < 1 || n > (1 << 16)) Fatal("%s: n = %d is not in 1..65536", fn, n);
  if (m < 1 || m > 1024 || m > n) Fatal("%s: m = %d is not in 1..min(n, 1024)", fn, m);
  check_cov(fn, d, cov_type, var, phi);
  if (stage == kFitcStGramOtherEval) check_cov(fn, d, cov_type, var2, phi2);
  if (X == nullptr || Z == nullptr || y == nullptr || outs == nullptr || out_lens == nullptr)
    Fatal("%s: X, Z, y, outs or out_lens is NULL", fn);
  if (n_outs != kNumFitcStageOuts) Fatal("%s: %d outputs, not %d", fn, n_outs, (int)kNumFitcStageOuts);
  check_finite(fn, "X", X, (int64_t)n * d);
  check_finite(fn, "Z", Z, (int64_t)m * d);
  check_finite(fn, "y", y, n);
  const bool pred = stage == kFitcStPredict;
  if (pred) {
    if (np < 1 || np > 4096 || Xp == nullptr || match == nullptr) Fatal("%s: Predict takes np in 1..4096, Xp and match", fn);
    check_finite(fn, "Xp", Xp, (int64_t)np * d);
    for (int i = 0; i < np; ++i)
      if (match[i] < -1 || match[i] >= n) Fatal("%s: match[%d] = %d is not in -1..%d", fn, i, match[i], n - 1);
  } else if (np != 0) {
    Fatal("%s: np = %d without Predict", fn, np);
  }
  const int ldm = round_ldm(m);
  for (int k = 0; k < n_outs; ++k) {
    if (outs[k] == nullptr) continue;
    int64_t want;
    if (k == kFsSums) want = 6;
    else if (k == kFsMean || k == kFsVar) want = np;
    else if (k == kFsCov) want = (int64_t)np * np;
    else if (k == kFsKmn || k == kFsV || k == kFsKd || k == kFsA) want = (int64_t)n * ldm;
    else if (k == kFsD || k == kFsDy || k == kFsYaux) want = n;
    else if (k == kFsU || k == kFsWvec || k == kFsAvec) want = m;
    else want = (int64_t)m * ldm;
    if (out_lens[k] != want || want == 0)
      Fatal("%s: outs[%d] holds %lld entries, not %lld", fn, k, (long long)out_lens[k], (long long)want);
    if (pred != (k >= kFsMean) && k >= kFsSums) Fatal("%s: outs[%d] does not belong to stage %d", fn, k, stage);
  }

  hipStream_t s = nullptr;
  HIP_CHECK(hipStreamCreate(&s));
  {
    DevBuf<double> dX, dy;
    upload(dX, X, (size_t)n * d);
    upload(dy, y, n);
    FitcSolver f(n, d, dX.get(), std::vector<double>(Z, Z + (size_t)m * d), s);
    double sums[6], ms[2];
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (double& v : sums) v = nan;
    if (stage == kFitcStGramEval || stage == kFitcStGramOtherEval) {
      const bool same = stage == kFitcStGramEval;
      double G = nan;
      f.Gram(cov_type, same ? var : var2, same ? phi : phi2, dy.get(), 1, &G);
      if (!std::isfinite(G)) Fatal("%s: Gram is not finite", fn);
    }
    if (stage == kFitcStFactor) {
      FitcTestAccess::Factor(f, cov_type, var, phi, dy.get());
    } else if (pred) {
      std::vector<int> mt(match, match + np);
      f.Predict(cov_type, var, phi, dy.get(), Xp, np, mt, outs[kFsVar] != nullptr, outs[kFsCov] != nullptr, false,
                outs[kFsMean] ? outs[kFsMean] : std::vector<double>(np).data(), outs[kFsVar], outs[kFsCov]);
    } else {
      f.Eval(cov_type, var, phi, dy.get(), true, sums, ms);
    }
    HIP_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < kFsSums; ++k) {
      if (outs[k] == nullptr) continue;
      size_t len = 0;
      const double* src = FitcTestAccess::Buffer(f, k, &len);
      HIP_CHECK(hipMemcpy(outs[k], src, sizeof(double) * len, hipMemcpyDeviceToHost));
    }
    if (outs[kFsSums] && !pred) std::memcpy(outs[kFsSums], sums, sizeof(sums));
  }
  HIP_CHECK(hipStreamDestroy(s));
}

}  // namespace gpb_amd
