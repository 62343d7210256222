// Test entries of the full-scale Vecchia kernels (GPB_TestVif*, include/gpboost_amd.h): the residual row factor in
// both forms, the sparse B / B^T products and the small vector kernels, on host arrays through the launch functions
// of vif.h (the ones VifSolver calls). Every extent and index is checked on the host before any device call;
// outputs and scratch sit between guard bands and start as NaN, so a write out of range or an entry left unwritten
// is seen without a fault; the ld-m padding of every input column holds the caller's fill value.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "common.h"
#include "vif.h"
#include "vif_test.h"

namespace gpb_amd {

namespace {
constexpr size_t kGuard = 64;   // guard doubles on both sides of an output block
constexpr int kMaxM = 4096;

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

// host n x m row-major -> device n columns of ldm doubles, the padding filled
void upload_padded(DevBuf<double>& dst, const double* src, int n, int m, int ldm, double fill) {
  std::vector<double> h((size_t)n * ldm, fill);
  for (int i = 0; i < n; ++i) std::memcpy(&h[(size_t)i * ldm], src + (size_t)i * m, sizeof(double) * m);
  dst.alloc(h.size());
  HIP_CHECK(hipMemcpy(dst.get(), h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
}

void upload(DevBuf<double>& dst, const double* src, size_t len) {
  dst.alloc(std::max<size_t>(len, 1));
  if (len) HIP_CHECK(hipMemcpy(dst.get(), src, sizeof(double) * len, hipMemcpyHostToDevice));
}

void upload_int(DevBuf<int>& dst, const int* src, size_t len) {
  dst.alloc(std::max<size_t>(len, 1));
  if (len) HIP_CHECK(hipMemcpy(dst.get(), src, sizeof(int) * len, hipMemcpyHostToDevice));
}

// row of point i (list index i - i0) holds min(i, nn) distinct indices in [0, i) and -1 after them
void check_lists(const char* fn, int n_total, int i0, int nn, const int32_t* nbr) {
  std::vector<int> seen(n_total, -1);
  for (int i = i0; i < n_total; ++i) {
    const int k = std::min(i, nn);
    const int32_t* row = nbr + (size_t)(i - i0) * nn;
    for (int r = 0; r < nn; ++r) {
      const int j = row[r];
      if (r >= k) {
        if (j != -1) Fatal("%s: nbr of point %d, slot %d = %d past its %d entries is not -1", fn, i, r, j, k);
        continue;
      }
      if (j < 0 || j >= i) Fatal("%s: nbr of point %d, slot %d = %d is not an earlier point", fn, i, r, j);
      if (seen[j] == i) Fatal("%s: nbr of point %d names point %d twice", fn, i, j);
      seen[j] = i;
    }
  }
}

void check_finite(const char* fn, const char* what, const double* x, int64_t len) {
  for (int64_t k = 0; k < len; ++k)
    if (!std::isfinite(x[k])) Fatal("%s: %s[%lld] is not finite", fn, what, (long long)k);
}
}  // namespace

void test_vif_rows(const VifRowsTest& t, int64_t x_len, int64_t nbr_len, int64_t mat_len, int64_t rows_len,
                   int* guard) {
  const char* fn = "GPB_TestVifRows";
  // ---- everything that can be refused is refused before the first device call
  if (t.n_total < 1 || t.n_total > (1 << 20) || t.i0 < 0 || t.i0 >= t.n_total)
    Fatal("%s: n_total = %d, i0 = %d", fn, t.n_total, t.i0);
  if (t.d < 1 || t.d > 3) Fatal("%s: d = %d is not in 1..3", fn, t.d);
  if (t.m < 1 || t.m > kMaxM) Fatal("%s: m = %d is not in 1..%d", fn, t.m, kMaxM);
  const bool grad = t.grad != 0;
  if (t.grad != 0 && t.grad != 1) Fatal("%s: grad = %d", fn, t.grad);
  const int nn_max = grad ? kVifMaxNnGrad : kVifMaxNn;
  if (t.nn < 1 || t.nn > nn_max)
    Fatal("%s: nn = %d is not in 1..%d %s derivatives", fn, t.nn, nn_max, grad ? "with" : "without");
  if (t.form < 0 || t.form > 2) Fatal("%s: form = %d", fn, t.form);
  if (t.form == 1 && t.nn > kVifMaxNnMfma)
    Fatal("%s: the MFMA form (form 1) takes nn <= %d, not %d", fn, kVifMaxNnMfma, t.nn);
  if (t.order != 0 && t.order != 1) Fatal("%s: order = %d", fn, t.order);
  if (t.cov_type < 0 || t.cov_type > 3) Fatal("%s: cov_type = %d", fn, t.cov_type);
  if (!(t.var > 0.) || !(t.phi > 0.) || !std::isfinite(t.var) || !std::isfinite(t.phi))
    Fatal("%s: var and phi must be finite and > 0", fn);
  if (!(t.nugget >= 0.) || !std::isfinite(t.nugget) || !(t.cjit > 0.) || !std::isfinite(t.cjit))
    Fatal("%s: nugget must be >= 0 and cjit > 0", fn);
  const int rows = t.n_total - t.i0;
  if (t.X == nullptr || t.nbr == nullptr || t.V == nullptr || t.D == nullptr || t.Bv == nullptr || guard == nullptr)
    Fatal("%s: X, nbr, V, D, Bv or guard_flag is NULL", fn);
  if (grad && (t.P0 == nullptr || t.P1 == nullptr || t.dD0 == nullptr || t.dD1 == nullptr || t.dBv0 == nullptr ||
               t.dBv1 == nullptr))
    Fatal("%s: grad = 1 needs P0, P1, dD0, dD1, dBv0 and dBv1", fn);
  if (!grad && (t.P0 != nullptr || t.P1 != nullptr)) Fatal("%s: P0 / P1 without grad", fn);
  if (x_len != (int64_t)t.n_total * t.d || nbr_len != (int64_t)rows * t.nn || mat_len != (int64_t)t.n_total * t.m ||
      rows_len != rows)
    Fatal("%s: X / nbr / matrices / outputs hold %lld / %lld / %lld / %lld entries, not %lld / %lld / %lld / %d", fn,
          (long long)x_len, (long long)nbr_len, (long long)mat_len, (long long)rows_len,
          (long long)t.n_total * t.d, (long long)rows * t.nn, (long long)t.n_total * t.m, rows);
  check_finite(fn, "X", t.X, x_len);
  check_lists(fn, t.n_total, t.i0, t.nn, t.nbr);

  // ---- device blocks
  const int ldm = round_ldm(t.m);
  DevBuf<double> dX, dV, dP0, dP1;
  DevBuf<int> dnbr, dord;
  upload(dX, t.X, (size_t)x_len);
  upload_int(dnbr, t.nbr, (size_t)nbr_len);
  upload_padded(dV, t.V, t.n_total, t.m, ldm, t.pad_fill);
  if (grad) {
    upload_padded(dP0, t.P0, t.n_total, t.m, ldm, t.pad_fill);
    upload_padded(dP1, t.P1, t.n_total, t.m, ldm, t.pad_fill);
  }
  if (t.order && rows > 1) {   // VifSolver's processing order, over the rows' own points
    const std::vector<int> ord = vif_morton_order(t.X + (size_t)t.i0 * t.d, rows, t.d);
    upload_int(dord, ord.data(), ord.size());
  }
  Guarded gD, gB, gD0, gD1, gB0, gB1;
  gD.make(rows);
  gB.make((size_t)rows * t.nn);
  if (grad) {
    gD0.make(rows);
    gD1.make(rows);
    gB0.make((size_t)rows * t.nn);
    gB1.make((size_t)rows * t.nn);
  }
  VifRowsLaunch L;
  L.X = dX.get();
  L.nbr = dnbr.get();
  L.n_total = t.n_total; L.d = t.d; L.nn = t.nn; L.m = t.m; L.ldm = ldm; L.i0 = t.i0;
  L.V = dV.get();
  L.P0 = grad ? dP0.get() : nullptr;
  L.P1 = grad ? dP1.get() : nullptr;
  L.cov_type = t.cov_type; L.var = t.var; L.phi = t.phi; L.nugget = t.nugget; L.cjit = t.cjit;
  L.grad = grad;
  L.form = t.form;
  L.ord = dord.size() ? dord.get() : nullptr;
  L.D = gD.p(); L.Bv = gB.p();
  if (grad) { L.dD0 = gD0.p(); L.dD1 = gD1.p(); L.dBv0 = gB0.p(); L.dBv1 = gB1.p(); }
  hipStream_t s = nullptr;
  vif_launch_rows(L, s);
  HIP_CHECK(hipDeviceSynchronize());
  bool touched = gD.fetch(t.D);
  touched = gB.fetch(t.Bv) || touched;
  if (grad) {
    touched = gD0.fetch(t.dD0) || touched;
    touched = gD1.fetch(t.dD1) || touched;
    touched = gB0.fetch(t.dBv0) || touched;
    touched = gB1.fetch(t.dBv1) || touched;
  }
  *guard = touched ? 1 : 0;
}

void test_vif_apply(int op, int n, int nn, int m, const int32_t* nbr, int64_t nbr_len, const double* coef,
                    int64_t coef_len, const double* D, const double* in, int64_t in_len, double self, int div,
                    int want_div, const double* X, int d, int order, double pad_fill, double* out, double* out2,
                    int64_t out_len, int* guard) {
  const char* fn = "GPB_TestVifApply";
  if (op < 0 || op >= kNumVifApplyOps) Fatal("%s: unknown op %d", fn, op);
  if (n < 1 || n >= (1 << 22) || nn < 1 || nn > kVifMaxNn) Fatal("%s: n = %d, nn = %d", fn, n, nn);
  if (m < 1 || m > kMaxM) Fatal("%s: m = %d is not in 1..%d", fn, m, kMaxM);
  const bool mat = op == kVifBRow || op == kVifBCol;
  const int ldm = round_ldm(m);
  if (nbr == nullptr || coef == nullptr || in == nullptr || out == nullptr || guard == nullptr)
    Fatal("%s: nbr, coef, in, out or guard_flag is NULL", fn);
  if (nbr_len != (int64_t)n * nn || coef_len != (int64_t)n * nn)
    Fatal("%s: nbr / coef hold %lld / %lld entries, n nn = %lld", fn, (long long)nbr_len, (long long)coef_len,
          (long long)n * nn);
  const int64_t want_in = mat ? (int64_t)n * m : n, want_out = mat ? (int64_t)n * ldm : n;
  if (in_len != want_in || out_len != want_out)
    Fatal("%s: in / out hold %lld / %lld entries, op %d takes %lld / %lld", fn, (long long)in_len, (long long)out_len, op,
          (long long)want_in, (long long)want_out);
  if ((div != 0 && div != 1) || (want_div != 0 && want_div != 1) || (order != 0 && order != 1))
    Fatal("%s: div = %d, want_div = %d, order = %d", fn, div, want_div, order);
  if ((div || want_div) && op != kVifBRow) Fatal("%s: div / want_div belong to op 0", fn);
  if ((div || want_div) && D == nullptr) Fatal("%s: div / want_div need D", fn);
  if (want_div && out2 == nullptr) Fatal("%s: want_div needs out2", fn);
  if (D != nullptr && (op == kVifBCol || op == kVifBtVec)) Fatal("%s: op %d takes no D", fn, op);
  if (order && (X == nullptr || d < 1 || d > 3)) Fatal("%s: order = 1 needs X with d in 1..3", fn);
  if (order && !mat) Fatal("%s: the vector products have no processing order", fn);
  if (order) check_finite(fn, "X", X, (int64_t)n * d);
  if (!std::isfinite(self)) Fatal("%s: self is not finite", fn);
  check_lists(fn, n, 0, nn, nbr);

  std::vector<int> tptr, trow, tslot;
  const int nnz = vif_transpose_lists(n, nn, nbr, tptr, trow, tslot);
  DevBuf<int> dnbr, dtptr, dtrow, dtslot, dord;
  upload_int(dnbr, nbr, (size_t)n * nn);
  upload_int(dtptr, tptr.data(), tptr.size());
  upload_int(dtrow, trow.data(), trow.size());
  upload_int(dtslot, tslot.data(), tslot.size());
  if (order && n > 1) {
    const std::vector<int> ord = vif_morton_order(X, n, d);
    upload_int(dord, ord.data(), ord.size());
  }
  DevBuf<double> dcoef, dD, din;
  upload(dcoef, coef, (size_t)n * nn);
  if (D) upload(dD, D, n);
  if (mat) upload_padded(din, in, n, m, ldm, pad_fill);
  else upload(din, in, n);
  Guarded gout, gout2, gT;
  gout.make((size_t)want_out);
  if (want_div) gout2.make((size_t)want_out);
  VifGraph g;
  g.n = n; g.nn = nn; g.m = m; g.ldm = ldm;
  g.nbr = dnbr.get(); g.tptr = dtptr.get(); g.trow = dtrow.get();
  g.ord = dord.size() ? dord.get() : nullptr;
  hipStream_t s = nullptr;
  if (op == kVifBCol || op == kVifBtVec) {   // the values in column order, as Prepare makes them
    gT.make(std::max(nnz, 1));
    vif_launch_gather(s, nnz, dtslot.get(), dcoef.get(), gT.p());
  }
  switch (op) {
    case kVifBRow:
      vif_launch_brow(s, g, din.get(), dcoef.get(), D ? dD.get() : nullptr, self, div != 0, gout.p(),
                      want_div ? gout2.p() : nullptr);
      break;
    case kVifBCol: vif_launch_bcol(s, g, din.get(), gT.p(), self, gout.p()); break;
    case kVifBVec: vif_launch_bvec(s, g, din.get(), dcoef.get(), D ? dD.get() : nullptr, self, gout.p()); break;
    default: vif_launch_btvec(s, g, din.get(), gT.p(), self, gout.p());
  }
  HIP_CHECK(hipDeviceSynchronize());
  bool touched = gout.fetch(out);
  if (want_div) touched = gout2.fetch(out2) || touched;
  if (gT.len) {
    std::vector<double> h(gT.len);
    touched = gT.fetch(h.data()) || touched;
    for (int k = 0; k < nnz; ++k)
      if (h[k] != coef[tslot[k]] && !(std::isnan(h[k]) && std::isnan(coef[tslot[k]]))) touched = true;
  }
  *guard = touched ? 1 : 0;
}

void test_vif_vector(int op, int n, int m, int d, int cov_type, double var, double phi, double pad_fill,
                     const double* const* arrays, const int64_t* lens, int n_arrays, const int32_t* sum_ops, int nt,
                     double* out, int64_t out_len, int* guard) {
  const char* fn = "GPB_TestVifVector";
  if (op < 0 || op >= kNumVifVecOps) Fatal("%s: unknown op %d", fn, op);
  if (n < 1 || n >= (1 << 22)) Fatal("%s: n = %d", fn, n);
  if (m < 1 || m > kMaxM) Fatal("%s: m = %d is not in 1..%d", fn, m, kMaxM);
  if (arrays == nullptr || lens == nullptr || out == nullptr || guard == nullptr)
    Fatal("%s: arrays, lens, out or guard_flag is NULL", fn);
  const int ldm = round_ldm(m);
  const int64_t nm = (int64_t)n * m;
  int need = 0;
  int64_t want[24] = {0};
  bool nullable[24] = {false};
  int64_t want_out = 0;
  switch (op) {
    case kVifGemv: need = 2; want[0] = nm; want[1] = n; want_out = m; break;
    case kVifColDotW: need = 2; want[0] = nm; want[1] = m; want_out = n; break;
    case kVifColDotM: need = 2; want[0] = nm; want[1] = nm; want_out = n; break;
    case kVifZvec: need = 4; for (int k = 0; k < 4; ++k) want[k] = n; want_out = n; break;
    case kVifSum:
      if (nt < 1 || nt > 8 || sum_ops == nullptr) Fatal("%s: nt = %d terms (1..8) with sum_ops", fn, nt);
      need = 3 * nt;
      for (int k = 0; k < need; ++k) { want[k] = n; nullable[k] = k % 3 != 0; }
      for (int k = 0; k < nt; ++k)
        if (sum_ops[k] < 0 || sum_ops[k] > 4) Fatal("%s: sum_ops[%d] = %d", fn, k, sum_ops[k]);
      want_out = nt;
      break;
    default:
      if (d < 1 || d > 3) Fatal("%s: d = %d is not in 1..3", fn, d);
      if (cov_type < 0 || cov_type > 3) Fatal("%s: cov_type = %d", fn, cov_type);
      if (!(var > 0.) || !(phi > 0.) || !std::isfinite(var) || !std::isfinite(phi))
        Fatal("%s: var and phi must be finite and > 0", fn);
      need = 2; want[0] = (int64_t)n * d; want[1] = (int64_t)m * d; want_out = (int64_t)n * ldm;
  }
  if (n_arrays != need) Fatal("%s: op %d takes %d arrays, not %d", fn, op, need, n_arrays);
  for (int k = 0; k < need; ++k) {
    if (arrays[k] == nullptr) {
      if (!nullable[k]) Fatal("%s: arrays[%d] is NULL", fn, k);
      if (lens[k] != 0) Fatal("%s: arrays[%d] is NULL with lens = %lld", fn, k, (long long)lens[k]);
    } else if (lens[k] != want[k]) {
      Fatal("%s: arrays[%d] holds %lld entries, not %lld", fn, k, (long long)lens[k], (long long)want[k]);
    }
  }
  if (out_len != want_out) Fatal("%s: out holds %lld entries, op %d writes %lld", fn, (long long)out_len, op, (long long)want_out);
  if (op == kVifDkmn) {
    check_finite(fn, "X", arrays[0], want[0]);
    check_finite(fn, "Z", arrays[1], want[1]);
  }

  DevBuf<double> in[24];
  Guarded gout, gpart;
  gout.make((size_t)want_out);
  hipStream_t s = nullptr;
  switch (op) {
    case kVifGemv:
      upload_padded(in[0], arrays[0], n, m, ldm, pad_fill);
      upload(in[1], arrays[1], n);
      gpart.make((size_t)((n + 63) / 64) * ldm);
      vif_launch_gemv(s, n, m, ldm, in[0].get(), in[1].get(), gpart.p(), gout.p());
      break;
    case kVifColDotW:
      upload_padded(in[0], arrays[0], n, m, ldm, pad_fill);
      upload(in[1], arrays[1], m);
      vif_launch_coldot(s, n, m, ldm, in[0].get(), in[1].get(), nullptr, gout.p());
      break;
    case kVifColDotM:
      upload_padded(in[0], arrays[0], n, m, ldm, pad_fill);
      upload_padded(in[1], arrays[1], n, m, ldm, pad_fill);
      vif_launch_coldot(s, n, m, ldm, in[0].get(), nullptr, in[1].get(), gout.p());
      break;
    case kVifZvec:
      for (int k = 0; k < 4; ++k) upload(in[k], arrays[k], n);
      vif_launch_zvec(s, n, in[0].get(), in[1].get(), in[2].get(), in[3].get(), gout.p());
      break;
    case kVifSum: {
      VifTerms T{};
      for (int k = 0; k < nt; ++k) {
        for (int q = 0; q < 3; ++q)
          if (arrays[3 * k + q]) upload(in[3 * k + q], arrays[3 * k + q], n);
        T.a[k] = in[3 * k].get();
        T.b[k] = arrays[3 * k + 1] ? in[3 * k + 1].get() : nullptr;
        T.c[k] = arrays[3 * k + 2] ? in[3 * k + 2].get() : nullptr;
        T.op[k] = sum_ops[k];
      }
      gpart.make((size_t)512 * 8);
      vif_launch_sum(s, n, nt, T, gpart.p(), gout.p());
      break;
    }
    default:
      upload(in[0], arrays[0], (size_t)want[0]);
      upload(in[1], arrays[1], (size_t)want[1]);
      vif_launch_dkmn(s, cov_type, in[0].get(), in[1].get(), n, m, d, ldm, var, phi, gout.p());
  }
  HIP_CHECK(hipDeviceSynchronize());
  bool touched = gout.fetch(out);
  if (gpart.len) touched = gpart.fetch(nullptr) || touched;
  *guard = touched ? 1 : 0;
}

}  // namespace gpb_amd
