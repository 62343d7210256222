// Test entries of the latent-Vecchia operator layer (GPB_TestLatentOps*, include/gpboost_amd.h): the sparse
// operators of sparse_kernels.hip in every selectable form, the production composition ApplyA and the VADU
// preconditioner, on a LatentVecchia built from an arbitrary valid neighbour table. Host arrays in and out in
// Vecchia order; every extent and index is checked on the host before any device call, outputs sit between
// guard bands and start as NaN, so a write out of range or a row left unwritten is seen without a fault.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "latent.h"
#include "latent_test.h"

namespace gpb_amd {

namespace {
constexpr size_t kGuard = 64;   // guard doubles on both sides of an output block

// Vecchia-order host block (n x t) -> storage-order device block
void upload_rows(const std::vector<int>& vo, int n, int t, const double* src, double* dst, hipStream_t s) {
  std::vector<double> h((size_t)n * t);
  for (int p = 0; p < n; ++p) std::memcpy(&h[(size_t)p * t], src + (size_t)vo[p] * t, sizeof(double) * t);
  HIP_CHECK(hipMemcpyAsync(dst, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// The selection each form code stands for. Returns false when the shape or the arguments do not admit it.
bool b_form(int form, int t, int m, bool alt, SpmvOptions& o) {
  o = SpmvOptions();
  switch (form) {
    case kBFormEll: return t == 1 && !alt;
    case kBFormGroups: o.groups1 = true; return t == 1 && m <= 32;
    case kBFormOld: o.old1 = true; return t == 1;
    case kBFormWave16: return t >= 2 && m <= 64;
    case kBFormWave32: o.ch = -2; return t >= 2 && m <= 64;
    case kBFormCh0: o.ch = 0; return t >= 2;
    case kBFormCh16: o.ch = 16; return t >= 2;
    case kBFormCh0Pers: o.ch = 0; o.pers = 1; o.cap = 8; return t >= 2;
    case kBFormCh16Pers: o.ch = 16; o.pers = 1; o.cap = 8; return t >= 2;
    default: return false;
  }
}
bool bt_form(int form, int t, bool alt, SpmvOptions& o) {
  o = SpmvOptions();
  const bool t1 = t == 1 && !alt;   // every t = 1 form reads the values in list order
  switch (form) {
    case kBtFormPaired: return t1;
    case kBtFormE2: o.epl = 2; return t1;
    case kBtFormE4: o.epl = 4; return t1;
    case kBtFormS2: o.epl = 1; return t1;
    case kBtFormShfl: o.scan_shfl = true; return t1;
    case kBtFormE1: o.e1 = true; return t1;
    case kBtFormGroups: o.bt_groups1 = true; return t1;
    case kBtFormOld: o.old1 = true; return t1;
    case kBtFormWave16: return t >= 2 && !alt;
    case kBtFormWave32: o.ch = -2; return t >= 2 && !alt;
    case kBtFormCh0: o.ch = 0; return t >= 2;
    case kBtFormCh16: o.ch = 16; return t >= 2;
    case kBtFormCh0Pers: o.ch = 0; o.pers = 1; o.cap = 8; return t >= 2;
    case kBtFormCh16Pers: o.ch = 16; o.pers = 1; o.cap = 8; return t >= 2;
    default: return false;
  }
}
}  // namespace

void LatentVecchia::TestSetValues(const double* Bv, const double* Dinv, const double* W, const double* dw,
                                  const double* alt) {
  const int n = n_, m = m_;
  std::vector<double> hb((size_t)n * m, 0.);
  auto rows = [&](const double* src, double* dst) {
    for (int p = 0; p < n; ++p) {
      const int i = vo_[p], k = std::min(i, m);
      for (int r = 0; r < k; ++r) hb[(size_t)p * m + r] = src[(size_t)i * m + r];
    }
    HIP_CHECK(hipMemcpyAsync(dst, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice, s_));
    HIP_CHECK(hipStreamSynchronize(s_));
  };
  rows(Bv, d_Bv_.get());
  if (alt) rows(alt, d_dBv_.get());
  upload_rows(vo_, n, 1, Dinv, d_Dinv_.get(), s_);
  upload_rows(vo_, n, 1, W, d_W_.get(), s_);
  upload_rows(vo_, n, 1, dw, d_dw_.get(), s_);
  // the refresh of Eval, in its order
  pre_->Refresh(d_Bv_.get());
  launch_gather(tnnz_, d_tslot_.get(), d_Bv_.get(), d_tval_.get(), s_);
  if (seg2_n_ > 0) launch_gather(seg2_n_, d_seg_slot2_.get(), d_Bv_.get(), d_seg_val2_.get(), s_);
  sp_.tval_of = d_Bv_.get();
  launch_gather(n * m_, d_ell_slot_.get(), d_Bv_.get(), d_ell_val_.get(), s_);
  sp_.vals_of = d_Bv_.get();
  factor_ready_ = true;
  piv_ = false;
  SetDiag();
  HIP_CHECK(hipStreamSynchronize(s_));
  test_values_ = true;
  test_alt_ = alt != nullptr;
}

void LatentVecchia::TestInfo(int64_t* stats, int* vo) const {
  for (int k = 0; k < kTestLatentStats; ++k) stats[k] = stats_[k];
  stats[kLsK0] = pre_->K0();
  stats[kLsK] = pre_->K();
  stats[kLsLd0] = pre_->ld0();
  stats[kLsTailBt] = pre_->tail_levels_bt();
  stats[kLsTailLow] = pre_->tail_levels_lower();
  stats[kLsSegPasses] = pre_->segment_passes();
  stats[kLsLaunches] = pre_->launches();
  if (vo) std::copy(vo_.begin(), vo_.end(), vo);
}

void LatentVecchia::TestApply(int op, int form, int t, int unit, int use_alt, const double* X, const double* pre,
                              const double* scale, const double* W, const double* H, double* Y, double* Y2,
                              int* guard) {
  const char* fn = "GPB_TestLatentOpsApply";
  const int n = n_;
  const bool alt = use_alt != 0;
  // ---- everything that can be refused is refused before the first device call
  if (!test_values_) Fatal("%s: no values set (GPB_TestLatentOpsSetValues)", fn);
  if (t < 1 || t > 4096) Fatal("%s: t = %d", fn, t);
  if (X == nullptr || Y == nullptr || guard == nullptr) Fatal("%s: X, Y or guard_flag is NULL", fn);
  if ((W == nullptr) != (H == nullptr)) Fatal("%s: W and H go together", fn);
  if (alt && !test_alt_) Fatal("%s: use_alt_vals without alt_vals", fn);
  SpmvOptions so;
  const SpmvOptions* sel = nullptr;
  bool tiled = false;
  if (op == kLatentOpB) {
    if (pre || W) Fatal("%s: op %d takes no pre / W / H", fn, op);
    tiled = form == kBFormTiled;
    if (tiled) {
      if (t < 2 || !unit) Fatal("%s: form %d is not admitted by t = %d, unit = %d", fn, form, t, unit);
    } else if (form != 0) {
      if (!b_form(form, t, m_, alt, so))
        Fatal("%s: form %d is not admitted by op %d, t = %d, m = %d, use_alt_vals = %d", fn, form, op, t, m_, use_alt);
      sel = &so;
    }
  } else if (op == kLatentOpBt) {
    if (scale) Fatal("%s: op %d takes no scale", fn, op);
    tiled = form == kBtFormTiled;
    if (tiled) {
      if (t < 2 || !unit || pre || alt)
        Fatal("%s: form %d is not admitted by t = %d, unit = %d, pre, use_alt_vals = %d", fn, form, t, unit, use_alt);
    } else if (form != 0) {
      if (!bt_form(form, t, alt, so))
        Fatal("%s: form %d is not admitted by op %d, t = %d, use_alt_vals = %d", fn, form, op, t, use_alt);
      sel = &so;
    }
  } else if (op == kLatentOpA) {
    if (pre || scale || W || alt || !unit) Fatal("%s: op %d takes X alone", fn, op);
    if (form != 0 && form != 1) Fatal("%s: form %d is not admitted by op %d", fn, form, op);
    tiled = form == 1;
    if (tiled && t < 2) Fatal("%s: form %d is not admitted by t = %d", fn, form, t);
  } else if (op == kLatentOpPrecond) {
    if (pre || scale || W || alt || !unit) Fatal("%s: op %d takes X alone", fn, op);
    if (form != 0) Fatal("%s: form %d is not admitted by op %d", fn, form, op);
    if (Y2 == nullptr) Fatal("%s: op %d needs the second output", fn, op);
  } else {
    Fatal("%s: unknown op %d", fn, op);
  }

  // ---- device blocks: inputs, and outputs between guard bands, all NaN before the launch. The buffers stay
  // with the object while n t is unchanged, so a second application of op 3 replays the captured graph.
  const size_t nt = (size_t)n * t, padded = nt + 2 * kGuard;
  if (test_buf_[0].size() != padded) pre_->DropGraphs();   // captured launches hold the old addresses
  for (auto& b : test_buf_) b.alloc(padded);
  DevBuf<double> dpre, dscale, dW, dH;
  double* dX = test_buf_[0].get() + kGuard;
  double* dY = test_buf_[1].get() + kGuard;
  double* dY2 = test_buf_[2].get() + kGuard;
  double* dG = test_buf_[3].get() + kGuard;
  const std::vector<double> nanv(padded, std::numeric_limits<double>::quiet_NaN());
  for (int b = 1; b < 4; ++b)
    HIP_CHECK(hipMemcpyAsync(test_buf_[b].get(), nanv.data(), sizeof(double) * padded, hipMemcpyHostToDevice, s_));
  HIP_CHECK(hipStreamSynchronize(s_));
  upload_rows(vo_, n, t, X, dX, s_);
  if (pre) { dpre.alloc(n); upload_rows(vo_, n, 1, pre, dpre.get(), s_); }
  if (scale) { dscale.alloc(n); upload_rows(vo_, n, 1, scale, dscale.get(), s_); }
  if (W) {
    dW.alloc(n);
    dH.alloc(nt);
    upload_rows(vo_, n, 1, W, dW.get(), s_);
    upload_rows(vo_, n, t, H, dH.get(), s_);
  }
  const double* vals = alt ? d_dBv_.get() : d_Bv_.get();
  if (op == kLatentOpB) {
    if (tiled) launch_b_apply_tiled(sp_, tile_b_.op, vals, dX, t, dscale.get(), dY, s_);
    else launch_b_apply(sp_, vals, unit != 0, dX, t, dscale.get(), dY, s_, sel);
  } else if (op == kLatentOpBt) {
    if (tiled) launch_bt_apply_tiled(sp_, tile_bt_.op, d_tval_.get(), dX, t, dW.get(), dH.get(), dY, s_);
    else launch_bt_apply(sp_, vals, unit != 0, dX, t, dpre.get(), dW.get(), dH.get(), dY, s_, sel);
  } else if (op == kLatentOpA) {
    if (tiled) {
      launch_b_apply_tiled(sp_, tile_b_.op, d_Bv_.get(), dX, t, d_Dinv_.get(), dG, s_);
      launch_bt_apply_tiled(sp_, tile_bt_.op, d_tval_.get(), dG, t, d_W_.get(), dX, dY, s_);
    } else {
      ApplyA(dX, dY, dG, t);
    }
  } else {
    pre_->Apply(dX, dY, dY2, t);
  }
  HIP_CHECK(hipStreamSynchronize(s_));

  // ---- back to the host: payload to Vecchia order, guard bands compared with what was written
  std::vector<double> h(padded);
  int touched = 0;
  auto fetch = [&](const DevBuf<double>& buf, double* out, bool check) {
    HIP_CHECK(hipMemcpy(h.data(), buf.get(), sizeof(double) * padded, hipMemcpyDeviceToHost));
    if (check && (std::memcmp(h.data(), nanv.data(), sizeof(double) * kGuard) != 0 ||
                  std::memcmp(h.data() + kGuard + nt, nanv.data(), sizeof(double) * kGuard) != 0))
      touched = 1;
    if (out)
      for (int p = 0; p < n; ++p)
        std::memcpy(out + (size_t)vo_[p] * t, &h[kGuard + (size_t)p * t], sizeof(double) * t);
  };
  fetch(test_buf_[1], Y, true);
  fetch(test_buf_[2], op == kLatentOpPrecond ? Y2 : nullptr, op == kLatentOpPrecond);
  fetch(test_buf_[3], nullptr, op == kLatentOpA);
  *guard = touched;
}

void LatentVecchia::TestPcg(int t, int n_single, double delta, int pmax_single, int pmax_block, const double* RHS,
                            double* U, int* its, int* flags) {
  const char* fn = "GPB_TestLatentOpsPcg";
  if (!test_values_) Fatal("%s: no values set (GPB_TestLatentOpsSetValues)", fn);
  if (t < 1 || t > 1024 || n_single < 0 || n_single > t) Fatal("%s: t = %d, n_single = %d", fn, t, n_single);
  if (pmax_single < 1 || pmax_block < 1 || pmax_single > (1 << 20) || pmax_block > (1 << 20))
    Fatal("%s: pmax_single = %d, pmax_block = %d", fn, pmax_single, pmax_block);
  if (!(delta > 0.)) Fatal("%s: delta must be > 0", fn);
  if (RHS == nullptr || U == nullptr || its == nullptr || flags == nullptr) Fatal("%s: an argument is NULL", fn);
  const size_t nt = (size_t)n_ * t;
  Block& b = GetBlock(2, t, std::max(pmax_single, pmax_block));
  DevBuf<double> rhs(nt), u(nt);
  upload_rows(vo_, n_, t, RHS, rhs.get(), s_);
  const PcgResult r = Pcg(b, rhs.get(), u.get(), n_single, true, true, pmax_single, pmax_block, delta);
  HIP_CHECK(hipStreamSynchronize(s_));
  std::vector<double> h(nt);
  HIP_CHECK(hipMemcpy(h.data(), u.get(), sizeof(double) * nt, hipMemcpyDeviceToHost));
  for (int p = 0; p < n_; ++p) std::memcpy(U + (size_t)vo_[p] * t, &h[(size_t)p * t], sizeof(double) * t);
  its[0] = r.its_single;
  its[1] = r.its_block;
  flags[0] = r.nan ? 1 : 0;
  flags[1] = r.zero_rhs ? 1 : 0;
}

// The block-CG vector kernels on host arrays (no structure). Outputs between guard bands, NaN before the launch
// where the kernel writes every entry.
void test_latent_vector(int op, int n, int t, int np, int ia, int ib, double alpha, double beta,
                        const double* const* blocks, const double* sv0, const double* sv1, const int* act,
                        double* out0, double* out1, double* small_out, int* guard) {
  const char* fn = "GPB_TestLatentOpsVector";
  if (n < 1 || n > (1 << 22) || t < 1 || t > 1024) Fatal("%s: n = %d, t = %d", fn, n, t);
  if (guard == nullptr || blocks == nullptr) Fatal("%s: blocks or guard_flag is NULL", fn);
  auto need = [&](const void* p, const char* what) {
    if (p == nullptr) Fatal("%s: op %d needs %s", fn, op, what);
  };
  int nblocks = 0, nsmall = 0;
  switch (op) {
    case kVecColdots:
      if (np < 1 || np > 3) Fatal("%s: np = %d", fn, np);
      nblocks = 2 * np; nsmall = np * t; need(small_out, "small_out");
      break;
    case kVecCgUpdate: nblocks = 4; nsmall = t; need(sv0, "a"); need(out0, "U"); need(out1, "R"); need(small_out, "rr"); break;
    case kVecHUpdate: nblocks = 2; need(sv0, "b"); need(out0, "H"); break;
    case kVecAlpha: nsmall = 2 * t; need(sv0, "rz"); need(sv1, "hv"); need(small_out, "small_out"); break;
    case kVecBeta: nsmall = 3 * t; need(sv0, "rz_new"); need(sv1, "rz"); need(small_out, "small_out"); break;
    case kVecAxpby: nblocks = 2; need(out0, "Z"); break;
    case kVecCapMode: nblocks = 2; need(out0, "mnew"); break;
    case kVecPack:
      nblocks = 2; need(out0, "dst");
      if (np < 1 || ia < 0 || ib < 0 || ia + np > t || ib + np > t)
        Fatal("%s: pack_columns of %d columns from %d to %d in blocks of %d", fn, np, ia, ib, t);
      break;
    default: Fatal("%s: unknown op %d", fn, op);
  }
  for (int k = 0; k < nblocks; ++k) need(blocks[k], "its input blocks");
  const size_t nt = (size_t)n * t;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  // device copies; index 6 / 7: guarded outputs that start as NaN
  struct Guarded {
    DevBuf<double> buf;
    size_t len = 0;
    double* p() const { return buf.get() + kGuard; }
  };
  auto make = [&](Guarded& g, size_t len, const double* init) {
    g.len = len;
    g.buf.alloc(len + 2 * kGuard);
    std::vector<double> h(len + 2 * kGuard, nan);
    if (init) std::memcpy(h.data() + kGuard, init, sizeof(double) * len);
    HIP_CHECK(hipMemcpy(g.buf.get(), h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  };
  int touched = 0;
  auto fetch = [&](const Guarded& g, double* out) {
    std::vector<double> h(g.len + 2 * kGuard);
    HIP_CHECK(hipMemcpy(h.data(), g.buf.get(), sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < kGuard; ++k)
      if (!std::isnan(h[k]) || !std::isnan(h[kGuard + g.len + k])) touched = 1;
    std::memcpy(out, h.data() + kGuard, sizeof(double) * g.len);
  };
  DevBuf<double> in[6], s0, s1, partials;
  DevBuf<int> dact;
  for (int k = 0; k < nblocks; ++k) {
    in[k].alloc(nt);
    HIP_CHECK(hipMemcpy(in[k].get(), blocks[k], sizeof(double) * nt, hipMemcpyHostToDevice));
  }
  if (sv0) { s0.alloc(t); HIP_CHECK(hipMemcpy(s0.get(), sv0, sizeof(double) * t, hipMemcpyHostToDevice)); }
  if (sv1) { s1.alloc(t); HIP_CHECK(hipMemcpy(s1.get(), sv1, sizeof(double) * t, hipMemcpyHostToDevice)); }
  if (act) { dact.alloc(t); HIP_CHECK(hipMemcpy(dact.get(), act, sizeof(int) * t, hipMemcpyHostToDevice)); }
  partials.alloc((size_t)kMaxRedBlocks * 3 * t);
  Guarded g0, g1, gs;
  hipStream_t s = nullptr;
  if (nsmall > 0) make(gs, nsmall, nullptr);
  switch (op) {
    case kVecColdots: {
      const double* A[3] = {in[0].get(), in[2].get(), in[4].get()};
      const double* Bm[3] = {in[1].get(), in[3].get(), in[5].get()};
      launch_coldots(n, t, np, A, Bm, partials.get(), gs.p(), s);
      break;
    }
    case kVecCgUpdate:
      make(g0, nt, blocks[2]);
      make(g1, nt, blocks[3]);
      launch_cg_update(n, t, s0.get(), in[0].get(), in[1].get(), g0.p(), g1.p(), partials.get(), gs.p(), s);
      break;
    case kVecHUpdate:
      make(g0, nt, blocks[1]);
      launch_h_update(n, t, s0.get(), in[0].get(), g0.p(), s);
      break;
    case kVecAlpha:
      launch_cg_alpha(t, s0.get(), s1.get(), dact.get(), gs.p(), gs.p() + t, s);
      break;
    case kVecBeta:
      HIP_CHECK(hipMemcpy(gs.p() + 2 * t, sv1, sizeof(double) * t, hipMemcpyHostToDevice));
      launch_cg_beta(t, s0.get(), gs.p() + 2 * t, dact.get(), gs.p(), gs.p() + t, s);
      break;
    case kVecAxpby:
      make(g0, nt, nullptr);
      launch_axpby(nt, alpha, in[0].get(), beta, in[1].get(), g0.p(), s);
      break;
    case kVecCapMode:
      make(g0, nt, blocks[1]);
      launch_cap_mode_change(nt, in[0].get(), g0.p(), s);
      break;
    case kVecPack:
      make(g0, nt, blocks[1]);
      launch_pack_columns(n, np, in[0].get(), t, ia, g0.p(), t, ib, s);
      break;
  }
  HIP_CHECK(hipDeviceSynchronize());
  if (g0.len) fetch(g0, out0);
  if (g1.len) fetch(g1, out1);
  if (gs.len) fetch(gs, small_out);
  *guard = touched;
}

// ---------------------------------------------------------------- the C ABI's object
void test_latent_check_graph(const char* fn, int n, int m, const int* nbr, int64_t nbr_len, int d, const double* X,
                             int64_t x_len) {
  if (n < 1 || m < 1 || d < 1 || n >= (1 << 24) || m > 4096) Fatal("%s: n = %d, m = %d, d = %d", fn, n, m, d);
  if (nbr == nullptr || X == nullptr) Fatal("%s: nbr or X is NULL", fn);
  if (nbr_len != (int64_t)n * m || x_len != (int64_t)n * d)
    Fatal("%s: nbr / X hold %lld / %lld entries, n m = %lld, n d = %lld", fn, (long long)nbr_len, (long long)x_len,
          (long long)n * m, (long long)n * d);
  std::vector<int> seen(n, -1);
  for (int i = 0; i < n; ++i) {
    const int k = std::min(i, m);
    for (int r = 0; r < k; ++r) {
      const int j = nbr[(size_t)i * m + r];
      if (j < 0 || j >= i) Fatal("%s: nbr[%d][%d] = %d is not an earlier row", fn, i, r, j);
      if (seen[j] == i) Fatal("%s: nbr[%d] names row %d twice", fn, i, j);
      seen[j] = i;
    }
  }
  for (int64_t k = 0; k < x_len; ++k)
    if (!std::isfinite(X[k])) Fatal("%s: X[%lld] is not finite", fn, (long long)k);
}

LatentOptions test_latent_options(const char* fn, const int64_t* opts, int n) {
  LatentOptions o;
  if (opts == nullptr) return o;
  auto val = [&](int k, int64_t lo, int64_t hi, const char* name) {
    if (opts[k] < 0) return -1;
    if (opts[k] < lo || opts[k] > hi) Fatal("%s: opts %s = %lld, not in [%lld, %lld]", fn, name, (long long)opts[k],
                                            (long long)lo, (long long)hi);
    return (int)opts[k];
  };
  o.relabel = val(0, 0, 1, "relabel");
  o.dense_rows = val(1, 0, 1 << 30, "dense_rows");
  o.head_rows = val(2, 0, 1 << 30, "head_rows");
  o.vadu.tail_merge = val(3, 1, 64, "tail_merge");
  o.vadu.seg_form = val(4, 0, 1, "seg_form");
  o.vadu.tail_order = val(5, 0, 1, "tail_order");
  o.vadu.tail_form = val(6, 0, 1, "tail_form");
  o.vadu.tail_w = val(7, 1, 64, "tail_w");
  o.vadu.no_graph = val(8, 0, 1, "no_graph");
  (void)n;
  return o;
}

TestLatentOps::TestLatentOps(int n, int m, const int* nbr, int d, const double* X, const LatentOptions& opt)
    : n_(n), m_(m) {
  HIP_CHECK(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
  X_.alloc((size_t)n * d);
  HIP_CHECK(hipMemcpy(X_.get(), X, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice));
  lv_.reset(new LatentVecchia(n, d, m, X_.get(), nbr, s_, opt));
}

TestLatentOps::~TestLatentOps() {
  (void)hipDeviceSynchronize();
  lv_.reset();
  if (s_) (void)hipStreamDestroy(s_);
}

}  // namespace gpb_amd
