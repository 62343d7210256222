// Test entries of the grouped random-effects engine (GPB_TestGrouped*, include/gpboost_amd.h; grouped_test.h): the
// launch functions of grouped_kernels.h on a GroupedRE's own structure and chunk plans, GroupedRE::Precond and
// SolveVec, and the segmented sums and gradient kernels of GroupedLaplace, on host arrays. Every extent and index
// is checked on the host before any device call; outputs and scratch (the chunk partials included) sit between
// guard bands and start as NaN, so a write out of range or an entry left unwritten is seen without a fault; the
// ld - M padding of every dense input holds NaN.
#include "grouped_test.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "common.h"
#include "grouped_kernels.h"
#include "latent_kernels.h"
#include "lik_test.h"

namespace gpb_amd {

namespace {
constexpr size_t kGuard = 64;   // guard doubles on both sides of an output block
constexpr int kMaxN = 1 << 22;
constexpr int kMaxT = 1024;
constexpr int kMaxDenseM = 4096;
const double kNaN = std::numeric_limits<double>::quiet_NaN();

// a device block of `len` doubles between guard bands, `fill` before the launch
struct Guarded {
  DevBuf<double> buf;
  size_t len = 0;
  double* p() const { return buf.get() + kGuard; }
  void make(size_t n, double fill = kNaN) {
    len = n;
    buf.alloc(n + 2 * kGuard);
    std::vector<double> h(n + 2 * kGuard, kNaN);
    std::fill(h.begin() + kGuard, h.begin() + kGuard + n, fill);
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

const double* upload(DevBuf<double>& dst, const double* src, size_t len) {
  dst.alloc(std::max<size_t>(len, 1));
  if (len) HIP_CHECK(hipMemcpy(dst.get(), src, sizeof(double) * len, hipMemcpyHostToDevice));
  return dst.get();
}

// host M x M column-major -> device M columns of ld doubles, the padding NaN
const double* upload_dense(DevBuf<double>& dst, const double* src, int M, int ld) {
  std::vector<double> h((size_t)M * ld, kNaN);
  for (int c = 0; c < M; ++c) std::memcpy(&h[(size_t)c * ld], src + (size_t)c * M, sizeof(double) * M);
  dst.alloc(h.size());
  HIP_CHECK(hipMemcpy(dst.get(), h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  return dst.get();
}

template <typename T>
std::vector<T> download(const T* src, size_t len) {
  std::vector<T> h(len);
  if (len) HIP_CHECK(hipMemcpy(h.data(), src, sizeof(T) * len, hipMemcpyDeviceToHost));
  return h;
}

void check_arrays(const char* fn, int op, const void* const* p, const int64_t* len, int n, const int64_t* want, int n_want,
                  const char* what) {
  if (n != n_want) Fatal("%s: op %d takes %d %s arrays, not %d", fn, op, n_want, what, n);
  if (n > 0 && (p == nullptr || len == nullptr)) Fatal("%s: the %s arrays or their lengths are NULL", fn, what);
  for (int k = 0; k < n; ++k) {
    if (len[k] != want[k])
      Fatal("%s: op %d, %s array %d holds %lld entries, not %lld", fn, op, what, k, (long long)len[k], (long long)want[k]);
    if (want[k] > 0 && p[k] == nullptr) Fatal("%s: op %d, %s array %d is NULL", fn, op, what, k);
  }
}
}  // namespace

// ---- the GroupedRE half of the friend
GroupedOp GroupedTestAccess::Op(GroupedRE& re, int t) { return re.Op(t); }
void GroupedTestAccess::PlanQ(GroupedRE& re, int tc, std::vector<int>& lower_q, std::vector<int>& upper_q) {
  const GroupedRE::ChunkPlan& pl = re.Plan(tc);
  lower_q = pl.lower_q;
  upper_q = pl.upper_q;
}
void GroupedTestAccess::Precond(GroupedRE& re, const double* R, double* Z, double* S, int t) { re.Precond(R, Z, S, t); }
const std::vector<int>& GroupedTestAccess::Cum(const GroupedRE& re) { return re.cum_; }
const int* GroupedTestAccess::ObsPtr(const GroupedRE& re) { return re.d_obs_ptr_.get(); }
const int* GroupedTestAccess::Obs(const GroupedRE& re) { return re.d_obs_.get(); }
const double* GroupedTestAccess::ObsW(const GroupedRE& re) { return re.weighted_ ? re.d_obs_w_.get() : nullptr; }
const int* GroupedTestAccess::DevCum(const GroupedRE& re) { return re.d_cum_.get(); }
const int* GroupedTestAccess::Split(const GroupedRE& re) { return re.d_split_.get(); }
const double* GroupedTestAccess::Val(const GroupedRE& re) { return re.d_val_.get(); }
const double* GroupedTestAccess::Cnt(const GroupedRE& re) { return re.d_cnt_.get(); }

GroupedTest::GroupedTest(int n, int K, const int32_t* levels, const double* weights, const int32_t* has_weight)
    : n_(n), K_(K) {
  levels_.resize(K);
  for (int k = 0; k < K; ++k) levels_[k].assign(levels + (size_t)k * n, levels + (size_t)(k + 1) * n);
  if (weights != nullptr) {
    weights_.resize(K);
    wptr_.assign(K, nullptr);
    for (int k = 0; k < K; ++k) {
      if (has_weight != nullptr && has_weight[k] == 0) continue;
      weights_[k].assign(weights + (size_t)k * n, weights + (size_t)(k + 1) * n);
      wptr_[k] = weights_[k].data();
    }
  }
  HIP_CHECK(hipStreamCreate(&s_));
  re_.reset(new GroupedRE(n, levels_, s_, wptr_));
}

GroupedTest::~GroupedTest() {
  glp_.reset();
  re_.reset();
  if (s_) (void)hipStreamDestroy(s_);
}

GroupedLaplace& GroupedTest::Laplace() {
  if (K_ > kGlpMaxK) Fatal("GPB_TestGrouped: the Laplace kernels take at most %d effects", kGlpMaxK);
  if (!glp_) glp_.reset(new GroupedLaplace(re_.get(), levels_, kLikPoisson, wptr_));
  return *glp_;
}

void GroupedTest::Info(int t, int64_t* stats, int64_t stats_len, int32_t* ints, int64_t ints_len, double* dbls,
                       int64_t dbls_len) {
  const char* fn = "GPB_TestGroupedInfo";
  if (t < 1 || t > kMaxT) Fatal("%s: t = %d is not in 1..%d", fn, t, kMaxT);
  if (stats == nullptr || stats_len != kGroupedInfoStats)
    Fatal("%s: stats holds %lld entries, not %d", fn, (long long)stats_len, kGroupedInfoStats);
  const GroupedRE::View v = re_->view();
  const int M = v.M, K = v.K, nnz = v.nnz;
  const GroupedOp op = GroupedTestAccess::Op(*re_, t);
  const GreChunks* ch[3] = {&op.full, &op.lower, &op.upper};
  int64_t total = (int64_t)(K + 1) + (M + 1) + M + nnz + (M + 1) + (int64_t)n_ * K + 2 * (K + 1);
  for (int kind = 0; kind < 3; ++kind) total += 2 * (int64_t)ch[kind]->n + (M + 1);
  int seg[4] = {0, 0, 0, 0};
  if (K <= kGlpMaxK) GroupedTestAccess::SegCounts(Laplace(), seg);
  const int64_t st[kGroupedInfoStats] = {M, nnz, n_, K, op.tc, gre_chunk_len(op.tc), op.full.n, op.lower.n, op.upper.n,
                                         total, seg[0], seg[1], seg[2], seg[3]};
  std::memcpy(stats, st, sizeof(st));
  if (ints == nullptr && dbls == nullptr) return;
  if (ints == nullptr || dbls == nullptr || ints_len != total || dbls_len != (int64_t)nnz + M)
    Fatal("%s: ints / dbls hold %lld / %lld entries, not %lld / %lld", fn, (long long)ints_len, (long long)dbls_len,
          (long long)total, (long long)nnz + M);
  int32_t* w = ints;
  auto put = [&](const std::vector<int>& a) {
    for (int x : a) *w++ = x;
  };
  put(GroupedTestAccess::Cum(*re_));
  put(download(op.rowptr, M + 1));
  put(download(GroupedTestAccess::Split(*re_), M));
  put(download(op.col, nnz));
  put(download(GroupedTestAccess::ObsPtr(*re_), M + 1));
  put(download(GroupedTestAccess::Obs(*re_), (size_t)n_ * K));
  for (int kind = 0; kind < 3; ++kind) {
    put(download(ch[kind]->e0, ch[kind]->n));
    put(download(ch[kind]->e1, ch[kind]->n));
    put(download(ch[kind]->ptr, M + 1));
  }
  std::vector<int> lq, uq;
  GroupedTestAccess::PlanQ(*re_, op.tc, lq, uq);
  put(lq);
  put(uq);
  if (w - ints != total) Fatal("%s: internal error, %lld of %lld entries written", fn, (long long)(w - ints), (long long)total);
  const std::vector<double> val = download(GroupedTestAccess::Val(*re_), nnz);
  const std::vector<double> cnt = download(GroupedTestAccess::Cnt(*re_), M);
  std::copy(val.begin(), val.end(), dbls);
  std::copy(cnt.begin(), cnt.end(), dbls + nnz);
}

void GroupedTest::Apply(int op_id, int t, const double* val, const double* dg, const double* dis, const double* In,
                        double* Out0, double* Out1, int64_t block_len, int* guard) {
  const char* fn = "GPB_TestGroupedApply";
  if (op_id < 0 || op_id >= kNumGroupedApplyOps) Fatal("%s: unknown op %d", fn, op_id);
  if (t < 1 || t > kMaxT) Fatal("%s: t = %d is not in 1..%d", fn, t, kMaxT);
  const GroupedRE::View v = re_->view();
  const int M = v.M, nnz = v.nnz;
  if (block_len != (int64_t)M * t) Fatal("%s: the blocks hold %lld entries, not M t = %lld", fn, (long long)block_len, (long long)M * t);
  const bool two = op_id == kGreSsor || op_id == kGrePrecond;
  const bool needs_dis = op_id == kGreLdsMult || two;
  if (dg == nullptr || In == nullptr || Out0 == nullptr || guard == nullptr) Fatal("%s: dg, In, Out0 or guard is NULL", fn);
  if (needs_dis != (dis != nullptr)) Fatal("%s: op %d %s dis", fn, op_id, needs_dis ? "needs" : "takes no");
  if (two != (Out1 != nullptr)) Fatal("%s: op %d %s Out1", fn, op_id, two ? "needs" : "takes no");
  if (re_->K() < 2) Fatal("%s: the products need at least two effects", fn);

  DevBuf<double> dval, ddg, ddis, din;
  if (val != nullptr) upload(dval, val, nnz);
  upload(ddg, dg, M);
  if (dis != nullptr) upload(ddis, dis, M);
  upload(din, In, (size_t)block_len);
  Guarded g0, g1, gP;
  g0.make((size_t)block_len);
  if (two) g1.make((size_t)block_len);
  if (op_id == kGrePrecond) {   // the production wiring: the engine's own operator slots, plans and partials
    re_->SetOperator(val != nullptr ? dval.get() : nullptr, nullptr, ddg.get(), ddis.get());
    GroupedTestAccess::Precond(*re_, din.get(), g1.p(), g0.p(), t);
    HIP_CHECK(hipStreamSynchronize(s_));
    re_->SetOperator(nullptr, nullptr, nullptr, nullptr);
  } else {
    GroupedOp op = GroupedTestAccess::Op(*re_, t);
    if (val != nullptr) op.val = dval.get();
    gP.make((size_t)std::max(1, std::max(op.full.n, std::max(op.lower.n, op.upper.n))) * t);
    op.P = gP.p();
    switch (op_id) {
      case kGreApply: launch_gre_apply(op, ddg.get(), din.get(), g0.p(), t, s_); break;
      case kGreApplyLower: launch_gre_apply_lower(op, ddg.get(), din.get(), g0.p(), t, s_); break;
      case kGreLdsMult: launch_gre_lds_mult(op, ddg.get(), ddis.get(), din.get(), g0.p(), t, s_); break;
      case kGreUpper: launch_gre_upper(op, ddg.get(), din.get(), g0.p(), t, s_); break;
      default: {
        std::vector<int> lq, uq;
        GroupedTestAccess::PlanQ(*re_, op.tc, lq, uq);
        launch_gre_ssor(op, GroupedTestAccess::Cum(*re_), lq, uq, ddg.get(), ddis.get(), din.get(), g0.p(), g1.p(), t, s_);
      }
    }
    HIP_CHECK(hipStreamSynchronize(s_));
  }
  bool touched = g0.fetch(Out0);
  if (two) touched = g1.fetch(Out1) || touched;
  if (gP.len) touched = gP.fetch(nullptr) || touched;
  *guard = touched ? 1 : 0;
}

void GroupedTest::Small(int op, const double* const* in, const int64_t* in_len, int n_in, double* const* out,
                        const int64_t* out_len, int n_out, int* guard) {
  const char* fn = "GPB_TestGroupedSmall";
  if (op < 0 || op >= kNumGroupedSmallOps) Fatal("%s: unknown op %d", fn, op);
  if (guard == nullptr) Fatal("%s: guard is NULL", fn);
  const GroupedRE::View v = re_->view();
  const int M = v.M, K = v.K;
  int64_t wi[kGroupedMaxArrays] = {0}, wo[kGroupedMaxArrays] = {0};
  int ni = 0, no = 0;
  const int64_t len0 = (n_in > 0 && in_len != nullptr) ? in_len[0] : 0;
  switch (op) {
    case kGreZty: ni = 1; wi[0] = n_; no = 1; wo[0] = M; break;
    case kGreDiag: ni = 2; wi[0] = M; wi[1] = K; no = 3; wo[0] = M; wo[1] = M; wo[2] = 2 * K; break;
    case kGreSingle:
      if (len0 < 1 || len0 > kMaxN) Fatal("%s: op %d on %lld rows", fn, op, (long long)len0);
      ni = 3; wi[0] = wi[1] = wi[2] = len0; no = 2; wo[0] = len0; wo[1] = 2;
      break;
    default:
      if (len0 < 0 || len0 > ((int64_t)1 << 26)) Fatal("%s: op %d on %lld entries", fn, op, (long long)len0);
      ni = 2; wi[0] = wi[1] = len0; no = 1; wo[0] = len0;
  }
  check_arrays(fn, op, reinterpret_cast<const void* const*>(in), in_len, n_in, wi, ni, "input");
  check_arrays(fn, op, reinterpret_cast<const void* const*>(out), out_len, n_out, wo, no, "output");
  if (op == kGreDiag)
    for (int k = 0; k < K; ++k)
      if (!(in[1][k] > 0.) || !std::isfinite(in[1][k])) Fatal("%s: tau[%d] must be finite and > 0", fn, k);
  DevBuf<double> d[kGroupedMaxArrays];
  Guarded g[kGroupedMaxArrays];
  for (int k = 0; k < ni; ++k) upload(d[k], in[k], (size_t)wi[k]);
  for (int k = 0; k < no; ++k) g[k].make((size_t)wo[k]);
  switch (op) {
    case kGreZty:
      launch_gre_zty(M, GroupedTestAccess::ObsPtr(*re_), GroupedTestAccess::Obs(*re_), GroupedTestAccess::ObsW(*re_),
                     d[0].get(), g[0].p(), s_);
      break;
    case kGreDiag:
      launch_gre_diag(K, GroupedTestAccess::DevCum(*re_), d[0].get(), d[1].get(), g[0].p(), g[1].p(), g[2].p(), s_);
      break;
    case kGreSingle: launch_gre_single((int)len0, d[0].get(), d[1].get(), d[2].get(), g[0].p(), g[1].p(), s_); break;
    default: launch_gre_residual((size_t)len0, d[0].get(), d[1].get(), g[0].p(), s_);
  }
  HIP_CHECK(hipStreamSynchronize(s_));
  bool touched = false;
  for (int k = 0; k < no; ++k) touched = g[k].fetch(out[k]) || touched;
  *guard = touched ? 1 : 0;
}

void GroupedTest::Dense(int op, int ld, int np, const int32_t* idx, const double* const* in, const int64_t* in_len,
                        int n_in, double* const* out, const int64_t* out_len, int n_out, int* guard) {
  const char* fn = "GPB_TestGroupedDense";
  if (op < 0 || op >= kNumGroupedDenseOps) Fatal("%s: unknown op %d", fn, op);
  if (guard == nullptr) Fatal("%s: guard is NULL", fn);
  const GroupedRE::View v = re_->view();
  const int M = v.M, K = v.K, nnz = v.nnz;
  if (M > kMaxDenseM) Fatal("%s: M = %d exceeds %d", fn, M, kMaxDenseM);
  if (ld < M || ld > 2 * kMaxDenseM) Fatal("%s: ld = %d with M = %d", fn, ld, M);
  const int64_t mm = (int64_t)M * M;
  const bool pred = op == kGrePredE || op == kGrePredVar;
  if (pred) {
    if (np < 1 || np > 4096 || idx == nullptr) Fatal("%s: np = %d points (1..4096) with idx", fn, np);
    for (int64_t k = 0; k < (int64_t)np * K; ++k)
      if (idx[k] < -1 || idx[k] >= M) Fatal("%s: idx[%lld] = %d is not in -1..%d", fn, (long long)k, idx[k], M - 1);
  }
  int64_t wi[kGroupedMaxArrays] = {0}, wo[kGroupedMaxArrays] = {0};
  int ni = 0, no = 0;
  switch (op) {
    case kGreDenseBuild:
      ni = 2; wi[0] = (n_in > 0 && in_len != nullptr && in_len[0] == 0) ? 0 : nnz; wi[1] = M;
      no = 1; wo[0] = (int64_t)ld * M;
      break;
    case kGreInvDiag: ni = 1; wi[0] = mm; no = 1; wo[0] = M; break;
    case kGrePredE: ni = 1; wi[0] = mm; no = 1; wo[0] = (int64_t)ld * np; break;
    case kGrePredVar: ni = 1; wi[0] = mm; no = 1; wo[0] = np; break;
    default: ni = 2; wi[0] = M; wi[1] = mm; no = 2; wo[0] = (int64_t)M * K; wo[1] = M;
  }
  const bool pred_wt = pred && re_->weighted();   // one more input: wt (np K)
  if (pred_wt) {
    ni = 2;
    wi[1] = (int64_t)np * K;
  }
  check_arrays(fn, op, reinterpret_cast<const void* const*>(in), in_len, n_in, wi, ni, "input");
  check_arrays(fn, op, reinterpret_cast<const void* const*>(out), out_len, n_out, wo, no, "output");
  DevBuf<double> d[2];
  const double* dwt = pred_wt ? upload(d[1], in[1], (size_t)np * K) : nullptr;
  DevBuf<int> didx;
  Guarded g[2];
  g[0].make((size_t)wo[0], op == kGreDenseBuild ? 0. : kNaN);   // the build writes into a zero-filled matrix
  if (no > 1) g[1].make((size_t)wo[1]);
  if (pred) {
    didx.alloc((size_t)np * K);
    HIP_CHECK(hipMemcpy(didx.get(), idx, sizeof(int) * (size_t)np * K, hipMemcpyHostToDevice));
  }
  switch (op) {
    case kGreDenseBuild: {
      const GroupedOp gop = GroupedTestAccess::Op(*re_, 1);
      const double* dv = wi[0] ? upload(d[0], in[0], nnz) : GroupedTestAccess::Val(*re_);
      launch_gre_dense_build(M, ld, gop.rowptr, gop.col, dv, upload(d[1], in[1], M), g[0].p(), s_);
      break;
    }
    case kGreInvDiag: launch_gre_inv_diag(M, ld, upload_dense(d[0], in[0], M, ld), g[0].p(), s_); break;
    case kGrePredE:
      launch_gre_pred_cols(M, ld, K, np, didx.get(), dwt, upload_dense(d[0], in[0], M, ld), g[0].p(), nullptr, s_);
      break;
    case kGrePredVar:
      launch_gre_pred_cols(M, ld, K, np, didx.get(), dwt, upload_dense(d[0], in[0], M, ld), nullptr, g[0].p(), s_);
      break;
    default:
      launch_gre_fisher_cols(M, ld, K, GroupedTestAccess::DevCum(*re_), upload(d[0], in[0], M),
                             upload_dense(d[1], in[1], M, ld), g[0].p(), g[1].p(), s_);
  }
  HIP_CHECK(hipStreamSynchronize(s_));
  bool touched = false;
  for (int k = 0; k < no; ++k) touched = g[k].fetch(out[k]) || touched;
  *guard = touched ? 1 : 0;
}

void GroupedTest::Solve(const double* val, const double* cnt, const double* D, const double* dis, const double* rhs,
                        int warm, const double* u0, int pmax, double delta, double* u, int* its, int* guard) {
  const char* fn = "GPB_TestGroupedSolve";
  const GroupedRE::View v = re_->view();
  const int M = v.M, nnz = v.nnz;
  if (re_->K() < 2) Fatal("%s: the solve needs at least two effects", fn);
  if (D == nullptr || dis == nullptr || rhs == nullptr || u == nullptr || its == nullptr || guard == nullptr)
    Fatal("%s: D, dis, rhs, u, its or guard is NULL", fn);
  if ((warm != 0 && warm != 1) || (warm == 1) != (u0 != nullptr)) Fatal("%s: warm = %d %s u0", fn, warm, u0 ? "with" : "without");
  if (pmax < 1 || pmax > 100000 || !(delta > 0.) || !std::isfinite(delta)) Fatal("%s: pmax = %d, delta = %g", fn, pmax, delta);
  for (int r = 0; r < M; ++r)
    if (!(D[r] > 0.) || !(dis[r] > 0.) || !std::isfinite(D[r]) || !std::isfinite(dis[r]))
      Fatal("%s: D[%d] and dis[%d] must be finite and > 0", fn, r, r);
  DevBuf<double> dval, dcnt, dD, ddis, drhs;
  if (val != nullptr) upload(dval, val, nnz);
  if (cnt != nullptr) upload(dcnt, cnt, M);
  upload(dD, D, M);
  upload(ddis, dis, M);
  upload(drhs, rhs, M);
  Guarded gu;
  gu.make(M);
  if (warm) HIP_CHECK(hipMemcpy(gu.p(), u0, sizeof(double) * M, hipMemcpyHostToDevice));
  re_->SetOperator(val != nullptr ? dval.get() : nullptr, cnt != nullptr ? dcnt.get() : nullptr, dD.get(), ddis.get());
  struct Reset {
    GroupedRE* re;
    ~Reset() { re->SetOperator(nullptr, nullptr, nullptr, nullptr); }
  } reset{re_.get()};
  *its = re_->SolveVec(drhs.get(), gu.p(), pmax, delta, warm != 0);
  HIP_CHECK(hipStreamSynchronize(s_));
  *guard = gu.fetch(u) ? 1 : 0;
}

void GroupedTest::LaplaceOps(int op, int sub, int t, int ld, double alpha, const double* const* in, const int64_t* in_len,
                             int n_in, double* const* out, const int64_t* out_len, int n_out, int* guard) {
  const char* fn = "GPB_TestGroupedLaplaceOps";
  if (op < 0 || op >= kNumGroupedLaplaceOps) Fatal("%s: unknown op %d", fn, op);
  if (guard == nullptr) Fatal("%s: guard is NULL", fn);
  const GroupedRE::View v = re_->view();
  const int M = v.M, K = v.K, nnz = v.nnz, n = n_;
  const int64_t mm = (int64_t)M * M;
  int64_t wi[kGroupedMaxArrays] = {0}, wo[kGroupedMaxArrays] = {0};
  int ni = 0, no = 0;
  const bool flag = sub != 0;
  switch (op) {
    case kGlpAssemble:
      if (sub != 0 && sub != 1) Fatal("%s: diag_only = %d", fn, sub);
      ni = 1; wi[0] = n; no = 1; wo[0] = flag ? M : (int64_t)M + nnz;
      break;
    case kGlpQ:
      if (sub != 0 && sub != 1) Fatal("%s: aux = %d", fn, sub);
      if (K > 1 && (M > kMaxDenseM || ld < M || ld > 2 * kMaxDenseM)) Fatal("%s: M = %d, ld = %d", fn, M, ld);
      ni = 5; wi[0] = K > 1 ? mm : 0; wi[1] = M; wi[2] = wi[3] = n; wi[4] = flag ? n : 0;
      no = 2; wo[0] = n; wo[1] = K + (flag ? 1 : 0);
      break;
    case kGlpRowTrace:
      if (t < 1 || t > kMaxT) Fatal("%s: t = %d is not in 1..%d", fn, t, kMaxT);
      ni = 3; wi[0] = wi[1] = (int64_t)M * t; wi[2] = n; no = 1; wo[0] = n;
      break;
    case kGlpGradF: ni = 4; wi[0] = wi[1] = wi[2] = n; wi[3] = M; no = 1; wo[0] = n; break;
    case kGlpVec:
      if (sub < 0 || sub > 4) Fatal("%s: form = %d", fn, sub);
      ni = 3; wi[0] = K; wi[1] = M; wi[2] = (sub == 1 || sub == 2 || sub == 3) ? M : 0; no = 1; wo[0] = M;
      break;
    default:
      if (sub < 0 || sub > 3) Fatal("%s: mode = %d", fn, sub);
      ni = 3; wi[0] = K; wi[1] = M; wi[2] = (sub == 0 || sub == 3) ? M : 0; no = 1; wo[0] = K;
  }
  check_arrays(fn, op, reinterpret_cast<const void* const*>(in), in_len, n_in, wi, ni, "input");
  check_arrays(fn, op, reinterpret_cast<const void* const*>(out), out_len, n_out, wo, no, "output");
  if (op == kGlpVec || op == kGlpEffectDots)
    for (int k = 0; k < K; ++k)
      if (!(in[0][k] > 0.) || !std::isfinite(in[0][k])) Fatal("%s: sigma2[%d] must be finite and > 0", fn, k);
  GroupedLaplace& glp = Laplace();
  const int* glev = GroupedTestAccess::Glev(glp);
  const double* zw = GroupedTestAccess::Zw(glp);
  DevBuf<double> d[kGroupedMaxArrays];
  const double* p[kGroupedMaxArrays] = {nullptr};
  for (int k = 0; k < ni; ++k) {
    if (wi[k] == 0) continue;
    const bool host_only = (op == kGlpVec || op == kGlpEffectDots) && k == 0;
    if (host_only) continue;
    p[k] = (op == kGlpQ && k == 0) ? upload_dense(d[k], in[k], M, ld) : upload(d[k], in[k], (size_t)wi[k]);
  }
  Guarded g[2], gpart;
  for (int k = 0; k < no; ++k) g[k].make((size_t)wo[k]);
  switch (op) {
    case kGlpAssemble: GroupedTestAccess::Assemble(glp, p[0], g[0].p(), flag); break;
    case kGlpQ:
      gpart.make((size_t)(K + 1) * test_glp_blocks(n));
      test_glp_q(n, K, glev, zw, p[0], ld, p[1], p[2], p[3], p[4], flag, g[0].p(), gpart.p(), g[1].p(), s_);
      break;
    case kGlpRowTrace: test_glp_row_trace(n, K, t, glev, zw, p[0], p[1], p[2], g[0].p(), s_); break;
    case kGlpGradF: test_glp_grad_f(n, K, glev, zw, p[0], p[1], p[2], p[3], g[0].p(), s_); break;
    case kGlpVec: test_glp_vec(sub, v, in[0], alpha, p[1], p[2], g[0].p(), s_); break;
    default: test_glp_effect_dots(sub, v, in[0], p[1], p[2], g[0].p(), s_);
  }
  HIP_CHECK(hipStreamSynchronize(s_));
  bool touched = false;
  for (int k = 0; k < no; ++k) touched = g[k].fetch(out[k]) || touched;
  // the partials of glp_q_kernel: K (+ 1 with aux) columns of the block count are written, the rest stays NaN
  if (gpart.len) touched = gpart.fetch(nullptr) || touched;
  *guard = touched ? 1 : 0;
}

}  // namespace gpb_amd
