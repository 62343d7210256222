// Vecchia neighbour search on the GPU.
//
// Reference replaced: find_nearest_neighbors_Vecchia_fast / _fast_internal
// (Vecchia_utils.cpp:732-1058; neighbour lists by ascending squared distance, insertion sort
// with stable ties, utils.h:245-257). The reference sweeps, for row i, the points in the order
// of their coordinate sums outward from i's position (one step down, one step up), skips
// candidates that are not earlier than i, stops a direction once (sum_c - sum_i)^2 > d * r_k^2
// and keeps the m best by insertion. That walk is serial per row but independent across rows:
// here one thread runs it for one row, with the same candidate order, the same fp64
// operations (contraction into FMA disabled, so products and sums round exactly as on the
// host) and the same insertion, so the lists are bit-identical to the host search
// (vecchia_host.cpp) and to the reference — including ties. The host computes the coordinate
// sums and the std::sort sweep order once (same code as vecchia_host.cpp).
//
// m <= 64: per-thread best lists live in LDS, slot-major ([k][thread]) so a wave's accesses to slot k
// are consecutive words. 65 <= m <= 128: one wave per row with the list in registers (knn_wide_kernel
// below). Rows i <= m take all earlier points in index order (host side).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>
#include <vector>

#include "common.h"
#include "vecchia_host.h"

#pragma clang fp contract(off)

namespace gpb_amd {
namespace {

constexpr int kKnnThreads = 64;
constexpr int kKnnMaxM = 64;

__global__ void __launch_bounds__(kKnnThreads) knn_kernel(const double* __restrict__ x,
                                                         const double* __restrict__ csum,
                                                         const int* __restrict__ order,
                                                         const int* __restrict__ pos, int n, int d, int m,
                                                         int r0, int r1, int last_cand, int* __restrict__ out) {
  __shared__ double bd_s[kKnnMaxM * kKnnThreads];
  __shared__ int bi_s[kKnnMaxM * kKnnThreads];
  const int tid = threadIdx.x;
  double* bd = bd_s + tid;   // slot k at bd[k * kKnnThreads]
  int* bi = bi_s + tid;
  const int i = r0 + blockIdx.x * kKnnThreads + tid;
  if (i >= r1 || i <= m) return;   // rows i <= m: all earlier points (host)
  for (int k = 0; k < m; ++k) {
    bd[k * kKnnThreads] = INFINITY;
    bi[k * kKnnThreads] = 0;
  }
  double xi[3];
  for (int q = 0; q < d; ++q) xi[q] = x[(size_t)i * d + q];
  const double si = csum[i];
  const double dd = (double)d;
  bool go_down = true, go_up = true;
  int lo = pos[i], hi = pos[i];
  double worst = INFINITY;   // bd[m - 1]
  auto visit = [&](int cand, bool& alive) {
    if (cand >= i || cand > last_cand) return;
    const double ds = csum[cand] - si;
    if (ds * ds > dd * worst) { alive = false; return; }
    double sq = 0.;
    for (int q = 0; q < d; ++q) {
      const double t = x[(size_t)cand * d + q] - xi[q];
      sq += t * t;
    }
    if (sq < worst) {
      int j = m - 1;
      // insertion from the end: shift larger entries up (same result as the swap loop)
      while (j > 0 && sq < bd[(j - 1) * kKnnThreads]) {
        bd[j * kKnnThreads] = bd[(j - 1) * kKnnThreads];
        bi[j * kKnnThreads] = bi[(j - 1) * kKnnThreads];
        --j;
      }
      bd[j * kKnnThreads] = sq;
      bi[j * kKnnThreads] = cand;
      worst = bd[(m - 1) * kKnnThreads];
    }
  };
  while (go_up || go_down) {
    if (lo == 0) go_down = false;
    if (hi == n - 1) go_up = false;
    if (go_down) visit(order[--lo], go_down);
    if (go_up) visit(order[++hi], go_up);
  }
  int* o = out + (size_t)(i - r0) * m;
  for (int k = 0; k < m; ++k) o[k] = bi[k * kKnnThreads];
}

// ---- 65 <= m <= 128: one wave per row ----
//
// A thread-per-row list of 128 slots would need 96 KiB of LDS per 64 rows and an O(m) serial shift per insertion
// with the other 63 lanes idle. Here a wave owns a row and its sorted best list lives in registers across the wave:
// slot k in lane k % 64, half k / 64 (bd0 / bi0: slots 0..63, bd1 / bi1: slots 64..127; the slots >= m only catch
// what falls off slot m - 1, so the 128 slots stay sorted as a whole). No LDS, no barriers: kKnnWideWaves rows per
// workgroup cost nothing.
//
// The sweep is the host's: step s visits order[pos - s] (down) and then order[pos + s] (up) while both directions
// live, so the s-th candidate of a direction is visited at step s whatever became of the other direction. A batch is
// the next 64 visits in that order: with both directions alive lane l holds step k + 1 + l / 2, even lanes down and odd
// lanes up (32 steps); with one alive lane l holds its step k + 1 + l (64 steps). Every lane loads its candidate and
// evaluates (csum[cand] - csum[i])^2 and the squared distance, with the host's operations in the host's order.
//
// The decisions are serial, because the stop test and the strict sq < worst both read the worst kept distance as it
// stands at that visit, and it shrinks with every insertion: ballots of "would stop" and "would insert" against the
// current worst, the lowest undecided lane among them acts, and only an insertion (which changes worst) makes the
// ballots stale and has them taken again over the lanes behind it. A stop takes its direction's later lanes out of
// the batch; the other direction's keep their order. An insertion finds its slot by a ballot of !(sq < slot) over
// both halves (an equal distance goes behind the earlier entry, as the host's strict swap loop leaves it) and moves
// the tail up by one slot with one lane shuffle per register: O(1), not O(m).
constexpr int kKnnWideMaxM = 128;
constexpr int kKnnWideWaves = 4;   // rows per workgroup

__device__ __forceinline__ double wave_read(double v, int lane) {   // lane: wave-uniform
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                          __builtin_amdgcn_readlane(__double2loint(v), lane));
}

__global__ void __launch_bounds__(64 * kKnnWideWaves) knn_wide_kernel(const double* __restrict__ x,
                                                                     const double* __restrict__ csum,
                                                                     const int* __restrict__ order,
                                                                     const int* __restrict__ pos, int n, int d, int m,
                                                                     int r0, int r1, int last_cand,
                                                                     int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int i = r0 + blockIdx.x * kKnnWideWaves + (threadIdx.x >> 6);
  if (i >= r1) return;   // a whole wave; r0 > m, so every row here runs the sweep
  double bd0 = INFINITY, bd1 = INFINITY;
  int bi0 = 0, bi1 = 0;
  double xi[3] = {0., 0., 0.};
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (q < d) xi[q] = x[(size_t)i * d + q];
  const double si = csum[i];
  const double dd = (double)d;
  const int p0 = pos[i];
  const int wslot = m - 1 - 64;   // slot m - 1 is in the upper half
  constexpr unsigned long long kDownLanes = 0x5555555555555555ull;   // the even lanes of a two-direction batch
  bool go_down = true, go_up = true;
  int k = 0;                  // steps taken: lo = pos - k, hi = pos + k
  double worst = INFINITY;   // slot m - 1
  for (;;) {
    if (p0 - k <= 0) go_down = false;
    if (p0 + k >= n - 1) go_up = false;
    if (!go_down && !go_up) break;
    const bool both = go_down && go_up;
    const int step = k + 1 + (both ? (lane >> 1) : lane);
    const bool up = both ? (lane & 1) != 0 : go_up;
    const int idx = up ? p0 + step : p0 - step;
    bool valid = idx >= 0 && idx <= n - 1;   // past an end of the array: that direction has ended
    int cand = 0;
    if (valid) {
      cand = order[idx];
      valid = !(cand >= i || cand > last_cand);
    }
    double t2 = 0., sq = 0.;
    if (valid) {
      const double ds = csum[cand] - si;
      t2 = ds * ds;
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (q < d) {
          const double t = x[(size_t)cand * d + q] - xi[q];
          sq += t * t;
        }
    }
    unsigned long long live = ~0ull;   // lanes whose direction is alive
    unsigned long long rem = ~0ull;    // lanes behind the last decision
    for (;;) {
      const unsigned long long stopb = __ballot(valid && t2 > dd * worst);
      const unsigned long long insb = __ballot(valid && sq < worst);
      bool inserted = false;
      unsigned long long act = (stopb | insb) & rem & live;
      while (act != 0) {
        const int b = __builtin_ctzll(act);
        rem = b == 63 ? 0ull : ~0ull << (b + 1);
        if ((stopb >> b) & 1ull) {   // the stop test comes first, as on the host
          if (!both) {
            go_down = go_up = false;
            live = 0ull;
          } else if (b & 1) {
            go_up = false;
            live &= kDownLanes;
          } else {
            go_down = false;
            live &= ~kDownLanes;
          }
          act = (stopb | insb) & rem & live;
          continue;
        }
        const double sqb = wave_read(sq, b);
        const int cb = __builtin_amdgcn_readlane(cand, b);
        const int p = __popcll(__ballot(!(sqb < bd0))) + __popcll(__ballot(!(sqb < bd1)));   // p <= m - 1
        const double u0 = __shfl_up(bd0, 1), u1 = __shfl_up(bd1, 1), w = wave_read(bd0, 63);
        const int ui0 = __shfl_up(bi0, 1), ui1 = __shfl_up(bi1, 1), wi = __builtin_amdgcn_readlane(bi0, 63);
        if (lane >= p) {
          bd0 = lane == p ? sqb : u0;
          bi0 = lane == p ? cb : ui0;
        }
        if (lane + 64 >= p) {
          bd1 = lane + 64 == p ? sqb : (lane == 0 ? w : u1);
          bi1 = lane + 64 == p ? cb : (lane == 0 ? wi : ui1);
        }
        worst = wave_read(bd1, wslot);
        inserted = true;
        break;
      }
      if (!inserted) break;
    }
    k += both ? 32 : 64;
  }
  int* o = out + (size_t)(i - r0) * m;
  o[lane] = bi0;
  if (lane + 64 < m) o[lane + 64] = bi1;
}

}  // namespace

void vecchia_neighbors_gpu(const double* x, int n, int d, int m, int row_begin, int row_end, int* nbr,
                           hipStream_t s, int end_search_at) {
  const int last_cand = end_search_at < 0 ? n - 2 : end_search_at;
  if (m > kKnnWideMaxM) Fatal("GPU neighbour search supports num_neighbors <= %d", kKnnWideMaxM);
  if (d < 1 || d > 3) Fatal("GPU neighbour search supports 1 <= dim_gp_coords <= 3");
  const int rows = row_end - row_begin;
  if (rows <= 0) return;
  // coordinate sums and the sweep order: same code as the host search (utils.h:228-236)
  std::vector<double> csum(n);
  for (int i = 0; i < n; ++i) {
    double v = 0.;
    for (int q = 0; q < d; ++q) v += x[(size_t)i * d + q];
    csum[i] = v;
  }
  std::vector<int> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return csum[a] < csum[b]; });
  std::vector<int> pos(n);
  for (int i = 0; i < n; ++i) pos[order[i]] = i;
  // rows i <= m (and i = 0) on the host: all earlier points in index order, the rest -1
  for (int i = row_begin; i < row_end; ++i) {
    int* o = nbr + (size_t)(i - row_begin) * m;
    if (i <= m) {
      std::fill(o, o + m, -1);
      for (int j = 0; j < i; ++j) o[j] = j;
    }
  }
  const int g0 = std::max(row_begin, m + 1);
  if (g0 >= row_end) return;
  DevBuf<double> dx, dcs;
  DevBuf<int> dord, dpos, dout;
  dx.alloc((size_t)n * d);
  dcs.alloc(n);
  dord.alloc(n);
  dpos.alloc(n);
  dout.alloc((size_t)(row_end - g0) * m);
  HIP_CHECK(hipMemcpyAsync(dx.get(), x, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(dcs.get(), csum.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(dord.get(), order.data(), sizeof(int) * n, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(dpos.get(), pos.data(), sizeof(int) * n, hipMemcpyHostToDevice, s));
  if (m > kKnnMaxM) {   // a wave per row
    const int blocks = (row_end - g0 + kKnnWideWaves - 1) / kKnnWideWaves;
    hipLaunchKernelGGL(knn_wide_kernel, dim3(blocks), dim3(64 * kKnnWideWaves), 0, s, dx.get(), dcs.get(), dord.get(),
                       dpos.get(), n, d, m, g0, row_end, last_cand, dout.get());
  } else {
    const int blocks = (row_end - g0 + kKnnThreads - 1) / kKnnThreads;
    hipLaunchKernelGGL(knn_kernel, dim3(blocks), dim3(kKnnThreads), 0, s, dx.get(), dcs.get(), dord.get(), dpos.get(),
                       n, d, m, g0, row_end, last_cand, dout.get());
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(nbr + (size_t)(g0 - row_begin) * m, dout.get(), sizeof(int) * (size_t)(row_end - g0) * m,
                           hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

void test_vecchia_neighbors(const double* x, int n, int d, int m, int row_begin, int row_end, int end_search_at,
                            int use_gpu, int32_t* out, int64_t out_len) {
  const char* fn = "GPB_TestVecchiaNeighbors";
  if (x == nullptr || out == nullptr) Fatal("%s: NULL argument", fn);
  if (n < 2 || d < 1 || (use_gpu && d > 3)) Fatal("%s: n = %d, d = %d", fn, n, d);
  if (m < 1 || m > n - 1) Fatal("%s: m = %d outside [1, n - 1 = %d]", fn, m, n - 1);
  if (row_begin < 0 || row_end < row_begin || row_end > n)
    Fatal("%s: rows [%d, %d) outside [0, n = %d)", fn, row_begin, row_end, n);
  if (end_search_at < -1 || end_search_at > n - 1)
    Fatal("%s: end_search_at = %d outside [-1, n - 1]", fn, end_search_at);
  if (out_len != (int64_t)(row_end - row_begin) * m)
    Fatal("%s: out holds %lld entries, rows m = %lld", fn, (long long)out_len, (long long)(row_end - row_begin) * m);
  for (int64_t k = 0; k < (int64_t)n * d; ++k)
    if (!std::isfinite(x[k])) Fatal("%s: coordinate %lld is not finite", fn, (long long)k);
  if (use_gpu) vecchia_neighbors_gpu(x, n, d, m, row_begin, row_end, out, nullptr, end_search_at);
  else vecchia_neighbors(x, n, d, m, row_begin, row_end, out, end_search_at);
}

}  // namespace gpb_amd
