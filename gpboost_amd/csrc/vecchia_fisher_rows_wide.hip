// Vecchia factor rows WITH both derivative rows for 64 < num_neighbors <= kRowsWideMaxM (gfx950, wave64): the row
// kernel of the Fisher information (VecchiaFisher, standard errors of the covariance parameters).
//
// Per Vecchia row i with k = min(i, m) neighbours N it writes what latent_factor_kernel<K, COV> writes in its nugget
// form (LatentFactorArgs::dBv_var != nullptr), with C = cov(N, N) + (var (jitter - 1) + nugget) I and c = cov(N, i):
//   a = C^-1 c,  Bv = -a,  Dinv = 1 / (var + nugget - a.c),
//   dBv_var = -C^-1 a,  dD_var = var - a.c - a.a,
//   t = (dC / dlog phi) a (zero diagonal),  dBv = -C^-1 (dc - t),  dD = -(2 dc.a - t.a).
// So a row has three solves with one factor, and two of them need the first one's result.
//
// Layout and factorization are those of vecchia_rows_wide.hip (its stages 1 to 3; the blocked Cholesky is a copy, so
// that kernel's registers and results stay what they are): one 256-thread workgroup per row, KP = k rounded up to a
// multiple of 16 with identity padding, ONE square LDS array A (odd row stride S = MP + 1, MP = m rounded up to 16)
// with C in the lower triangle and dC / dlog phi in the upper one, every pair covariance evaluated once, 16-column
// right-looking panels whose trailing updates are v_mfma_f64_16x16x4 tiles dealt round-robin to the four waves.
// What this kernel adds:
//
//  1b. the matrix takes the row's neighbours in descending order of their covariance with point i (a rank found by
//      counting over the keys in LDS; ties by slot, so the order is fixed), and the outputs go back to their slots.
//      The elimination meets the entries that carry a.c first, after the fewest roundings: with a neighbour table
//      that is not sorted by distance, one close neighbour late in the row cost 6 ulp in a.c.
//  3b. c rides through the factorization as a BORDER ROW zb (row KP of the matrix, kept in a vector of its own): in
//      every panel the thread after the last panel row solves the border's 16 entries against L_bb with the panel
//      rows, and after the panel barrier thread jj updates zb[jj] -= sum_s zb[j0 + s] L[jj][j0 + s] (16 terms, fixed
//      order) beside the MFMA tiles. When the last panel is done zb = L^-1 c: the first forward chain never runs.
//  4.  a = L^-T zb: one backward column sweep on wave 0 (lane l owns entries l and l + 64, one shuffle per column).
//  5.  t = dC a as a k x k matrix-vector product on the WHOLE workgroup: thread (r = tid & 127, h = tid >> 7) sums
//      row r over the columns [h KP / 2, (h + 1) KP / 2) into four interleaved partial sums, ((p0 + p1) + (p2 + p3))
//      goes to LDS, and t_r = half 0 + half 1. The trip count KP / 2 is uniform over the workgroup; rows >= KP are
//      predicated off.
//  6.  the two remaining right-hand sides, a and dc - t, go through ONE forward and ONE backward sweep on wave 0:
//      every load of L and of L_cc serves both. Then the four dot products [a.c, a.a, dc.a, t.a] by a fixed
//      shuffle tree (a.c as |L^-1 c|^2 from the border row: a sum of squares, which a.c over the entries of a is
//      not); the solutions go to LDS and thread r writes slot r of the three output rows (r >= k: exactly 0).
// Chains per row: 8 panels' pivots, then 3 sweeps of KP steps (5 without 3b and the fused pair). Not built: inverted
// 16 x 16 diagonal blocks for block-wise sweeps.
//
// Every loop's trip count is uniform over the workgroup or the wave; where the work per lane differs the lanes are
// predicated. Every sum has a fixed order, there is no atomic, and a row's outputs depend only on its data and the
// parameters (not on the grid). A failed pivot has no path of its own: sqrt of a negative pivot is NaN, which
// reaches the row's outputs.
//
// LDS per workgroup: MP S + 9 MP doubles (A, the coordinates, dc, zb, a, L_kk and the two halves of t):
// 141312 bytes at m = 128, 81408 at m = 96, 57600 at m = 80; sized by the model's m and checked against the device's
// per-workgroup limit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "cov.h"
#include "kernels.h"
#include "latent_kernels.h"

namespace gpb_amd {
namespace {

constexpr int kDMax = 3;
constexpr int kWideThreads = 256;
constexpr int kPanel = 16;   // panel width = MFMA tile edge
constexpr int kFisherWideMaxBlocks = 2048;
typedef double double4_t __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int wide_mp(int m) { return (m + kPanel - 1) & ~(kPanel - 1); }
// A (MP x S) | coordinates (MP x 3) | dc, zb, a, L_kk, t half 0, t half 1 (6 MP)
__host__ __device__ constexpr size_t fisher_wide_lds_doubles(int m) {
  return (size_t)wide_mp(m) * (wide_mp(m) + 1) + (size_t)(kDMax + 6) * wide_mp(m);
}

template <int COV>
__global__ void __launch_bounds__(kWideThreads) vecchia_fisher_rows_wide_kernel(LatentFactorArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int MP = wide_mp(a.m), S = MP + 1;
  double* A = smem;
  double* nbx = A + MP * S;
  double* dcv = nbx + MP * kDMax;  // dc / dlog(phi)
  double* zb = dcv + MP;           // border row: c, then L^-1 c
  double* av = zb + MP;            // a = C^-1 c
  double* dg = av + MP;            // L_kk
  double* tp = dg + MP;            // t = dC a, the two column halves (2 MP)

  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int d = a.d;
  const double var = a.var, phi = a.phi;
  const double cdiag = var * a.jitter + a.nugget;

  for (int i = blockIdx.x; i < a.n; i += gridDim.x) {
    const int k = min(i, a.m);
    const int KP = (k + kPanel - 1) & ~(kPanel - 1);
    __syncthreads();   // the previous row's reads are done

    // ---- 1. gather: thread r < KP loads neighbour r; the matrix takes the neighbours in descending order of
    // c_r (ties by slot, padding last), pos = the rank of slot r, found by counting over the keys in LDS
    const bool rv = tid < k;
    double gx[kDMax] = {0., 0., 0.}, gc = 0., gdc = 0.;
    if (tid < KP) {
      const int nb = rv ? a.nbr[(size_t)i * a.m + tid] : 0;
      double s = 0.;
#pragma unroll
      for (int q = 0; q < kDMax; ++q) {
        gx[q] = (q < d && rv) ? a.X[(size_t)nb * d + q] : 0.;
        const double xi = q < d ? a.X[(size_t)i * d + q] : 0.;
        s += (xi - gx[q]) * (xi - gx[q]);
      }
      cov_dcov_sq<COV>(s, var, phi, gc, gdc);
      tp[tid] = rv ? gc : -1.;   // covariances are >= 0
    }
    __syncthreads();
    int pos = 0;
    if (tid < KP) {
      const double key = rv ? gc : -1.;
      for (int j = 0; j < KP; ++j) {   // wave-uniform trip count
        const double kj = tp[j];
        pos += (kj > key || (kj == key && j < tid)) ? 1 : 0;
      }
#pragma unroll
      for (int q = 0; q < kDMax; ++q) nbx[pos * kDMax + q] = gx[q];
      zb[pos] = rv ? gc : 0.;
      dcv[pos] = rv ? gdc : 0.;
      A[pos * S + pos] = rv ? cdiag : 1.;
    }
    __syncthreads();

    // ---- 2. pairs: e -> (h, q); q < h: (row h, column q), else (row KP - 1 - h, column q - h)
    const int npairs = (KP / 2) * (KP - 1);
    for (int e0 = 0; e0 < npairs; e0 += kWideThreads) {   // workgroup-uniform trip count; the last trip is partial
      const int e = min(e0 + tid, npairs - 1);
      const int h = e / (KP - 1), q = e - h * (KP - 1);
      const int r = q < h ? h : KP - 1 - h;
      const int c = q < h ? q : q - h;
      double s = 0.;
#pragma unroll
      for (int qq = 0; qq < kDMax; ++qq) {
        const double t = nbx[r * kDMax + qq] - nbx[c * kDMax + qq];
        s += t * t;
      }
      double cc, dc;
      cov_dcov_sq<COV>(s, var, phi, cc, dc);
      const bool valid = r < k;   // c < r
      if (e0 + tid < npairs) {
        A[r * S + c] = valid ? cc : 0.;
        A[c * S + r] = valid ? dc : 0.;
      }
    }
    __syncthreads();

    // ---- 3. blocked Cholesky of the lower triangle, the border row zb riding along
    const int NB = KP / kPanel;
    for (int p = 0; p < NB; ++p) {
      const int j0 = p * kPanel;
      // block row lr (entries c > lr hold dC and are never used) and L_jj. Entries of L and of the solves are
      // divided by the pivot, not multiplied by its reciprocal: one rounding fewer in every entry, which the
      // derivative rows' cancelling sums (var - a.c - a.a) show; the row is a latency chain, so it costs little
      double row[kPanel], ll[kPanel];
#pragma unroll
      for (int c = 0; c < kPanel; ++c) row[c] = A[(j0 + lr) * S + j0 + c];
#pragma unroll
      for (int j = 0; j < kPanel; ++j) {
        const double l = sqrt(__shfl(row[j], j, kPanel));
        ll[j] = l;
        const double lik = row[j] / l;   // L[lr][j] for lr > j
        row[j] = lr == j ? l : lik;
#pragma unroll
        for (int jj = j + 1; jj < kPanel; ++jj) row[jj] = fma(-lik, __shfl(lik, jj, kPanel), row[jj]);   // lr >= jj
      }
      // panel rows below the block and the border row (t == KP): x L_bb^T = P, thread = row (threads past the
      // border redo the last row and store nothing)
      const int t = j0 + kPanel + tid;
      double* px = t == KP ? zb + j0 : A + min(t, KP - 1) * S + j0;
      double x[kPanel];
#pragma unroll
      for (int c = 0; c < kPanel; ++c) x[c] = px[c];
#pragma unroll
      for (int j = 0; j < kPanel; ++j) {
        double s = x[j];
#pragma unroll
        for (int q = 0; q < j; ++q) s = fma(-x[q], __shfl(row[q], j, kPanel), s);   // L[j][q] from lane j
        x[j] = s / ll[j];
      }
      if (t <= KP) {
#pragma unroll
        for (int c = 0; c < kPanel; ++c) px[c] = x[c];
      }
      __syncthreads();   // the panel is final; every wave has read the diagonal block
      if (tid < kPanel) {
#pragma unroll
        for (int c = 0; c < kPanel; ++c) {
          if (c <= lr) A[(j0 + lr) * S + j0 + c] = row[c];
          if (c == lr) dg[j0 + c] = ll[c];
        }
      }
      // border update: column t of the border against panel row t (both final since the barrier)
      if (t < KP) {
        double s = zb[t];
#pragma unroll
        for (int c = 0; c < kPanel; ++c) s = fma(-zb[j0 + c], A[t * S + j0 + c], s);
        zb[t] = s;
      }
      // trailing update, tiles I >= J > p round-robin over the waves. MFMA operands: a = P_I[lr][4 s + lq],
      // b = P_J[lr][4 s + lq]; result entry rg of a lane is row lq + 4 rg, column lr of the tile
      int cnt = 0;
      for (int I = p + 1; I < NB; ++I) {
        for (int J = p + 1; J <= I; ++J, ++cnt) {
          if ((cnt & 3) != wave) continue;
          const double* pa = A + (I * kPanel + lr) * S + j0 + lq;
          const double* pb = A + (J * kPanel + lr) * S + j0 + lq;
          double4_t u = {0., 0., 0., 0.};
#pragma unroll
          for (int s4 = 0; s4 < kPanel; s4 += 4) u = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[s4], pb[s4], u, 0, 0, 0);
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const int ii = I * kPanel + lq + 4 * rg, jj = J * kPanel + lr;
            if (jj <= ii) A[ii * S + jj] -= u[rg];
          }
        }
      }
      __syncthreads();
    }

    // wave 0 owns the sweeps: lane l holds entries l and l + 64 (absent entries are zeros that stay zeros)
    const int t0 = lane, t1 = lane + 64;
    const bool h0 = t0 < KP, h1 = t1 < KP;
    const int K0 = min(KP, 64);
    double a0 = 0., a1 = 0., b0 = 0., b1 = 0.;

    // ---- 4. a = L^-T zb (row c of L is contiguous)
    if (wave == 0) {
      a0 = b0 = h0 ? zb[t0] : 0.;
      a1 = b1 = h1 ? zb[t1] : 0.;
      for (int c = KP - 1; c >= 64; --c) {
        const double xk = __shfl(a1, c - 64) / dg[c];
        const double l1 = t1 < c ? A[c * S + t1] : 0.;
        const double l0 = A[c * S + t0];
        a1 = t1 == c ? xk : fma(-l1, xk, a1);
        a0 = fma(-l0, xk, a0);
      }
      for (int c = K0 - 1; c >= 0; --c) {
        const double xk = __shfl(a0, c) / dg[c];
        const double l0 = t0 < c ? A[c * S + t0] : 0.;
        a0 = t0 == c ? xk : fma(-l0, xk, a0);
      }
      if (h0) av[t0] = a0;
      if (h1) av[t1] = a1;
    }
    __syncthreads();

    // ---- 5. t = dC a on the whole workgroup: row r, column half h, four interleaved partial sums
    {
      const int r = tid & 127, h = tid >> 7;
      const bool act = r < KP;
      const int cb = h * (KP / 2), ce = cb + KP / 2;   // KP / 2 is a multiple of 8
      double pq[4] = {0., 0., 0., 0.};
      for (int c4 = cb; c4 < ce; c4 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = c4 + u;
          const double w = (act && c != r) ? A[c < r ? c * S + r : r * S + c] : 0.;
          pq[u] = fma(w, av[c], pq[u]);
        }
      }
      if (act) tp[h * MP + r] = (pq[0] + pq[1]) + (pq[2] + pq[3]);
    }
    __syncthreads();

    // ---- 6. w = C^-1 a and g = C^-1 (dc - t) in one forward and one backward sweep, the dot products, the outputs
    if (wave == 0) {
      const double tt0 = h0 ? tp[t0] + tp[MP + t0] : 0., tt1 = h1 ? tp[t1] + tp[MP + t1] : 0.;
      const double d0 = h0 ? dcv[t0] : 0., d1 = h1 ? dcv[t1] : 0.;
      // a.c = c^T C^-1 c = |L^-1 c|^2: a sum of squares of the border row, not a sum of mixed signs over a
      double s[4] = {b0 * b0 + b1 * b1, a0 * a0 + a1 * a1, d0 * a0 + d1 * a1, tt0 * a0 + tt1 * a1};
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += __shfl_xor(s[q], off);
      }
      double z0 = a0, z1 = a1;
      double w0 = d0 - tt0, w1 = d1 - tt1;
      for (int c = 0; c < K0; ++c) {   // L z = rhs
        const double lcc = dg[c], xk = __shfl(z0, c) / lcc, yk = __shfl(w0, c) / lcc;
        const double l0 = (h0 && t0 > c) ? A[t0 * S + c] : 0.;
        const double l1 = h1 ? A[t1 * S + c] : 0.;
        z0 = t0 == c ? xk : fma(-l0, xk, z0);
        w0 = t0 == c ? yk : fma(-l0, yk, w0);
        z1 = fma(-l1, xk, z1);
        w1 = fma(-l1, yk, w1);
      }
      for (int c = 64; c < KP; ++c) {
        const double lcc = dg[c], xk = __shfl(z1, c - 64) / lcc, yk = __shfl(w1, c - 64) / lcc;
        const double l1 = (h1 && t1 > c) ? A[t1 * S + c] : 0.;
        z1 = t1 == c ? xk : fma(-l1, xk, z1);
        w1 = t1 == c ? yk : fma(-l1, yk, w1);
      }
      for (int c = KP - 1; c >= 64; --c) {   // L^T x = z
        const double lcc = dg[c], xk = __shfl(z1, c - 64) / lcc, yk = __shfl(w1, c - 64) / lcc;
        const double l1 = t1 < c ? A[c * S + t1] : 0.;
        const double l0 = A[c * S + t0];
        z1 = t1 == c ? xk : fma(-l1, xk, z1);
        w1 = t1 == c ? yk : fma(-l1, yk, w1);
        z0 = fma(-l0, xk, z0);
        w0 = fma(-l0, yk, w0);
      }
      for (int c = K0 - 1; c >= 0; --c) {
        const double lcc = dg[c], xk = __shfl(z0, c) / lcc, yk = __shfl(w0, c) / lcc;
        const double l0 = t0 < c ? A[c * S + t0] : 0.;
        z0 = t0 == c ? xk : fma(-l0, xk, z0);
        w0 = t0 == c ? yk : fma(-l0, yk, w0);
      }
      if (h0) { tp[t0] = z0; tp[MP + t0] = w0; }   // t is in registers: its two halves take the solutions
      if (h1) { tp[t1] = z1; tp[MP + t1] = w1; }
      if (lane == 0) {
        const double ac = s[0], aa = s[1], dca = s[2], ta = s[3];
        a.Dinv[i] = 1. / (var + a.nugget - ac);
        a.dD_var[i] = var - ac - aa;
        if (a.dD != nullptr) a.dD[i] = -(2. * dca - ta);
      }
    }
    __syncthreads();
    // slot r of the row's outputs is position pos of the solutions (r < k has pos < k); slots r >= k: exactly 0
    if (tid < a.m) {
      const size_t o = (size_t)i * a.m + tid;
      a.Bv[o] = rv ? -av[pos] : 0.;
      a.dBv_var[o] = rv ? -tp[pos] : 0.;
      if (a.dBv != nullptr) a.dBv[o] = rv ? -tp[MP + pos] : 0.;
    }
  }
}

}  // namespace

void launch_vecchia_fisher_rows_wide(int cov_type, const LatentFactorArgs& a, hipStream_t s) {
  if (a.d < 1 || a.d > kDMax) Fatal("GPU Vecchia kernel supports 1 <= dim_gp_coords <= %d, got %d", kDMax, a.d);
  if (a.m <= 64 || a.m > kRowsWideMaxM)
    Fatal("num_neighbors = %d is outside the wide Vecchia Fisher row kernel's range 65 to %d", a.m, kRowsWideMaxM);
  if (a.Bv == nullptr || a.Dinv == nullptr || a.dBv_var == nullptr || a.dD_var == nullptr)
    Fatal("the wide Vecchia Fisher row kernel needs Bv, Dinv, dBv_var and dD_var");
  if (a.n <= 0) return;
  int dev = 0, cus = 0, lds_max = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  HIP_CHECK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  const size_t bytes = fisher_wide_lds_doubles(a.m) * sizeof(double);
  if (bytes > (size_t)lds_max)
    Fatal("num_neighbors = %d needs %zu bytes of LDS per workgroup for the Vecchia Fisher information, this device "
          "has %d", a.m, bytes, lds_max);
  dispatch_cov(cov_type, [&](auto cov) {
    constexpr int COV = decltype(cov)::value;
    auto kern = vecchia_fisher_rows_wide_kernel<COV>;
    if (bytes > 64 * 1024)   // above the default dynamic-LDS limit
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)bytes));
    // the grid is the resident capacity: every workgroup strides over an equal share of the rows
    int per_cu = 0;
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kWideThreads, bytes));
    const int blocks = std::min({a.n, std::max(per_cu, 1) * std::max(cus, 1), kFisherWideMaxBlocks});
    static const bool info = std::getenv("GPBOOST_AMD_ROWS_PROF") != nullptr;
    if (info)
      std::fprintf(stderr, "[fisher rows wide] m=%d grid=%d workgroups/CU=%d LDS bytes/workgroup=%zu\n", a.m, blocks,
                   per_cu, bytes);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWideThreads), bytes, s, a);
  });
  HIP_CHECK(hipGetLastError());
}

}  // namespace gpb_amd
