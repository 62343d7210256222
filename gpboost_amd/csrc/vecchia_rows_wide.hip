// Vecchia factor + likelihood/gradient row kernel for 64 < num_neighbors <= kRowsWideMaxM (gfx950, wave64).
//
// The lane-group kernels of vecchia_kernels.hip keep one row of the k x k between-neighbour matrix C per lane, so a
// wavefront bounds them at m = 64. Here one 256-thread workgroup (four waves) owns a Vecchia row i with
// k = min(i, m) neighbours, and C lives in LDS. The per-row quantities are those of vecchia_rows_kernel (steps 1-3
// of its header) and the row's six sums those of the reduction contract; only the way they are computed
// differs. With KP = k rounded up to a multiple of 16 (rows >= k are identity padding with zero right-hand sides,
// which leaves every solution unchanged):
//
//  1. gather: thread r < KP loads neighbour r (index, coordinates, response) and evaluates c_r and dc_r / dlog(phi);
//  2. pairs: the KP (KP - 1) / 2 covariances are evaluated once, split evenly over the 256 threads (rows h and
//     KP - 1 - h together hold KP - 1 pairs, so the pairs form a KP / 2 x (KP - 1) rectangle), and stored in ONE
//     square array A (KP x KP, odd row stride S = MP + 1, MP = m rounded up to 16): C_rc in the lower triangle
//     (r > c), dC_rc / dlog(phi) in the upper one (A[c][r]). No second matrix and no second exp pass;
//  3. blocked right-looking Cholesky of the lower triangle in place, 16-column panels. Per panel: every wave loads
//     the 16 x 16 diagonal block (lane & 15 = block row, 16 registers), factors it by a column sweep whose
//     broadcasts are 16-lane shuffles, and solves X L_bb^T = P for the panel rows below with the same shuffles
//     (thread = row, 16 registers; the four waves hold the same L_bb, so no barrier separates factor and solve);
//     then the trailing update A_IJ -= P_I P_J^T runs as 16 x 16 tiles of four v_mfma_f64_16x16x4 each, the
//     tiles I >= J dealt round-robin to the four waves. Diagonal tiles store only their lower half: the upper
//     triangle keeps dC. Two barriers per panel;
//  4. a = C^-1 c and v = C^-1 y_nbr together on wave 0: lane l holds entries l and l + 64 of both, forward and
//     backward column sweeps with one wave shuffle per column and right-hand side, one load of L per column for
//     both, and the reciprocal pivots from LDS (no barrier inside the solves);
//  5. still on wave 0 and in registers: t = dC a from the upper triangle (entries l and l + 64, four partial sums
//     each, wave-uniform column loop), the eight dot products of the lane-group kernel by a fixed shuffle tree, and
//     lane 0 forms D, u and the derivative terms and adds the row's six sums to its accumulators. Stages 4 and 5
//     are latency chains of one wave; the other three wait at the next row's barrier.
// Workgroups stride over rows; thread 0 writes the workgroup's six partials, which launch_sum_blocks adds in block
// order. Every sum has a fixed order, there is no atomic, and a row's outputs depend only on its data and the
// parameters (not on the grid). Every loop's trip count is uniform over the workgroup or the wave; where the work
// per lane differs, the lanes are predicated instead. A failed pivot has no path of its own: sqrt of a negative
// pivot is NaN, which reaches the sums, where the host's NaN check reports it.
//
// LDS per workgroup: MP S + 9 MP doubles (A, the coordinates and six vectors): 141312 bytes at m = 128,
// 81408 at m = 96, 57600 at m = 80. The allocation is sized by the model's m and checked against the device's
// per-workgroup limit, which bounds the largest m. The kernel's registers (256 VGPRs and 175 AGPRs per lane) allow
// one workgroup per CU at every m; measurements are in DESIGN.md section 5.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "cov.h"
#include "kernels.h"

namespace gpb_amd {
namespace {

constexpr int kDMax = 3;
constexpr int kWideThreads = 256;
constexpr int kPanel = 16;   // panel width = MFMA tile edge
typedef double double4_t __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int wide_mp(int m) { return (m + kPanel - 1) & ~(kPanel - 1); }
// A (MP x S) | coordinates (MP x 3) | c, dc, y_nbr, a, v, 1 / L_kk (6 MP)
__host__ __device__ constexpr size_t wide_lds_doubles(int m) {
  return (size_t)wide_mp(m) * (wide_mp(m) + 1) + (size_t)(kDMax + 6) * wide_mp(m);
}

template <int COV>
__global__ void __launch_bounds__(kWideThreads) vecchia_rows_wide_kernel(VecchiaRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int MP = wide_mp(a.m), S = MP + 1;
  double* A = smem;
  double* nbx = A + MP * S;
  double* cv = nbx + MP * kDMax;   // c
  double* dcv = cv + MP;           // dc / dlog(phi)
  double* yv = dcv + MP;           // y_nbr
  double* av = yv + MP;            // a = C^-1 c
  double* vv = av + MP;            // v = C^-1 y_nbr
  double* rd = vv + MP;            // 1 / L_kk

  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int d = a.d;
  const double var = a.var, phi = a.phi;
  const double cdiag = var * a.diag_mult + a.diag_add;
  const double delta = cdiag - var;   // C - C_nonugget on the diagonal
  const bool want_like = a.Y != nullptr;
  double acc[kVecchiaSums] = {0., 0., 0., 0., 0., 0.};   // thread 0

  for (int i = a.r0 + blockIdx.x; i < a.r1; i += gridDim.x) {
    const int k = min(i, a.m);
    const int KP = (k + kPanel - 1) & ~(kPanel - 1);
    __syncthreads();   // the previous row's reads are done

    // ---- 1. gather
    if (tid < KP) {
      const bool rv = tid < k;
      const int nb = rv ? a.nbr[(size_t)(i - a.row_base) * a.m + tid] : 0;
      double s = 0.;
#pragma unroll
      for (int q = 0; q < kDMax; ++q) {
        const double x = (q < d && rv) ? a.X[(size_t)nb * d + q] : 0.;
        const double xi = q < d ? a.X[(size_t)i * d + q] : 0.;
        nbx[tid * kDMax + q] = x;
        s += (xi - x) * (xi - x);
      }
      double c, dc;
      cov_dcov_sq<COV>(s, var, phi, c, dc);
      cv[tid] = rv ? c : 0.;
      dcv[tid] = rv ? dc : 0.;
      yv[tid] = (rv && want_like) ? a.Y[nb] : 0.;
      A[tid * S + tid] = rv ? cdiag : 1.;
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

    // ---- 3. blocked Cholesky of the lower triangle
    const int NB = KP / kPanel;
    for (int p = 0; p < NB; ++p) {
      const int j0 = p * kPanel;
      double row[kPanel], rl[kPanel];   // block row lr (entries c > lr hold dC and are never used); 1 / L_jj
#pragma unroll
      for (int c = 0; c < kPanel; ++c) row[c] = A[(j0 + lr) * S + j0 + c];
#pragma unroll
      for (int j = 0; j < kPanel; ++j) {
        const double l = sqrt(__shfl(row[j], j, kPanel));
        rl[j] = 1. / l;
        const double lik = row[j] * rl[j];   // L[lr][j] for lr > j
        row[j] = lr == j ? l : lik;
#pragma unroll
        for (int jj = j + 1; jj < kPanel; ++jj) row[jj] = fma(-lik, __shfl(lik, jj, kPanel), row[jj]);   // lr >= jj
      }
      // panel rows below the block: x L_bb^T = P, thread = row (threads past the last row redo it and store nothing)
      const int t = j0 + kPanel + tid;
      const int tc = min(t, KP - 1);
      double x[kPanel];
#pragma unroll
      for (int c = 0; c < kPanel; ++c) x[c] = A[tc * S + j0 + c];
#pragma unroll
      for (int j = 0; j < kPanel; ++j) {
        double s = x[j];
#pragma unroll
        for (int q = 0; q < j; ++q) s = fma(-x[q], __shfl(row[q], j, kPanel), s);   // L[j][q] from lane j
        x[j] = s * rl[j];
      }
      if (t < KP) {
#pragma unroll
        for (int c = 0; c < kPanel; ++c) A[t * S + j0 + c] = x[c];
      }
      __syncthreads();   // the panel is final; every wave has read the diagonal block
      if (tid < kPanel) {
#pragma unroll
        for (int c = 0; c < kPanel; ++c) {
          if (c <= lr) A[(j0 + lr) * S + j0 + c] = row[c];
          if (c == lr) rd[j0 + c] = rl[c];
        }
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

    // ---- 4. a = C^-1 c and v = C^-1 y_nbr on wave 0: entries lane and lane + 64 of both, one load of L per step
    if (wave == 0) {
      const int t0 = lane, t1 = lane + 64;
      const bool h0 = t0 < KP, h1 = t1 < KP;
      const int K0 = min(KP, 64);
      double z0 = h0 ? cv[t0] : 0., z1 = h1 ? cv[t1] : 0.;
      double w0 = h0 ? yv[t0] : 0., w1 = h1 ? yv[t1] : 0.;
      for (int c = 0; c < K0; ++c) {   // L z = rhs
        const double xk = __shfl(z0, c) * rd[c], yk = __shfl(w0, c) * rd[c];
        const double l0 = (h0 && t0 > c) ? A[t0 * S + c] : 0.;
        const double l1 = h1 ? A[t1 * S + c] : 0.;
        z0 = t0 == c ? xk : fma(-l0, xk, z0);
        w0 = t0 == c ? yk : fma(-l0, yk, w0);
        z1 = fma(-l1, xk, z1);
        w1 = fma(-l1, yk, w1);
      }
      for (int c = 64; c < KP; ++c) {
        const double xk = __shfl(z1, c - 64) * rd[c], yk = __shfl(w1, c - 64) * rd[c];
        const double l1 = (h1 && t1 > c) ? A[t1 * S + c] : 0.;
        z1 = t1 == c ? xk : fma(-l1, xk, z1);
        w1 = t1 == c ? yk : fma(-l1, yk, w1);
      }
      for (int c = KP - 1; c >= 64; --c) {   // L^T x = z (row c of L is contiguous)
        const double xk = __shfl(z1, c - 64) * rd[c], yk = __shfl(w1, c - 64) * rd[c];
        const double l1 = t1 < c ? A[c * S + t1] : 0.;
        const double l0 = A[c * S + t0];
        z1 = t1 == c ? xk : fma(-l1, xk, z1);
        w1 = t1 == c ? yk : fma(-l1, yk, w1);
        z0 = fma(-l0, xk, z0);
        w0 = fma(-l0, yk, w0);
      }
      for (int c = K0 - 1; c >= 0; --c) {
        const double xk = __shfl(z0, c) * rd[c], yk = __shfl(w0, c) * rd[c];
        const double l0 = t0 < c ? A[c * S + t0] : 0.;
        z0 = t0 == c ? xk : fma(-l0, xk, z0);
        w0 = t0 == c ? yk : fma(-l0, yk, w0);
      }
      if (h0) { av[t0] = z0; vv[t0] = w0; }
      if (h1) { av[t1] = z1; vv[t1] = w1; }
    }
    __syncthreads();

    if (tid < a.m && a.B_out != nullptr) a.B_out[(size_t)(i - a.row_base) * a.m + tid] = tid < k ? -av[tid] : 0.;
    // ---- 5. on wave 0, lane l owning entries l and l + 64 (loops are wave-uniform, absent entries are zeros):
    // t = dC a over the upper triangle (four partial sums per entry), then the dot products
    // [c.a, y.a, a.a, a.v, dc.a, dc.v, t.a, t.v] by a fixed shuffle tree; lane 0 goes on with the sums
    double sums[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    if (wave == 0) {
      const int r0 = lane, r1 = lane + 64;
      const bool h0 = r0 < KP, h1 = r1 < KP;
      double tq0[4] = {0., 0., 0., 0.}, tq1[4] = {0., 0., 0., 0.};
      for (int cb = 0; cb < KP; cb += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = cb + u;
          const double ac = av[c];
          const double w0 = (h0 && c != r0) ? A[c < r0 ? c * S + r0 : r0 * S + c] : 0.;
          const double w1 = (h1 && c != r1) ? A[c < r1 ? c * S + r1 : r1 * S + c] : 0.;
          tq0[u] = fma(w0, ac, tq0[u]);
          tq1[u] = fma(w1, ac, tq1[u]);
        }
      }
      const double t0 = (tq0[0] + tq0[1]) + (tq0[2] + tq0[3]), t1 = (tq1[0] + tq1[1]) + (tq1[2] + tq1[3]);
      const double a0 = h0 ? av[r0] : 0., a1 = h1 ? av[r1] : 0.;
      const double v0 = h0 ? vv[r0] : 0., v1 = h1 ? vv[r1] : 0.;
      const double c0 = h0 ? cv[r0] : 0., c1 = h1 ? cv[r1] : 0.;
      const double d0 = h0 ? dcv[r0] : 0., d1 = h1 ? dcv[r1] : 0.;
      const double y0 = h0 ? yv[r0] : 0., y1 = h1 ? yv[r1] : 0.;
      double s[8] = {c0 * a0 + c1 * a1, y0 * a0 + y1 * a1, a0 * a0 + a1 * a1, a0 * v0 + a1 * v1,
                     d0 * a0 + d1 * a1, d0 * v0 + d1 * v1, t0 * a0 + t1 * a1, t0 * v0 + t1 * v1};
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 8; ++q) s[q] += __shfl_xor(s[q], off);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) sums[q] = s[q];
    }
    if (tid == 0) {
      const double ac = sums[0], ay = sums[1], aa = sums[2], avv = sums[3];
      const double dD_rng = -(2. * sums[4] - sums[6]);   // dD/dlog phi
      const double uk_rng = -(sums[5] - sums[7]);        // (dB_range y)_i
      const double D = var + a.d_nugget - ac;
      const double Dinv = 1. / D;
      if (a.Dinv_out != nullptr) a.Dinv_out[i - a.row_base] = Dinv;
      if (want_like) {
        const double By = a.Y[i] - ay;                 // (B y)_i
        const double u = By * Dinv;                    // (D^-1 B y)_i
        const double dD_var = var - delta * aa - ac;   // dD/dlog var
        const double uk_var = -delta * avv;            // (dB_var y)_i
        acc[0] += log(D);
        acc[1] += By * u;
        acc[2] += uk_var * u - 0.5 * u * u * dD_var;
        acc[3] += uk_rng * u - 0.5 * u * u * dD_rng;
        acc[4] += Dinv * dD_var;
        acc[5] += Dinv * dD_rng;
      }
    }
  }
  if (want_like && tid == 0) {
#pragma unroll
    for (int s = 0; s < kVecchiaSums; ++s) a.block_sums[(size_t)blockIdx.x * kVecchiaSums + s] = acc[s];
  }
}

}  // namespace

int launch_vecchia_rows_wide(int cov_type, const VecchiaRowsArgs& a, hipStream_t s) {
  if (a.d < 1 || a.d > kDMax) Fatal("GPU Vecchia kernel supports 1 <= dim_gp_coords <= %d, got %d", kDMax, a.d);
  if (a.m < 1 || a.m > kRowsWideMaxM)
    Fatal("num_neighbors = %d > %d is not supported by the GPU Vecchia kernel", a.m, kRowsWideMaxM);
  if (a.r1 <= a.r0) return 0;
  int dev = 0, cus = 0, lds_max = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  HIP_CHECK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  const size_t bytes = wide_lds_doubles(a.m) * sizeof(double);
  if (bytes > (size_t)lds_max)
    Fatal("num_neighbors = %d needs %zu bytes of LDS per workgroup, this device has %d", a.m, bytes, lds_max);
  int blocks = 0;
  dispatch_cov(cov_type, [&](auto cov) {
    constexpr int COV = decltype(cov)::value;
    auto kern = vecchia_rows_wide_kernel<COV>;
    if (bytes > 64 * 1024)   // above the default dynamic-LDS limit
      HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)bytes));
    // the grid is the resident capacity, so every workgroup strides over an equal share of the rows in one round
    int per_cu = 0;
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kWideThreads, bytes));
    blocks = std::min({a.r1 - a.r0, std::max(per_cu, 1) * std::max(cus, 1), kRowsWideMaxBlocks});
    static const bool info = std::getenv("GPBOOST_AMD_ROWS_PROF") != nullptr;
    if (info)
      std::fprintf(stderr, "[rows wide] m=%d grid=%d workgroups/CU=%d LDS bytes/workgroup=%zu\n", a.m, blocks, per_cu,
                   bytes);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kWideThreads), bytes, s, a);
  });
  HIP_CHECK(hipGetLastError());
  return blocks;
}

}  // namespace gpb_amd
