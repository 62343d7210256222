// Vecchia factor + likelihood/gradient row kernel for 64 < num_neighbors <= kRowsWideMaxM (gfx950, wave64).
//
// The lane-group kernels of vecchia_kernels.hip keep one row of the k x k between-neighbour matrix C per lane, so a
// wavefront bounds them at m = 64. Here one 256-thread workgroup (four waves) owns a Vecchia row i with
// k = min(i, m) neighbours, and C lives in LDS. The per-row quantities are those of vecchia_rows_kernel (steps 1-3
// of its header) and the row's six sums those of the reduction contract; only the way they are computed
// differs. The layout (one square LDS array A with C below and dC / dlog(phi) above the diagonal, KP = k rounded up
// to a multiple of 16), the pair phase (stage 2), the blocked Cholesky (stage 3) and the column sweeps of stage 4 are
// those of vecchia_wide_core.h, shared with the Fisher row kernel; here with reciprocal pivots and no border row.
// What is this kernel's own:
//
//  1. gather: thread r < KP loads neighbour r (index, coordinates, response) and evaluates c_r and dc_r / dlog(phi);
//  4. a = C^-1 c and v = C^-1 y_nbr together on wave 0: one forward and one backward sweep for both right-hand
//     sides (no barrier inside the solves);
//  5. still on wave 0 and in registers: t = dC a from the upper triangle (entries l and l + 64, four partial sums
//     each, wave-uniform column loop), the eight dot products of the lane-group kernel by a fixed shuffle tree, and
//     lane 0 forms D, u and the derivative terms and adds the row's six sums to its accumulators. Stages 4 and 5
//     are latency chains of one wave; the other three wait at the next row's barrier.
// Workgroups stride over rows; thread 0 writes the workgroup's six partials, which launch_sum_blocks adds in block
// order. Every sum has a fixed order, there is no atomic, and a row's outputs depend only on its data and the
// parameters (not on the grid). A failed pivot's NaN reaches the sums, where the host's NaN check reports it.
//
// LDS per workgroup: see the core header; the six vectors are c, dc, y_nbr, a, v and 1 / L_kk. The kernel's
// registers allow one workgroup per CU at every m; measurements are in DESIGN.md section 5.
#include "vecchia_wide_core.h"

namespace gpb_amd {
namespace {

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

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int d = a.d;
  const double var = a.var, phi = a.phi;
  const CovShape<COV> sh = [&] {
    if constexpr (COV == kMaternGeneral) return a.mg;
    else return NoShape{};
  }();
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
      cov_dcov_sq_s<COV>(s, var, phi, sh, c, dc);
      cv[tid] = rv ? c : 0.;
      dcv[tid] = rv ? dc : 0.;
      yv[tid] = (rv && want_like) ? a.Y[nb] : 0.;
      A[tid * S + tid] = rv ? cdiag : 1.;
    }
    __syncthreads();

    wide_pairs<COV>(A, S, nbx, KP, k, var, phi, tid, sh);   // ---- 2.
    __syncthreads();
    wide_chol<false, false>(A, S, KP, rd, nullptr, tid, lane, wave);   // ---- 3.

    // ---- 4. a = C^-1 c and v = C^-1 y_nbr on wave 0: entries lane and lane + 64 of both, one load of L per step
    if (wave == 0) {
      const int t0 = lane, t1 = lane + 64;
      const bool h0 = t0 < KP, h1 = t1 < KP;
      double z0[2] = {h0 ? cv[t0] : 0., h0 ? yv[t0] : 0.}, z1[2] = {h1 ? cv[t1] : 0., h1 ? yv[t1] : 0.};
      wide_forward<2, false>(A, S, KP, rd, lane, z0, z1);
      wide_backward<2, false>(A, S, KP, rd, lane, z0, z1);
      if (h0) { av[t0] = z0[0]; vv[t0] = z0[1]; }
      if (h1) { av[t1] = z1[0]; vv[t1] = z1[1]; }
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
  int blocks = 0;
  if (cov_type == kMaternGeneral) {   // not one of dispatch_cov's: this kernel and the wave-per-row one serve it
    if (!(a.mg.nu > 0.)) Fatal("the Matern shape (cov_fct_shape) has not been set for the general-shape row kernel");
    return wide_launch(vecchia_rows_wide_kernel<kMaternGeneral>, a, a.m, a.r1 - a.r0, "rows wide", "", s);
  }
  dispatch_cov(cov_type, [&](auto cov) {
    blocks = wide_launch(vecchia_rows_wide_kernel<decltype(cov)::value>, a, a.m, a.r1 - a.r0, "rows wide", "", s);
  });
  return blocks;
}

}  // namespace gpb_amd
