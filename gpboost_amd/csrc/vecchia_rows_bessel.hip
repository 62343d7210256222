// Vecchia factor + likelihood/gradient row kernel for the Matern covariance with a general smoothness
// (kMaternGeneral, cov.h matern_general) and num_neighbors <= 64 (gfx950, wave64).
//
// One covariance costs a Bessel evaluation here (a Temme series or a Steed continued fraction: some tens of
// divisions and on the order of 50 exponentials' worth of work), not the 30 instructions the lane-group kernels of
// vecchia_kernels.hip and the 16-lane kernel are shaped around; those evaluate every between-neighbour pair twice
// (one matrix row per lane). The workgroup-per-row wide kernel evaluates each pair once but keeps one row per CU,
// which at m = 30 is a chain of latencies. So: ONE WAVE owns a Vecchia row i with k = min(i, m) neighbours, the
// waves of a workgroup work on different rows and never wait for each other (no __syncthreads in the row loop), and
// a CU keeps as many rows in flight as LDS and registers allow. The per-row quantities are those of
// vecchia_rows_kernel (steps 1-3 of its header), the six sums those of the reduction contract.
//
// A wave's LDS slice is laid out as the wide kernels' workgroup array (vecchia_wide_core.h): A (KP x KP, stride
// S = MP + 1, KP = k rounded up to 16, identity padding) with C below and dC / dlog(phi) above the diagonal, the
// neighbours' coordinates, and six vectors. Per row:
//  1. gather: lane r < k loads neighbour r (index, coordinates, response) and evaluates c_r, dc_r against point i;
//  2. pairs: the KP (KP - 1) / 2 pairs once each, dealt evenly over the 64 lanes by the rectangle mapping of
//     wide_pairs (m = 30: 496 pairs, 8 evaluations per lane). Distances come from the coordinates;
//  3. factor: wide_chol with NW = 1: 16-column panels, the diagonal block factored in registers with 16-lane
//     shuffles, the panel rows solved one per lane, the trailing update by v_mfma_f64_16x16x4 tiles, all on this
//     wave, separated by wave-level fences only. The register-resident right-looking form was not chosen: it
//     needs the row length at compile time (64 doubles = 128 VGPRs per lane at m = 64, whatever k is), and the
//     registers are what the Bessel evaluation of stage 2 and the occupancy that hides its latency live on;
//  4. a = C^-1 c and v = C^-1 y_nbr: one forward and one backward column sweep for both, lane = entry;
//  5. t = dC a from the upper triangle, the eight dot products by a fixed shuffle tree, and lane 0 forms D, u and
//     the row's six sums exactly as vecchia_rows_wide_kernel does.
// Waves stride over rows; after the loop the workgroup's waves add their six partials in wave order (the only
// barrier) and thread 0 writes them for launch_sum_blocks. No atomics; a row's outputs depend on its data only.
//
// LDS per wave: MP S + 9 MP doubles (37888 bytes at m = 64, 10752 at m <= 32, 3328 at m <= 16); the launcher
// takes four waves per workgroup if the device's per-workgroup limit allows (m = 64: 151552 bytes), else two or
// one, and the grid is the resident capacity.
#include "vecchia_wide_core.h"

namespace gpb_amd {
namespace {

template <int COV, int NW>
__global__ void __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2))) vecchia_rows_bessel_kernel(VecchiaRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int MP = wide_mp(a.m), S = MP + 1;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* A = smem + (size_t)wave * wide_lds_doubles(a.m);
  double* nbx = A + MP * S;
  double* cv = nbx + MP * kDMax;   // c
  double* dcv = cv + MP;           // dc / dlog(phi)
  double* yv = dcv + MP;           // y_nbr
  double* av = yv + MP;            // a = C^-1 c
  double* rd = av + MP;            // 1 / L_kk (v = C^-1 y_nbr stays in registers)

  const int d = a.d;
  const double var = a.var, phi = a.phi;
  const CovShape<COV> sh = [&] {
    if constexpr (COV == kMaternGeneral) return a.mg;
    else return NoShape{};
  }();
  const double cdiag = var * a.diag_mult + a.diag_add;
  const double delta = cdiag - var;   // C - C_nonugget on the diagonal
  const bool want_like = a.Y != nullptr;
  double acc[kVecchiaSums] = {0., 0., 0., 0., 0., 0.};   // lane 0

  for (int i = a.r0 + blockIdx.x * NW + wave; i < a.r1; i += gridDim.x * NW) {
    const int k = min(i, a.m);
    const int KP = (k + kPanel - 1) & ~(kPanel - 1);   // <= MP <= 64
    wide_sync<1>();   // the previous row's reads are done

    // ---- 1. gather
    if (lane < KP) {
      const bool rv = lane < k;
      const int nb = rv ? a.nbr[(size_t)(i - a.row_base) * a.m + lane] : 0;
      double s = 0.;
#pragma unroll
      for (int q = 0; q < kDMax; ++q) {
        const double x = (q < d && rv) ? a.X[(size_t)nb * d + q] : 0.;
        const double xi = q < d ? a.X[(size_t)i * d + q] : 0.;
        nbx[lane * kDMax + q] = x;
        s += (xi - x) * (xi - x);
      }
      double c, dc;
      cov_dcov_sq_s<COV>(s, var, phi, sh, c, dc);
      cv[lane] = rv ? c : 0.;
      dcv[lane] = rv ? dc : 0.;
      yv[lane] = (rv && want_like) ? a.Y[nb] : 0.;
      A[lane * S + lane] = rv ? cdiag : 1.;
    }
    wide_sync<1>();

    wide_pairs<COV, 64>(A, S, nbx, KP, k, var, phi, lane, sh);   // ---- 2.
    wide_sync<1>();
    wide_chol<false, false, 1>(A, S, KP, rd, nullptr, lane, lane, 0);   // ---- 3. (ends with the wave's fence)

    // ---- 4. lane = entry of both right-hand sides; one load of L and of the pivot per column
    const bool has = lane < KP;
    double xa = has ? cv[lane] : 0., xy = has ? yv[lane] : 0.;
    for (int c = 0; c < KP; ++c) {   // L z = rhs
      const double pv = rd[c];
      const double ka = __shfl(xa, c) * pv, ky = __shfl(xy, c) * pv;
      const double l = (has && lane > c) ? A[lane * S + c] : 0.;
      xa = lane == c ? ka : fma(-l, ka, xa);
      xy = lane == c ? ky : fma(-l, ky, xy);
    }
    for (int c = KP - 1; c >= 0; --c) {   // L^T x = z (row c of L is contiguous)
      const double pv = rd[c];
      const double ka = __shfl(xa, c) * pv, ky = __shfl(xy, c) * pv;
      const double l = lane < c ? A[c * S + lane] : 0.;
      xa = lane == c ? ka : fma(-l, ka, xa);
      xy = lane == c ? ky : fma(-l, ky, xy);
    }
    if (has) av[lane] = xa;
    if (lane < a.m && a.B_out != nullptr) a.B_out[(size_t)(i - a.row_base) * a.m + lane] = lane < k ? -xa : 0.;
    wide_sync<1>();

    // ---- 5. t = dC a over the upper triangle (four partial sums, wave-uniform column loop), then the dot products
    // [c.a, y.a, a.a, a.v, dc.a, dc.v, t.a, t.v] by a fixed shuffle tree
    double tq[4] = {0., 0., 0., 0.};
    for (int cb = 0; cb < KP; cb += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = cb + u;
        const double w = (has && c != lane) ? A[c < lane ? c * S + lane : lane * S + c] : 0.;
        tq[u] = fma(w, av[c], tq[u]);
      }
    }
    const double t = (tq[0] + tq[1]) + (tq[2] + tq[3]);
    const double c0 = has ? cv[lane] : 0., d0 = has ? dcv[lane] : 0., y0 = has ? yv[lane] : 0.;
    double s[8] = {c0 * xa, y0 * xa, xa * xa, xa * xy, d0 * xa, d0 * xy, t * xa, t * xy};
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int q = 0; q < 8; ++q) s[q] += __shfl_xor(s[q], off);
    }
    if (lane == 0) {
      const double ac = s[0], ay = s[1], aa = s[2], avv = s[3];
      const double dD_rng = -(2. * s[4] - s[6]);   // dD/dlog phi
      const double uk_rng = -(s[5] - s[7]);        // (dB_range y)_i
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
  if (want_like) {   // the waves' partials in wave order: each wave's own slice holds its six
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < kVecchiaSums; ++q) A[q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < kVecchiaSums) {
      double t = 0.;
      for (int w = 0; w < NW; ++w) t += smem[(size_t)w * wide_lds_doubles(a.m) + threadIdx.x];
      a.block_sums[(size_t)blockIdx.x * kVecchiaSums + threadIdx.x] = t;
    }
  }
}

// the device form of matern_general at var = 1 on n arguments (GPB_TestMaternGeneral)
__global__ void __launch_bounds__(64) matern_general_test_kernel(MaternGeneralPars p, int n, const double* x, double* c,
                                                                 double* dc) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) matern_general(x[i], 1., p, c[i], dc[i]);
}

}  // namespace

void test_matern_general(double nu, int n, const double* x, double* c, double* dc) {
  if (!(nu > 0.) || nu > kMaternGeneralMaxShape) Fatal("GPB_TestMaternGeneral: nu = %g outside (0, %g]", nu, kMaternGeneralMaxShape);
  if (n <= 0 || x == nullptr || c == nullptr || dc == nullptr) Fatal("GPB_TestMaternGeneral: n <= 0 or a NULL array");
  double* buf = nullptr;
  HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&buf), sizeof(double) * 3 * n));
  HIP_CHECK(hipMemcpy(buf, x, sizeof(double) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(matern_general_test_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, matern_general_pars(nu), n, buf,
                     buf + n, buf + 2 * (size_t)n);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(c, buf + n, sizeof(double) * n, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(dc, buf + 2 * (size_t)n, sizeof(double) * n, hipMemcpyDeviceToHost);
  (void)hipFree(buf);
  HIP_CHECK(e);
}

int launch_vecchia_rows_bessel(const VecchiaRowsArgs& a, hipStream_t s) {
  if (a.d < 1 || a.d > kDMax) Fatal("GPU Vecchia kernel supports 1 <= dim_gp_coords <= %d, got %d", kDMax, a.d);
  if (a.m < 1 || a.m > 64) Fatal("the wave-per-row Vecchia kernel serves num_neighbors <= 64, got %d", a.m);
  if (!(a.mg.nu > 0.)) Fatal("the Matern shape (cov_fct_shape) has not been set for the general-shape row kernel");
  if (a.r1 <= a.r0) return 0;
  return wave_rows_launch(vecchia_rows_bessel_kernel<kMaternGeneral, 4>, vecchia_rows_bessel_kernel<kMaternGeneral, 2>,
                          vecchia_rows_bessel_kernel<kMaternGeneral, 1>, a, a.m, a.r1 - a.r0, "rows bessel", s);
}

}  // namespace gpb_amd
