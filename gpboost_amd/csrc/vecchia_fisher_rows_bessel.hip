// Vecchia factor rows WITH both derivative rows for the Matern covariance with a general smoothness (kMaternGeneral,
// cov.h matern_general) and num_neighbors <= 64 (gfx950, wave64): the row kernel of the Fisher information
// (VecchiaFisher, standard errors of the covariance parameters) where one covariance is a Bessel evaluation.
//
// Per Vecchia row i with k = min(i, m) neighbours N it writes what latent_factor_kernel<K, COV> writes in its nugget
// form (LatentFactorArgs::dBv_var != nullptr), with C = cov(N, N) + (var (jitter - 1) + nugget) I and c = cov(N, i):
//   a = C^-1 c,  Bv = -a,  Dinv = 1 / (var + nugget - a.c),
//   dBv_var = -C^-1 a,  dD_var = var - a.c - a.a,
//   t = (dC / dlog phi) a (zero diagonal),  dBv = -C^-1 (dc - t),  dD = -(2 dc.a - t.a).
// The lane-group kernel evaluates every between-neighbour pair twice (one matrix row per lane), which is the wrong
// shape at some tens of divisions and 50 exponentials' worth of work per covariance (vecchia_rows_bessel.hip gives the
// figures); the workgroup-per-row kernel of vecchia_fisher_rows_wide.hip keeps one row per CU. So, as in
// vecchia_rows_bessel.hip: ONE WAVE owns a row, the waves of a workgroup work on different rows and never wait for
// each other (no __syncthreads in the row loop), and a CU keeps as many rows in flight as LDS and registers allow.
//
// A wave's LDS slice is laid out as the wide kernels' workgroup array (vecchia_wide_core.h): A (KP x KP, stride
// S = MP + 1, KP = k rounded up to 16, identity padding) with C below and dC / dlog(phi) above the diagonal, the
// neighbours' coordinates, and six vectors: dc, zb, a, L_kk and two for the solutions. Per row:
//  1. gather: lane r loads neighbour r and evaluates c_r, dc_r against point i. The matrix takes the neighbours in
//     descending order of c_r (ties by slot, padding last), for the reason the wide Fisher kernel's header gives: the
//     elimination meets the entries that carry a.c first. The rank of slot r is counted over the KP keys by lane
//     shuffles (no LDS); the outputs go back to their slots;
//  2. pairs: wide_pairs over the wave's 64 lanes, each of the KP (KP - 1) / 2 pairs once (m = 30: 8 evaluations per
//     lane, against 31 in the lane-group mapping);
//  3. factor: wide_chol<DIV, BORDER, NW = 1>: entries divided by the pivots, c riding along as the border row zb, so
//     zb = L^-1 c when the last panel is done and a.c = |zb|^2. The border's lane KP - j0 - 16 is below 64 for every
//     panel (KP <= 64), and the wave-level fence between the panel store and the border update keeps the two in
//     program order, which for one wave's LDS accesses is completion order;
//  4. a = L^-T zb: one backward column sweep, lane = entry (KP <= 64: one register per right-hand side);
//  5. t = dC a from the upper triangle, lane = row: four interleaved partial sums, wave-uniform column loop;
//  6. the two remaining right-hand sides, a and dc - t, through ONE forward and ONE backward sweep (every load of L
//     and of L_cc serves both); the four dot products [|zb|^2, a.a, dc.a, t.a] by a fixed shuffle tree; lane 0 writes
//     Dinv, dD_var and dD; the solutions go to LDS at their positions and lane r writes slot r of the three output
//     rows (r >= k: exactly 0).
// Every sum has a fixed order, there is no atomic, and a row's outputs depend only on its data and the parameters
// (not on the grid or on which wave took the row). A failed pivot's NaN reaches the row's outputs.
//
// LDS per wave: MP S + 9 MP doubles (37888 bytes at m = 64, 10752 at m <= 32, 3328 at m <= 16); wave_rows_launch
// takes four waves per workgroup where the device allows. Registers and measurements: DESIGN.md section 5.
#include "latent_kernels.h"
#include "vecchia_wide_core.h"

namespace gpb_amd {
namespace {

template <int COV, int NW>
__global__ void __launch_bounds__(64 * NW) vecchia_fisher_rows_bessel_kernel(LatentFactorArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int MP = wide_mp(a.m), S = MP + 1;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* A = smem + (size_t)wave * wide_lds_doubles(a.m);
  double* nbx = A + MP * S;
  double* dcv = nbx + MP * kDMax;  // dc / dlog(phi)
  double* zb = dcv + MP;           // border row: c, then L^-1 c
  double* av = zb + MP;            // a = C^-1 c
  double* dg = av + MP;            // L_kk
  double* wv = dg + MP;            // the solutions C^-1 a and C^-1 (dc - t) (2 MP)

  const int d = a.d;
  const double var = a.var, phi = a.phi;
  const CovShape<COV> sh = [&] {
    if constexpr (COV == kMaternGeneral) return a.mg;
    else return NoShape{};
  }();
  const double cdiag = var * a.jitter + a.nugget;

  for (int i = blockIdx.x * NW + wave; i < a.n; i += gridDim.x * NW) {
    const int k = min(i, a.m);
    const int KP = (k + kPanel - 1) & ~(kPanel - 1);   // <= MP <= 64
    const bool has = lane < KP, rv = lane < k;
    wide_sync<1>();   // the previous row's reads are done

    // ---- 1. gather on every lane (lanes >= k take the origin and are masked), so that the keys can be shuffled;
    // pos = the rank of slot `lane` in descending order of c (ties by slot, padding last)
    const int nb = rv ? a.nbr[(size_t)i * a.m + lane] : 0;
    double gx[kDMax], s = 0.;
#pragma unroll
    for (int q = 0; q < kDMax; ++q) {
      gx[q] = (q < d && rv) ? a.X[(size_t)nb * d + q] : 0.;
      const double xi = q < d ? a.X[(size_t)i * d + q] : 0.;
      s += (xi - gx[q]) * (xi - gx[q]);
    }
    double gc, gdc;
    cov_dcov_sq_s<COV>(s, var, phi, sh, gc, gdc);
    const double key = rv ? gc : -1.;   // covariances are >= 0
    int pos = 0;
    for (int j = 0; j < KP; ++j) {   // wave-uniform trip count
      const double kj = __shfl(key, j);
      pos += (kj > key || (kj == key && j < lane)) ? 1 : 0;
    }
    if (has) {   // pos < KP
#pragma unroll
      for (int q = 0; q < kDMax; ++q) nbx[pos * kDMax + q] = gx[q];
      zb[pos] = rv ? gc : 0.;
      dcv[pos] = rv ? gdc : 0.;
      A[pos * S + pos] = rv ? cdiag : 1.;
    }
    wide_sync<1>();

    wide_pairs<COV, 64>(A, S, nbx, KP, k, var, phi, lane, sh);   // ---- 2.
    wide_sync<1>();
    wide_chol<true, true, 1>(A, S, KP, dg, zb, lane, lane, 0);   // ---- 3. (ends with the wave's fence)

    // ---- 4. a = L^-T zb, lane = entry (row c of L is contiguous; absent entries are zeros that stay zeros)
    const double b = has ? zb[lane] : 0.;
    double xa = b;
    for (int c = KP - 1; c >= 0; --c) {
      const double ka = __shfl(xa, c) / dg[c];
      const double l = lane < c ? A[c * S + lane] : 0.;
      xa = lane == c ? ka : fma(-l, ka, xa);
    }
    if (has) av[lane] = xa;
    wide_sync<1>();

    // ---- 5. t = dC a over the upper triangle, lane = row
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
    const double d0 = has ? dcv[lane] : 0.;

    // ---- 6. the dot products (a.c = c^T C^-1 c = |L^-1 c|^2 from the border row: a sum of squares, which a.c over
    // the entries of a is not; one product per lane and sum, so there is nothing for the compiler to contract) ...
    double sm[4] = {b * b, xa * xa, d0 * xa, t * xa};
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) sm[q] += __shfl_xor(sm[q], off);
    }
    // ... and w = C^-1 a, g = C^-1 (dc - t) in one forward and one backward sweep
    double zw = xa, zg = d0 - t;
    for (int c = 0; c < KP; ++c) {   // L z = rhs
      const double pv = dg[c];
      const double kw = __shfl(zw, c) / pv, kg = __shfl(zg, c) / pv;
      const double l = (has && lane > c) ? A[lane * S + c] : 0.;
      zw = lane == c ? kw : fma(-l, kw, zw);
      zg = lane == c ? kg : fma(-l, kg, zg);
    }
    for (int c = KP - 1; c >= 0; --c) {   // L^T x = z
      const double pv = dg[c];
      const double kw = __shfl(zw, c) / pv, kg = __shfl(zg, c) / pv;
      const double l = lane < c ? A[c * S + lane] : 0.;
      zw = lane == c ? kw : fma(-l, kw, zw);
      zg = lane == c ? kg : fma(-l, kg, zg);
    }
    if (has) { wv[lane] = zw; wv[MP + lane] = zg; }
    if (lane == 0) {
      const double ac = sm[0], aa = sm[1], dca = sm[2], ta = sm[3];
      a.Dinv[i] = 1. / (var + a.nugget - ac);
      a.dD_var[i] = var - ac - aa;
      if (a.dD != nullptr) a.dD[i] = -(2. * dca - ta);
    }
    wide_sync<1>();
    // slot r of the row's outputs is position pos of the solutions (r < k has pos < k); slots r >= k: exactly 0
    if (lane < a.m) {
      const size_t o = (size_t)i * a.m + lane;
      const int p = rv ? pos : 0;
      a.Bv[o] = rv ? -av[p] : 0.;
      a.dBv_var[o] = rv ? -wv[p] : 0.;
      if (a.dBv != nullptr) a.dBv[o] = rv ? -wv[MP + p] : 0.;
    }
  }
}

}  // namespace

void launch_vecchia_fisher_rows_bessel(const LatentFactorArgs& a, hipStream_t s) {
  if (a.d < 1 || a.d > kDMax) Fatal("GPU Vecchia kernel supports 1 <= dim_gp_coords <= %d, got %d", kDMax, a.d);
  if (a.m < 1 || a.m > 64) Fatal("the wave-per-row Vecchia Fisher kernel serves num_neighbors <= 64, got %d", a.m);
  if (!(a.mg.nu > 0.)) Fatal("the Matern shape (cov_fct_shape) has not been set for the general-shape Fisher row kernel");
  if (a.Bv == nullptr || a.Dinv == nullptr || a.dBv_var == nullptr || a.dD_var == nullptr)
    Fatal("the wave-per-row Vecchia Fisher kernel needs Bv, Dinv, dBv_var and dD_var");
  if ((a.dBv == nullptr) != (a.dD == nullptr)) Fatal("the wave-per-row Vecchia Fisher kernel: dBv goes with dD");
  if (a.n <= 0) return;
  wave_rows_launch(vecchia_fisher_rows_bessel_kernel<kMaternGeneral, 4>,
                   vecchia_fisher_rows_bessel_kernel<kMaternGeneral, 2>,
                   vecchia_fisher_rows_bessel_kernel<kMaternGeneral, 1>, a, a.m, a.n, "fisher rows bessel", s);
}

}  // namespace gpb_amd
