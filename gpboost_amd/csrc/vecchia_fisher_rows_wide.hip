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
// The layout (one 256-thread workgroup per row, one square LDS array A with C below and dC / dlog phi above the
// diagonal, KP = k rounded up to a multiple of 16), the pair phase (stage 2), the blocked Cholesky (stage 3) and the
// column sweeps are those of vecchia_wide_core.h, shared with vecchia_rows_wide.hip; here entries are divided by the
// pivots (not multiplied by reciprocals) and c rides through the factorization as the border row zb, so zb = L^-1 c
// when the last panel is done and the first forward chain never runs. What is this kernel's own:
//
//  1.  gather, and the matrix takes the row's neighbours in descending order of their covariance with point i (a
//      rank found by counting over the keys in LDS; ties by slot, so the order is fixed); the outputs go back to
//      their slots. The elimination meets the entries that carry a.c first, after the fewest roundings: with a
//      neighbour table that is not sorted by distance, one close neighbour late in the row cost 6 ulp in a.c
//      (DESIGN.md section 3).
//  4.  a = L^-T zb: one backward sweep on wave 0.
//  5.  t = dC a as a k x k matrix-vector product on the WHOLE workgroup: thread (r = tid & 127, h = tid >> 7) sums
//      row r over the columns [h KP / 2, (h + 1) KP / 2) into four interleaved partial sums, ((p0 + p1) + (p2 + p3))
//      goes to LDS, and t_r = half 0 + half 1. The trip count KP / 2 is uniform over the workgroup; rows >= KP are
//      predicated off.
//  6.  the two remaining right-hand sides, a and dc - t, go through ONE forward and ONE backward sweep on wave 0:
//      every load of L and of L_cc serves both. Then the four dot products [a.c, a.a, dc.a, t.a] by a fixed
//      shuffle tree (a.c as |L^-1 c|^2 from the border row: a sum of squares, which a.c over the entries of a is
//      not); the solutions go to LDS and thread r writes slot r of the three output rows (r >= k: exactly 0).
// Chains per row: 8 panels' pivots, then 3 sweeps of KP steps (5 without the border row and the fused pair). Not
// built: inverted 16 x 16 diagonal blocks for block-wise sweeps.
//
// Every sum has a fixed order, there is no atomic, and a row's outputs depend only on its data and the parameters
// (not on the grid). A failed pivot's NaN reaches the row's outputs.
//
// LDS per workgroup: see the core header; the six vectors are dc, zb, a, L_kk and the two halves of t.
#include "latent_kernels.h"
#include "vecchia_wide_core.h"

namespace gpb_amd {
namespace {

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

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int d = a.d;
  const double var = a.var, phi = a.phi;
  const CovShape<COV> sh = [&] {
    if constexpr (COV == kMaternGeneral) return a.mg;
    else return NoShape{};
  }();
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
      cov_dcov_sq_s<COV>(s, var, phi, sh, gc, gdc);
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

    wide_pairs<COV>(A, S, nbx, KP, k, var, phi, tid, sh);   // ---- 2.
    __syncthreads();
    wide_chol<true, true>(A, S, KP, dg, zb, tid, lane, wave);   // ---- 3., the border row zb riding along

    // wave 0 owns the sweeps: lane l holds entries l and l + 64 (absent entries are zeros that stay zeros)
    const int t0 = lane, t1 = lane + 64;
    const bool h0 = t0 < KP, h1 = t1 < KP;
    double a0[1] = {0.}, a1[1] = {0.}, b0 = 0., b1 = 0.;

    // ---- 4. a = L^-T zb (row c of L is contiguous)
    if (wave == 0) {
      a0[0] = b0 = h0 ? zb[t0] : 0.;
      a1[0] = b1 = h1 ? zb[t1] : 0.;
      wide_backward<1, true>(A, S, KP, dg, lane, a0, a1);
      if (h0) av[t0] = a0[0];
      if (h1) av[t1] = a1[0];
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
      // a.a with its fma written out: which of the two products a contracted a0 a0 + a1 a1 rounds is the compiler's
      // choice, and dD_var's last bit follows it
      double s[4] = {b0 * b0 + b1 * b1, fma(a1[0], a1[0], a0[0] * a0[0]), d0 * a0[0] + d1 * a1[0],
                     tt0 * a0[0] + tt1 * a1[0]};
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += __shfl_xor(s[q], off);
      }
      double z0[2] = {a0[0], d0 - tt0}, z1[2] = {a1[0], d1 - tt1};
      wide_forward<2, true>(A, S, KP, dg, lane, z0, z1);
      wide_backward<2, true>(A, S, KP, dg, lane, z0, z1);
      if (h0) { tp[t0] = z0[0]; tp[MP + t0] = z0[1]; }   // t is in registers: its two halves take the solutions
      if (h1) { tp[t1] = z1[0]; tp[MP + t1] = z1[1]; }
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
  if (cov_type == kMaternGeneral) {   // not one of dispatch_cov's: this kernel and the wave-per-row one serve it
    if (!(a.mg.nu > 0.)) Fatal("the Matern shape (cov_fct_shape) has not been set for the general-shape Fisher row kernel");
    wide_launch(vecchia_fisher_rows_wide_kernel<kMaternGeneral>, a, a.m, a.n, "fisher rows wide",
                " for the Vecchia Fisher information", s);
    return;
  }
  dispatch_cov(cov_type, [&](auto cov) {
    wide_launch(vecchia_fisher_rows_wide_kernel<decltype(cov)::value>, a, a.m, a.n, "fisher rows wide",
                " for the Vecchia Fisher information", s);
  });
}

}  // namespace gpb_amd
