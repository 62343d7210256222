// Vecchia factor + likelihood/gradient rows, 16-lane form (m <= 30), gfx950.
//
// Same row math as vecchia_rows_kernel's bordered form (vecchia_kernels.hip; reference:
// CalcCovFactorGradientVecchia Vecchia_utils.cpp:1307-1632 fused with re_model_template.h:8885-9120,
// 1768-1791), laid out so the Gauss-Jordan broadcasts never touch LDS: one row problem (the 32 x 32
// bordered matrix [[C, c, y_nbr], [c^T ...], [y_nbr^T ...]], 30 pivots) per 16-lane DPP row, lane h
// holding matrix rows h and h + 16. Column j of the current matrix is row j by symmetry, and row c's
// entry sits in lane c mod 16 (register set c / 16), so one row_newbcast DPP move (a single 64-bit
// VALU op) hands M[j][c] to the 16 lanes of the problem, where it feeds TWO FMAs (rows h, h + 16).
// Four problems per wave, one per DPP row. The 32-lane form broadcasts every value through an LDS
// slot (a 16-byte read per two values per lane): at 2 waves/SIMD its LDS return traffic, not the FP64
// VALU, set the pace.
//   1. a 31-point circulant over the 30 neighbours and the row's own point (slot 30 = lane 14's second
//      slot): slot v pairs with (v + delta) mod 31, delta = 1..15, so the 465 pairs are each evaluated
//      once (30 kernel evaluations per lane; slot 30's pairs are the border column c). Coordinates in
//      LDS with copies of slots 0..15 at 31..46 (partner v + delta is an immediate-offset read). C to
//      the packed lower triangle, dC/dlog(phi) in registers until the rows are loaded, then over the
//      packed C in the circulant layout W[(delta - 1) 32 + v];
//   2. rows h and h + 16 of the bordered matrix into registers (lane address + immediate; the columns
//      that cross the packed triangle's diagonal by two reads under compile-time lane masks); 30
//      Gauss-Jordan steps by DPP broadcasts, each broadcast folded into its FMAs (v_fmac_f64_dpp):
//        pivots 0..15  update the B rows (h + 16) in all columns j + 1..31, the A rows (h) only in
//                      columns j + 1..15; the A rows' multipliers stay in the dead column registers r0[j];
//        pivots 16..29 update the B rows only;
//        A rows        M[h][30..31] -= sum_{c = 16..29} M[h][c] x_c with their original columns 16..29
//                      (block back-substitution), then the 16 stored row operations replayed on these
//                      two right-hand sides in pivot order (by linearity the same solution);
//      675 DPP fmacs per problem set: 376 + 119 on the B rows, 120 + 28 + 32 on the A rows (899 with
//      the A rows' columns 16..31 carried through pivots 0..15: 376 + 119 and 376 + 28; 990 for the
//      plain 30-pivot Gauss-Jordan on both rows).
//      a_v = M[v][30] / M[v][v], w_v = M[v][31] / M[v][v] (each pivot's reciprocal is kept by its own lane);
//   3. a^T dC a and w^T dC a over each lane's circulant pairs ([a, w] pairs with the same wrap copies);
//   4. the eight group sums by DPP within the 16-lane row, reduced together (sum16x8), then the row partials
//      (DESIGN.md §6); log(D) is kept per lane and taken once per 16 problem sets (flush_logs).
// Two kernels run this loop (rows16_body): vecchia_rows16_kernel computes every pair's distance from the
// coordinates as described in 1.; vecchia_rows16d_kernel (VecchiaRowsArgs::R set) reads the distances
// that vecchia_rows16_dist_kernel stored once per structure, loaded one problem set ahead, and holds no
// coordinates at all. Both feed the same bits to the same operation sequence.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "common.h"
#include "cov.h"
#include "kernels.h"

namespace gpb_amd {
namespace {

constexpr int kD3 = 3;   // coordinate dimension bound (VecchiaRowsArgs.d <= 3)
// Measured choices (MI355X, n = 100k, m = 30, exponential; evals/s of the headline bench, medians of 5
// alternated runs, the parent's own min-max spread 30; profiles/rows16_issue/RESULTS.md). Each was an
// A/B macro of this file (GPBOOST_AMD_VARIANT / GPBOOST_AMD_DEFS builds); the losing branches are gone.
//   - every broadcast folded into its FMAs as one v_fmac_f64_dpp: 0.1968 vs 0.2140 ms per launch against
//     separate DPP moves + FMAs (profiles/r04/round_r04c.log);
//   - pivots 16..29 eliminate only the B rows (h + 16), the A rows' solution completed by one block
//     back-substitution x_A -= M_AB x_B (28 instead of 119 broadcasts per problem; 4950 vs 4780);
//   - the A rows' columns 16..31 stay out of pivots 0..15, the multipliers kept in the dead column
//     registers and the 16 row operations replayed on the two right-hand sides after the
//     back-substitution (120 + 32 instead of 376 A-row fmacs per problem): 5616 vs 5299 with it off;
//   - the matrix rows read from the packed triangle at lane address + immediate, the columns that cross
//     the diagonal by two reads under compile-time lane masks, instead of a per-lane address select per
//     entry (about 290 VALU ops per problem set): 5616 vs 5458;
//   - exp's constants held in scalar registers across the loop (ExpCoef::scalar(), cov.h) instead of
//     64-bit VALU moves at each use (63 per problem set): 5616 vs 5500.
//   - the pair distances stored per structure and streamed (profiles/rows16_dist/RESULTS.md; the parent's
//     spread 28): 6378 vs 5628, 2183 instead of 2661 VALU instructions per problem set for 384 MB more HBM
//     reads per launch at n = 100k. Non-temporal loads of the records: 6241 vs 6230, inside the noise.
//   - the per-set scalar and select overhead (profiles/rows16_epilogue/RESULTS.md; five sessions, each on the
//     card it was given; the parent's spread 42 - 77): 6760 vs 6391, 6714 vs 6522, 6390 vs 6161, 6372 vs 6127,
//     6337 vs 6055 with all four of the following, 1914 instead of 2174 VALU instructions executed per
//     problem set.
//     Without one of them (first session; all four 6760):
//       log(D) per lane, taken once per 16 sets with all lanes useful, instead of once per set with 4 of 64
//       lanes (flush_logs; the same additions in the same order, nll bit-equal): 6474 without;
//       the pivot's own lane by two 64-bit moves under a scalar lane mask, the reciprocal kept instead of
//       the pivot, instead of a compare and two 64-bit selects per pivot and two reciprocals at the end
//       (own_lane): 6555 without;
//       the covariances' store addresses by one add per pair and an immediate, the wrapped slots by two
//       stores under compile-time lane masks (lds_write_at, lds_write_wrap): 6652 without;
//       the eight group sums reduced together, 61 instead of 96 instructions (sum16x8): 6707 without; its
//       margin (53, then 36, 52, 47 in the later sessions) is at or below the parent's spread, see RESULTS.
// Rejected with them: the next set's loads issued after pivot 15 or 21 instead of after the elimination
// (6198 and 6304 vs 6338: slower the earlier they go); the own lane zeroing its entry of column j and
// keeping the pivot right after the broadcast, beside the reciprocal, with the two reciprocals back at the end
// (10 instructions more, a shorter dependent chain per pivot: 6320 vs 6372).
//   - the waves' issue priorities (profiles/rows16_phase/RESULTS.md): 2 or 3 outside the elimination, 0 or 1
//     inside it, the higher of each to the even-slot and the odd-slot wave of a SIMD by turns, trip by trip.
//     Left alone the older wave (slot 0) is preferred and done after 208 k cycles, its partner after 284 k, a
//     quarter of the kernel at one wave per SIMD. Figures in the record.
// Rejected with it: a start delay of the odd-slot waves (s_sleep, 20 to 320 units of 64 cycles; the supposition
// was that the two waves wait in phase: the clock records show their offsets spread over the whole half trip
// without it): 6763, 6799, 6795, 6776, 6682 vs 6731 without and 6812 for the parent, the parent's spread 84;
// the priority by turns alone, and the lower priority in the elimination alone (same level for both waves): each
// about half of the two together (6428 and 6439 vs 6537 with both, ties to the older wave, 6263 without, a
// session with a spread of 230).
// Rejected: the next pivot's broadcast, reciprocal and multipliers issued after the step's first three
// columns and left to the compiler to schedule under the rest of the step's fmacs (it did interleave
// them): 5616 with vs 5628 without, inside the noise; round 4 had measured the hand-pinned form slower.

__device__ __forceinline__ void lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void cfence() { asm volatile("" ::: "memory"); }

// s_getreg operands (size - 1 << 11 | offset << 6 | register): HW_ID is register 4 on gfx9, WAVE_ID (the wave's
// slot of its SIMD) its bits 3:0, SIMD_ID 5:4, CU_ID 11:8, SH_ID 12, SE_ID 14:13; XCC_ID is register 20, bits 3:0
constexpr int kHwWaveSlot = 3 << 11 | 4;

// Instrumented variant (GPBOOST_AMD_DEFS=-DGPBOOST_AMD_ROWS16_PHASE=1 builds; never in the default library):
// every wave writes, by lane 0's ordinary stores, kPhaseStride 64-bit words to a.phase: HW_ID, XCC_ID, the
// shader clock at entry, the trips it ran, then for each of its first kPhaseTrips trips the clock at the top of
// the trip, after the covariances (the records' vmcnt wait is behind it) and after the elimination (a mark
// after the row load, where every register is live, spilled). With GPBOOST_AMD_ROWS16_PHASE_DUMP=<file> the launcher waits for the kernel and writes the
// records of that launch to the file (scripts/rows16_phase_offsets.py reads it).
#ifdef GPBOOST_AMD_ROWS16_PHASE
constexpr int kHwId = 31 << 11 | 4, kHwXcc = 3 << 11 | 20;
constexpr int kPhaseTrips = 16, kPhaseMarks = 3, kPhaseHead = 4;
constexpr int kPhaseStride = kPhaseHead + kPhaseTrips * kPhaseMarks;
#define PHASE_ID()                                                      \
  unsigned long long* const phase_rec = a.phase + (size_t)blockIdx.x * kPhaseStride; \
  if (threadIdx.x == 0) {                                               \
    phase_rec[0] = __builtin_amdgcn_s_getreg(kHwId);                    \
    phase_rec[1] = __builtin_amdgcn_s_getreg(kHwXcc);                   \
    phase_rec[2] = clock64();                                           \
  }
#define PHASE_MARK(IT, K)                                               \
  asm volatile("" ::: "memory");                                        \
  if (threadIdx.x == 0 && (IT) < kPhaseTrips) phase_rec[kPhaseHead + (IT) * kPhaseMarks + (K)] = clock64()
#define PHASE_END(IT) \
  if (threadIdx.x == 0) phase_rec[3] = (IT)
#else
#define PHASE_ID()
#define PHASE_MARK(IT, K)
#define PHASE_END(IT)
#endif

template <int CTRL>
__device__ __forceinline__ double dpp32x2(double v) {   // all controls used have a source lane for every lane
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

template <int L>
__device__ __forceinline__ double bcast16(double v) {   // lane L of each 16-lane row, to the whole row
  const long b = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(long, v), 0x150 + L, 0xF, 0xF, true);
  return __builtin_bit_cast(double, b);
}

// acc += (src of lane L of the 16-lane row) * mul, one instruction. NOP: the VALU-write -> DPP-read
// wait states (2) emitted inside the same asm statement, so no compiler-scheduled VALU op can land
// between them and the DPP read (the hazard recognizer does not see into inline asm). The first
// broadcast of every sequence whose source was just written carries them; tests/test_isa_hazards.py
// disassembles the built kernels and checks every DPP source against the preceding VALU writes.
template <int L, bool NOP = false>
__device__ __forceinline__ void fmac_bcast16(double& acc, double src, double mul) {
  if constexpr (NOP)
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc)
                 : "v"(src), "v"(mul), "n"(L));
  else
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc)
                 : "v"(src), "v"(mul), "n"(L));
}

__device__ __forceinline__ unsigned lds_addr(const double* p) {   // the 32-bit LDS byte address of a __shared__ pointer
  return (unsigned)(size_t)(const __attribute__((address_space(3))) double*)p;
}

// Rows h and h + 16, columns C and C + 16 (C = 1..15), of a packed lower triangle: every lane reads
// the entry past the diagonal at `up + tri(column)`, then the lanes with h >= C (the same compile-time
// lane mask for both rows) read theirs at `lo + column` over it; LDS returns in order, so the second
// read wins. No address select, no VALU op. The exec mask is saved and restored inside the statement
// (no compiler-scheduled instruction runs under the narrowed mask); the results are in flight when it
// ends: the caller waits (s_waitcnt lgkmcnt(0)) before it uses them, and tests/test_isa_rows16_loads.py
// checks in the built code that nothing names their registers before that wait.
template <int C>
__device__ __forceinline__ void lds_read_split2(double& a, double& b, unsigned up_a, unsigned up_b, unsigned lo_a,
                                                unsigned lo_b) {
  constexpr unsigned m16 = (0xFFFFu << C) & 0xFFFFu;
  constexpr unsigned long mask = m16 | m16 << 16;   // both halves of exec
  constexpr int CB = C + 16;
  unsigned long saved;
  asm volatile(
      "ds_read_b64 %0, %3 offset:%7\n\t"
      "ds_read_b64 %1, %4 offset:%8\n\t"
      "s_mov_b64 %2, exec\n\t"
      "s_and_b32 exec_lo, exec_lo, %11\n\t"
      "s_and_b32 exec_hi, exec_hi, %11\n\t"
      "ds_read_b64 %0, %5 offset:%9\n\t"
      "ds_read_b64 %1, %6 offset:%10\n\t"
      "s_mov_b64 exec, %2"
      : "=&v"(a), "=&v"(b), "=&s"(saved)
      : "v"(up_a), "v"(up_b), "v"(lo_a), "v"(lo_b), "n"(C * (C + 1) / 2 * 8), "n"(CB * (CB + 1) / 2 * 8), "n"(C * 8),
        "n"(CB * 8), "n"(mask)
      : "memory", "scc");
}

// 16-bit lane mask of one 16-lane row, for the two rows of an exec half. The statements below narrow exec
// by immediates (masks in scalar registers were hoisted out of the loop and spilled) and write the mask as
// the first source: the `exec_lo, exec_lo, mask` form marks lds_read_split2's blocks for
// tests/test_isa_rows16_loads.py.
constexpr unsigned rows2(unsigned m16) { return (m16 & 0xFFFFu) * 0x00010001u; }

// Pivot J's own lane (lane J of each 16-lane row) alone: it keeps the pivot's reciprocal and its multiplier
// becomes 0. Two 64-bit moves under a scalar lane mask instead of a lane compare and two 64-bit selects;
// the exec mask is saved and restored inside the statement.
template <int J>
__device__ __forceinline__ void own_lane(double& inv, double& mul, double rinv) {
  unsigned long saved;
  asm volatile(
      "s_mov_b64 %2, exec\n\t"
      "s_and_b32 exec_lo, %4, exec_lo\n\t"
      "s_and_b32 exec_hi, %4, exec_hi\n\t"
      "v_mov_b64 %0, %3\n\t"
      "v_mov_b64 %1, 0\n\t"
      "s_mov_b64 exec, %2"
      : "+v"(inv), "+v"(mul), "=&s"(saved)
      : "v"(rinv), "n"(rows2(1u << J))
      : "scc");
}

template <int OFF>
__device__ __forceinline__ void lds_write_at(unsigned addr, double v) {   // LDS byte address + immediate
  asm volatile("ds_write_b64 %0, %1 offset:%2" : : "v"(addr), "v"(v), "n"(OFF) : "memory");
}

// Slot h + 16's pair at delta DL: packed(h + 16 + DL, h + 16) at `in + tri(DL)`, or, in the lanes whose
// partner wraps past slot 30 (h > 14 - DL, a compile-time lane mask), packed(h + 16, h + DL - 15) at
// `wrap + DL`: two stores under complementary masks, no compare and no address select.
template <int DL>
__device__ __forceinline__ void lds_write_wrap(unsigned in, unsigned wrap, double v) {
  if constexpr (DL >= 15) {
    lds_write_at<DL * 8>(wrap, v);
  } else {
    unsigned long saved;
    asm volatile(
        "s_mov_b64 %0, exec\n\t"
        "s_and_b32 exec_lo, %4, exec_lo\n\t"
        "s_and_b32 exec_hi, %4, exec_hi\n\t"
        "ds_write_b64 %2, %3 offset:%6\n\t"
        "s_andn2_b64 exec, %0, exec\n\t"
        "ds_write_b64 %1, %3 offset:%5\n\t"
        "s_mov_b64 exec, %0"
        : "=&s"(saved)
        : "v"(in), "v"(wrap), "v"(v), "n"(rows2(0xFFFFu << (15 - DL))), "n"(DL * (DL + 1) / 2 * 8), "n"(DL * 8)
        : "memory", "scc");
  }
}

// One level of the transposed reduction of two quantities over the lane exchange CTRL, which swaps the
// banks (4-lane groups of the 16-lane row) in KEEP_X with the others: the lanes of KEEP_X end with
// x + x', the others with y + y' (' = the exchange partner's). Bank masks do the selects inside the DPP
// moves: 6 moves and one add for two quantities instead of 4 moves and two adds each level.
template <int CTRL, int KEEP_X>
__device__ __forceinline__ double pair_level(double x, double y) {
  constexpr int KEEP_Y = 0xF & ~KEEP_X, SELF = 0xE4;   // quad_perm [0,1,2,3]
  int plo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xF, KEEP_X, false);
  int phi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xF, KEEP_X, false);
  plo = __builtin_amdgcn_update_dpp(plo, __double2loint(y), CTRL, 0xF, KEEP_Y, false);
  phi = __builtin_amdgcn_update_dpp(phi, __double2hiint(y), CTRL, 0xF, KEEP_Y, false);
  const int klo = __builtin_amdgcn_update_dpp(__double2loint(x), __double2loint(y), SELF, 0xF, KEEP_Y, false);
  const int khi = __builtin_amdgcn_update_dpp(__double2hiint(x), __double2hiint(y), SELF, 0xF, KEEP_Y, false);
  return __hiloint2double(khi, klo) + __hiloint2double(phi, plo);
}

// The eight group sums together: q[0..7] of every lane in, the totals out in lane 0 (t[0] in all 16 lanes).
// Two transposed levels (row_mirror, row_half_mirror: whole banks change places) take 8 registers to 2, each
// bank then holding one quantity's four partial sums per register; two plain levels sum within the bank.
__device__ __forceinline__ void sum16x8(const double (&q)[8], double (&t)[8]) {
  double a[4], b[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) a[k] = pair_level<0x140, 0x3>(q[2 * k], q[2 * k + 1]);   // banks 0,1: q[2k]; 2,3: q[2k+1]
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    double v = pair_level<0x141, 0x5>(a[2 * k], a[2 * k + 1]);   // banks 0..3: q[4k], q[4k+2], q[4k+1], q[4k+3]
    v += dpp32x2<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp32x2<0x4E>(v);   // quad_perm [2,3,0,1]
    b[k] = v;
  }
  t[0] = bcast16<0>(b[0]);
  t[1] = bcast16<8>(b[0]);
  t[2] = bcast16<4>(b[0]);
  t[3] = bcast16<12>(b[0]);
  t[4] = b[1];
  t[5] = bcast16<8>(b[1]);
  t[6] = bcast16<4>(b[1]);
  t[7] = bcast16<12>(b[1]);
}

__device__ __forceinline__ double recip(double x) {   // hardware reciprocal + two Newton steps (~1 ulp)
  double r = __builtin_amdgcn_rcp(x);
  r = fma(r, fma(-x, r, 1.), r);
  return fma(r, fma(-x, r, 1.), r);
}

template <int B, int E, class F>
__device__ __forceinline__ void sfor(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    sfor<B + 1, E>(f);
  }
}

__device__ __forceinline__ int tri(int x) { return x * (x + 1) / 2; }

constexpr int kK = 32, kMK = 30;
constexpr int kPacked = kK * (kK + 1) / 2;   // 528

template <int CS>
constexpr int problem_doubles() { return kPacked + 48 * CS; }   // packed C (then dC) | 48 coordinate rows

typedef double v2d __attribute__((ext_vector_type(2)));

// ---- the pieces of phase 1 that do not depend on the covariance parameters, shared by the row kernel
// and the distance kernel below (the same source, so the stored distances are the bits the row kernel
// computes on the fly)

// Coordinates of the row's own point and of slots h and h + 16. Padding slots sit at distinct far-away
// points: covariances exactly 0 (see vecchia_rows_kernel); slot 30 (lane 14's second slot) is the row's
// own point, lane 15's second slot (31) holds no point.
template <int ND>
__device__ __forceinline__ void load_points(const VecchiaRowsArgs& a, int d, int irow, int h, bool rv0, bool rv1,
                                            int nb0, int nb1, double (&xi)[ND], double (&x0)[ND], double (&x1)[ND]) {
#pragma unroll
  for (int q = 0; q < ND; ++q) {
    xi[q] = (q < d) ? a.X[(size_t)irow * d + q] : 0.;
    x0[q] = (q < d && rv0) ? a.X[(size_t)nb0 * d + q] : 0.;
    x1[q] = (q < d && rv1) ? a.X[(size_t)nb1 * d + q] : 0.;
  }
}

template <int ND>
__device__ __forceinline__ void pad_points(int h, bool rv0, bool rv1, const double (&xi)[ND], double (&x0)[ND],
                                           double (&x1)[ND]) {
  const int v1 = h + 16;
  const bool own1 = v1 == kMK;
#pragma unroll
  for (int q = 0; q < ND; ++q) x1[q] = own1 ? xi[q] : x1[q];
  x0[0] = rv0 ? x0[0] : 1e30 * (h + 1);
  x1[0] = (rv1 || own1) ? x1[0] : 1e30 * (v1 + 1);
}

// ... into the problem's 48 coordinate rows: partners past slot 30 wrap, copies of slots 0..15 at 31..46
template <int ND>
__device__ __forceinline__ void put_points(double* nbx, int h, const double (&x0)[ND], const double (&x1)[ND]) {
  const int v1 = h + 16;
#pragma unroll
  for (int q = 0; q < ND; ++q) {
    nbx[h * ND + q] = x0[q];
    nbx[(h + 31) * ND + q] = x0[q];
    if (v1 <= kMK) nbx[v1 * ND + q] = x1[q];
  }
}

template <int ND>
__device__ __forceinline__ double sq_dist(const double (&x)[ND], const double* xp) {
  double s = 0.;
#pragma unroll
  for (int q = 0; q < ND; ++q) {
    const double t = x[q] - xp[q];
    s += t * t;
  }
  return s;
}

// Stored distances (VecchiaRowsArgs::R): row i owns 15 x 16 records of two doubles, record (q, h) =
// { r(h, q + 1), r(h + 16, q + 1) }, r(v, delta) the distance of slot v's pair at that delta as phase 1
// computes it (wrap copies, slot 30 and the padding points included). A wave's 16-byte load of one q
// reads four contiguous 256-byte segments, one per row of the set.
constexpr int kDistRecs = 15 * 16;   // v2d records per row (kRows16DistDoubles = 2 kDistRecs)
static_assert(2 * kDistRecs == kRows16DistDoubles, "record layout");

// The row kernel's loop, in two forms: STORED = false computes every pair's distance from the
// coordinates (DIM = 2 or 0 for the generic d <= 3); STORED = true reads it from a.R (DIM unused).
template <int COV, int DIM, bool STORED>
__device__ __forceinline__ void rows16_body(const VecchiaRowsArgs& a) {
  constexpr int ND = DIM > 0 ? DIM : kD3;
  constexpr int CS = STORED ? 2 : ND;   // stored: the area holds only the stash and the [a, w] array (96 doubles)
  constexpr int PD = problem_doubles<CS>();
  static_assert(PD % 2 == 0, "16-byte aligned problems");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  const int g = lane >> 4;
  double* Cp = smem + g * PD;
  double* nbx = Cp + kPacked;
  const double var = a.var, phi = a.phi;
  const double cdiag = var * a.diag_mult + a.diag_add;
  const double delta = cdiag - var;
  const bool want_like = a.Y != nullptr;
  [[maybe_unused]] const int d = DIM > 0 ? DIM : a.d;

  // the row partials accumulate in LDS (4 problems x 6 doubles after the problems' areas): a register
  // accumulator would be live across the elimination, where the registers run out
  double* acc = smem + 4 * PD + g * kVecchiaSums;
  if ((lane & 15) < kVecchiaSums) acc[lane & 15] = 0.;
  const int total = a.r1 - a.r0;
  const ExpCoef ek = ExpCoef::scalar();
  // problem sets (4 rows) over the G waves: full rounds w + it G; the last round's E sets either on
  // waves 0..E-1 (sched 0/2) or spread evenly over the grid (sched 1), so its waves do not crowd the
  // first SIMDs the dispatcher fills
  const int nsets = (total + 3) / 4, G = gridDim.x, w = blockIdx.x;
  const int R = (nsets + G - 1) / G, E = nsets - (R - 1) * G;
  int last_set = (R - 1) * G + w;
  if (a.sched == 1) {
    const long lo = (long)w * E / G, hi = (long)(w + 1) * E / G;
    last_set = hi > lo ? (R - 1) * G + (int)lo : nsets;
  }
  auto set_at = [&](int it) { return it + 1 < R ? it * G + w : last_set; };
  // Stored form, software pipeline: a set's neighbour indices and its 15 distance records per lane (60
  // VGPRs) are loaded one set ahead, right after the elimination, when the 128 row registers are dead;
  // the traces, the sums, the next gather and the SIMD's other wave cover the stream. The indices go
  // first: the gather's Y loads wait for them alone (loads return in order), the records are waited for
  // at the first pair. Rows past r1 in a partial last set read row r0's records.
  v2d rr[STORED ? 15 : 1];
  int pnb0 = 0, pnb1 = 0;
  auto prefetch = [&](int set) {
    if constexpr (STORED) {
      const int h = lane & 15;
      const int i = a.r0 + set * 4 + g;
      const bool active = i < a.r1;
      const int k = active ? min(i, a.m) : 0;
      pnb0 = h < k ? a.nbr[(size_t)(i - a.row_base) * a.m + h] : 0;
      pnb1 = h + 16 < k ? a.nbr[(size_t)(i - a.row_base) * a.m + h + 16] : 0;
      const v2d* rp = reinterpret_cast<const v2d*>(a.R) + (size_t)((active ? i : a.r0) - a.row_base) * kDistRecs + h;
#pragma unroll
      for (int q = 0; q < 15; ++q) rr[q] = rp[q * 16];
    }
  };
  // The two waves of a SIMD hold wave slots 0 and 1 (HW_ID's WAVE_ID, bits 3:0; the instrumented variant's
  // records show it on every SIMD) and the issue arbiter prefers the older one, slot 0: left alone it runs its
  // trips in 17 k cycles, its partner in 24 k, and the partner then runs its last third alone at one wave per
  // SIMD (profiles/rows16_phase/RESULTS.md). a.prio shares the SIMD out by s_setprio, see the loop.
  PHASE_ID();
  const int odd = __builtin_amdgcn_s_getreg(kHwWaveSlot) & 1;
  if (set_at(0) < nsets) prefetch(set_at(0));
  // log(D) leaves the set loop: lane (it & 15) of each 16-lane row keeps trip it's D (1 where the slot has
  // no row), and every 16th trip, and once after the loop, all lanes take the log of theirs at once and
  // the 16 logs go to the slot's acc[0] in trip order (the additions the per-trip form made, in its order)
  double keepD = 1.;
  bool kept = false;
  auto flush_logs = [&]() {
    const double lg = log(keepD);
    double s = acc[0];
    sfor<0, 16>([&](auto L) { fmac_bcast16<decltype(L)::value, decltype(L)::value == 0>(s, lg, 1.); });
    if ((lane & 15) == 0) acc[0] = s;
    keepD = 1.;
    kept = false;
  };
  for (int it = 0; it < R; ++it) {
    const int set = set_at(it);
    if (set >= nsets) break;
    // Priority 2 or 3 outside the elimination, 0 or 1 inside it, the higher of each to the waves in even and in odd
    // slots by turns (trip parity): a wave at one of the trip's waits or LDS round trips is served before a wave
    // that has 986 independent instructions to issue, and neither wave of a SIMD is the preferred one for longer
    // than a trip, so both finish together. Issue order only: no result depends on it.
    const bool turn = (it ^ odd) & 1;
    if (a.prio) {
      if (turn) __builtin_amdgcn_s_setprio(3);
      else __builtin_amdgcn_s_setprio(2);
    }
    PHASE_MARK(it, 0);
    PHASE_END(it + 1);
    const int base = set * 4;
    int h = lane & 15;
    asm volatile("" : "+v"(h));   // lane-dependent addresses / masks recomputed per problem (not hoisted)
    const int v1 = h + 16;
    const int i = a.r0 + base + g;
    const bool active = i < a.r1;
    const int k = active ? min(i, a.m) : 0;
    const bool rv0 = h < k, rv1 = v1 < k;
    const int irow = active ? i : a.r0;

    // ---- gather (rows h and h + 16)
    int nb0, nb1;
    double xi[ND], x0[ND], x1[ND];
    if constexpr (STORED) {
      nb0 = pnb0;
      nb1 = pnb1;
    } else {
      nb0 = rv0 ? a.nbr[(size_t)(i - a.row_base) * a.m + h] : 0;
      nb1 = rv1 ? a.nbr[(size_t)(i - a.row_base) * a.m + v1] : 0;
      load_points<ND>(a, d, irow, h, rv0, rv1, nb0, nb1, xi, x0, x1);
    }
    const double yi = want_like ? a.Y[irow] : 0.;
    double y0s = (want_like && rv0) ? a.Y[nb0] : 0.;
    double y1s = (want_like && rv1) ? a.Y[nb1] : 0.;
    if constexpr (!STORED) pad_points<ND>(h, rv0, rv1, xi, x0, x1);
    cfence();   // the previous problem's LDS reads are issued before these writes
    if constexpr (!STORED) put_points<ND>(nbx, h, x0, x1);
    Cp[tri(h) + h] = rv0 ? cdiag : 1.;
    Cp[tri(v1) + v1] = rv1 ? cdiag : 1.;   // slots 30, 31: 1 (border rows, not pivots)
    lds_sync();

    // ---- 1. circulant pairs: slot v with (v + delta) mod 31, delta = 1..15, for v = h and v = h + 16
    double w0[15], w1[15];
    {
      const int b0 = tri(h) + h, b1 = tri(v1) + v1;
      // packed(v + dl, v) = b + v dl + tri(dl): the lane part carried by one add per pair, tri(dl) in the
      // store's immediate
      const unsigned h8 = h * 8, v8 = v1 * 8;
      unsigned p0 = lds_addr(Cp + b0), p1 = lds_addr(Cp + b1);
      const unsigned pw = lds_addr(Cp + b1 - 31);
      sfor<1, 16>([&](auto DL) {
        constexpr int dl = decltype(DL)::value;
        double cv, dcv;
        if constexpr (STORED) cov_dcov_r<COV>(rr[dl - 1].x, var, phi, cv, dcv, ek);
        else cov_dcov_sq<COV>(sq_dist<ND>(x0, nbx + (h + dl) * CS), var, phi, cv, dcv, ek);
        p0 += h8;
        asm("" : "+v"(p0));   // stays an add (not re-formed as h8 * dl)
        lds_write_at<dl * (dl + 1) / 2 * 8>(p0, cv);   // packed(h + dl, h)
        w0[dl - 1] = dcv;
      });
      sfor<1, 16>([&](auto DL) {
        constexpr int dl = decltype(DL)::value;
        double cv, dcv;
        if constexpr (STORED) cov_dcov_r<COV>(rr[dl - 1].y, var, phi, cv, dcv, ek);
        else cov_dcov_sq<COV>(sq_dist<ND>(x1, nbx + (v1 + dl) * CS), var, phi, cv, dcv, ek);
        // packed(v1 + dl, v1), or past slot 30 packed(v1, v1 + dl - 31) (slot 31: row 31, overwritten below)
        if constexpr (dl < 15) {
          p1 += v8;
          asm("" : "+v"(p1));
        }
        lds_write_wrap<dl>(p1, pw, cv);
        w1[dl - 1] = dcv;
      });
    }
    lds_sync();
    PHASE_MARK(it, 1);
    // border row 31 (y_nbr); row 30 (c) came from the slot-30 pairs
    Cp[tri(kMK + 1) + h] = y0s;
    if (v1 < kMK) Cp[tri(kMK + 1) + v1] = y1s;
    else if (v1 == kMK) Cp[tri(kMK + 1) + kMK] = 0.;
    lds_sync();

    // ---- 2. rows h and h + 16 into registers; c and y_nbr (their columns 30, 31) wait out the
    // elimination in the coordinate area; dC over the packed C (circulant layout W[(delta - 1) 32 + v])
    double r0[kK], r1[kK];
    {
      // M[v][c] is packed(v, c) = Cp[tri(v) + c] for c <= v and packed(c, v) = Cp[tri(c) + v] past the
      // diagonal: lane address + compile-time offset either way. Rows h <= 15 < 16 <= h + 16 settle the
      // choice for r0's columns 0 and 16..31 and r1's columns 0..16; r0[c] and r1[c + 16], c = 1..15,
      // share the lane mask h >= c and take the two-read form
      const unsigned lo0 = lds_addr(Cp + tri(h)), up0 = lds_addr(Cp + h);
      const unsigned lo1 = lds_addr(Cp + tri(v1)), up1 = lds_addr(Cp + v1);
      r0[0] = Cp[tri(h)];
#pragma unroll
      for (int c = 16; c < kK; ++c) r0[c] = Cp[tri(c) + h];
#pragma unroll
      for (int c = 0; c <= 16; ++c) r1[c] = Cp[tri(v1) + c];
      sfor<1, 16>([&](auto C) {
        constexpr int c = decltype(C)::value;
        double &p0 = r0[c], &p1 = r1[c + 16];
        lds_read_split2<c>(p0, p1, up0, up1, lo0, lo1);
      });
      // the reads above are not the compiler's to wait for: every use of their registers goes through
      // these statements, the first of which waits
      sfor<0, 3>([&](auto Q) {
        constexpr int q = 1 + 5 * decltype(Q)::value;
        double &a0 = r0[q], &a1 = r0[q + 1], &a2 = r0[q + 2], &a3 = r0[q + 3], &a4 = r0[q + 4];
        double &b0 = r1[q + 16], &b1 = r1[q + 17], &b2 = r1[q + 18], &b3 = r1[q + 19], &b4 = r1[q + 20];
        if constexpr (q == 1)
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4));
        else
          asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4));
      });
    }
    double c0, c1, dc0, dc1;
    cfence();
    {
      v2d* st = reinterpret_cast<v2d*>(__builtin_assume_aligned(nbx, 16)) + 2 * h;
      st[0] = v2d{r0[kMK], rv1 ? r1[kMK] : 0.};
      st[1] = v2d{y0s, y1s};
    }
#pragma unroll
    for (int dl = 1; dl <= 15; ++dl) {
      Cp[(dl - 1) * kK + h] = w0[dl - 1];
      Cp[(dl - 1) * kK + v1] = w1[dl - 1];
    }

    // Gauss-Jordan, 30 pivots: M[j][c] = M[c][j] from lane c mod 16 (register set c / 16)
    double i0 = 1., i1 = 1.;   // 1 / M[v][v] of rows h and h + 16, each taken in its pivot's own lane (rows 30, 31: 1)
    // pivot j's negated multipliers for rows h (pivots 0..15 only) and h + 16; the pivot row's own is 0
    auto pivot = [&](auto J, double& m0, double& m1) {
      constexpr int j = decltype(J)::value;
      constexpr int jl = j & 15;
      const double piv = bcast16<jl>(j >= 16 ? r1[j] : r0[j]);
      const double rinv = recip(piv);
      m1 = -(r1[j] * rinv);
      if constexpr (j >= 16) {
        m0 = 0.;
        own_lane<jl>(i1, m1, rinv);
      } else {
        m0 = -(r0[j] * rinv);
        own_lane<jl>(i0, m0, rinv);
      }
    };
    if (a.prio) {
      if (turn) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
    sfor<0, kMK>([&](auto J) {
      constexpr int j = decltype(J)::value;
      constexpr bool jhi = j >= 16;
      double nf0, nf1;
      pivot(J, nf0, nf1);
      // each broadcast folded into its FMAs: v_fmac_f64_dpp row_newbcast (gfx950 takes DPP on the 64-bit
      // fmac; the compiler never folds a 64-bit DPP move into its uses), so a column costs one VALU op
      // per updated row and no move -> FMA dependency
      constexpr int cA = jhi ? 0 : 16;   // the A rows take columns j + 1 .. cA - 1
      sfor<j + 1, kK>([&](auto C) {
        constexpr int c = decltype(C)::value;
        constexpr bool first = c == j + 1;   // wait states before the step's first DPP read
        const double& src = c >= 16 ? r1[j] : r0[j];
        if constexpr (c < cA) fmac_bcast16<c & 15, first>(r0[c], src, nf0);
        fmac_bcast16<c & 15, first && !(c < cA)>(r1[c], src, nf1);
      });
      // pin this step's updates (otherwise the broadcasts stay live)
      sfor<j + 1, kK>([&](auto C) {
        constexpr int c = decltype(C)::value;
        double &p0 = r0[c], &p1 = r1[c];
        if constexpr (c < cA) asm volatile("" : "+v"(p0), "+v"(p1));
        else asm volatile("" : "+v"(p1));
      });
      if constexpr (!jhi) r0[j] = nf0;   // column j of the A rows is dead: keep the step's multiplier there
    });
    {   // A rows: M[h][30..31] -= sum_{c=16..29} M[h][c] x_c, x_c = M[c][30..31] / M[c][c] (lane c - 16)
      const double na = rv1 ? -(r1[kMK] * i1) : 0., nw = rv1 ? -(r1[kMK + 1] * i1) : 0.;
      sfor<16, kMK>([&](auto C) {
        constexpr int c = decltype(C)::value;
        fmac_bcast16<c & 15, c == 16>(r0[kMK], na, r0[c]);
        fmac_bcast16<c & 15, c == 16>(r0[kMK + 1], nw, r0[c]);
      });
      // ... with the A rows' original columns 16..29; now the 16 Jordan steps on the two right-hand
      // sides alone, z_h -= f_j[h] z_j in pivot order (the same row operations, by linearity the same
      // solution). Each step reads, by DPP, what the step before wrote: the two sides alternate and
      // the first carries the remaining wait states.
      sfor<0, 16>([&](auto J) {
        constexpr int j = decltype(J)::value;
        fmac_bcast16<j, true>(r0[kMK], r0[kMK], r0[j]);
        fmac_bcast16<j>(r0[kMK + 1], r0[kMK + 1], r0[j]);
      });
    }
    PHASE_MARK(it, 2);
    if constexpr (STORED) {   // the row registers are dead: the next set's loads go out here
      cfence();
      // no branch around the loads (the records just consumed would stay live through the elimination on the
      // path that skips them): the wave's last set loads its own records again
      const int nxt = it + 1 < R ? set_at(it + 1) : nsets;
      prefetch(nxt < nsets ? nxt : set);
    }
    {   // the stashed c, y_nbr back (read before the [a, w] array below overwrites the area); dc_v = dC(v, 30):
        // the slot-30 pair at delta = v + 1 (v <= 14), slot v's pair at delta = 30 - v (v = 15..29)
      lds_sync();
      const v2d* st = reinterpret_cast<const v2d*>(__builtin_assume_aligned(nbx, 16)) + 2 * h;
      const v2d s0 = st[0], s1 = st[1];
      c0 = s0.x;
      c1 = s0.y;
      y0s = s1.x;
      y1s = s1.y;
      dc0 = Cp[h <= 14 ? h * kK + kMK : 14 * kK + 15];
      dc1 = h <= 13 ? Cp[(13 - h) * kK + v1] : 0.;
    }
    const double a0 = rv0 ? r0[kMK] * i0 : 0., w0v = rv0 ? r0[kMK + 1] * i0 : 0.;
    const double a1 = rv1 ? r1[kMK] * i1 : 0., w1v = rv1 ? r1[kMK + 1] * i1 : 0.;
    if (active && a.B_out != nullptr) {
      double* Bo = a.B_out + (size_t)(i - a.row_base) * a.m;
      if (h < a.m) Bo[h] = rv0 ? -a0 : 0.;
      if (v1 < a.m) Bo[v1] = rv1 ? -a1 : 0.;
    }

    // ---- 3. a^T dC a, w^T dC a over the circulant pairs (see vecchia_rows_kernel, bordered form)
    double tA, tV;
    {
      v2d* av2 = reinterpret_cast<v2d*>(__builtin_assume_aligned(nbx, 16));
      cfence();
      av2[h] = v2d{a0, w0v};
      if (v1 <= kMK) av2[v1] = v2d{a1, w1v};   // slot 30: a = w = 0
      av2[h + 31] = v2d{a0, w0v};
      lds_sync();
      double s10 = 0., s20 = 0., s11 = 0., s21 = 0.;
#pragma unroll
      for (int dl = 1; dl <= 15; ++dl) {
        const double wa = Cp[(dl - 1) * kK + h], wb = Cp[(dl - 1) * kK + v1];
        const v2d pa = av2[h + dl], pb = av2[v1 + dl];
        s10 = fma(wa, pa.x, s10);
        s20 = fma(wa, pa.y, s20);
        s11 = fma(wb, pb.x, s11);
        s21 = fma(wb, pb.y, s21);
      }
      tA = 2. * (a0 * s10 + a1 * s11);
      tV = w0v * s10 + a0 * s20 + w1v * s11 + a1 * s21;
    }

    // ---- 4. group sums (16 lanes) and the row partials
    double gs[8];   // ac in every lane, the others in lane 0 alone (the block below)
    sum16x8({a0 * c0 + a1 * c1, a0 * y0s + a1 * y1s, a0 * a0 + a1 * a1, a0 * w0v + a1 * w1v, dc0 * a0 + dc1 * a1,
             dc0 * w0v + dc1 * w1v, tA, tV}, gs);
    const double ac = gs[0], ay = gs[1], aa = gs[2], avv = gs[3], dca = gs[4], dcv = gs[5], ta = gs[6], tv = gs[7];
    const double D = var + a.d_nugget - ac;          // Vecchia_utils.cpp:1351, 1507, 1562
    const double Dinv = 1. / D;
    if (active && h == 0 && a.Dinv_out != nullptr) a.Dinv_out[i - a.row_base] = Dinv;
    if (want_like && active && h == 0) {
      const double By = yi - ay;
      const double u = By * Dinv;
      const double dD_var = var - delta * aa - ac;
      const double uk_var = -delta * avv;
      const double dD_rng = -(2. * dca - ta);
      const double uk_rng = -(dcv - tv);
      acc[1] += By * u;
      acc[2] += uk_var * u - 0.5 * u * u * dD_var;
      acc[3] += uk_rng * u - 0.5 * u * u * dD_rng;
      acc[4] += Dinv * dD_var;
      acc[5] += Dinv * dD_rng;
    }
    if (want_like) {
      keepD = (active && h == (it & 15)) ? D : keepD;
      kept = true;
      if ((it & 15) == 15) flush_logs();
    }
  }
  if (!want_like) return;
  if (kept) flush_logs();
  __syncthreads();
  const double* red = smem + 4 * PD;   // 4 x kVecchiaSums
  if (lane < kVecchiaSums) {
    const double v = ((red[lane] + red[kVecchiaSums + lane]) + red[2 * kVecchiaSums + lane]) + red[3 * kVecchiaSums + lane];
    a.block_sums[(size_t)blockIdx.x * kVecchiaSums + lane] = v;
  }
}

template <int COV, int DIM>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) vecchia_rows16_kernel(VecchiaRowsArgs a) {
  rows16_body<COV, DIM, false>(a);
}

// The stored-distance form (a.R set): no coordinate is read, so one instantiation serves every d.
template <int COV>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) vecchia_rows16d_kernel(VecchiaRowsArgs a) {
  rows16_body<COV, 2, true>(a);
}

// The distances of rows r0..r1, once per structure: phase 1's gather, padding, wrap copies and squared
// distance, then the device sqrt, written in the record layout above. Four rows per wave as in the row
// kernel, a set per wave and grid stride.
template <int DIM>
__global__ void __launch_bounds__(64) vecchia_rows16_dist_kernel(VecchiaRowsArgs a, double* R) {
  constexpr int ND = DIM > 0 ? DIM : kD3;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  const int g = lane >> 4, h = lane & 15, v1 = h + 16;
  double* nbx = smem + g * 48 * ND;
  const int d = DIM > 0 ? DIM : a.d;
  const int nsets = (a.r1 - a.r0 + 3) / 4;
  for (int set = blockIdx.x; set < nsets; set += gridDim.x) {
    const int i = a.r0 + set * 4 + g;
    const bool active = i < a.r1;
    const int k = active ? min(i, a.m) : 0;
    const bool rv0 = h < k, rv1 = v1 < k;
    const int irow = active ? i : a.r0;
    const int nb0 = rv0 ? a.nbr[(size_t)(i - a.row_base) * a.m + h] : 0;
    const int nb1 = rv1 ? a.nbr[(size_t)(i - a.row_base) * a.m + v1] : 0;
    double xi[ND], x0[ND], x1[ND];
    load_points<ND>(a, d, irow, h, rv0, rv1, nb0, nb1, xi, x0, x1);
    pad_points<ND>(h, rv0, rv1, xi, x0, x1);
    cfence();   // the previous set's LDS reads are issued before these writes
    put_points<ND>(nbx, h, x0, x1);
    lds_sync();
    v2d* out = reinterpret_cast<v2d*>(R) + (size_t)(irow - a.row_base) * kDistRecs + h;
#pragma unroll
    for (int dl = 1; dl <= 15; ++dl) {
      const double ra = sqrt_nonneg(sq_dist<ND>(x0, nbx + (h + dl) * ND));
      const double rb = sqrt_nonneg(sq_dist<ND>(x1, nbx + (v1 + dl) * ND));
      if (active) out[(dl - 1) * 16] = v2d{ra, rb};
    }
  }
}

constexpr int kMaxGrid = 2048;   // vecchia_rows_blocks' bound (kernels.h)

int g_last_trips = 0, g_last_prio = 0;   // vecchia_rows16_last_launch

#ifdef GPBOOST_AMD_ROWS16_PHASE
unsigned long long* phase_buffer() {   // kMaxGrid records, allocated once and kept
  static unsigned long long* buf = nullptr;
  if (buf == nullptr) HIP_CHECK(hipMalloc(&buf, sizeof(unsigned long long) * kMaxGrid * kPhaseStride));
  return buf;
}

void phase_dump(int blocks, int prio, hipStream_t s) {
  const char* path = std::getenv("GPBOOST_AMD_ROWS16_PHASE_DUMP");
  if (path == nullptr) return;
  std::vector<unsigned long long> h((size_t)blocks * kPhaseStride + 4);
  h[0] = blocks; h[1] = kPhaseStride; h[2] = kPhaseTrips | kPhaseMarks << 16; h[3] = prio;
  HIP_CHECK(hipStreamSynchronize(s));
  HIP_CHECK(hipMemcpy(h.data() + 4, phase_buffer(), sizeof(unsigned long long) * blocks * kPhaseStride, hipMemcpyDeviceToHost));
  if (FILE* f = std::fopen(path, "wb")) {
    std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
    std::fclose(f);
  }
}
#endif

template <auto KERN>
int launch16_at(size_t lds, const VecchiaRowsArgs& args, hipStream_t s) {
  VecchiaRowsArgs a = args;
  static int cap = 0;   // per kernel instance
  if (cap == 0) {
    int dev = 0, cus = 0, per_cu = 0;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KERN, 64, lds));
    cap = std::max(1, std::min(per_cu * cus, kMaxGrid));
  }
  const int need = (a.r1 - a.r0 + 3) / 4;
  int blocks = std::min(need, cap);
  // GPBOOST_AMD_ROWS16_GRID=<G> clamps the grid to [1, cap] (read at every launch): a small model can give a
  // wave many problem sets, for the tests of what the loop carries from trip to trip
  if (const char* e = std::getenv("GPBOOST_AMD_ROWS16_GRID")) blocks = std::min(blocks, std::max(1, std::atoi(e)));
  if (a.sched == 2) {   // the same number of sets per wave
    const int rounds = (need + blocks - 1) / blocks;
    blocks = (need + rounds - 1) / rounds;
  }
  g_last_trips = (need + blocks - 1) / blocks;
  // GPBOOST_AMD_ROWS16_PRIO=0 (read at every launch) leaves every wave at the default priority: A/B and tests
  const char* pe = std::getenv("GPBOOST_AMD_ROWS16_PRIO");
  g_last_prio = a.prio = (pe == nullptr || std::atoi(pe) != 0) ? 1 : 0;
#ifdef GPBOOST_AMD_ROWS16_PHASE
  a.phase = phase_buffer();
  HIP_CHECK(hipMemsetAsync(a.phase, 0, sizeof(unsigned long long) * blocks * kPhaseStride, s));
#endif
  hipLaunchKernelGGL(KERN, dim3(blocks), dim3(64), lds, s, a);
  HIP_CHECK(hipGetLastError());
#ifdef GPBOOST_AMD_ROWS16_PHASE
  phase_dump(blocks, a.prio, s);
#endif
  return blocks;
}

}  // namespace

void vecchia_rows16_last_launch(int* trips, int* prio) {
  *trips = g_last_trips;
  *prio = g_last_prio;
}

namespace {

template <int COV, int DIM>
int launch16(const VecchiaRowsArgs& a, hipStream_t s) {
  if (a.R != nullptr)
    return launch16_at<vecchia_rows16d_kernel<COV>>((size_t)(4 * problem_doubles<2>() + 4 * kVecchiaSums) * sizeof(double), a, s);
  constexpr int CS = DIM > 0 ? DIM : kD3;
  return launch16_at<vecchia_rows16_kernel<COV, DIM>>((size_t)(4 * problem_doubles<CS>() + 4 * kVecchiaSums) * sizeof(double), a, s);
}

}  // namespace

int launch_vecchia_rows16(int cov_type, const VecchiaRowsArgs& a, hipStream_t s) {
  if (a.m > kMK) Fatal("16-lane row kernel: num_neighbors %d > %d", a.m, kMK);
  if (a.r1 <= a.r0) return 0;
  const bool planar = a.d == 2;
  switch (cov_type) {
    case kMatern05: return planar ? launch16<kMatern05, 2>(a, s) : launch16<kMatern05, 0>(a, s);
    case kMatern15: return planar ? launch16<kMatern15, 2>(a, s) : launch16<kMatern15, 0>(a, s);
    case kMatern25: return planar ? launch16<kMatern25, 2>(a, s) : launch16<kMatern25, 0>(a, s);
    case kGaussian: return planar ? launch16<kGaussian, 2>(a, s) : launch16<kGaussian, 0>(a, s);
    default: Fatal("unsupported covariance type %d", cov_type);
  }
  return 0;
}

void launch_vecchia_rows16_dist(const VecchiaRowsArgs& a, double* R, hipStream_t s) {
  if (a.m > kMK) Fatal("16-lane row kernel: num_neighbors %d > %d", a.m, kMK);
  if (a.d < 1 || a.d > kD3) Fatal("16-lane row kernel: dim_gp_coords %d", a.d);
  if (a.r1 <= a.r0) return;
  const int blocks = std::min((a.r1 - a.r0 + 3) / 4, 1 << 16);
  if (a.d == 2) hipLaunchKernelGGL(vecchia_rows16_dist_kernel<2>, dim3(blocks), dim3(64), 4 * 48 * 2 * sizeof(double), s, a, R);
  else hipLaunchKernelGGL(vecchia_rows16_dist_kernel<0>, dim3(blocks), dim3(64), 4 * 48 * kD3 * sizeof(double), s, a, R);
  HIP_CHECK(hipGetLastError());
}

}  // namespace gpb_amd
