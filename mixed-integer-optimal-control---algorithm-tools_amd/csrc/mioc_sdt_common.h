// mioc_sdt_common.h -- device helpers shared by the separable L1 transform kernels (mioc_sdt.hip: the per-step
// kernel, the one-workgroup-per-row persistent driver; mioc_sdt2.hip: the two-workgroups-per-row persistent driver).
// See mioc_sdt.hip's header for the certified fixed-point transform these constants describe.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mioc {

constexpr int SD_RB = 12;                // payload rank bits (L <= 4096)
constexpr int SD_CB = 6;                 // payload near-tie count bits, below the rank (at most 56 merges per value)
constexpr int SD_CNT = (1 << SD_CB) - 1; // near-tie count mask: nonzero = flagged
constexpr int SD_PAY = (1 << (SD_CB + SD_RB)) - 1;  // payload mask: 18 low mantissa bits
constexpr int SD_GRID = 52 - SD_CB - SD_RB;         // g = 2^(E - SD_GRID) for the binade [2^E, 2^(E+1))
constexpr int SD_COOP = 8;               // listed targets up to this many: whole-workgroup scans, else one wave each
constexpr int SD_FEW = 4;                // rows with at most this many targets go straight to the exact scan
constexpr int SD_SPARSE = 4;             // rows with at most this many finite sources: direct minimum over them
constexpr int SD_LCAP = 512;             // listed targets kept in LDS; beyond, the scan sweeps every rank

// v_min_f64 without llvm.minnum's canonicalising v_max_f64 x,x on every operand (inputs are finite or +Inf)
__device__ __forceinline__ double sd_min(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// min(a, |b|) in one instruction (the abs is an operand modifier; fabs() on an asm operand would cost a v_and)
__device__ __forceinline__ double sd_min_abs(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double sd_max(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// One pass's forward and backward sweep over a line of eight values (unit step `c`, a register: 1.0 plus one ulp of the
// row's binade, so that payload bits 0..5 count the steps -- sdt_body's scale()) as ONE asm statement: per merge of
// o[x] with its neighbour o[y] + c, `t = o[y] + c; d = o[x] - t; o[x] = min(o[x], t); dmin = min(dmin, |d|)` -- the
// operations and operand order of sd_min(a, b) / sd_min_abs(dmin, a - b), 14 merges.  As separate asm statements every
// v_min_f64 pair drew the compiler's boundary wait state (`s_nop 0`) before the next merge's v_add_f64, which no
// hardware rule asks for between these instructions; inside one statement nothing is padded.  The fold into dmin sits
// behind the value's own min, off the value chain; +Inf - +Inf is NaN, which v_min_f64 ignores.
#define SD_MG(X, Y)                      \
  "v_add_f64 %9, %" #Y ", %11\n\t"       \
  "v_add_f64 %10, %" #X ", -%9\n\t"      \
  "v_min_f64 %" #X ", %" #X ", %9\n\t"   \
  "v_min_f64 %8, %8, |%10|\n\t"
__device__ __forceinline__ void sd_sweeps(double (&o)[8], double &dmin, double c) {
  double t, d;
  asm(SD_MG(1, 0) SD_MG(2, 1) SD_MG(3, 2) SD_MG(4, 3) SD_MG(5, 4) SD_MG(6, 5) SD_MG(7, 6)
      SD_MG(6, 7) SD_MG(5, 6) SD_MG(4, 5) SD_MG(3, 4) SD_MG(2, 3) SD_MG(1, 2) SD_MG(0, 1)
      : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]), "+v"(o[4]), "+v"(o[5]), "+v"(o[6]), "+v"(o[7]), "+v"(dmin),
        "=&v"(t), "=&v"(d)
      : "v"(c));
}
#undef SD_MG

// The thread index as a value the compiler cannot hoist out of the persistent driver's row loop: everything the
// row body derives from it (LDS addresses of the passes, swizzles, store offsets) is recomputed per row instead of
// being kept live in VGPRs across the whole loop, which would leave the body no registers (spills to scratch join
// the vector-memory queue the driver keeps busy).
__device__ __forceinline__ int sd_tid() {
  int t = (int)threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// LDS-only workgroup barrier: __syncthreads() would also wait for every outstanding global load and store of
// the wave, which the persistent driver keeps in flight across the row body on purpose
__device__ __forceinline__ void sd_bar() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// merge two disjoint candidate sets (their minima a, b): the smaller keeps its payload; a near tie counts
// one.  |a - b| is exact (one binade), +Inf - +Inf is NaN and never flags.
__device__ __forceinline__ double sd_merge(double a, double b, double tol) {
  const double m = sd_min(a, b);
  const bool close = fabs(a - b) <= tol;
  return __hiloint2double(__double2hiint(m), (int)((unsigned)__double2loint(m) + (close ? 1u : 0u)));  // v_addc
}

// Wave-wide reductions through DPP (no LDS round trip, unlike __shfl_xor's ds_bpermute): four steps leave every
// lane with its 16-lane row's result (quad_perm xor 1, xor 2, row_half_mirror, row_mirror), then the four row
// results are read as scalars.  bound_ctrl: every lane has a source under these controls, so no old value is
// needed (and no register initialised for it).
template <int CTRL>
__device__ __forceinline__ int sd_dpp_i(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ double sd_dpp_d(double x) {
  return __hiloint2double(sd_dpp_i<CTRL>(__double2hiint(x)), sd_dpp_i<CTRL>(__double2loint(x)));
}
__device__ __forceinline__ double sd_rdl(double x, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
// (min and max without llvm.minnum's canonicalisation: the operands are finite, ±Inf or a quiet NaN, which v_min_f64 /
// v_max_f64 ignore).  The result is valid in lanes 0..15 only (lane 0 stores it): after the four DPP steps each lane
// holds its row's result, and row 0 folds in the other three rows' as scalar operands.  Each step's min and max share
// one asm statement, so the compiler's wait state before the next DPP read comes once per step.
__device__ __forceinline__ void sd_minmax(double &mn, double &mx, double a, double b) {
  asm("v_min_f64 %0, %0, %2\n\tv_max_f64 %1, %1, %3" : "+v"(mn), "+v"(mx) : "v"(a), "v"(b));
}
__device__ __forceinline__ void sd_minmax_s(double &mn, double &mx, double a, double b) {  // a, b wave-uniform
  asm("v_min_f64 %0, %2, %0\n\tv_max_f64 %1, %3, %1" : "+v"(mn), "+v"(mx) : "s"(a), "s"(b));
}
__device__ __forceinline__ void sd_wave_stats(double &mn, double &mx) {
#define SD_STEP(C) sd_minmax(mn, mx, sd_dpp_d<C>(mn), sd_dpp_d<C>(mx));
  SD_STEP(0xB1) SD_STEP(0x4E) SD_STEP(0x141) SD_STEP(0x140)
#undef SD_STEP
  const double n1 = sd_rdl(mn, 16), n2 = sd_rdl(mn, 32), n3 = sd_rdl(mn, 48);
  const double x1 = sd_rdl(mx, 16), x2 = sd_rdl(mx, 32), x3 = sd_rdl(mx, 48);
  sd_minmax_s(mn, mx, n1, x1);
  sd_minmax_s(mn, mx, n2, x2);
  sd_minmax_s(mn, mx, n3, x3);
}

// The wave's (value, rank) minimum, ties to the lower rank, wave-uniform in every lane.  bj < 0: the lane has no
// candidate (its bv is +Inf and never the only holder of a finite minimum); compared as unsigned, such a lane loses to
// every rank, and a wave without a candidate returns bj = -1.  Every lane active.
// The value by DPP as in sd_wave_stats (min and max in one statement per step: no wait state after the v_min_f64; the
// max is not used), then the smallest rank among the lanes that hold the minimum, by the same steps on integers.  The
// 16-lane rows are folded with row_bcast:15 (rows 1 and 3 take lane 15 of the row below) and row_bcast:31 (rows 2 and 3
// take lane 31), which leaves the wave's result in lane 63: three scalar registers in all, where reading the four row
// results as scalars takes twelve -- the persistent driver's row loop has none to spare.
template <int CTRL, int ROWS>
__device__ __forceinline__ int sd_dpp_rows_i(int x) {  // lanes of the rows outside ROWS keep x
  return __builtin_amdgcn_update_dpp(x, x, CTRL, ROWS, 0xF, false);
}
template <int CTRL, int ROWS>
__device__ __forceinline__ double sd_dpp_rows_d(double x) {
  return __hiloint2double(sd_dpp_rows_i<CTRL, ROWS>(__double2hiint(x)), sd_dpp_rows_i<CTRL, ROWS>(__double2loint(x)));
}
__device__ __forceinline__ void sd_wave_argmin(double &bv, int &bj) {
  double mn = bv, mx = bv;
#define SD_STEP(C) sd_minmax(mn, mx, sd_dpp_d<C>(mn), sd_dpp_d<C>(mx));
  SD_STEP(0xB1) SD_STEP(0x4E) SD_STEP(0x141) SD_STEP(0x140)
#undef SD_STEP
  sd_minmax(mn, mx, sd_dpp_rows_d<0x142, 0xA>(mn), sd_dpp_rows_d<0x142, 0xA>(mx));
  sd_minmax(mn, mx, sd_dpp_rows_d<0x143, 0xC>(mn), sd_dpp_rows_d<0x143, 0xC>(mx));
  const double wm = sd_rdl(mn, 63);
  unsigned c = bv == wm ? (unsigned)bj : ~0u;
#define SD_STEP(C) c = min(c, (unsigned)sd_dpp_i<C>((int)c));
  SD_STEP(0xB1) SD_STEP(0x4E) SD_STEP(0x141) SD_STEP(0x140)
#undef SD_STEP
  c = min(c, (unsigned)sd_dpp_rows_i<0x142, 0xA>((int)c));
  c = min(c, (unsigned)sd_dpp_rows_i<0x143, 0xC>((int)c));
  bv = wm;
  bj = __builtin_amdgcn_readlane((int)c, 63);
}

// LDS position of rank r (3 bits per dimension): XOR swizzle so that each 32-lane half of a pass reads
// 32 distinct 8-byte bank slots in every pass: slot = (x0 ^ x1) + 8·((x1 ^ x2) & 3)
__device__ __forceinline__ int sd_swz(int r) { return r ^ ((r >> 3) & 7) ^ (((r >> 6) & 3) << 3); }

// sd_swz(q + 8^(M-1)·s), the LDS position of rank q with top coordinate s (q < 8^(M-1)).  The swizzle reads rank bits
// 3..7 only: at M = 4 the top coordinate (bits 9..11) is outside them, so it is sd_swz(q) plus the top term, and a
// loop over s hoists the swizzle; at M = 3 the top coordinate's low bits (6, 7) feed the swizzle
template <int M>
__device__ __forceinline__ int sd_swz_top(int q, int s) {
  constexpr int T = 1 << (3 * (M - 1));
  if constexpr (3 * (M - 1) >= 8)
    return sd_swz(q) + T * s;
  else
    return sd_swz(q + T * s);
}

// rank of element x of line q in the pass over dimension m (q enumerates the other coordinates, lowest
// dimension fastest)
__device__ __forceinline__ int sd_rank(int q, int m, int x) {
  const int lo = q & ((1 << (3 * m)) - 1);
  return lo | (x << (3 * m)) | ((q >> (3 * m)) << (3 * (m + 1)));
}

// L1 distance between two ranks of the 8^M grid with one v_sad_u8: a rank spread to one byte per dimension
__device__ __forceinline__ unsigned sd_bytes(unsigned r) {
  return (r & 7u) | ((r & 0x38u) << 5) | ((r & 0x1C0u) << 10) | ((r & 0xE00u) << 15);
}
__device__ __forceinline__ unsigned sd_l1(unsigned pa, unsigned pb) { return __builtin_amdgcn_sad_u8(pa, pb, 0u); }

typedef unsigned int sd_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int sd_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sd_rsrc(const double *base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(base), 0, bytes, 0x00020000);
}

// Wave-local LDS ordering: this wave's LDS stores are complete before its next LDS reads (LDS instructions of one
// wave execute in order; the wait also keeps the compiler from moving accesses across)
__device__ __forceinline__ void sd_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

}  // namespace mioc
