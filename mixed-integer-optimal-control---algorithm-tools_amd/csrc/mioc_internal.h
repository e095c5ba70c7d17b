// mioc_internal.h -- context and kernel-launch declarations shared by the C ABI (mioc_api.cpp)
// and the gfx950 kernels (mioc_*.hip).
// Device memory is owned: every buffer of the context, of its two DP slots (mioc_ctx::Slot) and of the heat and
// convolution objectives is a DevBuf (pointer + capacity, freed by its destructor), pinned host words are
// PinnedWords.  The strides of the last DP's tables are computed once per bellman call into mioc_ctx::lay (DpLayout),
// which the backtrack and the read-back entry points use.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mioc.h"

namespace mioc {

constexpr int kMaxM = 8;          // controls per tuple supported by the kernels
constexpr int kRowTile = 64;      // budget rows per lane-tile; fronts are padded to a multiple

// An owned device buffer: a pointer and its capacity in bytes.  Move-only (no copies: the move members suppress
// them); the destructor frees.
template <typename T>
struct DevBuf {
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) reset(), p = o.p, cap = o.cap, o.p = nullptr, o.cap = 0;
    return *this;
  }
  ~DevBuf() { reset(); }
  T *get() const { return p; }
  size_t bytes() const { return cap; }
  void reset() {
    if (p) hipFree(p);
    p = nullptr, cap = 0;
  }
  // exactly `bytes`, contents not kept; false (and empty) when the device has no room.  No synchronisation: for
  // buffers that nothing in flight reads, and callers that word their own error
  bool alloc(size_t bytes) {
    reset();
    if (hipMalloc(reinterpret_cast<void **>(&p), bytes) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      return false;
    }
    cap = bytes;
    return true;
  }
  // at least need_bytes (contents not kept): the buffer stays if it is large enough, else the device is synchronised
  // (the old buffer may still be read by a backtrack in flight on the other stream) and it is replaced
  int grow(mioc_ctx *ctx, size_t need_bytes, const char *what);

 private:
  T *p = nullptr;
  size_t cap = 0;
};

// One pinned host allocation of four 32-bit words, the target of small device-to-host copies.
struct PinnedWord {
  PinnedWord() = default;
  PinnedWord(const PinnedWord &) = delete;
  PinnedWord &operator=(const PinnedWord &) = delete;
  ~PinnedWord() {
    if (p) hipHostFree(p);
  }
  bool alloc() { return hipHostMalloc(reinterpret_cast<void **>(&p), 16, 0) == hipSuccess; }
  int32_t *get() const { return p; }
  int32_t &operator[](int i) const { return p[i]; }

 private:
  int32_t *p = nullptr;
};

// Device-side view of the flattened level table + switching cost, passed by value to kernels.
struct LevelsDev {
  int M = 0;
  int L = 0;
  const double *nuval = nullptr;   // [L][M] level values per iterator rank
  const int32_t *nuint = nullptr;  // [L][M] same, as int32 (distance keys)
  const int32_t *gidx = nullptr;   // [L] grid linear index per rank (argmin tie-break)
  const int32_t *vals = nullptr;   // [Σ counts] level values per dimension, concatenated
  const int32_t *voff = nullptr;   // [M+1] offsets of each dimension's values in vals
  const int32_t *g2r = nullptr;    // [Lgrid] rank of each grid tuple (-1: not admissible); null if too large
  int p_kind = MIOC_P_INF;
  int p_int = 1;
  double beta = 0.0;
  double inv_beta = 0.0;           // fl(1/beta) for beta > 0 (separable transform scale)
  const double *costlut = nullptr; // beta*weight by integer key (P_INF: [beta], P_ONE/P_INTLUT)
  const double *costtab = nullptr; // [L][L] beta*weight (P_TABLE only)
};

// One batch of K subproblems sharing levels, cost, nt, B.
struct ProblemDev {
  int K = 0;
  int M = 0;
  int nt = 0;
  int B = 0;
  int RP = 0;                      // padded rows per front column: roundup(B+1, 64)
  double dt = 0.0;
  const double *df = nullptr;      // [K][nt][M]  (each subproblem nx x nt column-major)
  const double *uold = nullptr;    // [K][nt][M]
  const int32_t *Bvec = nullptr;   // backtrack: per-subproblem budget B'_k (null: one B' for the batch)
  const int32_t *gate = nullptr;   // device TRM control (mioc_trm_attach): backtrack kernels return at once while *gate == 0
  // the one-workgroup p = Inf recursion as the device-side redo of a segmented one: it runs only if the segmented
  // launch's error word (a timed-out wait) is set, and then counts itself in *redo_count (null: an ordinary launch)
  const int32_t *redo_gate = nullptr;
  int32_t *redo_count = nullptr;
};
// the kernels of a gated call return at once (uniformly) while the device TRM control's gate word is 0
__device__ __forceinline__ bool gate_closed(const int32_t *gate) { return gate && *gate == 0; }
// a redo launch (ProblemDev::redo_gate) returns at once unless the launch it backs up timed out
__device__ __forceinline__ bool redo_skip(const ProblemDev &P) {
  if (!P.redo_gate) return false;
  if (*P.redo_gate == 0) return true;
  if (P.redo_count && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(P.redo_count, 1);
  return false;
}

// Product grid with consecutive integer levels per dimension (the L1-ball pyramid's domain).
struct PyrGeom {
  int M = 0;
  int ncol = 0;                    // grid columns: L / n[0]
  int Smax = 0;                    // largest L1 distance: sum_m (n_m - 1)
  int n[kMaxM] = {};               // levels per dimension
  int base[kMaxM] = {};            // first level value per dimension
  int cstride[kMaxM] = {};         // column-index stride of dimension m >= 1
};

struct Start {                      // backtrack start cell per subproblem
  double phi;
  int32_t c;
  int32_t r;
  int32_t status;
  int32_t pad;
};

// The backtrack budget of subproblem k: the per-subproblem B'_k when the call passed a device vector
// (mioc_backtrack_batch_budgets_device), else the call's B'.  A B'_k outside [0, B] is checked here, on the device,
// so that the call needs no host read-back of the budgets: the start kernel records MIOC_ESTATE as the
// subproblem's status (its u row becomes NaN in k_expand, the walk skips it) and returns -1.
__device__ __forceinline__ int start_budget(const ProblemDev &P, int k, int Bu, Start *start) {
  if (!P.Bvec) return Bu;
  const int b = P.Bvec[k];
  if (b >= 0 && b <= P.B) return b;
  if (threadIdx.x == 0) {
    Start st;
    st.phi = __builtin_nan("");
    st.c = 0;
    st.r = -1;
    st.status = MIOC_ESTATE;
    st.pad = 0;
    start[k] = st;
  }
  return -1;
}

// ---- kernel launchers (mioc_generic.hip) ------------------------------------------------------
hipError_t launch_validate(hipStream_t s, const ProblemDev &P, double *uold_own, const double *numin,
                           const double *numax, int32_t *flags);
hipError_t launch_generic_terminal(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, double *front,
                                   size_t front_stride);
hipError_t launch_generic_step(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, int i,
                               const double *psi, double *phi, void *U, int ubytes, size_t front_stride,
                               size_t u_stride_k);
hipError_t launch_generic_argmin0(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const double *front0,
                                  size_t front_stride, int Bu, Start *start);
hipError_t launch_uold_rank(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, int32_t *urank);
hipError_t launch_generic_walk(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const void *U, int ubytes,
                               size_t u_stride_k, const Start *start, const int32_t *urank, int32_t *ranks,
                               int32_t *counters);
hipError_t launch_expand(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const Start *start,
                         const int32_t *ranks, double *u_out, double *phi_star, int32_t *status);

// ---- L1-ball pyramid (mioc_pyramid.hip) + staging-layout backtrack (mioc_generic.hip) -------------
// same2 (nullable): [K][nt] int32, u_old(s) == u_old(s + 2) bit for bit (0 for s >= nt - 2); strad (nullable):
// [K][nt][8 waves][32] uint16, per wave of the persistent separable driver the in-wave offsets of the second elements
// of seam-straddling position pairs
// counters (nullable): [3] += seams a wave's list could not hold (an internal-consistency failure, must stay 0)
// k_pinf_recur_ws's segment flags: this many 32-bit words apart (packed, one line held all 13 segments' flags of
// C2 / C3; 128 bytes apart the single-subproblem recursion is 2-3 % faster, profiles/round6_flag_stride.txt); the
// segmented p = Inf kernels' error word sits at K · pinf_recur_segments · this (k_pinf_recur_mcw keeps its
// flags packed: spaced out, it was 6 % slower)
#ifndef PINF_WS_FLAG_STRIDE
#define PINF_WS_FLAG_STRIDE 32
#endif
// k_fsep2's segment records {outbox token, consumed token}: this many 32-bit words apart (>= 2)
#ifndef FSEP_FLAG_STRIDE
#define FSEP_FLAG_STRIDE 2
#endif
// k_sdt_run's row flags (done, loaded): this many 32-bit words apart.  Packed (1), one 128-byte line carried the flags
// of 32 rows, each stored every item by its own row and polled by the 28 rows around it; 32-byte spacing is 2 % faster
// at full C4 and cuts the run-to-run spread (7.02-7.28 -> 6.94-7.03 us per DP step, profiles/round6_flag_stride.txt)
#ifndef SDT_FLAG_STRIDE
#define SDT_FLAG_STRIDE 8
#endif
hipError_t launch_pyr_order(hipStream_t s, const ProblemDev &P, const PyrGeom &G, uint32_t *perm,
                            int32_t *same2 = nullptr, uint16_t *strad = nullptr, int32_t *counters = nullptr);
hipError_t launch_pyr_terminal(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const uint32_t *perm, double *S,
                               size_t s_stride);
hipError_t launch_pyr_step(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const PyrGeom &G, int i,
                           const uint32_t *perm, const double *Sin, double *Sout, uint16_t *UU, size_t s_stride,
                           size_t uu_stride_k, int32_t *counters);
size_t pyr_lds_bytes(const PyrGeom &G);
// separable L1 transform (mioc_sdt.hip): same staging layout, 8^M grids (M = 3, 4), beta > 0
bool sdt_supported(const PyrGeom &G);
bool sdt_seam_lists(const PyrGeom &G);  // the persistent driver loads straddling pair elements by seam lists (k_pyr_order)
size_t sdt_lds_bytes(const PyrGeom &G);
constexpr int kSdtMaxBuffers = 256;  // persistent separable transform: staging buffers S_i, step i in buffer i % NB
constexpr int kSdtDefaultBuffers = 256;  // at most (C4: 255 x 8.4 MB + the 2.1 GB row-0 array fit the 4 GiB buffer range)
hipError_t launch_sdt_step(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const PyrGeom &G, int i,
                           const uint32_t *perm, const double *Sin, double *Sout, uint16_t *UU, size_t s_stride,
                           size_t uu_stride_k, int32_t *counters);
// persistent driver: per subproblem one region of kstride doubles = NB staging buffers of (B+1)·L, then row 0 of
// every step (nt·L, at r0off); k_sdt_chain + k_sdt_row0 fill row 0, its U rows and S_0 row 0, then k_sdt_run
hipError_t launch_sdt_prep(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const PyrGeom &G,
                           const uint32_t *perm, double *V, double *S, size_t kstride, size_t r0off, uint16_t *UU,
                           size_t uu_stride_k);
// same2[k][s] = (u_old(s) == u_old(s + 2)), written by launch_pyr_order: the persistent driver's sphere-order reuse
hipError_t launch_sdt_run(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const PyrGeom &G,
                          const uint32_t *perm, const int32_t *same2, const uint16_t *strad, double *S, size_t kstride,
                          int NB, uint16_t *UU,
                          size_t uu_stride_k, int32_t *counters, int32_t *flags, int nwg, unsigned spin_limit,
                          size_t lds, bool one_row);  // one_row: nwg = K·B, every workgroup owns one row (k_sdt_run1)
int sdt_run_blocks_per_cu(const PyrGeom &G, size_t lds);
hipError_t launch_stage_argmin0(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const uint32_t *perm,
                                const double *S0, size_t s_stride, int Bu, Start *start);
hipError_t launch_stage_walk(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const uint16_t *UU,
                             size_t uu_stride_k, const Start *start, const int32_t *urank, int32_t *ranks,
                             int32_t *counters);

// ---- fused small-state DP (mioc_fused.hip): one workgroup per subproblem, front in LDS -------------
bool fused_supported(int L, int B, size_t *lds_out);
hipError_t launch_fused_run(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, double *front0,
                            size_t front_stride, uint8_t *U, size_t u_stride_k);
// p = 1 on a 2-D product grid of consecutive levels: the fused DP with the separable L1 transform
bool fsep_supported(const PyrGeom &G, int B, size_t *lds_out, int *threads_out);
int fused_blocks_per_cu(int algo_sep, const PyrGeom &G, int L, int B);  // occupancy query (diagnostics [7])
hipError_t launch_fsep_run(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const PyrGeom &G, double *front0,
                           size_t front_stride, uint8_t *U, size_t u_stride_k, int32_t *counters);
// ... round-3 layout (mioc_fsep.hip): two lanes per row, the front updated in place, optionally S row segments per
// subproblem on S workgroups chained by an outbox ring (strong scaling)
struct FsepPlan {
  int S = 1, RS = 0, W = 0;  // segments, rows per segment (at most W waves of rows), waves per workgroup
  int rows = 0, koff = 0;    // LDS front rows, K table offset (doubles)
  int stg = 0, slot_bytes = 0;  // S > 1: inbox staging offset (doubles), ring slot bytes
  int threads = 0;
  int lanes = 2;  // lanes per budget row (4: row segments of small batches)
  size_t lds = 0;
};
bool fsep2_plan(const PyrGeom &G, int B, int S, FsepPlan *out);
int fsep2_blocks_per_cu(const PyrGeom &G, const FsepPlan &p);
hipError_t launch_fsep2(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const PyrGeom &G, const FsepPlan &p,
                        double *front0, size_t front_stride, uint8_t *U, size_t u_stride_k, int32_t *counters,
                        double *ring, int NB, int32_t *flags, unsigned spin_limit);

// ---- p = Inf collapse (mioc_pinf.hip) -----------------------------------------------------------
struct PinfDev {
  int BW = 0;                      // budget classes tracked: bmax+1 <= B+1
  int BWP = 0;                     // padded class-row width: pow2 >= max(8, BW) (pad = +Inf / -1)
  double *kmin = nullptr;          // [K][nt][BWP] min over ranks of class b of K_r (T1 at terminal)
  double *k2 = nullptr;            // [K][nt][BWP] second-smallest distinct value in the class
  int32_t *kfirst = nullptr;       // [K][nt][BWP] first rank attaining kmin
  double *R = nullptr;             // [K][nt][RP] row minima R_i[c] = min_r Φ_i[c, r]
  double *kabs = nullptr;          // [K][nt] max |K_l(i)| over the levels of classes < BW (rounding bound)
  int CH = 0, W = 0;               // the walk's staged steps per chunk and LDS row width (pinf_plan)
  // segmented walk (mioc_pinf.hip): the step's winning class per row, when it does not depend on the state
  uint8_t *ftab = nullptr;         // [K][nt][RP] class b* of row c' at step j, 0xFF: state-dependent / +Inf
  int32_t *fseg = nullptr;         // [K][nseg][RP] row after the G steps of segment g entered at row c' (-1: none)
  int32_t *fneed = nullptr;        // [K + 1] 1: subproblem left to the serial walk; [K]: their count
};
// the walk's chunk and band for a p = Inf problem (mioc_pinf.hip)
void pinf_plan(int RP, int nt, PinfDev &D);
// variant (nullable): the name of the class-table kernel launched (k_pinf_prep, k_pinf_prep_m or k_pinf_prep_small),
// which names timing window 2 (mioc_kernel_stats)
hipError_t launch_pinf_prep(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const PinfDev &D,
                            const char **variant = nullptr);
// ncu: the device's CUs; flags (K·pinf_recur_segments·PINF_WS_FLAG_STRIDE + 1 zeroed words, or null): lets few
// subproblems run in row segments on several CUs, *segmented then says so (the caller checks the error word, the last
// of those words, after it: check_run)
// variant (nullable): the name of the recursion kernel launched (k_pinf_recur_ws, k_pinf_recur_mcw, k_pinf_recur_xr or
// k_pinf_recur), which names the timing window (mioc_kernel_stats)
hipError_t launch_pinf_recur(hipStream_t s, const ProblemDev &P, const PinfDev &D, int ncu, int32_t *flags,
                             unsigned spin_limit, bool *segmented, const char **variant = nullptr);
int pinf_recur_segments(const ProblemDev &P);  // 8-row segments of k_pinf_recur_mcw per subproblem (the error word's offset)
hipError_t launch_pinf_start(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const PinfDev &D, int Bu,
                             Start *start, int32_t *zero2 = nullptr, int32_t *fneed = nullptr);
hipError_t launch_pinf_walk(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const PinfDev &D,
                            const Start *start, int32_t *ranks, int32_t *nfallback, const int32_t *need);
// segmented walk: steps per segment and segment count for nt steps
void pinf_fplan(int nt, int *G, int *nseg);
hipError_t launch_pinf_fwalk(hipStream_t s, const ProblemDev &P, const LevelsDev &Lv, const PinfDev &D,
                             const Start *start, int32_t *ranks);


// ---- trust-region quantities around the DP (mioc_trm.hip) ---------------------------------------
struct TrmDev {
  int K = 0, M = 0, nt = 0, L = 0;
  double dt = 0.0, beta = 0.0;
  int p_kind = MIOC_P_ONE, p_int = 1;
  int mode = 0;                    // 1: int_val, 2: TV(u_old), 4: TV(u)
  int fma = 0;                     // int_val accumulated with fma (MIOC_OPT_PRED_FMA)
  const double *df = nullptr;      // [K][nt][M]
  const double *uold = nullptr;    // [K][nt][M]
  const double *u = nullptr;       // [K][nt][M] control values, or null: the levels of `ranks`
  const int32_t *ranks = nullptr;  // [K][nt] iterator ranks of u (u == null)
  const double *nuval = nullptr;   // [L][M]
  const int32_t *vals = nullptr, *voff = nullptr, *g2r = nullptr;  // grid lookup (MIOC_P_TABLE)
  const double *tvw = nullptr;     // unscaled weights: by key (MIOC_P_INTLUT) or [L][L] (MIOC_P_TABLE)
  long long tvw_len = 0;
  double *out_int = nullptr, *out_told = nullptr, *out_tnew = nullptr, *out_pred = nullptr;  // [K] each
  int32_t *err = nullptr;          // bit 0: a TV key / rank outside the weight table
  const int32_t *gate = nullptr;   // device TRM control gate (see ProblemDev::gate)
};
hipError_t launch_trm_pred(hipStream_t s, const TrmDev &T);
hipError_t launch_trm_decide(hipStream_t s, int K, const double *J_old, const double *J_new, const double *tv_old,
                             const double *tv_new, const double *pred, double beta, double sigma, double *ared,
                             int32_t *decision);

// dynamic LDS of k_rand_start: one bit per step in 32-bit words, then one count per thread of its 256
constexpr size_t rand_start_lds(int64_t nt) { return ((size_t)(nt + 31) / 32 + 256) * sizeof(uint32_t); }
constexpr int64_t kRandStartMaxNt = (65536 / 4 - 256) * 32;  // the largest nt with rand_start_lds(nt) <= 64 KB
static_assert(rand_start_lds(kRandStartMaxNt) == 65536 && rand_start_lds(kRandStartMaxNt + 1) > 65536, "LDS bound");
hipError_t launch_rand_start(hipStream_t s, int K, int nt, int jumps, uint64_t seed, const LevelsDev &Lv, double *U);
// device-resident TRM control (mioc_trm.hip): the state block's layout and flag bits, shared with the mixed control
// (mioc_mixed.hip), which reads and clears the stop flag
constexpr int TRM_INNER = 1, TRM_HALVED = 2, TRM_STOP = 4, TRM_COPY_U = 8, TRM_COPY_UOLD = 16;

struct TrmState {
  int32_t *gate, *any_active, *any_copy;
  double *Dk, *tv_old;
  int32_t *k, *flags, *iters;
};
__host__ __device__ inline TrmState trm_state_layout(void *base, int K) {
  TrmState S;
  char *b = static_cast<char *>(base);
  S.gate = reinterpret_cast<int32_t *>(b);
  S.any_active = S.gate + 1;
  S.any_copy = S.gate + 2;
  S.Dk = reinterpret_cast<double *>(b + 16);
  S.tv_old = S.Dk + K;
  S.k = reinterpret_cast<int32_t *>(S.tv_old + K);
  S.flags = S.k + K;
  S.iters = S.flags + K;
  return S;
}

// block-wide OR of one flag per thread into *out (one workgroup)
__device__ __forceinline__ void trm_block_or(int v, int32_t *out) {
  __shared__ int s_or;
  if (threadIdx.x == 0) s_or = 0;
  __syncthreads();
  if (__ballot(v) && (threadIdx.x & 63) == 0) atomicOr(&s_or, 1);
  __syncthreads();
  if (threadIdx.x == 0) *out = s_or;
}

// acc + x[0] + x[1] + ... in this order, by one lane (the sequential sums of k_trm_pred and k_mixed_fan)
__device__ __forceinline__ double fold(const double *x, int n, double acc) {
  int j = 0;
  for (; j + 8 <= n; j += 8) {
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = x[j + q];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc = acc + v[q];
  }
  for (; j < n; ++j) acc = acc + x[j];
  return acc;
}

// ---- mixed control: the continuous step beside the DP (mioc_mixed.hip) -----------------------------------------
constexpr int kMixedChunk = 2048;  // per-element slope terms folded per LDS chunk of k_mixed_fan
size_t mixed_state_bytes(int K);
hipError_t launch_rows_copy(hipStream_t s, const int32_t *gate, int K, int nt, double *dst, int dst_nx, int dst_row0,
                            const double *src, int src_nx, int src_row0, int nrows);
hipError_t launch_mixed_fan(hipStream_t s, int K, int R, int nu, int nx, int nt, double tau, const double *x,
                            const double *df, const double *lo, const double *hi, void *mstate, double *xfan,
                            double *slope);
hipError_t launch_mixed_select(hipStream_t s, int K, int R, int nu, int nx, int nt, double c1, double smax, double ctol,
                               void *mstate, void *trm_state, const double *xfan, const double *slope,
                               const double *Jfan, double *J_old, double *x);
hipError_t launch_mixed_live(hipStream_t s, int K, void *mstate, void *trm_state);

size_t trm_state_bytes(int K);
hipError_t launch_trm_outer_begin(hipStream_t s, int K, void *state, const double *tv_u, double D0, int B,
                                  int32_t *budgets);
hipError_t launch_trm_inner_end(hipStream_t s, int K, void *state, double beta, double sigma, int kmax, double tau,
                                int B, const double *int_val, const double *tv_new, const double *J_new,
                                double *J_old, double *J, double *tv_u, int32_t *budgets, int32_t *decision,
                                size_t n, const double *trial, double *u, double *u_old);
hipError_t launch_ode_eval(hipStream_t s, const int32_t *gate, int problem, int K, int nt, double tau, const double *params, int y0off,
                           const double *X, double *J, double *DF, double *ST);

// orders the context's stream after its in-flight p = Inf backtracks (mioc_api.cpp); every C ABI call that is not a
// bellman or a backtrack calls it first
int join_bt(mioc_ctx *ctx);
#define MIOC_JOIN_BT(ctx)                         \
  do {                                            \
    const int rcj_ = mioc::join_bt(ctx);          \
    if (rcj_) return rcj_;                        \
  } while (0)

struct HeatState;  // mioc_heat.hip: the PDE heat objective's device matrices (mioc_heat_setup)
void heat_free(HeatState *h);
struct ConvState;  // mioc_conv.hip: the convolution objective's device tables (mioc_conv_setup)
void conv_free(ConvState *c);

// Where the tables of the last DP lie: filled once by run_bellman (mioc_api.cpp), read by the backtrack, the timeout
// check and the read-back entry points.
struct DpLayout {
  int algo = 0;
  int ubytes = 1;            // bytes per argmin cell
  size_t s_stride = 0;       // cells of one step's front / argmin table: (B + 1)·L
  size_t stage_kstride = 0;  // doubles between two subproblems' staging blocks (pyramid / separable)
  size_t uu_stride_k = 0;    // cells between two subproblems' staged argmin tables UU
  size_t u_stride_k = 0;     // cells between two subproblems' argmin tables U (generic / fused)
  size_t front_stride = 0;   // doubles of one subproblem's front: L·RP
  // the timeout word of a DP whose workgroups hand rows to each other (run_pending): buffer and word offset
  const DevBuf<int32_t> *err_buf = nullptr;
  size_t err_off = 0;
};

}  // namespace mioc

// ---- the context ----------------------------------------------------------------------------------
struct mioc_ctx {
  template <typename T>
  using Buf = mioc::DevBuf<T>;

  int device = 0;
  int ncu = 0;                     // the device's compute units, a CU's LDS and a workgroup's largest LDS share
  int cu_lds = 0, wg_lds = 0;      // (queried once, mioc_create)
  hipStream_t stream = nullptr;
  std::string err;
  int64_t opt_algo = MIOC_ALGO_AUTO;
  bool timing = false;

  // levels (host copies + device tables)
  bool have_levels = false;
  int64_t M = 0, L = 0, Lgrid = 0;
  std::vector<int64_t> counts, values;
  std::vector<int32_t> tuples;     // [L][M] 1-based
  std::vector<double> nuval_h;     // [L][M]
  std::vector<int32_t> gidx_h;     // [L] grid-linear index of each admissible tuple
  std::vector<double> numin_h, numax_h;
  Buf<double> d_nuval;
  Buf<int32_t> d_nuint, d_gidx, d_vals, d_voff, d_g2r;
  Buf<double> d_numin, d_numax;

  // cost
  bool have_cost = false;
  int32_t p_kind = MIOC_P_INF;
  int64_t p_int = 1;
  double beta = 0.0;
  std::vector<double> table;
  Buf<double> d_costlut, d_costtab;
  Buf<double> d_tvw;               // unscaled weight table for TV_p (MIOC_P_INTLUT / MIOC_P_TABLE)
  int64_t tvw_len = 0;
  bool pred_fma = false;           // MIOC_OPT_PRED_FMA
  Buf<double> d_pred_own;          // mioc_pred staging: 4 doubles, then the TV error flag (int32)
  bool trm_pending = false;
  const int32_t *Bvec = nullptr;   // per-subproblem B' of the running backtrack (mioc_backtrack_batch_budgets_device)
  Buf<double> d_ode_state;         // forward states: [K][nt][2] of mioc_ode_eval_device, [nt][ny][K] of an ODE program
  mioc::HeatState *heat = nullptr; // mioc_heat_setup / mioc_heat_eval_device
  mioc::ConvState *conv = nullptr; // mioc_conv_setup / mioc_conv_eval_device
  int64_t costlut_len = 0;

  // last DP (its inputs are the current slot's, below)
  bool have_dp = false;
  mioc::DpLayout lay;
  int K = 0, nt = 0, B = 0, RP = 0;
  double dt = 0.0;

  // pyramid (p = 1, product grid, unit gaps)
  bool pyr_ok = false;
  bool grid_ok = false;            // product grid of consecutive integer levels in grid order (PyrGeom valid)
  mioc::PyrGeom pyr;
  Buf<double> d_stage;             // [2][K][B+1][L] source-row-major fronts, each row in sphere order
  Buf<uint32_t> d_perm;            // [K][nt][L] sphere order of u_old(i): rank | (L1 distance << 16)
  Buf<int32_t> d_same2;            // [K][nt] u_old(i) == u_old(i+2) (the persistent separable driver's order reuse)
  Buf<uint16_t> d_strad;           // [K][nt][8][32] seam-straddling pairs per wave (k_sdt_run's 8-wave layout)
  bool opt_persist = true;         // separable transform: one persistent launch (MIOC_OPT_PERSIST)
  bool opt_row_owner = true;       // ... with one row per workgroup where the plan allows (MIOC_OPT_SDT_ROW_OWNER)
  int last_sdt_driver = 0;         // the last separable DP: 0 per-step launches, 1 k_sdt_run, 2 k_sdt_run1
  bool force_steps = false;        // redo of a persistent DP whose waits timed out: per-step launches
  int64_t n_persist_fallbacks = 0; // persistent DPs redone with per-step launches (mioc_diagnostics slot 6 after a separable DP)
  Buf<int32_t> d_runflags;         // persistent DP: [K][B+1] done, [K][B+1] loaded, err; p = Inf: segment flags, err
  Buf<double> d_chain;             // persistent DP: V[k][i] = Φ_i[j0(i), 0], the row-0 chain (k_sdt_chain)
  unsigned spin_limit = 1u << 24;  // persistent DP: polls before a dependency wait gives up (MIOC_OPT_SPIN_LIMIT)
  int opt_nb = mioc::kSdtDefaultBuffers;  // staging buffers of a persistent separable DP (MIOC_OPT_SDT_BUFFERS)
  const int32_t *gate = nullptr;   // device TRM control (mioc_trm_attach): the state block's gate word
  mioc::PinnedWord h_trm_poll;     // pinned: the gate and any-active words (mioc_trm_poll, mioc_mixed_poll)
  const void *mixed_state = nullptr;  // the mixed state block of the last mioc_mixed_select_device and its K: what
  int mixed_K = 0;                    // mioc_mixed_poll may reduce
  int opt_fsep_seg = 0;            // fused separable DP: row segments (MIOC_OPT_FSEP_SEGMENTS)
  Buf<double> d_ring;              // fused separable DP, S > 1: the segments' outbox rings
  Buf<int32_t> d_segflags;         // ... and their flags (+ err)
  int last_fsep_seg = 0;           // segments of the last fused separable launch (0: the mioc_fused.hip kernel)
  mioc::PinnedWord h_run_err;      // pinned copy of err (lay.err_buf, lay.err_off)
  bool run_pending = false;
  Buf<int32_t> d_counters;         // [8] diagnostics: value-collision targets, multi-level targets, ...
  int64_t occupancy = 0;           // diagnostics [7]: resident workgroups per CU of the last fused launch

  // generic buffers
  Buf<double> d_front;             // [2][K][L][RP]
  Buf<unsigned char> d_U;          // [K][nt-1][L][B+1] uint8 / uint16

  // p = Inf: the class-row geometry and walk plan of the last DP (PinfDev, built by pinf_dev), the segmented walk's tables
  int pinf_BW = 0, pinf_BWP = 0, pinf_CH = 0, pinf_W = 0;
  Buf<uint8_t> d_ftab;
  Buf<int32_t> d_fseg, d_fneed;
  int opt_pinf_walk = 0;           // p = Inf backtrack: 0 auto, 1 segmented walk, -1 serial (MIOC_OPT_PINF_WALK)
  bool last_pinf_fwalk = false;    // the last p = Inf backtrack ran the segmented walk

  // backtrack scratch
  bool have_path = false;          // d_ranks holds the controls of the last backtrack
  Buf<mioc::Start> d_start;
  Buf<int32_t> d_ranks;            // [K][nt] level ranks of the path, then [K][nt] ranks of u_old
  Buf<int32_t> d_flags;            // [4] validation flags / counters
  mioc::PinnedWord h_flags;        // pinned mirror
  Buf<double> d_uout_own;          // host-API backtrack output staging
  Buf<double> d_phistar_own;
  Buf<int32_t> d_status_own;

  // p = Inf backtrack overlapping the next DP: it runs on bstream (the next bellman's kernels on `stream` meanwhile),
  // so every DP owns one of two slots of its inputs and p = Inf tables (the backtrack of DP n reads slot n % 2 while
  // DP n + 1 writes the other).  ev_bt[s]: the last backtrack that read slot s (the bellman that reuses s waits on it);
  // join_bt orders `stream` after the backtracks before any other call reads their outputs.
  hipStream_t bstream = nullptr;
  hipEvent_t ev_dp = nullptr, ev_bt[2] = {nullptr, nullptr};
  bool bt_rec[2] = {false, false};
  bool bt_pending = false;
  int bt_last = 0;
  int slot = 0;  // the last bellman's slot
  struct Slot {
    Buf<double> df, uold;          // [K][nt][M] each
    Buf<double> kmin, k2, R, kabs; // the p = Inf tables (PinfDev)
    Buf<int32_t> kfirst;
  } slots[2];
  Slot &cur() { return slots[slot]; }
  const Slot &cur() const { return slots[slot]; }

  // timing
  struct EvPair {
    hipEvent_t begin = nullptr, end = nullptr;
    int64_t launches = 0;
  };
  std::vector<EvPair> ev_pool, ev_pending[4];
  EvPair ev_open[4];
  double stat_ms[4] = {};
  int64_t stat_launches[4] = {};
  const char *stat_name[4] = {"", "", "", ""};
};

template <typename T>
int mioc::DevBuf<T>::grow(mioc_ctx *ctx, size_t need_bytes, const char *what) {
  if (p && cap >= need_bytes) return MIOC_OK;
  if (p) (void)hipDeviceSynchronize();
  if (need_bytes == 0) need_bytes = 16;
  if (alloc(need_bytes)) return MIOC_OK;
  char buf[160];
  std::snprintf(buf, sizeof buf, "cannot allocate %.3f GB for %s", need_bytes / 1e9, what);
  if (ctx) ctx->err = buf;
  return MIOC_ENOMEM;
}
