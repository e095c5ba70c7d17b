// mioc_mixed.hip -- the continuous step of the mixed trust-region method, on gfx950 (include/mioc.h, "Mixed
// controls").
//
// A mixed control x has nx = nu + nv rows per time step: rows 0..nu-1 continuous (c), rows nu..nx-1 integer (v), as
// the reference's rand_func lays them out (HelpFunctions.jl:136-148).  The integer rows go through the DP as before;
// the continuous rows take one projected-gradient step per outer iteration, with a backtracking line search whose R
// candidate step sizes are all evaluated at once:
//   k_mixed_fan     candidate j of restart k: c_j = P_[lo,hi](c - s_k 2^-j g), the integer rows copied, and the
//                   Armijo slope tau * sum g (c - c_j), summed in the order i ascending, m ascending by one lane
//                   (fold, as k_trm_pred sums int_val), so that a host loop reproduces every bit;
//   (the ODE program's kernel evaluates J of all R*K candidates in one value-only launch)
//   k_mixed_select  per restart the first candidate that passes the Armijo test, the step-size update, and the
//                   finality rule that couples the continuous step with the DP's stop flag;
//   k_mixed_live    any restart that can still move, for mioc_mixed_poll;
//   k_rows_copy     the split (df -> df_v, x -> v_old) and the join (c, trial_v -> x_trial) around the DP.
// The file is built with -ffp-contract=off like the rest: t = x - s_j*g is one product and one difference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mioc_internal.h"

namespace mioc {

namespace {

constexpr int kMixThreads = 256;
constexpr int MIX_FINAL = 1, MIX_MOVED = 2;

// State block (mioc_mixed_state_bytes): the any-live word, then per restart the step size s, flags, jsel, csteps.
struct MixState {
  int32_t *any_live;
  double *s;
  int32_t *flags, *jsel, *csteps;
};
__host__ __device__ inline MixState mixed_state_layout(void *base, int K) {
  MixState S;
  char *b = static_cast<char *>(base);
  S.any_live = reinterpret_cast<int32_t *>(b);
  S.s = reinterpret_cast<double *>(b + 16);
  S.flags = reinterpret_cast<int32_t *>(S.s + K);
  S.jsel = S.flags + K;
  S.csteps = S.jsel + K;
  return S;
}

// steps per LDS chunk of the fan: at most kMixedChunk terms, and an even number of steps, so that a chunk of an even
// nt*nx starts on a 16-byte boundary
__host__ __device__ inline int fan_chunk_steps(int nu) { return (kMixedChunk / nu) & ~1; }

// element f = i*nx + m of restart k: the candidate's value; a continuous element also leaves its slope term in LDS
__device__ __forceinline__ double fan_elem(int f, int i0, int nu, int nx, double xv, double gv, double sj,
                                           const double *lo, const double *hi, double *s_term) {
  const int i = f / nx, m = f - i * nx;
  if (m >= nu) return xv;
  const double l = lo[i * nu + m], h = hi[i * nu + m];
  const double t = xv - sj * gv;
  const double c = t < l ? l : (t > h ? h : t);  // a NaN fails both comparisons and stays
  s_term[(i - i0) * nu + m] = gv * (xv - c);
  return c;
}

// grid (K, R): workgroup (k, j) writes candidate j of restart k into xfan[j][k] and its slope into slope[j*K + k].
// VEC: nt*nx is even and the arrays are 16-byte aligned, so every restart's block is read and written as double2.
template <bool VEC>
__global__ __launch_bounds__(kMixThreads) void k_mixed_fan(int K, int nu, int nx, int nt, double tau, const double *x,
                                                          const double *df, const double *lo, const double *hi,
                                                          MixState S, double *xfan, double *slope) {
  __shared__ double s_term[kMixedChunk];
  const int k = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
  const double sj = ldexp(S.s[k], -j);  // s * 2^-j, exact
  const size_t n = (size_t)nt * nx;
  const double *xk = x + (size_t)k * n, *gk = df + (size_t)k * n;
  double *out = xfan + ((size_t)j * K + k) * n;
  const int cs = fan_chunk_steps(nu);
  double acc = 0.0;
  for (int i0 = 0; i0 < nt; i0 += cs) {
    const int ci = min(cs, nt - i0);
    const int e0 = i0 * nx, ne = ci * nx;
    if (VEC) {  // e0 and ne are even
      for (int q = 2 * tid; q < ne; q += 2 * kMixThreads) {
        const int f = e0 + q;
        const double2 xv = *reinterpret_cast<const double2 *>(xk + f);
        const double2 gv = *reinterpret_cast<const double2 *>(gk + f);
        double2 o;
        o.x = fan_elem(f, i0, nu, nx, xv.x, gv.x, sj, lo, hi, s_term);
        o.y = fan_elem(f + 1, i0, nu, nx, xv.y, gv.y, sj, lo, hi, s_term);
        *reinterpret_cast<double2 *>(out + f) = o;
      }
    } else {
      for (int q = tid; q < ne; q += kMixThreads) {
        const int f = e0 + q;
        out[f] = fan_elem(f, i0, nu, nx, xk[f], gk[f], sj, lo, hi, s_term);
      }
    }
    __syncthreads();
    if (tid == 0) acc = fold(s_term, ci * nu, acc);
    __syncthreads();
  }
  if (tid == 0) slope[(size_t)j * K + k] = tau * acc;
}

// one workgroup per restart: the decision by thread 0, then the accepted candidate's continuous rows into x
__global__ __launch_bounds__(kMixThreads) void k_mixed_select(int K, int R, int nu, int nx, int nt, double c1,
                                                             double smax, double ctol, MixState S, TrmState T,
                                                             const double *xfan, const double *slope,
                                                             const double *Jfan, double *J_old, double *x) {
  __shared__ int s_j;
  const int k = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    int mf = S.flags[k], tf = T.flags[k], jsel = -1;
    const bool stop = tf & TRM_STOP;
    if (mf & MIX_FINAL) {                         // 1. a final restart is left alone
    } else if (stop && !(mf & MIX_MOVED)) {       // 2. neither part moved: final
      S.flags[k] = mf | MIX_FINAL;
    } else {                                      // 3. the first candidate that passes the Armijo test
      const double Jo = J_old[k], s = S.s[k];
      for (int j = 0; j < R && jsel < 0; ++j) {
        const double sl = slope[(size_t)j * K + k], Jj = Jfan[(size_t)j * K + k];
        if (sl > 0.0 && Jj <= Jo - c1 * sl) jsel = j;
      }
      bool moved = false;
      if (jsel >= 0) {
        const double Jj = Jfan[(size_t)jsel * K + k], s2 = 2.0 * ldexp(s, -jsel);
        moved = (Jo - Jj) > ctol * fmax(1.0, fabs(Jo));
        J_old[k] = Jj;
        S.s[k] = s2 < smax ? s2 : smax;
        S.csteps[k] += 1;
      } else {
        S.s[k] = ldexp(s, -R);
      }
      S.jsel[k] = jsel;
      mf = (mf & ~MIX_MOVED) | (moved ? MIX_MOVED : 0);
      if (stop) {                                 // 4. the DP had stopped: it runs again only after a real move
        if (moved)
          T.flags[k] = tf & ~TRM_STOP;
        else
          mf |= MIX_FINAL;
      }
      S.flags[k] = mf;
    }
    s_j = jsel;
  }
  __syncthreads();
  const int j = s_j;
  if (j < 0) return;
  const size_t n = (size_t)nt * nx;
  const double *src = xfan + ((size_t)j * K + k) * n;
  double *dst = x + (size_t)k * n;
  const int ne = nt * nu;
  for (int e = tid; e < ne; e += kMixThreads) {
    const int i = e / nu, m = e - i * nu;
    dst[(size_t)i * nx + m] = src[(size_t)i * nx + m];
  }
}

// any restart that is not final and whose DP has not stopped or whose continuous part moved, into the any-live word
__global__ __launch_bounds__(1024) void k_mixed_live(int K, MixState S, TrmState T) {
  int any = 0;
  for (int r = threadIdx.x; r < K; r += blockDim.x) {
    const int mf = S.flags[r], tf = T.flags[r];
    any |= (!(mf & MIX_FINAL) && (!(tf & TRM_STOP) || (mf & MIX_MOVED))) ? 1 : 0;
  }
  trm_block_or(any, S.any_live);
}

// dst[k][i][dst_row0 + r] = src[k][i][src_row0 + r]; grid (chunks, K)
__global__ __launch_bounds__(kMixThreads) void k_rows_copy(const int32_t *gate, int nt, double *dst, int dst_nx,
                                                          int dst_row0, const double *src, int src_nx, int src_row0,
                                                          int nrows) {
  if (gate_closed(gate)) return;
  const int k = blockIdx.y;
  const int ne = nt * nrows;
  double *d = dst + (size_t)k * nt * dst_nx + dst_row0;
  const double *s = src + (size_t)k * nt * src_nx + src_row0;
  for (int e = blockIdx.x * kMixThreads + threadIdx.x; e < ne; e += gridDim.x * kMixThreads) {
    const int i = e / nrows, r = e - i * nrows;
    d[(size_t)i * dst_nx + r] = s[(size_t)i * src_nx + r];
  }
}

}  // namespace

size_t mixed_state_bytes(int K) { return 16 + (size_t)K * (sizeof(double) + 3 * sizeof(int32_t)); }

hipError_t launch_rows_copy(hipStream_t s, const int32_t *gate, int K, int nt, double *dst, int dst_nx, int dst_row0,
                            const double *src, int src_nx, int src_row0, int nrows) {
  const unsigned chunks = (unsigned)std::min<size_t>(((size_t)nt * nrows + kMixThreads - 1) / kMixThreads, 64);
  hipLaunchKernelGGL(k_rows_copy, dim3(chunks, (unsigned)K), dim3(kMixThreads), 0, s, gate, nt, dst, dst_nx, dst_row0,
                     src, src_nx, src_row0, nrows);
  return hipGetLastError();
}

hipError_t launch_mixed_fan(hipStream_t s, int K, int R, int nu, int nx, int nt, double tau, const double *x,
                            const double *df, const double *lo, const double *hi, void *mstate, double *xfan,
                            double *slope) {
  const MixState S = mixed_state_layout(mstate, K);
  const bool vec = ((size_t)nt * nx) % 2 == 0 &&
                   ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(df) |
                     reinterpret_cast<uintptr_t>(xfan)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(k_mixed_fan<true>, dim3((unsigned)K, (unsigned)R), dim3(kMixThreads), 0, s, K, nu, nx, nt, tau,
                       x, df, lo, hi, S, xfan, slope);
  else
    hipLaunchKernelGGL(k_mixed_fan<false>, dim3((unsigned)K, (unsigned)R), dim3(kMixThreads), 0, s, K, nu, nx, nt, tau,
                       x, df, lo, hi, S, xfan, slope);
  return hipGetLastError();
}

hipError_t launch_mixed_select(hipStream_t s, int K, int R, int nu, int nx, int nt, double c1, double smax, double ctol,
                               void *mstate, void *trm_state, const double *xfan, const double *slope,
                               const double *Jfan, double *J_old, double *x) {
  hipLaunchKernelGGL(k_mixed_select, dim3((unsigned)K), dim3(kMixThreads), 0, s, K, R, nu, nx, nt, c1, smax, ctol,
                     mixed_state_layout(mstate, K), trm_state_layout(trm_state, K), xfan, slope, Jfan, J_old, x);
  return hipGetLastError();
}

hipError_t launch_mixed_live(hipStream_t s, int K, void *mstate, void *trm_state) {
  hipLaunchKernelGGL(k_mixed_live, dim3(1), dim3(1024), 0, s, K, mixed_state_layout(mstate, K),
                     trm_state_layout(trm_state, K));
  return hipGetLastError();
}

}  // namespace mioc
