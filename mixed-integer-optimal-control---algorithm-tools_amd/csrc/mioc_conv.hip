// mioc_conv.hip -- the signal-reconstruction (convolution) objective's value and gradient, batched over restarts on
// gfx950 (Marko / Wachsmuth §6.2; the reference's main("convolution"), multi-trust.jl:190-192).
//
// Reference: julia_opt/example_convolution.jl:73-81 (f_to_vec: fvec[i] = target(T0 + τ·i), i = 1..nt+1 -- the grid
// starts one step AFTER T0; reproduced, the caller supplies fvec), :85-100 (Mmat: (nt+1)² tridiagonal, τ/3 at both
// ends of the diagonal, 2/3*τ = (2/3)·τ inside, τ/6 beside it), :104-125 (toeplitz: K is (nt+1) x nt with
// K[r, c] = κ[r − c] for r − c >= 1 and 0 otherwise -- strictly lower triangular, row 1 and the diagonal are zero;
// the caller supplies κ = K[2:nt+1, 1]), :128-135 (eval_f_helper: v = K·xᵀ − fvec, J = ½·vᵀ·M·v) and :138-141
// (eval_df_helper: df = (Kᵀ·(M·(K·xᵀ − fvec)))ᵀ).
//
// Design.  For K restarts both products are a restart panel times a triangular Toeplitz matrix that the nt numbers κ
// define, so the matrix is never stored: the restarts sit in the MFMA M dimension (a restart's row is contiguous in
// time, which is the A-operand order of v_mfma_f64_16x16x4_f64), and every lane builds its B operand from κ in LDS:
//   forward   Vᵀ (16 x (nt+1)) = X (16 x nt) · Kᵀ − fvec,   B[k][n] = κ[n0 + n − k]   (1-based κ; 0 when the index < 1)
//   adjoint   DF (16 x nt)     = W (16 x (nt+1)) · K,        B[k][n] = κ[k − n0 − n],  W = M·V
// Within a chunk of 16 k the four MFMAs take k = kc + 4·(l >> 4) + j (j = 0..3) instead of kc + 4·j + (l >> 4): the
// same products in another (fixed) order, and a lane's four A values are then contiguous in memory.  Chunks that lie
// entirely in K's zero triangle are skipped (half the work); only the chunk on the diagonal tests its indices.
// A wave owns 16 restarts x two neighbouring column tiles, which share every A load (measured at K = 1024,
// nt = 2048, J + df: one tile per wave 0.286 ms, two 0.237 ms, four 0.256 ms -- the A loads touch 16 cache lines
// each, and four tiles per wave leave too few waves for the triangle's long columns), or one tile when the batch is
// too small to give every SIMD a wave (launch_conv_mm; the results are the same bit for bit); four waves per
// workgroup, the workgroups of the longest columns first.  B is a plain LDS lookup (the four values of a chunk are
// neighbours: two ds_read2_b64 per four MFMAs; a register window over κ was not built).  V lives in a context-owned
// scratch (K x (nt+1)); J = ½·Σ_j v_j·w_j is one workgroup per restart with a fixed summation tree (k_conv_J), which
// also stores w = M·v for the adjoint product when a gradient is asked for (applying M while the adjoint loads its
// A operand was measured slower, 0.247 ms against 0.137 ms for the adjoint with one tile per wave: the tridiagonal
// product is FP64 VALU work that every column tile repeated).  No atomics: a restart's J and df depend on neither K, its
// position in the batch nor the padding of its tile.  The device evaluates no transcendental (κ and fvec hold the
// caller's exp / sin / cos), so results differ from the reference's BLAS products by summation order only: the
// tests hold them to 1e-9 relative.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "mioc_internal.h"

namespace mioc {

struct ConvState {
  bool ready = false;  // kappa / fvec on the device match nt (false after a failed setup)
  int64_t nt = 0;
  double tau = 0.0;
  DevBuf<double> d_kappa;  // [nt]
  DevBuf<double> d_fvec;   // [nt + 1]
  DevBuf<double> d_v;      // [K][nt + 1] v = K·xᵀ − fvec, then [K][nt + 16] w = M·v, between the launches
  DevBuf<double> d_io;     // host entry staging: x, df, J
};

void conv_free(ConvState *c) { delete c; }

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int CW = 4;            // waves per workgroup
constexpr int CMAXNT = 16384;    // κ (+ 32 zeros) in LDS: 128 KB
constexpr int CFILL = 1024;      // waves that give every SIMD of the device one (256 CUs x 4)
constexpr int CJT = 256;         // threads of k_conv_J

struct ConvArgs {
  const double *kappa, *fvec, *X;
  double *V, *W, *J, *DF;           // V = v, W = M·v: the context's scratch
  int K, nt, rtiles;
  double md_end, md_in, m_off;      // M's diagonal at both ends (τ/3), inside ((2/3)·τ), and beside it (τ/6)
  const int32_t *gate;              // device TRM control gate (see ProblemDev::gate)
};

// w_r = (M·v)_r from v_{r-1}, v_r, v_{r+1} (Mmat, example_convolution.jl:85-100); the sum order is fixed
__device__ __forceinline__ double conv_w(const ConvArgs &C, int r, double vm, double v0, double vp) {
  const double d = (r == 0 || r == C.nt) ? C.md_end : C.md_in;
  return (C.m_off * vm + d * v0) + C.m_off * vp;
}
__device__ __forceinline__ double conv_v(const double *vr, int r, int nt) { return (r >= 0 && r <= nt) ? vr[r] : 0.0; }

// the four MFMAs of one 16-k chunk on one column tile: two accumulators, alternating
__device__ __forceinline__ void conv_mfma4(const double (&a)[4], const double (&b)[4], d4 (&acc)[2]) {
  acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[0], acc[0], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], b[1], acc[1], 0, 0, 0);
  acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[2], b[2], acc[0], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[3], b[3], acc[1], 0, 0, 0);
}

// A wave owns 16 restarts x CNS neighbouring column tiles (columns n0 + 16s + n, s < CNS), which share every A load.
// ADJ = false: columns r of v, V = X·Kᵀ − fvec.  ADJ = true: columns c of df, DF = W·K.  Every column tile sums its
// chunks in ascending k from (forward: up to) its own diagonal with the same two accumulators whatever CNS is, so
// the results do not depend on CNS bit for bit.
template <bool ADJ, int CNS>
__global__ __launch_bounds__(CW * 64) void k_conv_mm(ConvArgs C) {
  if (gate_closed(C.gate)) return;
  extern __shared__ __attribute__((aligned(16))) double kl[];  // kl[i] = κ[i + 1] (1-based κ), zeros from nt on
  const int nt = C.nt, tid = threadIdx.x, w = tid >> 6, lane = tid & 63, n = lane & 15, g = lane >> 4;
  constexpr int SW = 16 * CNS;                                  // columns per wave
  const int T = ((ADJ ? nt : nt + 1) + SW - 1) / SW;            // wave tiles: nt columns of df, nt + 1 of v
  const int GC = (T + CW - 1) / CW;
  const int cg = blockIdx.x / C.rtiles, rt = blockIdx.x - cg * C.rtiles;
  const int grp = ADJ ? cg : GC - 1 - cg;  // the longest columns first
  // the part of κ this workgroup reads: differences below SW·CW·(grp + 1) (forward), up to nt − SW·CW·grp + 15 (adjoint)
  const int lim = min(nt + SW, ADJ ? nt - SW * CW * grp + 16 : SW * CW * (grp + 1));
  for (int i = tid; i < lim; i += CW * 64) kl[i] = i < nt ? C.kappa[i] : 0.0;
  __syncthreads();
  const int t = grp * CW + w;
  if (t >= T) return;
  const int n0 = SW * t;
  const int arow = min(rt * 16 + n, C.K - 1);  // the A operand's restart; rows past K repeat the last (never stored)
  d4 acc[CNS][2];
#pragma unroll
  for (int s = 0; s < CNS; ++s) acc[s][0] = acc[s][1] = d4{0.0, 0.0, 0.0, 0.0};
  double a[4], b[4], an[4];
  if (!ADJ) {
    const double *xr = C.X + (size_t)arow * nt;
    // chunks kc = 0, 16, .., n0 − 16 lie below every tile's diagonal: c = kc + 4g + j < n0 <= nt, and the κ index
    // n0 + 16s + n − c − 1 >= 0
    const int base = n0 + n - 1 - 4 * g;
    if (n0 > 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) an[j] = xr[4 * g + j];
    }
    for (int kc = 0; kc < n0; kc += 16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = an[j];
      if (kc + 16 < n0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) an[j] = xr[kc + 16 + 4 * g + j];
      }
#pragma unroll
      for (int s = 0; s < CNS; ++s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = kl[base + 16 * s - kc - j];
        conv_mfma4(a, b, acc[s]);
      }
    }
    // the chunks kc = n0 + 16d that cross a diagonal: tile s has K[r][c] = 0 unless r − c >= 1 (all of it when s < d);
    // x ends at nt
#pragma unroll
    for (int d = 0; d < CNS; ++d) {
      const int kc = n0 + 16 * d;
      if (kc < nt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = kc + 4 * g + j;
          a[j] = c < nt ? xr[c] : 0.0;
        }
#pragma unroll
        for (int s = d; s < CNS; ++s) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int idx = 16 * (s - d) + n - 4 * g - j - 1;
            b[j] = idx >= 0 ? kl[idx] : 0.0;
          }
          conv_mfma4(a, b, acc[s]);
        }
      }
    }
  } else {
    const double *wr = C.W + (size_t)arow * (nt + 16);
    // the chunks kc = n0 + 16d that cross a diagonal (rows r = kc + 4g + j of K; tile s has the κ index
    // r − c − 1 >= 0 only below its diagonal, and nothing when s > d); w is stored with zeros up to r = nt + 15
#pragma unroll
    for (int d = 0; d < CNS; ++d) {
      const int kc = n0 + 16 * d;
      if (kc <= nt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = wr[kc + 4 * g + j];
#pragma unroll
        for (int s = 0; s <= d; ++s) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int idx = 16 * (d - s) + 4 * g + j - n - 1;
            b[j] = idx >= 0 ? kl[idx] : 0.0;
          }
          conv_mfma4(a, b, acc[s]);
        }
      }
    }
    // chunks kc = n0 + SW, .., <= nt lie below every tile's diagonal: κ index kc + 4g + j − n0 − 16s − n − 1 >= 0
    const int base = 4 * g - n0 - n - 1;
    if (n0 + SW <= nt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) an[j] = wr[n0 + SW + 4 * g + j];
    }
    for (int kc = n0 + SW; kc <= nt; kc += 16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = an[j];
      if (kc + 16 <= nt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) an[j] = wr[kc + 16 + 4 * g + j];
      }
#pragma unroll
      for (int s = 0; s < CNS; ++s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = kl[base - 16 * s + kc + j];
        conv_mfma4(a, b, acc[s]);
      }
    }
  }
  // C/D map of v_mfma_f64_16x16x4_f64: register q of lane l is row (l >> 4) + 4q (the restart), column l & 15
#pragma unroll
  for (int s = 0; s < CNS; ++s) {
    const int col = n0 + 16 * s + n;
    if (ADJ ? col < nt : col <= nt) {
      const double f = ADJ ? 0.0 : C.fvec[col];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = rt * 16 + g + 4 * q;
        if (k < C.K) {
          const double sum = acc[s][0][q] + acc[s][1][q];
          if (ADJ)
            C.DF[(size_t)k * nt + col] = sum;
          else
            C.V[(size_t)k * (nt + 1) + col] = sum - f;
        }
      }
    }
  }
}

// J_k = ½·Σ_r v_r·w_r with w = M·v, one workgroup per restart: thread t sums r = t, t + 256, .. in order, then a fixed
// tree.  When the gradient follows, w goes to the scratch (row stride nt + 16, zeros from r = nt + 1 on) for the
// adjoint product's A operand.
__global__ __launch_bounds__(CJT) void k_conv_J(ConvArgs C) {
  if (gate_closed(C.gate)) return;
  __shared__ double red[CJT];
  const int nt = C.nt, tid = threadIdx.x;
  const double *vr = C.V + (size_t)blockIdx.x * (nt + 1);
  double *wr = C.DF ? C.W + (size_t)blockIdx.x * (nt + 16) : nullptr;
  double s = 0.0;
  for (int r = tid; r < nt + 16; r += CJT) {
    double w = 0.0;
    if (r <= nt) {
      const double v0 = vr[r];
      w = conv_w(C, r, conv_v(vr, r - 1, nt), v0, conv_v(vr, r + 1, nt));
      s += v0 * w;
    }
    if (wr) wr[r] = w;
  }
  if (!C.J) return;
  red[tid] = s;
  __syncthreads();
  for (int h = CJT / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) C.J[blockIdx.x] = 0.5 * red[0];
}

// Two column tiles per wave once that still gives every SIMD a wave; one per wave for small batches (a single
// ConvObj evaluation, K = 1, nt = 2048: 0.086 ms against 0.130 ms for J + df), whose longest column is the critical path.
template <bool ADJ, int CNS>
hipError_t launch_conv_mm_ns(hipStream_t s, const ConvArgs &C) {
  const int T = ((ADJ ? C.nt : C.nt + 1) + 16 * CNS - 1) / (16 * CNS), GC = (T + CW - 1) / CW;
  const size_t lds = (size_t)(C.nt + 16 * CNS) * sizeof(double);
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_conv_mm<ADJ, CNS>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((k_conv_mm<ADJ, CNS>), dim3((unsigned)((int64_t)GC * C.rtiles)), dim3(CW * 64), lds, s, C);
  return hipGetLastError();
}

// the one place that chooses: waves of two column tiles over the 16-restart tiles of K, against CFILL
int conv_tiles_per_wave(int64_t nt, int64_t K) {
  const int64_t waves2 = ((K + 15) / 16) * ((nt + 31) / 32);
  return waves2 >= CFILL ? 2 : 1;
}

template <bool ADJ>
hipError_t launch_conv_mm(hipStream_t s, const ConvArgs &C) {
  return conv_tiles_per_wave(C.nt, C.K) == 2 ? launch_conv_mm_ns<ADJ, 2>(s, C) : launch_conv_mm_ns<ADJ, 1>(s, C);
}

int conv_fail(mioc_ctx *ctx, int code, const std::string &msg) {
  ctx->err = msg;
  return code;
}

int conv_upload(mioc_ctx *ctx, DevBuf<double> &dst, const double *src, size_t n, const char *what) {
  if (!dst.alloc(n * sizeof(double)))
    return conv_fail(ctx, MIOC_ENOMEM, std::string("cannot allocate the convolution ") + what);
  if (hipMemcpy(dst.get(), src, n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    return conv_fail(ctx, MIOC_EHIP, std::string("convolution upload failed: ") + what);
  return MIOC_OK;
}

}  // namespace
}  // namespace mioc

using namespace mioc;

extern "C" {

int32_t mioc_conv_tiles_per_wave(int64_t nt, int64_t K) {
  if (nt < 1 || nt > CMAXNT || K < 1 || K > INT32_MAX) return 0;
  return conv_tiles_per_wave(nt, K);
}

int32_t mioc_conv_setup(mioc_ctx *ctx, int64_t nt, double T0, double T1, const double *kappa, const double *fvec) {
  if (!ctx) return MIOC_EINVAL;
  MIOC_JOIN_BT(ctx);
  if (nt < 1 || nt > CMAXNT)
    return conv_fail(ctx, MIOC_EINVAL, "convolution: need 1 <= nt <= " + std::to_string(CMAXNT));
  if (!(T1 > T0) || !std::isfinite(T0) || !std::isfinite(T1))
    return conv_fail(ctx, MIOC_EINVAL, "convolution: need finite T1 > T0");
  if (!kappa || !fvec) return conv_fail(ctx, MIOC_EINVAL, "convolution: null kappa / fvec");
  for (int64_t i = 0; i < nt; ++i)
    if (!std::isfinite(kappa[i])) return conv_fail(ctx, MIOC_EINVAL, "convolution: kappa has a non-finite entry");
  for (int64_t i = 0; i <= nt; ++i)
    if (!std::isfinite(fvec[i])) return conv_fail(ctx, MIOC_EINVAL, "convolution: fvec has a non-finite entry");
  ConvState *c = ctx->conv ? ctx->conv : new ConvState();
  ctx->conv = c;
  c->ready = false;  // until both tables are uploaded for the new nt
  c->nt = nt;
  c->tau = (T1 - T0) / (double)nt;  // example_convolution.jl:31
  if (hipSetDevice(ctx->device) != hipSuccess) return conv_fail(ctx, MIOC_EHIP, "hipSetDevice failed");
  // evals enqueued earlier may still read the tables that are replaced below
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return conv_fail(ctx, MIOC_EHIP, "hipStreamSynchronize failed");
  int rc;
  if ((rc = conv_upload(ctx, c->d_kappa, kappa, (size_t)nt, "kappa")) ||
      (rc = conv_upload(ctx, c->d_fvec, fvec, (size_t)nt + 1, "fvec")))
    return rc;
  c->ready = true;
  return MIOC_OK;
}

int32_t mioc_conv_eval_device(mioc_ctx *ctx, int64_t K, const double *d_x, double *d_J, double *d_df) {
  if (!ctx) return MIOC_EINVAL;
  MIOC_JOIN_BT(ctx);
  ConvState *c = ctx->conv;
  if (!c || !c->ready) return conv_fail(ctx, MIOC_ESTATE, "convolution: no successful mioc_conv_setup");
  const int64_t rtiles = (K + 15) / 16, gcmax = ((c->nt + 16) / 16 + CW - 1) / CW;
  if (K < 1 || K > INT32_MAX || !d_x || rtiles * gcmax > INT32_MAX)
    return conv_fail(ctx, MIOC_EINVAL, "convolution: bad K / x");
  if (hipSetDevice(ctx->device) != hipSuccess) return conv_fail(ctx, MIOC_EHIP, "hipSetDevice failed");
  const size_t nv = (size_t)K * (c->nt + 1), nw = d_df ? (size_t)K * (c->nt + 16) : 0;
  if (c->d_v.bytes() < (nv + nw) * sizeof(double) && !c->d_v.alloc((nv + nw) * sizeof(double)))
    return conv_fail(ctx, MIOC_ENOMEM, "convolution: cannot allocate the v / w scratch");
  ConvArgs A;
  A.kappa = c->d_kappa.get(), A.fvec = c->d_fvec.get(), A.X = d_x;
  A.V = c->d_v.get(), A.W = c->d_v.get() + nv, A.J = d_J, A.DF = d_df;
  A.K = (int)K, A.nt = (int)c->nt, A.rtiles = (int)rtiles;
  A.md_end = c->tau / 3, A.md_in = 2.0 / 3.0 * c->tau, A.m_off = c->tau / 6;  // example_convolution.jl:89-96
  A.gate = ctx->gate;
  hipError_t e = launch_conv_mm<false>(ctx->stream, A);
  if (e != hipSuccess) return conv_fail(ctx, MIOC_EHIP, std::string("k_conv_mm (forward): ") + hipGetErrorString(e));
  if (d_J || d_df) {
    hipLaunchKernelGGL(k_conv_J, dim3((unsigned)K), dim3(CJT), 0, ctx->stream, A);
    if ((e = hipGetLastError()) != hipSuccess)
      return conv_fail(ctx, MIOC_EHIP, std::string("k_conv_J: ") + hipGetErrorString(e));
  }
  if (d_df) {
    e = launch_conv_mm<true>(ctx->stream, A);
    if (e != hipSuccess) return conv_fail(ctx, MIOC_EHIP, std::string("k_conv_mm (adjoint): ") + hipGetErrorString(e));
  }
  return MIOC_OK;
}

int32_t mioc_conv_eval(mioc_ctx *ctx, int64_t K, const double *x, double *J, double *df) {
  if (!ctx) return MIOC_EINVAL;
  MIOC_JOIN_BT(ctx);
  ConvState *c = ctx->conv;
  if (!c || !c->ready) return conv_fail(ctx, MIOC_ESTATE, "convolution: no successful mioc_conv_setup");
  if (K < 1 || K > INT32_MAX || !x || (!J && !df)) return conv_fail(ctx, MIOC_EINVAL, "convolution: bad K / x / outputs");
  if (hipSetDevice(ctx->device) != hipSuccess) return conv_fail(ctx, MIOC_EHIP, "hipSetDevice failed");
  const size_t nxt = (size_t)K * c->nt;
  const size_t need = (2 * nxt + K) * sizeof(double);
  if (c->d_io.bytes() < need && !c->d_io.alloc(need))
    return conv_fail(ctx, MIOC_ENOMEM, "convolution: cannot allocate the host-entry staging");
  double *dx = c->d_io.get(), *ddf = dx + nxt, *dJ = dx + 2 * nxt;
  if (hipMemcpyAsync(dx, x, nxt * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    return conv_fail(ctx, MIOC_EHIP, "convolution: x copy-in failed");
  const int rc = mioc_conv_eval_device(ctx, K, dx, J ? dJ : nullptr, df ? ddf : nullptr);
  if (rc) return rc;
  if (J && hipMemcpyAsync(J, dJ, K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    return conv_fail(ctx, MIOC_EHIP, "convolution: J copy-out failed");
  if (df && hipMemcpyAsync(df, ddf, nxt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    return conv_fail(ctx, MIOC_EHIP, "convolution: df copy-out failed");
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return conv_fail(ctx, MIOC_EHIP, "hipStreamSynchronize failed");
  return MIOC_OK;
}

}  // extern "C"
