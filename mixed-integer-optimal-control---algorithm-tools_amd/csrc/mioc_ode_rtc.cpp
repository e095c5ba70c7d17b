// mioc_ode_rtc.cpp -- user-defined ODE objectives (the reference's extension point, AbstractODEObjective with the
// hooks F!, Fy!, Fu!, G, Gy!, Gu!: julia_opt/ODEObjective.jl:243-248) compiled at run time for gfx950.
//
// mioc_ode_program_create wraps the caller's six hooks (HIP source text, the contract is in include/mioc.h) in the
// kernel skeleton below and compiles the result with hiprtc; mioc_ode_program_eval_device loads the code object on
// the context's device at first use and launches it.  hiprtc is loaded lazily (dlopen at the first create), so
// libmioc.so carries no link-time dependency on it and loads as before where it is absent.
//
// The kernel: eval_f_helper / eval_df_helper of ODEObjective.jl:125-184, one lane per restart in 64-lane blocks like
// k_ode_eval (mioc_ode.hip), NY / NX / NP compile-time so that y, λ, fy, fu, gy, gu live in registers.  The forward
// states go to a scratch laid out [step][r][k]: the 64 lanes of a wave store and load 64 contiguous doubles
// (k_ode_eval's [k][step][r] gives every lane a cache line of its own per step).  Rounding order (no contraction, no
// fast-math): see the skeleton; for NY = 2, NX = 3, Gu = 0 it is k_ode_eval's, operation for operation.
//
// mioc_ode_program_create_ex also takes an integrator: Heun or classical RK4 with substeps inside each control
// interval, a quadrature cost and the scheme's discrete adjoint (kSkeletonRK; the scheme is defined in include/mioc.h).
// The program carries integrator and substeps; the Euler skeleton and what it compiles to are untouched.
// MIOC_ODE_INT_BEULER / _MIDPOINT are the one-stage implicit schemes (kSkeletonTheta): Newton with an in-register
// Gaussian elimination forward, one transposed solve per substep backward.
//
// mioc_ode_program_create_ad generates Fy / Fu / Gy / Gu from templated F and G with a dual-number type (kAdPrelude,
// kAdHooks) that is compiled into the same kernel; the skeletons and the launch are the same, and with derive == 0 so
// is the source text.
//
// mioc_ode_program_create_bolza adds a terminal cost E (and Ey), ND columns of sampled data behind the parameters and
// the state trajectory as an output (include/mioc.h, "Terminal cost, sampled data, state output").  Each is an #if in
// the three skeletons, switched by a macro of the head (ND, MIOC_TERMINAL, MIOC_STATES), and the kernel takes the data
// and the state pointer only then: with ndata == 0 and flags == 0 the head has no new byte and the skeletons preprocess
// to the tokens they had, so such a program's code object is the one it was.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "mioc_internal.h"

namespace {

constexpr int kMaxNY = 8, kMaxNX = 8, kMaxNP = 32, kMaxND = 16, kMaxSubsteps = 64;
constexpr size_t kMaxSource = 1u << 20;
const char *const kKernelName = "mioc_ode_program_kernel";
const char *const kNoinlineNote =
    "mioc_ad: with the generated hooks inlined the kernel needs more than 256 VGPRs; they are compiled as functions\n";

// The skeleton follows the user text.  NY, NX, NP are #defined in front of both.
const char *const kSkeleton = R"SKEL(
#ifndef ND
#define ND 0
#endif
#if ND > 0  // sampled data: p is a per-lane copy of the parameters with the data row of the current column behind them
#define MIOC_DATA_ARG , const double *__restrict__ DATA
#define MIOC_DATA_ROW(c)                                \
  {                                                     \
    const double *row = DATA + (size_t)(c) * ND;        \
    _Pragma("unroll") for (int e = 0; e < ND; ++e) pe[NP + e] = row[e]; \
  }
#else
#define MIOC_DATA_ARG
#define MIOC_DATA_ROW(c)
#endif
#ifdef MIOC_STATES  // YO: the states at the control-grid points, [k][i][r], i = 0..nt
#define MIOC_STATES_ARG , double *YO
#else
#define MIOC_STATES_ARG
#endif
namespace mioc_skeleton {
struct Par {
  double y0[NY];
  double p[NP > 0 ? NP : 1];
};
}  // namespace mioc_skeleton

extern "C" __global__ __launch_bounds__(64) void mioc_ode_program_kernel(
    int K, int nt, double T0, double tau, mioc_skeleton::Par P, const double *X, double *J, double *DF, double *ST,
    const int *gate MIOC_DATA_ARG MIOC_STATES_ARG) {
  if (gate && *gate == 0) return;  // device TRM control: no restart is inside its inner loop
  const unsigned ku = blockIdx.x * 64u + threadIdx.x;
  if (ku >= (unsigned)K) return;
  const size_t k = ku, KK = (size_t)K;
#if ND > 0
  double pe[NP + ND];
#pragma unroll
  for (int e = 0; e < NP; ++e) pe[e] = P.p[e];
  const double *p = pe;
#else
  const double *p = P.p;
#endif
  const double *x = X + k * (size_t)nt * NX;
  // ---- forward: explicit Euler, trapezoid cost (ODEObjective.jl:125-150) ----
  double y[NY], f[NY], xc[NX], xn[NX];
#pragma unroll
  for (int r = 0; r < NY; ++r) y[r] = P.y0[r];
#pragma unroll
  for (int m = 0; m < NX; ++m) xc[m] = x[m];
  MIOC_DATA_ROW(0)  // the data row is that of the control column: xc's for F, xn's for G, column nt - 1 at the end
#ifdef MIOC_STATES
  double *yo = YO ? YO + k * ((size_t)nt + 1) * NY : nullptr;
  if (yo) {
#pragma unroll
    for (int r = 0; r < NY; ++r) yo[r] = y[r];
  }
#endif
  double fval = 0.5 * G(p, 0, T0 + 0.0 * tau, y, xc);
  for (int i = 0; i < nt; ++i) {
    F(p, i, T0 + (double)i * tau, y, xc, f);
#pragma unroll
    for (int r = 0; r < NY; ++r) y[r] = y[r] + tau * f[r];
    if (DF) {
#pragma unroll
      for (int r = 0; r < NY; ++r) ST[((size_t)i * NY + r) * KK + k] = y[r];
    }
#ifdef MIOC_STATES
    if (yo) {
#pragma unroll
      for (int r = 0; r < NY; ++r) yo[((size_t)i + 1) * NY + r] = y[r];
    }
#endif
    if (i < nt - 1) {  // G at step i + 1 sees the control column of step i + 1
#pragma unroll
      for (int m = 0; m < NX; ++m) xn[m] = x[(size_t)(i + 1) * NX + m];
      MIOC_DATA_ROW(i + 1)
      fval = fval + G(p, i + 1, T0 + (double)(i + 1) * tau, y, xn);
#pragma unroll
      for (int m = 0; m < NX; ++m) xc[m] = xn[m];
    } else {
      fval = fval + 0.5 * G(p, nt - 1, T0 + (double)(nt - 1) * tau, y, xc);
    }
  }
#ifdef MIOC_TERMINAL  // the Mayer term at the end time and the last state, data column nt - 1
  if (J) J[k] = fval * tau + E(p, T0 + (double)nt * tau, y);
#else
  if (J) J[k] = fval * tau;
#endif
  if (!DF) return;
  // ---- backward: adjoint and df = Gu - Fu' lambda (ODEObjective.jl:153-184) ----
  // here y is the state after the last step and xc the last control column
  double *df = DF + k * (size_t)nt * NX;
  double gy[NY], gu[NX], fy[NY][NY], fu[NY][NX], lam[NY], a[NY], s[NY];
#pragma unroll
  for (int r = 0; r < NY; ++r) {  // zeroed once per evaluation (ODEObjective.jl:155-162)
    gy[r] = 0.0;
#pragma unroll
    for (int c = 0; c < NY; ++c) fy[r][c] = 0.0;
#pragma unroll
    for (int m = 0; m < NX; ++m) fu[r][m] = 0.0;
  }
#pragma unroll
  for (int m = 0; m < NX; ++m) gu[m] = 0.0;
  Gy(p, nt, T0 + (double)nt * tau, y, xc, gy);
#ifdef MIOC_TERMINAL
  double ey[NY];
#pragma unroll
  for (int r = 0; r < NY; ++r) ey[r] = 0.0;
  Ey(p, T0 + (double)nt * tau, y, ey);
#pragma unroll
  for (int r = 0; r < NY; ++r) lam[r] = (-0.5 * tau) * gy[r] - ey[r];
#else
#pragma unroll
  for (int r = 0; r < NY; ++r) lam[r] = (-0.5 * tau) * gy[r];
#endif
  for (int i = nt - 1; i >= 0; --i) {
    // df[:, i] needs lambda_i and the state before step i (state0 for i = 0); xc is the control column of step i
    const double t = T0 + (double)i * tau;
    if (i == 0) {
#pragma unroll
      for (int r = 0; r < NY; ++r) s[r] = P.y0[r];
    } else {
#pragma unroll
      for (int r = 0; r < NY; ++r) s[r] = ST[((size_t)(i - 1) * NY + r) * KK + k];
    }
    Fu(p, i, t, s, xc, fu);
    Gu(p, i, t, s, xc, gu);
#pragma unroll
    for (int m = 0; m < NX; ++m) {
      double acc = fu[0][m] * lam[0];
#pragma unroll
      for (int r = 1; r < NY; ++r) acc = acc + fu[r][m] * lam[r];
      df[(size_t)i * NX + m] = (0.0 - acc) + gu[m];
    }
    if (i == 0) break;
    // lambda_{i-1} = lambda_i + tau (Fy' lambda_i - Gy), Fy and Gy at (state_{i-1}, x_i)
    Gy(p, i, t, s, xc, gy);
    Fy(p, i, t, s, xc, fy);
#pragma unroll
    for (int c = 0; c < NY; ++c) {
      double acc = fy[0][c] * lam[0];
#pragma unroll
      for (int r = 1; r < NY; ++r) acc = acc + fy[r][c] * lam[r];
      a[c] = acc;
    }
#pragma unroll
    for (int c = 0; c < NY; ++c) lam[c] = lam[c] + tau * (a[c] - gy[c]);
#pragma unroll
    for (int m = 0; m < NX; ++m) xc[m] = x[(size_t)(i - 1) * NX + m];
    MIOC_DATA_ROW(i - 1)
  }
}
)SKEL";

// The Heun / classical RK4 skeleton (mioc_ode_program_create_ex; the scheme and its rounding order are written out in
// include/mioc.h).  NS, the stage count, is #defined in front with NY / NX / NP; the tableau follows from it.  Every
// stage loop is fully unrolled, so ch / ha / hb and the stage arrays are indexed by constants and stay in registers.
// ST holds y_n for every substep n = 0 .. nt*ms - 1, [n][r][k].
const char *const kSkeletonRK = R"SKEL(
#ifndef ND
#define ND 0
#endif
#if ND > 0  // sampled data: p is a per-lane copy of the parameters with the data row of the current column behind them
#define MIOC_DATA_ARG , const double *__restrict__ DATA
#define MIOC_DATA_ROW(c)                                \
  {                                                     \
    const double *row = DATA + (size_t)(c) * ND;        \
    _Pragma("unroll") for (int e = 0; e < ND; ++e) pe[NP + e] = row[e]; \
  }
#else
#define MIOC_DATA_ARG
#define MIOC_DATA_ROW(c)
#endif
#ifdef MIOC_STATES  // YO: the states at the control-grid points, [k][i][r], i = 0..nt
#define MIOC_STATES_ARG , double *YO
#else
#define MIOC_STATES_ARG
#endif
namespace mioc_skeleton {
struct Par {
  double y0[NY];
  double p[NP > 0 ? NP : 1];
};
}  // namespace mioc_skeleton

extern "C" __global__ __launch_bounds__(64) void mioc_ode_program_kernel(
    int K, int nt, int ms, double T0, double tau, double h, mioc_skeleton::Par P, const double *X, double *J,
    double *DF, double *ST, const int *gate MIOC_DATA_ARG MIOC_STATES_ARG) {
  if (gate && *gate == 0) return;  // device TRM control: no restart is inside its inner loop
  const unsigned ku = blockIdx.x * 64u + threadIdx.x;
  if (ku >= (unsigned)K) return;
  const size_t k = ku, KK = (size_t)K;
#if ND > 0
  double pe[NP + ND];
#pragma unroll
  for (int e = 0; e < NP; ++e) pe[e] = P.p[e];
  const double *p = pe;
#else
  const double *p = P.p;
#endif
  const double *x = X + k * (size_t)nt * NX;
  // stage time offsets c_s h, stage weights h a_{s,s-1} (ha[0] unused) and h b_s
  double ch[NS], ha[NS], hb[NS];
#if NS == 2  // Heun: c = (0, 1), a21 = 1, b = (1/2, 1/2)
  ch[0] = 0.0 * h, ch[1] = 1.0 * h;
  ha[0] = 0.0 * h, ha[1] = 1.0 * h;
  hb[0] = 0.5 * h, hb[1] = 0.5 * h;
#else  // classical RK4: c = (0, 1/2, 1/2, 1), a21 = a32 = 1/2, a43 = 1, b = (1/6, 1/3, 1/3, 1/6)
  ch[0] = 0.0 * h, ch[1] = 0.5 * h, ch[2] = 0.5 * h, ch[3] = 1.0 * h;
  ha[0] = 0.0 * h, ha[1] = 0.5 * h, ha[2] = 0.5 * h, ha[3] = 1.0 * h;
  hb[0] = (1.0 / 6.0) * h, hb[1] = (1.0 / 3.0) * h, hb[2] = (1.0 / 3.0) * h, hb[3] = (1.0 / 6.0) * h;
#endif
  // ---- forward: y_{n+1} = y_n + sum_s hb_s k_s, the running cost as the quadrature state q ----
  double y[NY], Y[NY], kk[NS][NY], g[NS], xc[NX];
#pragma unroll
  for (int r = 0; r < NY; ++r) y[r] = P.y0[r];
#ifdef MIOC_STATES
  double *yo = YO ? YO + k * ((size_t)nt + 1) * NY : nullptr;
  if (yo) {
#pragma unroll
    for (int r = 0; r < NY; ++r) yo[r] = y[r];
  }
#endif
  double q = 0.0;
  for (int i = 0; i < nt; ++i) {
#pragma unroll
    for (int m = 0; m < NX; ++m) xc[m] = x[(size_t)i * NX + m];
    MIOC_DATA_ROW(i)  // the data row of the control interval, for every stage and substep
    for (int j = 0; j < ms; ++j) {
      const long long n = (long long)i * ms + j;
      const double tn = T0 + (double)n * h;
      if (DF) {
#pragma unroll
        for (int r = 0; r < NY; ++r) ST[((size_t)n * NY + r) * KK + k] = y[r];
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int r = 0; r < NY; ++r) Y[r] = s == 0 ? y[r] : y[r] + ha[s] * kk[s > 0 ? s - 1 : 0][r];
        F(p, i, tn + ch[s], Y, xc, kk[s]);
        g[s] = G(p, i, tn + ch[s], Y, xc);
      }
#pragma unroll
      for (int r = 0; r < NY; ++r) {
        double inc = hb[0] * kk[0][r];
#pragma unroll
        for (int s = 1; s < NS; ++s) inc = inc + hb[s] * kk[s][r];
        y[r] = y[r] + inc;
      }
      double inc = hb[0] * g[0];
#pragma unroll
      for (int s = 1; s < NS; ++s) inc = inc + hb[s] * g[s];
      q = q + inc;
    }
#ifdef MIOC_STATES
    if (yo) {
#pragma unroll
      for (int r = 0; r < NY; ++r) yo[((size_t)i + 1) * NY + r] = y[r];
    }
#endif
  }
#ifdef MIOC_TERMINAL  // the Mayer term at the end time and the last state, data column nt - 1
  const double tend = T0 + (double)((long long)nt * ms) * h;
  if (J) J[k] = q + E(p, tend, y);
#else
  if (J) J[k] = q;
#endif
  if (!DF) return;
  // ---- backward: the scheme's discrete adjoint; df[:, i] = xbar_i / tau ----
  double *df = DF + k * (size_t)nt * NX;
  double gy[NY], gu[NX], fy[NY][NY], fu[NY][NX], w[NY], YS[NS][NY], kb[NY], Yb[NY], acc[NY], xbar[NX];
#pragma unroll
  for (int r = 0; r < NY; ++r) {  // zeroed once per evaluation, as in the Euler skeleton
    gy[r] = 0.0;
    w[r] = 0.0;
    Yb[r] = 0.0;
#pragma unroll
    for (int c = 0; c < NY; ++c) fy[r][c] = 0.0;
#pragma unroll
    for (int m = 0; m < NX; ++m) fu[r][m] = 0.0;
  }
#pragma unroll
  for (int m = 0; m < NX; ++m) gu[m] = 0.0;
#ifdef MIOC_TERMINAL  // the sweep starts from w = Ey at the last state (y still holds it; the data row is nt - 1's)
  double ey[NY];
#pragma unroll
  for (int r = 0; r < NY; ++r) ey[r] = 0.0;
  Ey(p, tend, y, ey);
#pragma unroll
  for (int r = 0; r < NY; ++r) w[r] = ey[r];
#endif
  for (int i = nt - 1; i >= 0; --i) {
#pragma unroll
    for (int m = 0; m < NX; ++m) {
      xc[m] = x[(size_t)i * NX + m];
      xbar[m] = 0.0;
    }
    MIOC_DATA_ROW(i)
    for (int j = ms - 1; j >= 0; --j) {
      const long long n = (long long)i * ms + j;
      const double tn = T0 + (double)n * h;
#pragma unroll
      for (int r = 0; r < NY; ++r) YS[0][r] = ST[((size_t)n * NY + r) * KK + k];
#pragma unroll
      for (int s = 1; s < NS; ++s) {  // the stage states again, from the stored y_n
        F(p, i, tn + ch[s - 1], YS[s - 1], xc, kk[s - 1]);
#pragma unroll
        for (int r = 0; r < NY; ++r) YS[s][r] = YS[0][r] + ha[s] * kk[s - 1][r];
      }
#pragma unroll
      for (int s = NS - 1; s >= 0; --s) {
#pragma unroll
        for (int r = 0; r < NY; ++r)
          kb[r] = s == NS - 1 ? hb[s] * w[r] : hb[s] * w[r] + ha[s < NS - 1 ? s + 1 : s] * Yb[r];
        Fy(p, i, tn + ch[s], YS[s], xc, fy);
        Gy(p, i, tn + ch[s], YS[s], xc, gy);
        Fu(p, i, tn + ch[s], YS[s], xc, fu);
        Gu(p, i, tn + ch[s], YS[s], xc, gu);
#pragma unroll
        for (int c = 0; c < NY; ++c) {
          double t = fy[0][c] * kb[0];
#pragma unroll
          for (int r = 1; r < NY; ++r) t = t + fy[r][c] * kb[r];
          Yb[c] = t + hb[s] * gy[c];
        }
#pragma unroll
        for (int m = 0; m < NX; ++m) {
          double t = fu[0][m] * kb[0];
#pragma unroll
          for (int r = 1; r < NY; ++r) t = t + fu[r][m] * kb[r];
          xbar[m] = xbar[m] + (t + hb[s] * gu[m]);
        }
#pragma unroll
        for (int c = 0; c < NY; ++c) acc[c] = s == NS - 1 ? Yb[c] : acc[c] + Yb[c];
      }
#pragma unroll
      for (int c = 0; c < NY; ++c) w[c] = w[c] + acc[c];
    }
#pragma unroll
    for (int m = 0; m < NX; ++m) df[(size_t)i * NX + m] = xbar[m] / tau;
  }
}
)SKEL";

// The backward Euler / implicit midpoint skeleton (one stage, Y = y_n + (theta h) k, k = F(Y); the scheme, its Newton
// rule and the rounding order are written out in include/mioc.h).  TH, theta as a double literal, is #defined in front
// with NY / NX / NP.  The kernel signature is kSkeletonRK's.  The stage equation is solved by Newton's method with a
// dense Gaussian elimination in registers: every loop over NY is fully unrolled and the pivoting is conditional row
// swaps, so no array is indexed by a run-time value.  ST holds the stage state Y of every substep, [n][r][k]: the
// backward sweep solves one transposed system per substep and calls neither F nor Newton.
const char *const kSkeletonTheta = R"SKEL(
#define MIOC_ODE_NEWTON_MAX 12
#define MIOC_ODE_NEWTON_TOL 1e-10
#ifndef ND
#define ND 0
#endif
#if ND > 0  // sampled data: p is a per-lane copy of the parameters with the data row of the current column behind them
#define MIOC_DATA_ARG , const double *__restrict__ DATA
#define MIOC_DATA_ROW(c)                                \
  {                                                     \
    const double *row = DATA + (size_t)(c) * ND;        \
    _Pragma("unroll") for (int e = 0; e < ND; ++e) pe[NP + e] = row[e]; \
  }
#else
#define MIOC_DATA_ARG
#define MIOC_DATA_ROW(c)
#endif
#ifdef MIOC_STATES  // YO: the states at the control-grid points, [k][i][r], i = 0..nt
#define MIOC_STATES_ARG , double *YO
#else
#define MIOC_STATES_ARG
#endif
namespace mioc_skeleton {
struct Par {
  double y0[NY];
  double p[NP > 0 ? NP : 1];
};

// A d = b by Gaussian elimination with partial pivoting; A and b are overwritten.  For column c and each r > c in
// turn, rows r and c change places if |A[r][c]| > |A[c][c]|; then f = A[r][c] / A[c][c] and row r = row r - f * row c
// (the entries left of the diagonal are never read again and stay as they are).  Back substitution, left to right:
// d[r] = ((b[r] - A[r][r+1]*d[r+1]) - ...) / A[r][r].  A singular A gives non-finite d.
__device__ __forceinline__ void solve(double (*A)[NY], double *b, double *d) {
#pragma unroll
  for (int c = 0; c < NY; ++c) {
#pragma unroll
    for (int r = c + 1; r < NY; ++r) {
      const bool sw = fabs(A[r][c]) > fabs(A[c][c]);
#pragma unroll
      for (int e = c; e < NY; ++e) {
        const double u = A[c][e], v = A[r][e];
        A[c][e] = sw ? v : u;
        A[r][e] = sw ? u : v;
      }
      const double u = b[c], v = b[r];
      b[c] = sw ? v : u;
      b[r] = sw ? u : v;
    }
#pragma unroll
    for (int r = c + 1; r < NY; ++r) {
      const double f = A[r][c] / A[c][c];
#pragma unroll
      for (int e = c + 1; e < NY; ++e) A[r][e] = A[r][e] - f * A[c][e];
      b[r] = b[r] - f * b[c];
    }
  }
#pragma unroll
  for (int r = NY - 1; r >= 0; --r) {
    double s = b[r];
#pragma unroll
    for (int e = r + 1; e < NY; ++e) s = s - A[r][e] * d[e];
    d[r] = s / A[r][r];
  }
}
}  // namespace mioc_skeleton

extern "C" __global__ __launch_bounds__(64) void mioc_ode_program_kernel(
    int K, int nt, int ms, double T0, double tau, double h, mioc_skeleton::Par P, const double *X, double *J,
    double *DF, double *ST, const int *gate MIOC_DATA_ARG MIOC_STATES_ARG) {
  if (gate && *gate == 0) return;  // device TRM control: no restart is inside its inner loop
  const unsigned ku = blockIdx.x * 64u + threadIdx.x;
  if (ku >= (unsigned)K) return;
  const size_t k = ku, KK = (size_t)K;
#if ND > 0
  double pe[NP + ND];
#pragma unroll
  for (int e = 0; e < NP; ++e) pe[e] = P.p[e];
  const double *p = pe;
#else
  const double *p = P.p;
#endif
  const double *x = X + k * (size_t)nt * NX;
  const double th = TH * h, thh = th * h;  // theta h and (theta h) h, each rounded once
  // ---- forward: Newton on k = F(y_n + th k) from k = F(y_n); y_{n+1} = y_n + h k, q_{n+1} = q_n + h G(Y) ----
  double y[NY], Y[NY], kv[NY], f[NY], d[NY], xc[NX], fy[NY][NY], A[NY][NY];
#pragma unroll
  for (int r = 0; r < NY; ++r) {
    y[r] = P.y0[r];
#pragma unroll
    for (int c = 0; c < NY; ++c) fy[r][c] = 0.0;  // zeroed once per evaluation, as in the other skeletons
  }
#ifdef MIOC_STATES
  double *yo = YO ? YO + k * ((size_t)nt + 1) * NY : nullptr;
  if (yo) {
#pragma unroll
    for (int r = 0; r < NY; ++r) yo[r] = y[r];
  }
#endif
  double q = 0.0;
  bool failed = false;
  for (int i = 0; i < nt && !failed; ++i) {
#pragma unroll
    for (int m = 0; m < NX; ++m) xc[m] = x[(size_t)i * NX + m];
    MIOC_DATA_ROW(i)  // the data row of the control interval, for every substep
    for (int j = 0; j < ms && !failed; ++j) {
      const long long n = (long long)i * ms + j;
      const double ts = (T0 + (double)n * h) + th;
      F(p, i, ts, y, xc, kv);
      bool conv = false;
#pragma nounroll
      for (int it = 0; it < MIOC_ODE_NEWTON_MAX && !conv; ++it) {
#pragma unroll
        for (int r = 0; r < NY; ++r) Y[r] = y[r] + th * kv[r];
        F(p, i, ts, Y, xc, f);
        Fy(p, i, ts, Y, xc, fy);
#pragma unroll
        for (int r = 0; r < NY; ++r) {
          f[r] = f[r] - kv[r];
#pragma unroll
          for (int c = 0; c < NY; ++c) A[r][c] = (r == c ? 1.0 : 0.0) - th * fy[r][c];
        }
        mioc_skeleton::solve(A, f, d);
        double kmax = 1.0;
#pragma unroll
        for (int r = 0; r < NY; ++r) {
          kv[r] = kv[r] + d[r];
          kmax = fmax(kmax, fabs(kv[r]));
        }
        // component by component: a NaN in d or kv fails the comparison, an infinite kv its own
        const double tol = MIOC_ODE_NEWTON_TOL * kmax;
        conv = true;
#pragma unroll
        for (int r = 0; r < NY; ++r) conv = conv && fabs(d[r]) <= tol && fabs(kv[r]) <= 1.7976931348623157e308;
      }
      failed = !conv;
#pragma unroll
      for (int r = 0; r < NY; ++r) Y[r] = y[r] + th * kv[r];
      if (DF) {
#pragma unroll
        for (int r = 0; r < NY; ++r) ST[((size_t)n * NY + r) * KK + k] = Y[r];
      }
      q = q + h * G(p, i, ts, Y, xc);
#pragma unroll
      for (int r = 0; r < NY; ++r) y[r] = y[r] + h * kv[r];
    }
#ifdef MIOC_STATES
    if (yo) {
#pragma unroll
      for (int r = 0; r < NY; ++r) yo[((size_t)i + 1) * NY + r] = y[r];
    }
#endif
  }
  if (failed) {  // a substep's Newton iteration did not converge: this restart's J and df row are NaN
    const double nan = __builtin_nan("");
    if (J) J[k] = nan;
    if (DF)
      for (size_t e = 0; e < (size_t)nt * NX; ++e) DF[k * (size_t)nt * NX + e] = nan;
#ifdef MIOC_STATES  // and so is its state trajectory, the rows already written included
    if (yo)
      for (size_t e = 0; e < ((size_t)nt + 1) * NY; ++e) yo[e] = nan;
#endif
    return;
  }
#ifdef MIOC_TERMINAL  // the Mayer term at the end time and the last state, data column nt - 1
  const double tend = T0 + (double)((long long)nt * ms) * h;
  if (J) J[k] = q + E(p, tend, y);
#else
  if (J) J[k] = q;
#endif
  if (!DF) return;
  // ---- backward: (I - th Fy)' mu = h w + (th h) Gy at the stored Y; df[:, i] = xbar_i / tau ----
  double *df = DF + k * (size_t)nt * NX;
  double gy[NY], gu[NX], fu[NY][NX], w[NY], kb[NY], mu[NY], xbar[NX];
#pragma unroll
  for (int r = 0; r < NY; ++r) {
    gy[r] = 0.0;
    w[r] = 0.0;
#pragma unroll
    for (int m = 0; m < NX; ++m) fu[r][m] = 0.0;
  }
#pragma unroll
  for (int m = 0; m < NX; ++m) gu[m] = 0.0;
#ifdef MIOC_TERMINAL  // the sweep starts from w = Ey at the last state (y still holds it; the data row is nt - 1's)
  double ey[NY];
#pragma unroll
  for (int r = 0; r < NY; ++r) ey[r] = 0.0;
  Ey(p, tend, y, ey);
#pragma unroll
  for (int r = 0; r < NY; ++r) w[r] = ey[r];
#endif
  for (int i = nt - 1; i >= 0; --i) {
#pragma unroll
    for (int m = 0; m < NX; ++m) {
      xc[m] = x[(size_t)i * NX + m];
      xbar[m] = 0.0;
    }
    MIOC_DATA_ROW(i)
    for (int j = ms - 1; j >= 0; --j) {
      const long long n = (long long)i * ms + j;
      const double ts = (T0 + (double)n * h) + th;
#pragma unroll
      for (int r = 0; r < NY; ++r) Y[r] = ST[((size_t)n * NY + r) * KK + k];
      Fy(p, i, ts, Y, xc, fy);
      Gy(p, i, ts, Y, xc, gy);
#pragma unroll
      for (int r = 0; r < NY; ++r) {
        kb[r] = h * w[r] + thh * gy[r];
#pragma unroll
        for (int c = 0; c < NY; ++c) A[r][c] = (r == c ? 1.0 : 0.0) - th * fy[c][r];
      }
      mioc_skeleton::solve(A, kb, mu);
      Fu(p, i, ts, Y, xc, fu);
      Gu(p, i, ts, Y, xc, gu);
#pragma unroll
      for (int m = 0; m < NX; ++m) {
        double t = fu[0][m] * mu[0];
#pragma unroll
        for (int r = 1; r < NY; ++r) t = t + fu[r][m] * mu[r];
        xbar[m] = xbar[m] + (t + h * gu[m]);
      }
#pragma unroll
      for (int c = 0; c < NY; ++c) {
        double t = fy[0][c] * mu[0];
#pragma unroll
        for (int r = 1; r < NY; ++r) t = t + fy[r][c] * mu[r];
        w[c] = w[c] + (t + h * gy[c]);
      }
    }
#pragma unroll
    for (int m = 0; m < NX; ++m) df[(size_t)i * NX + m] = xbar[m] / tau;
  }
}
)SKEL";

// The forward-mode AD prelude of mioc_ode_program_create_ad (derive != 0): mioc_ad::Dual<N>, a value and N tangents,
// all members indexed by constants under full unrolling, so a Dual lives in registers.  It stands in front of the
// caller's text, which defines F and G as templates over the scalar type; argument-dependent lookup resolves
// sqrt(T), fmin(T, T), ... to ::sqrt for T = double and to the overloads below for a Dual.  Every tangent rule and its
// rounding order is written out in include/mioc.h ("Derived hooks"); a double operand is never promoted to a Dual, and
// no product with a zero tangent is folded (no fast-math: 0.0 * v is not 0.0 for a non-finite or negative v).
const char *const kAdPrelude = R"SKEL(
namespace mioc_ad {
template <int N>
struct Dual {
  double v;
  double d[N];
  Dual() = default;
  __device__ __forceinline__ Dual(double c) : v(c) {
#pragma unroll
    for (int k = 0; k < N; ++k) d[k] = 0.0;
  }
};
__device__ __forceinline__ double value(double a) { return a; }
template <int N> __device__ __forceinline__ double value(const Dual<N> &a) { return a.v; }

#define MIOC_AD_FN template <int N> __device__ __forceinline__ Dual<N>
#define MIOC_AD_EACH _Pragma("unroll") for (int k = 0; k < N; ++k)
MIOC_AD_FN operator+(const Dual<N> &a) { return a; }
MIOC_AD_FN operator-(const Dual<N> &a) {
  Dual<N> r;
  r.v = -a.v;
  MIOC_AD_EACH r.d[k] = -a.d[k];
  return r;
}
MIOC_AD_FN operator+(const Dual<N> &a, const Dual<N> &b) {
  Dual<N> r;
  r.v = a.v + b.v;
  MIOC_AD_EACH r.d[k] = a.d[k] + b.d[k];
  return r;
}
MIOC_AD_FN operator+(const Dual<N> &a, double b) {
  Dual<N> r;
  r.v = a.v + b;
  MIOC_AD_EACH r.d[k] = a.d[k];
  return r;
}
MIOC_AD_FN operator+(double a, const Dual<N> &b) {
  Dual<N> r;
  r.v = a + b.v;
  MIOC_AD_EACH r.d[k] = b.d[k];
  return r;
}
MIOC_AD_FN operator-(const Dual<N> &a, const Dual<N> &b) {
  Dual<N> r;
  r.v = a.v - b.v;
  MIOC_AD_EACH r.d[k] = a.d[k] - b.d[k];
  return r;
}
MIOC_AD_FN operator-(const Dual<N> &a, double b) {
  Dual<N> r;
  r.v = a.v - b;
  MIOC_AD_EACH r.d[k] = a.d[k];
  return r;
}
MIOC_AD_FN operator-(double a, const Dual<N> &b) {
  Dual<N> r;
  r.v = a - b.v;
  MIOC_AD_EACH r.d[k] = -b.d[k];
  return r;
}
MIOC_AD_FN operator*(const Dual<N> &a, const Dual<N> &b) {
  Dual<N> r;
  r.v = a.v * b.v;
  MIOC_AD_EACH r.d[k] = a.d[k] * b.v + a.v * b.d[k];
  return r;
}
MIOC_AD_FN operator*(const Dual<N> &a, double b) {
  Dual<N> r;
  r.v = a.v * b;
  MIOC_AD_EACH r.d[k] = a.d[k] * b;
  return r;
}
MIOC_AD_FN operator*(double a, const Dual<N> &b) {
  Dual<N> r;
  r.v = a * b.v;
  MIOC_AD_EACH r.d[k] = a * b.d[k];
  return r;
}
MIOC_AD_FN operator/(const Dual<N> &a, const Dual<N> &b) {
  Dual<N> r;
  r.v = a.v / b.v;
  MIOC_AD_EACH r.d[k] = (a.d[k] - r.v * b.d[k]) / b.v;
  return r;
}
MIOC_AD_FN operator/(const Dual<N> &a, double b) {
  Dual<N> r;
  r.v = a.v / b;
  MIOC_AD_EACH r.d[k] = a.d[k] / b;
  return r;
}
MIOC_AD_FN operator/(double a, const Dual<N> &b) {
  Dual<N> r;
  r.v = a / b.v;
  MIOC_AD_EACH r.d[k] = (-(r.v * b.d[k])) / b.v;
  return r;
}
#define MIOC_AD_ASSIGN(op)                                                                                   \
  template <int N> __device__ __forceinline__ Dual<N> &operator op##=(Dual<N> &a, const Dual<N> &b) {        \
    a = a op b;                                                                                              \
    return a;                                                                                                \
  }                                                                                                          \
  template <int N> __device__ __forceinline__ Dual<N> &operator op##=(Dual<N> &a, double b) {                \
    a = a op b;                                                                                              \
    return a;                                                                                                \
  }
MIOC_AD_ASSIGN(+)
MIOC_AD_ASSIGN(-)
MIOC_AD_ASSIGN(*)
MIOC_AD_ASSIGN(/)
#undef MIOC_AD_ASSIGN
#define MIOC_AD_COMPARE(op)                                                                                  \
  template <int N> __device__ __forceinline__ bool operator op(const Dual<N> &a, const Dual<N> &b) {         \
    return a.v op b.v;                                                                                       \
  }                                                                                                          \
  template <int N> __device__ __forceinline__ bool operator op(const Dual<N> &a, double b) { return a.v op b; } \
  template <int N> __device__ __forceinline__ bool operator op(double a, const Dual<N> &b) { return a op b.v; }
MIOC_AD_COMPARE(<)
MIOC_AD_COMPARE(<=)
MIOC_AD_COMPARE(>)
MIOC_AD_COMPARE(>=)
MIOC_AD_COMPARE(==)
MIOC_AD_COMPARE(!=)
#undef MIOC_AD_COMPARE
MIOC_AD_FN sqrt(const Dual<N> &a) {
  Dual<N> r;
  r.v = ::sqrt(a.v);
  const double g = 2.0 * r.v;
  MIOC_AD_EACH r.d[k] = a.d[k] / g;
  return r;
}
MIOC_AD_FN exp(const Dual<N> &a) {
  Dual<N> r;
  r.v = ::exp(a.v);
  MIOC_AD_EACH r.d[k] = a.d[k] * r.v;
  return r;
}
MIOC_AD_FN log(const Dual<N> &a) {
  Dual<N> r;
  r.v = ::log(a.v);
  MIOC_AD_EACH r.d[k] = a.d[k] / a.v;
  return r;
}
MIOC_AD_FN sin(const Dual<N> &a) {
  Dual<N> r;
  r.v = ::sin(a.v);
  const double g = ::cos(a.v);
  MIOC_AD_EACH r.d[k] = a.d[k] * g;
  return r;
}
MIOC_AD_FN cos(const Dual<N> &a) {
  Dual<N> r;
  r.v = ::cos(a.v);
  const double g = -::sin(a.v);
  MIOC_AD_EACH r.d[k] = a.d[k] * g;
  return r;
}
MIOC_AD_FN tan(const Dual<N> &a) {
  Dual<N> r;
  r.v = ::tan(a.v);
  const double g = 1.0 + r.v * r.v;
  MIOC_AD_EACH r.d[k] = a.d[k] * g;
  return r;
}
MIOC_AD_FN tanh(const Dual<N> &a) {
  Dual<N> r;
  r.v = ::tanh(a.v);
  const double g = 1.0 - r.v * r.v;
  MIOC_AD_EACH r.d[k] = a.d[k] * g;
  return r;
}
MIOC_AD_FN atan(const Dual<N> &a) {
  Dual<N> r;
  r.v = ::atan(a.v);
  const double g = 1.0 + a.v * a.v;
  MIOC_AD_EACH r.d[k] = a.d[k] / g;
  return r;
}
MIOC_AD_FN fabs(const Dual<N> &a) {
  Dual<N> r;
  r.v = ::fabs(a.v);
  MIOC_AD_EACH r.d[k] = a.v < 0.0 ? -a.d[k] : a.d[k];
  return r;
}
MIOC_AD_FN pow(const Dual<N> &a, double b) {
  Dual<N> r;
  r.v = ::pow(a.v, b);
  const double g = b * ::pow(a.v, b - 1.0);
  MIOC_AD_EACH r.d[k] = g * a.d[k];
  return r;
}
MIOC_AD_FN pow(const Dual<N> &a, const Dual<N> &b) {
  Dual<N> r;
  r.v = ::pow(a.v, b.v);
  const double g = b.v * ::pow(a.v, b.v - 1.0), e = r.v * ::log(a.v);
  MIOC_AD_EACH r.d[k] = g * a.d[k] + e * b.d[k];
  return r;
}
MIOC_AD_FN fmin(const Dual<N> &a, const Dual<N> &b) { return b.v < a.v ? b : a; }
MIOC_AD_FN fmin(const Dual<N> &a, double b) { return b < a.v ? Dual<N>(b) : a; }
MIOC_AD_FN fmin(double a, const Dual<N> &b) { return b.v < a ? b : Dual<N>(a); }
MIOC_AD_FN fmax(const Dual<N> &a, const Dual<N> &b) { return b.v > a.v ? b : a; }
MIOC_AD_FN fmax(const Dual<N> &a, double b) { return b > a.v ? Dual<N>(b) : a; }
MIOC_AD_FN fmax(double a, const Dual<N> &b) { return b.v > a ? b : Dual<N>(a); }
#undef MIOC_AD_EACH
#undef MIOC_AD_FN
}  // namespace mioc_ad
)SKEL";

// The generated hooks: F, G or E once with T = mioc_ad::Dual<N>, the unit tangents on y (Fy, Gy, Ey: N = NY) or on x
// (Fu, Gu: N = NX), the other argument constant.  Every entry of the output is written.  Each stands under the guard
// macro that the head defines for a derived hook.  MIOC_AD_NOINLINE (the second compile of mioc_ode_program_create_ad) makes
// them functions that are called: one body each, where the Heun / RK4 skeleton would inline one per stage.
const char *const kAdHooks = R"SKEL(
#ifdef MIOC_AD_NOINLINE
#define MIOC_AD_HOOK __device__ __attribute__((noinline))
#else
#define MIOC_AD_HOOK __device__
#endif
#ifdef MIOC_DERIVE_FY
MIOC_AD_HOOK void Fy(const double *p, int i, double t, const double *y, const double *x, double (*fy)[NY]) {
  mioc_ad::Dual<NY> yd[NY], xd[NX], fd[NY];
#pragma unroll
  for (int r = 0; r < NY; ++r) {
    yd[r] = y[r];
    yd[r].d[r] = 1.0;
  }
#pragma unroll
  for (int m = 0; m < NX; ++m) xd[m] = x[m];
  F(p, i, t, (const mioc_ad::Dual<NY> *)yd, (const mioc_ad::Dual<NY> *)xd, fd);
#pragma unroll
  for (int r = 0; r < NY; ++r) {
#pragma unroll
    for (int c = 0; c < NY; ++c) fy[r][c] = fd[r].d[c];
  }
}
#endif
#ifdef MIOC_DERIVE_FU
MIOC_AD_HOOK void Fu(const double *p, int i, double t, const double *y, const double *x, double (*fu)[NX]) {
  mioc_ad::Dual<NX> yd[NY], xd[NX], fd[NY];
#pragma unroll
  for (int r = 0; r < NY; ++r) yd[r] = y[r];
#pragma unroll
  for (int m = 0; m < NX; ++m) {
    xd[m] = x[m];
    xd[m].d[m] = 1.0;
  }
  F(p, i, t, (const mioc_ad::Dual<NX> *)yd, (const mioc_ad::Dual<NX> *)xd, fd);
#pragma unroll
  for (int r = 0; r < NY; ++r) {
#pragma unroll
    for (int m = 0; m < NX; ++m) fu[r][m] = fd[r].d[m];
  }
}
#endif
#ifdef MIOC_DERIVE_GY
MIOC_AD_HOOK void Gy(const double *p, int i, double t, const double *y, const double *x, double *gy) {
  mioc_ad::Dual<NY> yd[NY], xd[NX];
#pragma unroll
  for (int r = 0; r < NY; ++r) {
    yd[r] = y[r];
    yd[r].d[r] = 1.0;
  }
#pragma unroll
  for (int m = 0; m < NX; ++m) xd[m] = x[m];
  const mioc_ad::Dual<NY> g = G(p, i, t, (const mioc_ad::Dual<NY> *)yd, (const mioc_ad::Dual<NY> *)xd);
#pragma unroll
  for (int r = 0; r < NY; ++r) gy[r] = g.d[r];
}
#endif
#ifdef MIOC_DERIVE_GU
MIOC_AD_HOOK void Gu(const double *p, int i, double t, const double *y, const double *x, double *gu) {
  mioc_ad::Dual<NX> yd[NY], xd[NX];
#pragma unroll
  for (int r = 0; r < NY; ++r) yd[r] = y[r];
#pragma unroll
  for (int m = 0; m < NX; ++m) {
    xd[m] = x[m];
    xd[m].d[m] = 1.0;
  }
  const mioc_ad::Dual<NX> g = G(p, i, t, (const mioc_ad::Dual<NX> *)yd, (const mioc_ad::Dual<NX> *)xd);
#pragma unroll
  for (int m = 0; m < NX; ++m) gu[m] = g.d[m];
}
#endif
#ifdef MIOC_DERIVE_EY
MIOC_AD_HOOK void Ey(const double *p, double t, const double *y, double *ey) {
  mioc_ad::Dual<NY> yd[NY];
#pragma unroll
  for (int r = 0; r < NY; ++r) {
    yd[r] = y[r];
    yd[r].d[r] = 1.0;
  }
  const mioc_ad::Dual<NY> e = E(p, t, (const mioc_ad::Dual<NY> *)yd);
#pragma unroll
  for (int r = 0; r < NY; ++r) ey[r] = e.d[r];
}
#endif
)SKEL";

// ---- hiprtc, loaded at the first mioc_ode_program_create -------------------------------------------------------
struct Rtc {
  bool ok = false;
  std::string why;
  decltype(&hiprtcCreateProgram) create = nullptr;
  decltype(&hiprtcCompileProgram) compile = nullptr;
  decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
  decltype(&hiprtcGetProgramLog) log = nullptr;
  decltype(&hiprtcGetCodeSize) code_size = nullptr;
  decltype(&hiprtcGetCode) code = nullptr;
  decltype(&hiprtcDestroyProgram) destroy = nullptr;
};

const Rtc &rtc() {
  static const Rtc r = [] {
    Rtc q;
    void *h = nullptr;
    for (const char *name : {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"}) {
      h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (h) break;
    }
    if (!h) {
      q.why = "libhiprtc.so not found (it is part of the ROCm install)";
      return q;
    }
    q.create = reinterpret_cast<decltype(q.create)>(dlsym(h, "hiprtcCreateProgram"));
    q.compile = reinterpret_cast<decltype(q.compile)>(dlsym(h, "hiprtcCompileProgram"));
    q.log_size = reinterpret_cast<decltype(q.log_size)>(dlsym(h, "hiprtcGetProgramLogSize"));
    q.log = reinterpret_cast<decltype(q.log)>(dlsym(h, "hiprtcGetProgramLog"));
    q.code_size = reinterpret_cast<decltype(q.code_size)>(dlsym(h, "hiprtcGetCodeSize"));
    q.code = reinterpret_cast<decltype(q.code)>(dlsym(h, "hiprtcGetCode"));
    q.destroy = reinterpret_cast<decltype(q.destroy)>(dlsym(h, "hiprtcDestroyProgram"));
    q.ok = q.create && q.compile && q.log_size && q.log && q.code_size && q.code && q.destroy;
    if (!q.ok) q.why = "libhiprtc.so lacks a hiprtc entry point";
    return q;
  }();
  return r;
}

void put_log(char *log, int64_t cap, const char *text, size_t n) {
  if (!log || cap < 1) return;
  const size_t m = n < (size_t)(cap - 1) ? n : (size_t)(cap - 1);
  std::memcpy(log, text, m);
  log[m] = '\0';
}

int fail(mioc_ctx *ctx, int code, const std::string &msg) {
  ctx->err = msg;
  return code;
}

// The number after `key` in the compiler's resource remarks of the kernel (-Rpass-analysis=kernel-resource-usage), -1
// if there is none.
long remark_value(const std::string &log, const char *key) {
  size_t at = log.find(std::string("Function Name: ") + kKernelName);
  if (at == std::string::npos) return -1;
  at = log.find(key, at);
  if (at == std::string::npos) return -1;
  return std::strtol(log.c_str() + at + std::strlen(key), nullptr, 10);
}

// Does the kernel need more than the 256 architectural VGPRs (AGPRs as spill space, or vector spills to scratch)?
bool over_vgpr_file(const std::string &log) {
  return remark_value(log, " AGPRs: ") > 0 || remark_value(log, " VGPRs Spill: ") > 0;
}

// The log without the remarks.  A diagnostic is its head line ("file:line:col: kind: ...") and the indented source lines
// under it; a note belongs to the diagnostic before it.  So a clean compile leaves an empty log as before.
std::string without_remarks(const std::string &log) {
  std::string out;
  bool drop = false;
  for (size_t at = 0; at < log.size();) {
    size_t end = log.find('\n', at);
    end = end == std::string::npos ? log.size() : end + 1;
    const std::string line = log.substr(at, end - at);
    if (line[0] != ' ' && line[0] != '\n' && line.find(": note: ") == std::string::npos)
      drop = line.find(": remark: ") != std::string::npos;
    if (!drop) out += line;
    at = end;
  }
  return out;
}

}  // namespace

struct mioc_ode_program {
  int ny = 0, nx = 0, np = 0, nd = 0, flags = 0;
  int integrator = MIOC_ODE_INT_EULER, substeps = 1;
  std::vector<char> code;  // the gfx950 code object
  struct Loaded {
    int device;
    hipModule_t mod;
    hipFunction_t fn;
  };
  std::mutex mu;
  std::vector<Loaded> loaded;  // one module per device the program ran on
};

extern "C" {

int32_t mioc_ode_program_create(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, mioc_ode_program **out,
                                char *log, int64_t log_cap) {
  return mioc_ode_program_create_ex(hooks, ny, nx, nparams, MIOC_ODE_INT_EULER, 1, out, log, log_cap);
}

int32_t mioc_ode_program_create_ex(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t integrator,
                                   int32_t substeps, mioc_ode_program **out, char *log, int64_t log_cap) {
  return mioc_ode_program_create_ad(hooks, ny, nx, nparams, integrator, substeps, 0, out, log, log_cap);
}

int32_t mioc_ode_program_create_ad(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t integrator,
                                   int32_t substeps, int32_t derive, mioc_ode_program **out, char *log,
                                   int64_t log_cap) {
  return mioc_ode_program_create_bolza(hooks, ny, nx, nparams, 0, integrator, substeps, derive, 0, out, log, log_cap);
}

int32_t mioc_ode_program_create_bolza(const char *hooks, int32_t ny, int32_t nx, int32_t nparams, int32_t ndata,
                                      int32_t integrator, int32_t substeps, int32_t derive, int32_t flags,
                                      mioc_ode_program **out, char *log, int64_t log_cap) {
  put_log(log, log_cap, "", 0);
  if (!out) return MIOC_EINVAL;
  *out = nullptr;
  if (!hooks || ny < 1 || ny > kMaxNY || nx < 1 || nx > kMaxNX || nparams < 0 || nparams > kMaxNP) return MIOC_EINVAL;
  if (ndata < 0 || ndata > kMaxND || (flags & ~(MIOC_ODE_TERMINAL | MIOC_ODE_STATES))) return MIOC_EINVAL;
  const bool implicit = integrator == MIOC_ODE_INT_BEULER || integrator == MIOC_ODE_INT_MIDPOINT;
  if (integrator != MIOC_ODE_INT_EULER && integrator != MIOC_ODE_INT_HEUN && integrator != MIOC_ODE_INT_RK4 && !implicit)
    return MIOC_EINVAL;
  if (substeps < 1 || substeps > kMaxSubsteps || (integrator == MIOC_ODE_INT_EULER && substeps != 1)) return MIOC_EINVAL;
  if (derive & ~(MIOC_ODE_DERIVE_ALL | MIOC_ODE_DERIVE_EY)) return MIOC_EINVAL;
  if ((derive & MIOC_ODE_DERIVE_EY) && !(flags & MIOC_ODE_TERMINAL)) return MIOC_EINVAL;
  // the reference scheme keeps its own skeleton and its head, so its source text is what it was
  const char *const skeleton = integrator == MIOC_ODE_INT_EULER ? kSkeleton : implicit ? kSkeletonTheta : kSkeletonRK;
  const size_t len = strnlen(hooks, kMaxSource + 1);
  if (len > kMaxSource) return MIOC_EINVAL;
  const Rtc &R = rtc();
  if (!R.ok) {
    put_log(log, log_cap, R.why.c_str(), R.why.size());
    return MIOC_EHIP;
  }
  std::string src;
  try {
    char head[128];
    if (integrator == MIOC_ODE_INT_EULER)
      std::snprintf(head, sizeof head, "#define NY %d\n#define NX %d\n#define NP %d\n", (int)ny, (int)nx, (int)nparams);
    else if (implicit)  // TH: theta, 1 for backward Euler and 1/2 for the implicit midpoint rule
      std::snprintf(head, sizeof head, "#define NY %d\n#define NX %d\n#define NP %d\n#define TH %s\n", (int)ny, (int)nx,
                    (int)nparams, integrator == MIOC_ODE_INT_BEULER ? "1.0" : "0.5");
    else  // NS: the stage count, which selects the tableau
      std::snprintf(head, sizeof head, "#define NY %d\n#define NX %d\n#define NP %d\n#define NS %d\n", (int)ny, (int)nx,
                    (int)nparams, integrator == MIOC_ODE_INT_HEUN ? 2 : 4);
    src.reserve(len + std::strlen(skeleton) + (derive ? std::strlen(kAdPrelude) + std::strlen(kAdHooks) : 0) + 512);
    src = head;
    // sampled data, the terminal cost and the state output are compiled in only when asked for: none adds a byte here
    if (ndata > 0) src += "#define ND " + std::to_string((int)ndata) + "\n";
    if (flags & MIOC_ODE_TERMINAL) src += "#define MIOC_TERMINAL 1\n";
    if (flags & MIOC_ODE_STATES) src += "#define MIOC_STATES 1\n";
    if (derive) {  // the guard macros and the dual type in front of the caller's text; derive == 0 adds no byte
      if (derive & MIOC_ODE_DERIVE_FY) src += "#define MIOC_DERIVE_FY 1\n";
      if (derive & MIOC_ODE_DERIVE_FU) src += "#define MIOC_DERIVE_FU 1\n";
      if (derive & MIOC_ODE_DERIVE_GY) src += "#define MIOC_DERIVE_GY 1\n";
      if (derive & MIOC_ODE_DERIVE_GU) src += "#define MIOC_DERIVE_GU 1\n";
      if (derive & MIOC_ODE_DERIVE_EY) src += "#define MIOC_DERIVE_EY 1\n";
      src += "#line 1 \"mioc_ad\"";
      src += kAdPrelude;
    }
    src += "#line 1 \"hooks\"\n";
    src.append(hooks, len);
    if (flags & MIOC_ODE_TERMINAL)  // still under "hooks": a text without E is diagnosed there (hooks:N) first
      src += "\n__device__ inline double mioc_terminal_needs_E(const double *p, double t, const double *y) "
             "{ return E(p, t, y); }";
    if (derive) {  // the generated hooks between the caller's text and the skeleton
      src += "\n#line 1 \"mioc_ad_hooks\"";
      src += kAdHooks;
    }
    src += "\n#line 1 \"mioc_ode_program_skeleton\"";
    src += skeleton;
  } catch (const std::bad_alloc &) {
    return MIOC_ENOMEM;
  }
  // the flags of csrc/Makefile that bear on the arithmetic: no FMA contraction, no fast-math.  With derived hooks the
  // compiler also reports the kernel's registers (remarks, taken out of the log again): a kernel that needs more than
  // the 256 architectural VGPRs with every generated hook inlined at each of its call sites is compiled a second time
  // with the generated hooks as functions (MIOC_AD_NOINLINE), one body each however many stages call it.
  const char *opts[] = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math",
                        "-Rpass-analysis=kernel-resource-usage"};
  const int nopts = derive ? 5 : 4;
  int ret = MIOC_OK;
  for (int pass = 0; pass < 2; ++pass) {
    hiprtcProgram prog = nullptr;
    if (R.create(&prog, src.c_str(), "mioc_ode_program.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
      const char msg[] = "hiprtcCreateProgram failed";
      put_log(log, log_cap, msg, sizeof msg - 1);
      return MIOC_ECOMPILE;
    }
    const hiprtcResult rc = R.compile(prog, nopts, opts);
    bool again = false;
    ret = MIOC_OK;
    try {
      size_t ln = 0;
      std::string text;
      if (R.log_size(prog, &ln) == HIPRTC_SUCCESS && ln > 1) {
        std::vector<char> buf(ln + 1, '\0');
        if (R.log(prog, buf.data()) == HIPRTC_SUCCESS) text.assign(buf.data(), strnlen(buf.data(), ln));
      }
      if (derive) {
        again = pass == 0 && rc == HIPRTC_SUCCESS && over_vgpr_file(text);
        text = without_remarks(text);
        if (pass == 1) text.insert(0, kNoinlineNote);
      }
      put_log(log, log_cap, text.c_str(), text.size());
      if (rc != HIPRTC_SUCCESS) {
        ret = MIOC_ECOMPILE;
      } else if (again) {
        src.insert(0, "#define MIOC_AD_NOINLINE 1\n");
      } else {
        size_t cn = 0;
        mioc_ode_program *p = new mioc_ode_program;
        p->ny = ny, p->nx = nx, p->np = nparams, p->nd = ndata, p->flags = flags;
        p->integrator = integrator, p->substeps = substeps;
        if (R.code_size(prog, &cn) != HIPRTC_SUCCESS || cn == 0) {
          ret = MIOC_ECOMPILE;
        } else {
          p->code.resize(cn);
          if (R.code(prog, p->code.data()) != HIPRTC_SUCCESS) ret = MIOC_ECOMPILE;
        }
        if (ret == MIOC_OK)
          *out = p;
        else
          delete p;
      }
    } catch (const std::bad_alloc &) {
      ret = MIOC_ENOMEM;
      again = false;
    }
    R.destroy(&prog);
    if (!again) break;
  }
  return ret;
}

int32_t mioc_ode_program_destroy(mioc_ode_program *prog) {
  if (!prog) return MIOC_EINVAL;
  int rc = MIOC_OK;
  if (!prog->loaded.empty()) {
    int prev = 0;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    for (const auto &l : prog->loaded) {  // a launch may still be in flight on this device
      if (hipSetDevice(l.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
          hipModuleUnload(l.mod) != hipSuccess)
        rc = MIOC_EHIP;
    }
    if (have_prev) (void)hipSetDevice(prev);
  }
  delete prog;
  return rc;
}

// The body of both eval entries.  nu = 0: every control is the DP's (mioc_ode_program_eval_device); nu >= 1: the first
// nu controls are continuous and the levels describe the other nx - nu (mioc_ode_program_eval_mixed_device).
static int32_t program_eval(mioc_ctx *ctx, mioc_ode_program *prog, int64_t nu, int64_t K, const double *d_x, int64_t nt,
                            double T0, double T1, const double *state0, const double *params, const double *d_data,
                            double *d_J, double *d_df, double *d_Y) {
  if (!ctx) return MIOC_EINVAL;
  MIOC_JOIN_BT(ctx);
  if (!prog) return fail(ctx, MIOC_EINVAL, "no ODE program");
  if (K < 1 || nt < 1 || K > INT32_MAX || nt > INT32_MAX || !d_x) return fail(ctx, MIOC_EINVAL, "bad K / nt / x");
  if (!state0 || (prog->np > 0 && !params)) return fail(ctx, MIOC_EINVAL, "state0 / params missing");
  if (!(T1 > T0)) return fail(ctx, MIOC_EINVAL, "need T1 > T0");
  if (prog->nd > 0 && !d_data) return fail(ctx, MIOC_EINVAL, "the program reads sampled data: d_data missing");
  if (d_Y && !(prog->flags & MIOC_ODE_STATES))
    return fail(ctx, MIOC_EINVAL, "the program was not created with MIOC_ODE_STATES");
  if (nu < 0 || nu >= prog->nx) return fail(ctx, MIOC_EINVAL, "need 1 <= nu < the program's nx");
  if (ctx->have_levels && ctx->M != prog->nx - nu)
    return fail(ctx, MIOC_EINVAL, nu ? "the program's nx differs from nu + the levels' number of controls"
                                     : "the program's nx differs from the levels' number of controls");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, MIOC_EHIP, "hipSetDevice failed");
  hipFunction_t fn = nullptr;
  {
    std::lock_guard<std::mutex> lock(prog->mu);
    for (const auto &l : prog->loaded)
      if (l.device == ctx->device) fn = l.fn;
    if (!fn) {
      mioc_ode_program::Loaded l{ctx->device, nullptr, nullptr};
      hipError_t e = hipModuleLoadData(&l.mod, prog->code.data());
      if (e == hipSuccess) {
        e = hipModuleGetFunction(&l.fn, l.mod, kKernelName);
        if (e != hipSuccess) (void)hipModuleUnload(l.mod);
      }
      if (e != hipSuccess) return fail(ctx, MIOC_EHIP, std::string("loading the ODE program: ") + hipGetErrorString(e));
      prog->loaded.push_back(l);
      fn = l.fn;
    }
  }
  const bool euler = prog->integrator == MIOC_ODE_INT_EULER;
  if (euler) {  // forward states [nt][ny][K]
    const int rc = ctx->d_ode_state.grow(ctx, (size_t)K * (size_t)nt * (size_t)prog->ny * sizeof(double), "ODE states");
    if (rc) return rc;
  } else if (d_df) {  // the state of every substep (Heun / RK4: at its start, implicit: its stage state)
    // [nt * substeps][ny][K]; a value-only call stores nothing
    // K * nt < 2^62 and per <= 64 * 8 * 8: the product is taken only once it is known to stay below 2^46
    const uint64_t cells = (uint64_t)K * (uint64_t)nt, per = (uint64_t)(prog->substeps * prog->ny) * sizeof(double);
    if (cells > ((uint64_t)1 << 46) / per) return fail(ctx, MIOC_ENOMEM, "the ODE states of all substeps exceed 64 TiB");
    const int rc = ctx->d_ode_state.grow(ctx, (size_t)(cells * per), "ODE states");
    if (rc) return rc;
  }
  int Ki = (int)K, nti = (int)nt, ms = prog->substeps;
  double t0 = T0, tau = (T1 - T0) / (double)nt;  // ODEObjective.jl: tau = (T1 - T0) / nt
  double h = tau / (double)ms;                   // the substep of every scheme but Euler
  double par[kMaxNY + kMaxNP] = {};              // the skeleton's Par: y0[NY], then p[max(NP, 1)]
  for (int r = 0; r < prog->ny; ++r) par[r] = state0[r];
  for (int q = 0; q < prog->np; ++q) par[prog->ny + q] = params[q];
  const double *X = d_x;
  double *ST = ctx->d_ode_state.get();
  const int32_t *gate = ctx->gate;
  // the data pointer and the state output follow the gate, each only in a kernel compiled with it
  void *args_euler[12] = {&Ki, &nti, &t0, &tau, par, &X, &d_J, &d_df, &ST, &gate};
  void *args_rk[14] = {&Ki, &nti, &ms, &t0, &tau, &h, par, &X, &d_J, &d_df, &ST, &gate};
  void **args = euler ? args_euler : args_rk;
  int na = euler ? 10 : 12;
  if (prog->nd > 0) args[na++] = &d_data;
  if (prog->flags & MIOC_ODE_STATES) args[na++] = &d_Y;
  const hipError_t e = hipModuleLaunchKernel(fn, (unsigned)((K + 63) / 64), 1, 1, 64, 1, 1, 0, ctx->stream, args, nullptr);
  if (e != hipSuccess) return fail(ctx, MIOC_EHIP, std::string("launching the ODE program: ") + hipGetErrorString(e));
  return MIOC_OK;
}

int32_t mioc_ode_program_eval_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t K, const double *d_x, int64_t nt,
                                     double T0, double T1, const double *state0, const double *params, double *d_J,
                                     double *d_df) {
  if (ctx && prog && prog->nd > 0)
    return fail(ctx, MIOC_EINVAL, "the program reads sampled data: use mioc_ode_program_eval_bolza_device");
  return program_eval(ctx, prog, 0, K, d_x, nt, T0, T1, state0, params, nullptr, d_J, d_df, nullptr);
}

int32_t mioc_ode_program_eval_mixed_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t nu, int64_t K,
                                           const double *d_x, int64_t nt, double T0, double T1, const double *state0,
                                           const double *params, double *d_J, double *d_df) {
  if (ctx && nu < 1) return fail(ctx, MIOC_EINVAL, "need 1 <= nu < the program's nx");
  if (ctx && prog && prog->nd > 0)
    return fail(ctx, MIOC_EINVAL, "the program reads sampled data: use mioc_ode_program_eval_bolza_device");
  return program_eval(ctx, prog, nu, K, d_x, nt, T0, T1, state0, params, nullptr, d_J, d_df, nullptr);
}

int32_t mioc_ode_program_eval_bolza_device(mioc_ctx *ctx, mioc_ode_program *prog, int64_t nu, int64_t K,
                                           const double *d_x, int64_t nt, double T0, double T1, const double *state0,
                                           const double *params, const double *d_data, double *d_J, double *d_df,
                                           double *d_Y) {
  return program_eval(ctx, prog, nu, K, d_x, nt, T0, T1, state0, params, d_data, d_J, d_df, d_Y);
}

}  // extern "C"
