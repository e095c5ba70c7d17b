// mioc_ode_skeleton.h -- the kernel text of the runtime-compiled ODE programs (mioc_ode_rtc.cpp assembles it and hands
// it to hiprtc; the order of the assembled text is in include/mioc.h).  NY, NX, NP (and NS or TH, ND, MIOC_TERMINAL,
// MIOC_STATES) are #defined in front of the caller's hooks; the skeleton follows them: kSkeletonHead, then one body.
//
// The kernel: eval_f_helper / eval_df_helper of ODEObjective.jl:125-184, one lane per restart in 64-lane blocks like
// k_ode_eval (mioc_ode.hip), NY / NX / NP compile-time so that y, λ, fy, fu, gy, gu live in registers.  The forward
// states go to a scratch laid out [step][r][k]: the 64 lanes of a wave store and load 64 contiguous doubles.  Rounding
// order (no contraction, no fast-math): see the bodies; kBodyEuler's is k_ode_eval's for NY = 2, NX = 3, Gu = 0.
//
// A terminal cost, ND columns of sampled data, the state output and scenarios are compiled in only when the head
// #defines MIOC_TERMINAL, ND, MIOC_STATES, MIOC_SCEN (and MIOC_SCEN_DATA): without them every macro and helper below
// preprocesses to the tokens of a program that never had them, and the kernel has neither the data nor the state
// pointer and takes state0 and the parameters by value.  The same holds for the sensitivities (MIOC_SENS, kBodyRK and
// kBodyTheta only): MIOC_BACKWARD is DF and every other MIOC_SENS_* / MIOC_DF_* macro is empty without it.
#pragma once

namespace mioc_kernel_text {

// What every integrator shares, written once.  The shared blocks are macros, not forced-inline helpers: a macro
// preprocesses to the tokens the block had when every body wrote it out, so every program compiles to the code it
// compiled to then; as helpers, the J write, the transposed products and the zeroing each changed the compiler's
// schedule of some program.  The blocks use the kernel's own names (J, k, p, y, gy, fy, fu, gu, yo, ...).
const char *const kSkeletonHead = R"SKEL(
#ifndef ND
#define ND 0
#endif
// Scenarios (MIOC_SCEN): the lane of restart q solves scenario sc = q % S, with its own state0 and parameters, read from
// Y0S[r][sc] and PS[e][sc] (the scenario fastest, like ST: 64 lanes load 64 contiguous doubles when S >= 64) in place
// of the by-value Par.  p is then always the per-lane copy pe.  With MIOC_SCEN_DATA the data rows are DATA[c][e][sc]
// and each lane loads its own; without it DATA stays the shared [c][e] table and its loads stay scalar.
#ifdef MIOC_SCEN
#define MIOC_PAR_ARG int S, const double *__restrict__ Y0S, const double *__restrict__ PS
#define MIOC_LANE_SCEN const size_t sc = ku % (unsigned)S;
#define MIOC_Y0(r) Y0S[(size_t)(r) * S + sc]
#define MIOC_LANE_PARAMS                                                                    \
  double pe[NP + ND > 0 ? NP + ND : 1];                                                     \
  _Pragma("unroll") for (int e = 0; e < NP; ++e) pe[e] = PS[(size_t)e * S + sc];            \
  const double *p = pe;
#else
#define MIOC_PAR_ARG mioc_skeleton::Par P
#define MIOC_LANE_SCEN
#define MIOC_Y0(r) P.y0[r]
#endif
#if ND > 0  // sampled data: p is a per-lane copy of the parameters with the data row of the current column behind them
#define MIOC_DATA_ARG , const double *__restrict__ DATA
#ifdef MIOC_SCEN_DATA
#define MIOC_DATA_ROW(c)                                                  \
  {                                                                       \
    const double *row = DATA + (size_t)(c) * ND * S + sc;                 \
    _Pragma("unroll") for (int e = 0; e < ND; ++e) pe[NP + e] = row[(size_t)e * S]; \
  }
#else
#define MIOC_DATA_ROW(c)                                \
  {                                                     \
    const double *row = DATA + (size_t)(c) * ND;        \
    _Pragma("unroll") for (int e = 0; e < ND; ++e) pe[NP + e] = row[e]; \
  }
#endif
#ifndef MIOC_SCEN
#define MIOC_LANE_PARAMS                                            \
  double pe[NP + ND];                                               \
  _Pragma("unroll") for (int e = 0; e < NP; ++e) pe[e] = P.p[e];    \
  const double *p = pe;
#endif
#else
#define MIOC_DATA_ARG
#define MIOC_DATA_ROW(c)
#ifndef MIOC_SCEN
#define MIOC_LANE_PARAMS const double *p = P.p;
#endif
#endif
#ifdef MIOC_STATES  // YO: the states at the control-grid points, [k][i][r], i = 0..nt
#define MIOC_STATES_ARG , double *YO
// yo, this lane's rows (null when the caller wants none), with row 0 = y; MIOC_YO_ROW stores y as row `row`
#define MIOC_YO_OPEN(y)                                              \
  double *yo = YO ? YO + k * ((size_t)nt + 1) * NY : nullptr;        \
  MIOC_YO_ROW(0, y)
#define MIOC_YO_ROW(row, y)                                                          \
  if (yo) {                                                                          \
    _Pragma("unroll") for (int r = 0; r < NY; ++r) yo[(size_t)(row) * NY + r] = y[r]; \
  }
#else
#define MIOC_STATES_ARG
#define MIOC_YO_OPEN(y)
#define MIOC_YO_ROW(row, y)
#endif
// Sensitivities (MIOC_SENS, bit 1: dJ/dparams into JP[k][e], bit 2: dJ/dstate0 into JY0[k][r]; include/mioc.h,
// "Sensitivities").  The backward sweep then runs when any of DF, JP, JY0 is given, and df is stored only with DF.
// pbar is the accumulator beside xbar that is never reset: MIOC_SENS_STAGE adds Fp(Y)' v + wgt Gp(Y) at one stage
// (v: kbar_s or mu, wgt: (b_s h) or h), every sum left to right.  MIOC_SENS_OUT stores pbar and w after substep 0.
#ifdef MIOC_SENS
#define MIOC_SENS_ARG , double *JP, double *JY0
#define MIOC_BACKWARD (DF || JP || JY0)
#define MIOC_DF_OPEN if (DF) {
#define MIOC_DF_CLOSE }
#define MIOC_SENS_NAN(nan)                                                                \
  if (JP)                                                                                 \
    for (int e = 0; e < NP; ++e) JP[k * NP + e] = nan;                                    \
  if (JY0)                                                                                \
    for (int r = 0; r < NY; ++r) JY0[k * NY + r] = nan;
#if MIOC_SENS & 1
#ifdef MIOC_TERMINAL  // pbar starts from Ep at the last state y, zeroed first like ey (the data row is nt - 1's)
#define MIOC_SENS_EP(tend)                                       \
  if (JP) {                                                      \
    double ep[NP];                                               \
    _Pragma("unroll") for (int e = 0; e < NP; ++e) ep[e] = 0.0;  \
    Ep(p, tend, y, ep);                                          \
    _Pragma("unroll") for (int e = 0; e < NP; ++e) pbar[e] = ep[e]; \
  }
#else
#define MIOC_SENS_EP(tend)
#endif
#define MIOC_SENS_OPEN(tend)                                       \
  double fp[NY][NP], gp[NP], pbar[NP];                             \
  _Pragma("unroll") for (int e = 0; e < NP; ++e) {                 \
    gp[e] = 0.0;                                                   \
    pbar[e] = 0.0;                                                 \
    _Pragma("unroll") for (int r = 0; r < NY; ++r) fp[r][e] = 0.0; \
  }                                                                \
  MIOC_SENS_EP(tend)
#define MIOC_SENS_STAGE(t, Y, v, wgt)                                            \
  if (JP) {                                                                      \
    Fp(p, i, t, Y, xc, fp);                                                      \
    Gp(p, i, t, Y, xc, gp);                                                      \
    _Pragma("unroll") for (int e = 0; e < NP; ++e) {                             \
      MIOC_TDOT(acc_e, fp, e, v)                                                 \
      pbar[e] = pbar[e] + (acc_e + (wgt) * gp[e]);                               \
    }                                                                            \
  }
#define MIOC_SENS_OUT_P                                                          \
  if (JP) {                                                                      \
    _Pragma("unroll") for (int e = 0; e < NP; ++e) JP[k * NP + e] = pbar[e];     \
  }
#else
#define MIOC_SENS_OPEN(tend)
#define MIOC_SENS_STAGE(t, Y, v, wgt)
#define MIOC_SENS_OUT_P
#endif
#define MIOC_SENS_OUT                                                            \
  MIOC_SENS_OUT_P                                                                \
  if (JY0) {                                                                     \
    _Pragma("unroll") for (int r = 0; r < NY; ++r) JY0[k * NY + r] = w[r];       \
  }
#else
#define MIOC_SENS_ARG
#define MIOC_BACKWARD DF
#define MIOC_DF_OPEN
#define MIOC_DF_CLOSE
#define MIOC_SENS_NAN(nan)
#define MIOC_SENS_OPEN(tend)
#define MIOC_SENS_STAGE(t, Y, v, wgt)
#define MIOC_SENS_OUT
#endif
// The lane prologue: the gate, the restart k of this lane (of KK), its parameters p and its control x.
#define MIOC_LANE_PROLOGUE                                                                                   \
  if (gate && *gate == 0) return; /* device TRM control: no restart is inside its inner loop */              \
  const unsigned ku = blockIdx.x * 64u + threadIdx.x;                                                        \
  if (ku >= (unsigned)K) return;                                                                             \
  const size_t k = ku, KK = (size_t)K;                                                                       \
  MIOC_LANE_SCEN                                                                                             \
  MIOC_LANE_PARAMS                                                                                           \
  const double *x = X + k * (size_t)nt * NX;
// The signature of every scheme with substeps (ms of them per control interval, of length h); Euler keeps its own.
#define MIOC_KERNEL_SUBSTEPS                                                                                    \
  extern "C" __global__ __launch_bounds__(64) void mioc_ode_program_kernel(                                     \
      int K, int nt, int ms, double T0, double tau, double h, MIOC_PAR_ARG, const double *X, double *J,         \
      double *DF, double *ST, const int *gate MIOC_DATA_ARG MIOC_STATES_ARG MIOC_SENS_ARG)

namespace mioc_skeleton {
struct Par {
  double y0[NY];
  double p[NP > 0 ? NP : 1];
};
}  // namespace mioc_skeleton

// The derivative outputs are zeroed once per evaluation (ODEObjective.jl:155-162), since a hook may leave a structural
// zero unwritten: gy, the scheme's own per-row vectors (`more`), fy and fu row by row, then gu.  The theta body zeroes
// fy with its forward sweep and writes its own loops: the order of these stores decides the compiler's schedule.
#define MIOC_ZERO_DERIVATIVES(more)                                \
  _Pragma("unroll") for (int r = 0; r < NY; ++r) {                  \
    gy[r] = 0.0;                                                    \
    more                                                            \
    _Pragma("unroll") for (int c = 0; c < NY; ++c) fy[r][c] = 0.0;  \
    _Pragma("unroll") for (int m = 0; m < NX; ++m) fu[r][m] = 0.0;  \
  }                                                                 \
  _Pragma("unroll") for (int m = 0; m < NX; ++m) gu[m] = 0.0;

// double acc = column m of a' v = sum_r a[r][m] v[r], accumulated left to right from r = 0
#define MIOC_TDOT(acc, a, m, v)  \
  double acc = a[0][m] * v[0];   \
  _Pragma("unroll") for (int r = 1; r < NY; ++r) acc = acc + a[r][m] * v[r];

// J of restart k: the running cost, and with MIOC_TERMINAL the Mayer term at the end time and the last state y (the
// data row is column nt - 1's)
#ifdef MIOC_TERMINAL
#define MIOC_WRITE_J(running, tend) if (J) J[k] = running + E(p, tend, y);
#else
#define MIOC_WRITE_J(running, tend) if (J) J[k] = running;
#endif

// double ey[NY] = Ey at the last state y, zeroed first like gy: the seed of the backward sweep (MIOC_TERMINAL only)
#define MIOC_EY_SEED(tend)                                      \
  double ey[NY];                                                \
  _Pragma("unroll") for (int r = 0; r < NY; ++r) ey[r] = 0.0;   \
  Ey(p, tend, y, ey);
)SKEL";

// Explicit Euler with the trapezoid cost, the reference's scheme.  Its kernel has no ms and h.
const char *const kBodyEuler = R"SKEL(
extern "C" __global__ __launch_bounds__(64) void mioc_ode_program_kernel(
    int K, int nt, double T0, double tau, MIOC_PAR_ARG, const double *X, double *J, double *DF, double *ST,
    const int *gate MIOC_DATA_ARG MIOC_STATES_ARG) {
  MIOC_LANE_PROLOGUE
  // ---- forward: explicit Euler, trapezoid cost (ODEObjective.jl:125-150) ----
  double y[NY], f[NY], xc[NX], xn[NX];
#pragma unroll
  for (int r = 0; r < NY; ++r) y[r] = MIOC_Y0(r);
#pragma unroll
  for (int m = 0; m < NX; ++m) xc[m] = x[m];
  MIOC_DATA_ROW(0)  // the data row is that of the control column: xc's for F, xn's for G, column nt - 1 at the end
  MIOC_YO_OPEN(y)
  double fval = 0.5 * G(p, 0, T0 + 0.0 * tau, y, xc);
  for (int i = 0; i < nt; ++i) {
    F(p, i, T0 + (double)i * tau, y, xc, f);
#pragma unroll
    for (int r = 0; r < NY; ++r) y[r] = y[r] + tau * f[r];
    if (DF) {
#pragma unroll
      for (int r = 0; r < NY; ++r) ST[((size_t)i * NY + r) * KK + k] = y[r];
    }
    MIOC_YO_ROW((size_t)i + 1, y)
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
  MIOC_WRITE_J(fval * tau, T0 + (double)nt * tau)
  if (!DF) return;
  // ---- backward: adjoint and df = Gu - Fu' lambda (ODEObjective.jl:153-184) ----
  // here y is the state after the last step and xc the last control column
  double *df = DF + k * (size_t)nt * NX;
  double gy[NY], gu[NX], fy[NY][NY], fu[NY][NX], lam[NY], a[NY], s[NY];
  MIOC_ZERO_DERIVATIVES()
  Gy(p, nt, T0 + (double)nt * tau, y, xc, gy);
#ifdef MIOC_TERMINAL
  MIOC_EY_SEED(T0 + (double)nt * tau)
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
      for (int r = 0; r < NY; ++r) s[r] = MIOC_Y0(r);
    } else {
#pragma unroll
      for (int r = 0; r < NY; ++r) s[r] = ST[((size_t)(i - 1) * NY + r) * KK + k];
    }
    Fu(p, i, t, s, xc, fu);
    Gu(p, i, t, s, xc, gu);
#pragma unroll
    for (int m = 0; m < NX; ++m) {
      MIOC_TDOT(acc, fu, m, lam)
      df[(size_t)i * NX + m] = (0.0 - acc) + gu[m];
    }
    if (i == 0) break;
    // lambda_{i-1} = lambda_i + tau (Fy' lambda_i - Gy), Fy and Gy at (state_{i-1}, x_i)
    Gy(p, i, t, s, xc, gy);
    Fy(p, i, t, s, xc, fy);
#pragma unroll
    for (int c = 0; c < NY; ++c) {
      MIOC_TDOT(acc, fy, c, lam)
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

// Heun / classical RK4 (mioc_ode_program_create_ex; the scheme and its rounding order are written out in
// include/mioc.h).  NS, the stage count, is #defined in front with NY / NX / NP; the tableau follows from it.  Every
// stage loop is fully unrolled, so ch / ha / hb and the stage arrays are indexed by constants and stay in registers.
// ST holds y_n for every substep n = 0 .. nt*ms - 1, [n][r][k].
const char *const kBodyRK = R"SKEL(
MIOC_KERNEL_SUBSTEPS {
  MIOC_LANE_PROLOGUE
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
  for (int r = 0; r < NY; ++r) y[r] = MIOC_Y0(r);
  MIOC_YO_OPEN(y)
  double q = 0.0;
  for (int i = 0; i < nt; ++i) {
#pragma unroll
    for (int m = 0; m < NX; ++m) xc[m] = x[(size_t)i * NX + m];
    MIOC_DATA_ROW(i)  // the data row of the control interval, for every stage and substep
    for (int j = 0; j < ms; ++j) {
      const long long n = (long long)i * ms + j;
      const double tn = T0 + (double)n * h;
      if (MIOC_BACKWARD) {
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
    MIOC_YO_ROW((size_t)i + 1, y)
  }
#ifdef MIOC_TERMINAL
  const double tend = T0 + (double)((long long)nt * ms) * h;
#endif
  MIOC_WRITE_J(q, tend)
  if (!MIOC_BACKWARD) return;
  // ---- backward: the scheme's discrete adjoint; df[:, i] = xbar_i / tau ----
  double *df = DF + k * (size_t)nt * NX;
  double gy[NY], gu[NX], fy[NY][NY], fu[NY][NX], w[NY], YS[NS][NY], kb[NY], Yb[NY], acc[NY], xbar[NX];
  MIOC_ZERO_DERIVATIVES(w[r] = 0.0; Yb[r] = 0.0;)
#ifdef MIOC_TERMINAL  // the sweep starts from w = Ey at the last state (y still holds it; the data row is nt - 1's)
  MIOC_EY_SEED(tend)
#pragma unroll
  for (int r = 0; r < NY; ++r) w[r] = ey[r];
#endif
  MIOC_SENS_OPEN(tend)
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
        MIOC_SENS_STAGE(tn + ch[s], YS[s], kb, hb[s])
#pragma unroll
        for (int c = 0; c < NY; ++c) {
          MIOC_TDOT(t, fy, c, kb)
          Yb[c] = t + hb[s] * gy[c];
        }
#pragma unroll
        for (int m = 0; m < NX; ++m) {
          MIOC_TDOT(t, fu, m, kb)
          xbar[m] = xbar[m] + (t + hb[s] * gu[m]);
        }
#pragma unroll
        for (int c = 0; c < NY; ++c) acc[c] = s == NS - 1 ? Yb[c] : acc[c] + Yb[c];
      }
#pragma unroll
      for (int c = 0; c < NY; ++c) w[c] = w[c] + acc[c];
    }
    MIOC_DF_OPEN
#pragma unroll
    for (int m = 0; m < NX; ++m) df[(size_t)i * NX + m] = xbar[m] / tau;
    MIOC_DF_CLOSE
  }
  MIOC_SENS_OUT
}
)SKEL";

// Backward Euler / implicit midpoint (one stage, Y = y_n + (theta h) k, k = F(Y); the scheme, its Newton rule and the
// rounding order are written out in include/mioc.h).  TH, theta as a double literal, is #defined in front with
// NY / NX / NP.  The stage equation is solved by Newton's method with a dense Gaussian elimination in registers: every
// loop over NY is fully unrolled and the pivoting is conditional row swaps, so no array is indexed by a run-time value.
// ST holds the stage state Y of every substep, [n][r][k]: the backward sweep solves one transposed system per substep
// and calls neither F nor Newton.
const char *const kBodyTheta = R"SKEL(
#define MIOC_ODE_NEWTON_MAX 12
#define MIOC_ODE_NEWTON_TOL 1e-10
namespace mioc_skeleton {
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

MIOC_KERNEL_SUBSTEPS {
  MIOC_LANE_PROLOGUE
  const double th = TH * h, thh = th * h;  // theta h and (theta h) h, each rounded once
  // ---- forward: Newton on k = F(y_n + th k) from k = F(y_n); y_{n+1} = y_n + h k, q_{n+1} = q_n + h G(Y) ----
  double y[NY], Y[NY], kv[NY], f[NY], d[NY], xc[NX], fy[NY][NY], A[NY][NY];
#pragma unroll
  for (int r = 0; r < NY; ++r) {
    y[r] = MIOC_Y0(r);
#pragma unroll
    for (int c = 0; c < NY; ++c) fy[r][c] = 0.0;  // zeroed once per evaluation, as in the other bodies
  }
  MIOC_YO_OPEN(y)
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
      if (MIOC_BACKWARD) {
#pragma unroll
        for (int r = 0; r < NY; ++r) ST[((size_t)n * NY + r) * KK + k] = Y[r];
      }
      q = q + h * G(p, i, ts, Y, xc);
#pragma unroll
      for (int r = 0; r < NY; ++r) y[r] = y[r] + h * kv[r];
    }
    MIOC_YO_ROW((size_t)i + 1, y)
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
    MIOC_SENS_NAN(nan)
    return;
  }
#ifdef MIOC_TERMINAL
  const double tend = T0 + (double)((long long)nt * ms) * h;
#endif
  MIOC_WRITE_J(q, tend)
  if (!MIOC_BACKWARD) return;
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
  MIOC_EY_SEED(tend)
#pragma unroll
  for (int r = 0; r < NY; ++r) w[r] = ey[r];
#endif
  MIOC_SENS_OPEN(tend)
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
      MIOC_SENS_STAGE(ts, Y, mu, h)
#pragma unroll
      for (int m = 0; m < NX; ++m) {
        MIOC_TDOT(t, fu, m, mu)
        xbar[m] = xbar[m] + (t + h * gu[m]);
      }
#pragma unroll
      for (int c = 0; c < NY; ++c) {
        MIOC_TDOT(t, fy, c, mu)
        w[c] = w[c] + (t + h * gy[c]);
      }
    }
    MIOC_DF_OPEN
#pragma unroll
    for (int m = 0; m < NX; ++m) df[(size_t)i * NX + m] = xbar[m] / tau;
    MIOC_DF_CLOSE
  }
  MIOC_SENS_OUT
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
// The parameter derivatives of a program with sensitivities: F, G or E (templates over the state type and the parameter
// type there) once with both = mioc_ad::Dual<NP>, the unit tangents on p[0..NP-1]; the data entries behind them, y and x
// are constants.
#if defined(MIOC_DERIVE_FP) || defined(MIOC_DERIVE_GP) || defined(MIOC_DERIVE_EP)
#ifdef ND  // the head defines ND only when it is positive
#define MIOC_AD_NPD (NP + ND)
#else
#define MIOC_AD_NPD NP
#endif
#define MIOC_AD_SEED_P(pd)                                    \
  mioc_ad::Dual<NP> pd[MIOC_AD_NPD];                          \
  _Pragma("unroll") for (int e = 0; e < MIOC_AD_NPD; ++e) {   \
    pd[e] = p[e];                                             \
    if (e < NP) pd[e].d[e] = 1.0;                             \
  }
#endif
#ifdef MIOC_DERIVE_FP
MIOC_AD_HOOK void Fp(const double *p, int i, double t, const double *y, const double *x, double (*fp)[NP]) {
  mioc_ad::Dual<NP> yd[NY], xd[NX], fd[NY];
  MIOC_AD_SEED_P(pd)
#pragma unroll
  for (int r = 0; r < NY; ++r) yd[r] = y[r];
#pragma unroll
  for (int m = 0; m < NX; ++m) xd[m] = x[m];
  F((const mioc_ad::Dual<NP> *)pd, i, t, (const mioc_ad::Dual<NP> *)yd, (const mioc_ad::Dual<NP> *)xd, fd);
#pragma unroll
  for (int r = 0; r < NY; ++r) {
#pragma unroll
    for (int e = 0; e < NP; ++e) fp[r][e] = fd[r].d[e];
  }
}
#endif
#ifdef MIOC_DERIVE_GP
MIOC_AD_HOOK void Gp(const double *p, int i, double t, const double *y, const double *x, double *gp) {
  mioc_ad::Dual<NP> yd[NY], xd[NX];
  MIOC_AD_SEED_P(pd)
#pragma unroll
  for (int r = 0; r < NY; ++r) yd[r] = y[r];
#pragma unroll
  for (int m = 0; m < NX; ++m) xd[m] = x[m];
  const mioc_ad::Dual<NP> g =
      G((const mioc_ad::Dual<NP> *)pd, i, t, (const mioc_ad::Dual<NP> *)yd, (const mioc_ad::Dual<NP> *)xd);
#pragma unroll
  for (int e = 0; e < NP; ++e) gp[e] = g.d[e];
}
#endif
#ifdef MIOC_DERIVE_EP
MIOC_AD_HOOK void Ep(const double *p, double t, const double *y, double *ep) {
  mioc_ad::Dual<NP> yd[NY];
  MIOC_AD_SEED_P(pd)
#pragma unroll
  for (int r = 0; r < NY; ++r) yd[r] = y[r];
  const mioc_ad::Dual<NP> v = E((const mioc_ad::Dual<NP> *)pd, t, (const mioc_ad::Dual<NP> *)yd);
#pragma unroll
  for (int e = 0; e < NP; ++e) ep[e] = v.d[e];
}
#endif
)SKEL";

}  // namespace mioc_kernel_text
