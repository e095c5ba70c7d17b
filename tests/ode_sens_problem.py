"""The problem of the tests of the sensitivities of user-defined ODE objectives (test_ode_sens.py, test_gpu_ode_sens.py;
include/mioc.h, "Sensitivities"): polynomial arithmetic only, so that the host mirror (tests/ode_sens_mirror.py)
restates every hook in Python floats bit for bit.  ny = 3 states, nx = 2 controls on the product grid [[0,1,2],[0,1]],
NP = 3 parameters p = [a, b, c] (three distinct values) and ND = 1 data column d0 = p[NP]:

  F  = [ -a y0 + y1 + (d0 t) x0,   -y0 - b y1 + x1 y2 + a c,   -c y2 + (x0 / 2) y0 + y1^2 / 10 ]
  G  = (y0 - d0)^2 / 2 + (b / 2) y1^2 + x0^2 / 20 + (x1 / 10) y0
  E  = (c / 2) (y2 - 1)^2 + y1^2 / 2 + (t / 100) y0

Every parameter appears in F (a and c also as a product), b in G and c in E.  fp[0][1], fp[0][2], fp[2][0], fp[2][1],
gp[0], gp[2], ep[0], ep[1] (and fy[0][2], gy[2], three entries of fu) are structural zeros that the hand-written hooks
never write.  The text has F, G and E as templates over the state type and the parameter type and every derivative hook
by hand under its ``#ifndef MIOC_DERIVE_*`` guard, so one text serves every derive mask, with and without
sensitivities.  Fd, Gd, Ed (the derivatives in the data entry d0) exist only in the Python hooks: the mirror's wrong
version "data entry differentiated" needs them.
"""
import types

NY, NX, NP, ND = 3, 2, 3, 1
V = [[0, 1, 2], [0, 1]]
PARAMS = [0.5, 0.8, 0.3]
STATE0 = [0.2, -0.1, 0.3]


def make_data(nt):
    """(nt, ND) samples of order one, different in every row: d0 a tracking target."""
    return [[0.5 + 0.25 * ((7 * i) % 5) / 4.0] for i in range(nt)]


_SIG = "(const double *p, int i, double t, const double *y, const double *x"
_TSIG = "(const P *p, int i, double t, const T *y, const T *x"
SOURCE = """
template <class T, class P> __device__ void F@TSIG@, T *f) {
  f[0] = (-p[0] * y[0] + y[1]) + (p[NP] * t) * x[0];
  f[1] = ((-y[0] - p[1] * y[1]) + x[1] * y[2]) + p[0] * p[2];
  f[2] = (-p[2] * y[2] + (0.5 * x[0]) * y[0]) + 0.1 * (y[1] * y[1]);
}
template <class T, class P> __device__ T G@TSIG@) {
  const T a = y[0] - p[NP];
  return ((0.5 * (a * a) + (0.5 * p[1]) * (y[1] * y[1])) + 0.05 * (x[0] * x[0])) + (0.1 * x[1]) * y[0];
}
template <class T, class P> __device__ T E(const P *p, double t, const T *y) {
  const T e = y[2] - 1.0;
  return ((0.5 * p[2]) * (e * e) + 0.5 * (y[1] * y[1])) + (0.01 * t) * y[0];
}
#ifndef MIOC_DERIVE_FY
__device__ void Fy@SIG@, double (*fy)[NY]) {  // fy[0][2] is a structural zero: never written
  fy[0][0] = -p[0];
  fy[0][1] = 1.0;
  fy[1][0] = -1.0;
  fy[1][1] = -p[1];
  fy[1][2] = x[1];
  fy[2][0] = 0.5 * x[0];
  fy[2][1] = 0.2 * y[1];
  fy[2][2] = -p[2];
}
#endif
#ifndef MIOC_DERIVE_FU
__device__ void Fu@SIG@, double (*fu)[NX]) {  // fu[0][1], fu[1][0], fu[2][1] are structural zeros: never written
  fu[0][0] = p[NP] * t;
  fu[1][1] = y[2];
  fu[2][0] = 0.5 * y[0];
}
#endif
#ifndef MIOC_DERIVE_GY
__device__ void Gy@SIG@, double *gy) {  // gy[2] is a structural zero: never written
  gy[0] = (y[0] - p[NP]) + 0.1 * x[1];
  gy[1] = p[1] * y[1];
}
#endif
#ifndef MIOC_DERIVE_GU
__device__ void Gu@SIG@, double *gu) {
  gu[0] = 0.1 * x[0];
  gu[1] = 0.1 * y[0];
}
#endif
#ifndef MIOC_DERIVE_EY
__device__ void Ey(const double *p, double t, const double *y, double *ey) {
  ey[0] = 0.01 * t;
  ey[1] = y[1];
  ey[2] = p[2] * (y[2] - 1.0);
}
#endif
#if defined(MIOC_SENS) && (MIOC_SENS & 1)
#ifndef MIOC_DERIVE_FP
__device__ void Fp@SIG@, double (*fp)[NP]) {  // fp[0][1], fp[0][2], fp[2][0], fp[2][1]: never written
  fp[0][0] = -y[0];
  fp[1][0] = p[2];
  fp[1][1] = -y[1];
  fp[1][2] = p[0];
  fp[2][2] = -y[2];
}
#endif
#ifndef MIOC_DERIVE_GP
__device__ void Gp@SIG@, double *gp) {  // gp[0], gp[2]: never written
  gp[1] = @GPSIGN@0.5 * (y[1] * y[1]);
}
#endif
#ifndef MIOC_DERIVE_EP
__device__ void Ep(const double *p, double t, const double *y, double *ep) {  // ep[0], ep[1]: never written
  const double e = y[2] - 1.0;
  ep[2] = 0.5 * (e * e);
}
#endif
#endif
""".replace("@SIG@", _SIG).replace("@TSIG@", _TSIG)
# the copy for check_hooks: the hand-written Gp with the wrong sign
SOURCE_WRONG_GP = SOURCE.replace("@GPSIGN@", "-")
SOURCE = SOURCE.replace("@GPSIGN@", "")
assert SOURCE != SOURCE_WRONG_GP


def _hooks():
    """The hooks above in Python floats, the same expressions with the same parentheses (tests/ode_sens_mirror.py)."""
    def F(p, i, t, y, x, f):
        f[0] = (-p[0] * y[0] + y[1]) + (p[NP] * t) * x[0]
        f[1] = ((-y[0] - p[1] * y[1]) + x[1] * y[2]) + p[0] * p[2]
        f[2] = (-p[2] * y[2] + (0.5 * x[0]) * y[0]) + 0.1 * (y[1] * y[1])

    def G(p, i, t, y, x):
        a = y[0] - p[NP]
        return ((0.5 * (a * a) + (0.5 * p[1]) * (y[1] * y[1])) + 0.05 * (x[0] * x[0])) + (0.1 * x[1]) * y[0]

    def E(p, t, y):
        e = y[2] - 1.0
        return ((0.5 * p[2]) * (e * e) + 0.5 * (y[1] * y[1])) + (0.01 * t) * y[0]

    def Fy(p, i, t, y, x, fy):
        fy[0][0] = -p[0]
        fy[0][1] = 1.0
        fy[1][0] = -1.0
        fy[1][1] = -p[1]
        fy[1][2] = x[1]
        fy[2][0] = 0.5 * x[0]
        fy[2][1] = 0.2 * y[1]
        fy[2][2] = -p[2]

    def Fu(p, i, t, y, x, fu):
        fu[0][0] = p[NP] * t
        fu[1][1] = y[2]
        fu[2][0] = 0.5 * y[0]

    def Gy(p, i, t, y, x, gy):
        gy[0] = (y[0] - p[NP]) + 0.1 * x[1]
        gy[1] = p[1] * y[1]

    def Gu(p, i, t, y, x, gu):
        gu[0] = 0.1 * x[0]
        gu[1] = 0.1 * y[0]

    def Ey(p, t, y, ey):
        ey[0] = 0.01 * t
        ey[1] = y[1]
        ey[2] = p[2] * (y[2] - 1.0)

    def Fp(p, i, t, y, x, fp):
        fp[0][0] = -y[0]
        fp[1][0] = p[2]
        fp[1][1] = -y[1]
        fp[1][2] = p[0]
        fp[2][2] = -y[2]

    def Gp(p, i, t, y, x, gp):
        gp[1] = 0.5 * (y[1] * y[1])

    def Ep(p, t, y, ep):
        e = y[2] - 1.0
        ep[2] = 0.5 * (e * e)

    # the derivatives in the data entry d0 = p[NP], which the product never forms
    def Fd(p, i, t, y, x, fd):
        fd[0] = t * x[0]

    def Gd(p, i, t, y, x):
        return -(y[0] - p[NP])

    return types.SimpleNamespace(F=F, G=G, E=E, Fy=Fy, Fu=Fu, Gy=Gy, Gu=Gu, Ey=Ey, Fp=Fp, Gp=Gp, Ep=Ep, Fd=Fd, Gd=Gd)


HOOKS = _hooks()

# ---- the known answer (ny = nx = 1, NP = 2, no data): F = p0 x, G = p1 y, E = 2 y; derived by hand ---------------------
# tau = 1/4, x = (1, 0, 2, 1), p = (2, 4), y0 = 1/2: y_i = y0 + tau p0 X_i with X = (0, 1, 1, 3, 4) = (.5, 1, 1, 2, 2.5).
# Heun and the midpoint rule integrate the piecewise linear p1 y exactly (the trapezoid sum):
#   J = tau p1 (4 y0 + tau p0 7) + 2 (y0 + tau p0 4) = 5.5 + 5,   7 = sum_i (X_i + X_{i+1}) / 2
#   dJ/dy0 = 4 tau p1 + 2 = 6,   dJ/dp0 = 7 tau^2 p1 + 8 tau = 3.75,   dJ/dp1 = tau (4 y0 + 7 tau p0) = 1.375
# backward Euler takes p1 y at the end of each step (9 = sum_i X_{i+1} in place of 7):
#   J = 6.5 + 5,   dJ/dy0 = 6,   dJ/dp0 = 9 tau^2 p1 + 8 tau = 4.25,   dJ/dp1 = tau (4 y0 + 9 tau p0) = 1.625
# df[i] = dJ/dx_i / tau = p0 (2 + tau p1 (n_i + c)) with n_i = 3 - i later steps and c = 1/2 (trapezoid) or 1.
# Every value is a small dyadic number: exact in doubles for Heun, backward Euler and the midpoint rule with any substeps;
# RK4's b weights do not sum to 1 in doubles.
KNOWN_SOURCE = """
__device__ void F@SIG@, double *f) { f[0] = p[0] * x[0]; }
__device__ void Fy@SIG@, double (*fy)[NY]) {}
__device__ void Fu@SIG@, double (*fu)[NX]) { fu[0][0] = p[0]; }
__device__ double G@SIG@) { return p[1] * y[0]; }
__device__ void Gy@SIG@, double *gy) { gy[0] = p[1]; }
__device__ void Gu@SIG@, double *gu) {}
__device__ double E(const double *p, double t, const double *y) { return 2.0 * y[0]; }
__device__ void Ey(const double *p, double t, const double *y, double *ey) { ey[0] = 2.0; }
__device__ void Fp@SIG@, double (*fp)[NP]) { fp[0][0] = x[0]; }
__device__ void Gp@SIG@, double *gp) { gp[1] = y[0]; }
__device__ void Ep(const double *p, double t, const double *y, double *ep) {}
""".replace("@SIG@", _SIG)
KNOWN = dict(T0=0.0, T1=1.0, nt=4, state0=[0.5], params=[2.0, 4.0], x=[[1.0], [0.0], [2.0], [1.0]],
             trapezoid=dict(J=10.5, Jp=[3.75, 1.375], Jy0=[6.0], df=[11.0, 9.0, 7.0, 5.0]),
             beuler=dict(J=11.5, Jp=[4.25, 1.625], Jy0=[6.0], df=[12.0, 10.0, 8.0, 6.0]))


def known(integrator):
    return KNOWN["beuler" if integrator == "beuler" else "trapezoid"]


def _known_hooks():
    def F(p, i, t, y, x, f):
        f[0] = p[0] * x[0]

    def Fu(p, i, t, y, x, fu):
        fu[0][0] = p[0]

    def Gy(p, i, t, y, x, gy):
        gy[0] = p[1]

    def Ey(p, t, y, ey):
        ey[0] = 2.0

    def Fp(p, i, t, y, x, fp):
        fp[0][0] = x[0]

    def Gp(p, i, t, y, x, gp):
        gp[1] = y[0]

    def none(*a):
        pass
    return types.SimpleNamespace(F=F, G=lambda p, i, t, y, x: p[1] * y[0], E=lambda p, t, y: 2.0 * y[0], Fy=none, Fu=Fu,
                                 Gy=Gy, Gu=none, Ey=Ey, Fp=Fp, Gp=Gp, Ep=none)


KNOWN_HOOKS = _known_hooks()


# ---- the largest square shape: ny = nx = nparams = 8, every hook derived ------------------------------------------------
def synthetic_source(n, np_):
    """Two-type templated F, G, E of a dense problem with ny = nx = n in which every parameter appears."""
    sig = "(const P *p, int i, double t, const T *y, const T *x"
    return f"""
template <class T, class P> __device__ void F{sig}, T *f) {{
  for (int r = 0; r < {n}; ++r) {{
    T a = -p[r % {np_}] * y[r] + (t * p[{np_ - 1}]) * x[r];
    for (int c = 0; c < {n}; ++c) a = a + (0.01 * (r + 1)) * (y[c] * x[(r + c) % {n}]);
    f[r] = a;
  }}
}}
template <class T, class P> __device__ T G{sig}) {{
  T g = 0.0 * y[0];
  for (int r = 0; r < {n}; ++r) g = g + ((0.5 * p[r % {np_}]) * (y[r] * y[r]) + 0.1 * (x[r] * y[r]));
  return g;
}}
template <class T, class P> __device__ T E(const P *p, double t, const T *y) {{
  T e = 0.0 * y[0];
  for (int r = 0; r < {n}; ++r) e = e + (p[0] * t) * (y[r] * y[r]);
  return e;
}}
"""
