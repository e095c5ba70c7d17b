"""The problem of the tests of a terminal cost, sampled data and the state output (test_ode_bolza.py,
test_gpu_ode_bolza.py): polynomial arithmetic only, so that the host mirror (tests/ode_bolza_mirror.py) restates every
hook in Python floats bit for bit.  ny = 3 states, nx = 2 controls on the product grid [[0,1,2],[0,1]], NP = 3
parameters p = [a, b, c] and ND = 2 data columns d0 = p[NP], d1 = p[NP + 1]:

  F  = [ -a y0 + y1 + (d0 t) x0,   -y0 - b y1 + x1 y2 + d1,   -c y2 + (x0 / 2) y0 + y1^2 / 10 ]
  G  = (y0 - d0)^2 / 2 + y1^2 / 2 + x0^2 / 20 + (x1 / 10) y0 + d1 y2
  E  = (d0 / 2) (y2 - 1)^2 + y1^2 / 2 + (t / 100) y0

fy[0][2], fu[0][1], fu[1][0] and fu[2][1] are structural zeros that the hand-written hooks never write.  The text has
F, G and E as templates over the scalar type and Fy, Fu, Gy, Gu, Ey by hand under their ``#ifndef MIOC_DERIVE_*``
guards, so one text serves every derive mask.  SOURCE_XFREE is the variant whose G does not depend on x (the terms
x0^2 / 20 and (x1 / 10) y0 dropped, Gu writes nothing): the reference's Euler gradient is the derivative of its
trapezoid J only then.  The same text serves the mixed variant (nu = 1: x0 continuous in [0, 2], x1 on [0, 1]).
"""
import types

from mioc.iterators import product_iterator
from mioc.ode import AbstractODEObjective

NY, NX, NP, ND = 3, 2, 3, 2
V = [[0, 1, 2], [0, 1]]
PARAMS = [0.5, 0.8, 0.3]
STATE0 = [0.2, -0.1, 0.3]


def make_data(nt):
    """(nt, ND) samples of order one, different in every row: d0 a tracking target, d1 an inflow."""
    return [[0.5 + 0.25 * ((7 * i) % 5) / 4.0, 0.1 * (((3 * i) % 7) - 3) / 3.0] for i in range(nt)]


_SIG = "(const double *p, int i, double t, const double *y, const double *x"
_TSIG = "(const double *p, int i, double t, const T *y, const T *x"
_G_X = " + 0.05 * (x[0] * x[0])) + ((0.1 * x[1]) * y[0] + p[NP + 1] * y[2])"
_G_NOX = ") + p[NP + 1] * y[2]"
SOURCE = """
template <class T> __device__ void F@TSIG@, T *f) {
  f[0] = (-p[0] * y[0] + y[1]) + (p[NP] * t) * x[0];
  f[1] = ((-y[0] - p[1] * y[1]) + x[1] * y[2]) + p[NP + 1];
  f[2] = (-p[2] * y[2] + (0.5 * x[0]) * y[0]) + 0.1 * (y[1] * y[1]);
}
template <class T> __device__ T G@TSIG@) {
  const T a = y[0] - p[NP];
  return ((0.5 * (a * a) + 0.5 * (y[1] * y[1]))@GTAIL@;
}
template <class T> __device__ T E(const double *p, double t, const T *y) {
  const T e = y[2] - 1.0;
  return ((0.5 * p[NP]) * (e * e) + 0.5 * (y[1] * y[1])) + (0.01 * t) * y[0];
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
__device__ void Gy@SIG@, double *gy) {
  gy[0] = (y[0] - p[NP])@GY0@;
  gy[1] = y[1];
  gy[2] = p[NP + 1];
}
#endif
#ifndef MIOC_DERIVE_GU
__device__ void Gu@SIG@, double *gu) {
@GU@}
#endif
#ifndef MIOC_DERIVE_EY
__device__ void Ey(const double *p, double t, const double *y, double *ey) {
  ey[0] = 0.01 * t;
  ey[1] = y[1];
  ey[2] = p[NP] * (y[2] - 1.0);
}
#endif
""".replace("@SIG@", _SIG).replace("@TSIG@", _TSIG)
SOURCE_XFREE = SOURCE.replace("@GTAIL@", _G_NOX).replace("@GY0@", "").replace("@GU@", "")
SOURCE = SOURCE.replace("@GTAIL@", _G_X).replace("@GY0@", " + 0.1 * x[1]").replace(
    "@GU@", "  gu[0] = 0.1 * x[0];\n  gu[1] = 0.1 * y[0];\n")

# the copy for check_hooks: the hand-written Ey's entry ey[1] = dE/dy1 with the wrong sign
_FLIP = "  ey[1] = y[1];\n"
assert SOURCE.count(_FLIP) == 1
SOURCE_WRONG_EY = SOURCE.replace(_FLIP, "  ey[1] = -y[1];\n")

# appended to a text without a terminal cost (the fourth problem's): with E = 0 the program must reproduce the plain one
SOURCE_E0 = """
__device__ double E(const double *p, double t, const double *y) { return 0.0; }
__device__ void Ey(const double *p, double t, const double *y, double *ey) {}
"""


def _hooks(xfree):
    """The hooks above in Python floats, the same expressions with the same parentheses (tests/ode_bolza_mirror.py)."""
    def F(p, i, t, y, x, f):
        f[0] = (-p[0] * y[0] + y[1]) + (p[NP] * t) * x[0]
        f[1] = ((-y[0] - p[1] * y[1]) + x[1] * y[2]) + p[NP + 1]
        f[2] = (-p[2] * y[2] + (0.5 * x[0]) * y[0]) + 0.1 * (y[1] * y[1])

    def G(p, i, t, y, x):
        a = y[0] - p[NP]
        if xfree:
            return (0.5 * (a * a) + 0.5 * (y[1] * y[1])) + p[NP + 1] * y[2]
        return ((0.5 * (a * a) + 0.5 * (y[1] * y[1])) + 0.05 * (x[0] * x[0])) + ((0.1 * x[1]) * y[0] + p[NP + 1] * y[2])

    def E(p, t, y):
        e = y[2] - 1.0
        return ((0.5 * p[NP]) * (e * e) + 0.5 * (y[1] * y[1])) + (0.01 * t) * y[0]

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
        gy[0] = (y[0] - p[NP]) if xfree else (y[0] - p[NP]) + 0.1 * x[1]
        gy[1] = y[1]
        gy[2] = p[NP + 1]

    def Gu(p, i, t, y, x, gu):
        if not xfree:
            gu[0] = 0.1 * x[0]
            gu[1] = 0.1 * y[0]

    def Ey(p, t, y, ey):
        ey[0] = 0.01 * t
        ey[1] = y[1]
        ey[2] = p[NP] * (y[2] - 1.0)

    return types.SimpleNamespace(F=F, G=G, E=E, Fy=Fy, Fu=Fu, Gy=Gy, Gu=Gu, Ey=Ey)


HOOKS, HOOKS_XFREE = _hooks(False), _hooks(True)

# ---- the known answer (ny = nx = ND = 1, NP = 0): F = d x, G = d x, E = 2 y; exact in doubles, derived by hand -------
KNOWN_SOURCE = """
__device__ void F@SIG@, double *f) { f[0] = p[0] * x[0]; }
__device__ void Fy@SIG@, double (*fy)[NY]) {}
__device__ void Fu@SIG@, double (*fu)[NX]) { fu[0][0] = p[0]; }
__device__ double G@SIG@) { return p[0] * x[0]; }
__device__ void Gy@SIG@, double *gy) {}
__device__ void Gu@SIG@, double *gu) { gu[0] = p[0]; }
__device__ double E(const double *p, double t, const double *y) { return 2.0 * y[0]; }
__device__ void Ey(const double *p, double t, const double *y, double *ey) { ey[0] = 2.0; }
""".replace("@SIG@", _SIG)
KNOWN = dict(T0=0.0, T1=1.0, nt=4, state0=[0.5], data=[[1.0], [2.0], [4.0], [8.0]], x=[[1.0], [0.0], [2.0], [1.0]],
             Y=[0.5, 0.75, 0.75, 2.75, 4.75], df=[3.0, 6.0, 12.0, 24.0], J_euler=14.625, J_other=13.75)


def _known_hooks():
    def F(p, i, t, y, x, f):
        f[0] = p[0] * x[0]

    def Fu(p, i, t, y, x, fu):
        fu[0][0] = p[0]

    def Gu(p, i, t, y, x, gu):
        gu[0] = p[0]

    def Ey(p, t, y, ey):
        ey[0] = 2.0

    def none(*a):
        pass
    return types.SimpleNamespace(F=F, G=lambda p, i, t, y, x: p[0] * x[0], E=lambda p, t, y: 2.0 * y[0], Fy=none,
                                 Fu=Fu, Gy=none, Gu=Gu, Ey=Ey)


KNOWN_HOOKS = _known_hooks()


# ---- the largest shape: every hook derived, the generated hooks compiled as called functions -------------------------
def synthetic_source(n, np_, nd):
    """Templated F, G, E of a dense problem with ny = nx = n that reads the last parameter and the last data entry."""
    sig = "(const double *p, int i, double t, const T *y, const T *x"
    last = np_ + nd - 1
    return f"""
template <class T> __device__ void F{sig}, T *f) {{
  for (int r = 0; r < {n}; ++r) {{
    T a = -y[r] + (t * p[{np_ - 1}]) * x[r];
    for (int c = 0; c < {n}; ++c) a = a + (0.01 * (r + 1)) * (y[c] * x[(r + c) % {n}]);
    f[r] = a + p[{last}];
  }}
}}
template <class T> __device__ T G{sig}) {{
  T g = 0.0 * y[0];
  for (int r = 0; r < {n}; ++r) g = g + (0.5 * (y[r] * y[r]) + (0.1 * p[{last}]) * (x[r] * y[r]));
  return g;
}}
template <class T> __device__ T E(const double *p, double t, const T *y) {{
  T e = 0.0 * y[0];
  for (int r = 0; r < {n}; ++r) e = e + (p[{np_ + (0 if nd else -1)}] * t) * (y[r] * y[r]);
  return e;
}}
"""


MIXED_NU, MIXED_V, MIXED_LO, MIXED_HI = 1, [[0, 1]], 0.0, 2.0


class BolzaMixedObj(AbstractODEObjective):
    """The shape of the mixed variant (x0 continuous in [0, 2], x1 on the levels [0, 1]) for the host loop TRM_mixed."""

    def __init__(self, nt=32, T0=0.0, T1=0.96):
        super().__init__(T0, T1, nt, MIXED_V, product_iterator(MIXED_V), STATE0, nu=MIXED_NU, umin=MIXED_LO,
                         umax=MIXED_HI)


class BolzaObj(AbstractODEObjective):
    """The shape of the problem for the host TRM loop (levels, horizon, state0).  The hooks have no host objective:
    the tests replace eval_f_helper / eval_df_helper by calls of the device program."""

    def __init__(self, nt=48, T0=0.0, T1=0.96):
        super().__init__(T0, T1, nt, V, product_iterator(V), STATE0)
