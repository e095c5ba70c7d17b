"""A fifth ODE problem for the tests of derived hooks (test_ode_program_ad.py, test_gpu_ode_program_ad.py): F and G as
templates over the scalar type, and Fy, Fu, Gy, Gu written by hand under the guards ``#ifndef MIOC_DERIVE_FY`` ...,
so the one text serves every ``derive`` mask (include/mioc.h, "Derived hooks").  ny = 3 states and nx = 2 controls on
the product grid [[0,1,2],[0,1]], six parameters p = [a, b, c, w, g, e], all used, as are t and i.

The linear part is the fourth problem's (tests/ode_program_problem.py: damped, the eigenvalues of the y-Jacobian have
real parts about -0.3 .. -0.65); the nonlinear terms carry the factor e = 0.05 and bounded derivatives, so the states
stay of order one and the dynamics damped:

  F  = [ -a y0 + y1 + (w t) x0 + e s,   -y0 - b y1 + x1 y2 + e q,   -c y2 + (x0 / 2) y0 + e r ]
       s = tanh(y0 - x0) + (y1 / 2) y2
       q = atan(y2 x0) - log(6 + y0) / (2 + x1)
       r = sqrt(5 + y1) - exp(1/2 - y2^2) + 1 / (3 + x0)
  G  = (y0 - 1)^2 / 2 + y1^2 / 2 + y2^2 / 2 + g x0^2 + (x1 / 10) y0 + (i mod 3) y1 / 1000 + e gate (m + n / 10 + r' / 2)
       m  = (tan(u) + sin(u) cos(u) + |y2 - 5| + |y0 + 5| - (2 + y0)^1.5 + (2 + y0)^(x1 + 1)) / (2 (2 + x1)),
            u = y1 / 10 + x1 / 2
       n  = min(y0, y1 + 5) + min(y2 + 5, y1) + max(y0, y2 - 5) + max(y1 - 5, x0) + min(y2, 5) + max(-5, y2) + max(y1, 5)
          = 2 y0 + y1 + 2 y2 + x0 + 5   while |y_r| < 5
       r' = y1 y2 / 8 - x1 + 3/4
       gate = 1 while |y_r| < 5: the 18 comparisons (six operators, three operand forms) are all true

Coverage of the dual type's list: every operator and function has a Dual argument at least once (both F and G are
instantiated with y the variable and with x the variable, and the other argument a Dual constant); + - * / appear as
Dual o Dual, Dual o double and double o Dual, each op= with a Dual and with a double on the right; fabs with a
negative (y2 - 5) and a positive (y0 + 5) argument, fmin and fmax taking the first and the second argument; every
kink is at least 4 away from the states (|y_r| < 1 on the tests' horizons).  mioc_ad::value exists only where the
dual type does (derive != 0), hence the FIFTH_VALUE macro.
"""
from mioc.iterators import product_iterator
from mioc.ode import AbstractODEObjective

NY, NX = 3, 2
V = [[0, 1, 2], [0, 1]]
PARAMS = [0.5, 0.8, 0.3, 0.2, 0.05, 0.05]
STATE0 = [0.2, -0.1, 0.3]

_SIG = "(const double *p, int i, double t, const double *y, const double *x"
_TSIG = "(const double *p, int i, double t, const T *y, const T *x"
SOURCE = """
#if defined(MIOC_DERIVE_FY) || defined(MIOC_DERIVE_FU) || defined(MIOC_DERIVE_GY) || defined(MIOC_DERIVE_GU)
#define FIFTH_VALUE(a) mioc_ad::value(a)
#else
#define FIFTH_VALUE(a) (a)
#endif
template <class T> __device__ double fifth_gate(const T *y, const T *x) {  // 18 of 18 while |y_r| < 5
  int n = 0;
  n += y[0] < y[1] + 5.0;
  n += y[0] < 5.0;
  n += -5.0 < y[0];
  n += y[1] <= y[2] + 5.0;
  n += y[1] <= 5.0;
  n += -5.0 <= y[1];
  n += y[2] + 5.0 > y[0];
  n += y[2] > -5.0;
  n += 5.0 > y[2];
  n += y[0] + 5.0 >= y[1];
  n += y[0] >= -5.0;
  n += 5.0 >= y[0];
  n += x[0] == x[0];
  n += x[1] == FIFTH_VALUE(x[1]);
  n += FIFTH_VALUE(x[0]) == x[0];
  n += y[0] != y[0] + 1.0;
  n += y[1] != 7.0;
  n += 7.0 != y[2];
  return n == 18 ? 1.0 : 0.0;
}
template <class T> __device__ void F@TSIG@, T *f) {
  const T s = tanh(y[0] - x[0]) + (y[1] * 0.5) * y[2];
  const T q = atan(y[2] * x[0]) - log(6.0 + y[0]) / (2.0 + x[1]);
  const T r = (sqrt(5.0 + y[1]) - exp(0.5 - y[2] * y[2])) + 1.0 / (3.0 + x[0]);
  f[0] = ((-p[0] * y[0] + (+y[1])) + (p[3] * t) * x[0]) + p[5] * s;
  f[1] = ((-y[0] - p[1] * y[1]) + x[1] * y[2]) + p[5] * q;
  f[2] = (-p[2] * y[2] + (0.5 * x[0]) * y[0]) + p[5] * r;
}
template <class T> __device__ T G@TSIG@) {
  const T a = y[0] - 1.0;
  const T u = 0.1 * y[1] + 0.5 * x[1];
  T m = tan(u);
  m += sin(u) * cos(u);
  m += fabs(y[2] - 5.0);
  m += fabs(y[0] + 5.0);
  m -= pow(2.0 + y[0], 1.5);
  m += pow(2.0 + y[0], x[1] + 1.0);
  m *= 0.5;
  m /= 2.0 + x[1];
  T n = (fmin(y[0], y[1] + 5.0) + fmin(y[2] + 5.0, y[1])) + (fmax(y[0], y[2] - 5.0) + fmax(y[1] - 5.0, x[0]));
  n = (n + fmin(y[2], 5.0)) + (fmax(-5.0, y[2]) + fmax(y[1], 5.0));
  T r = y[1] / 4.0;
  r *= y[2];
  r /= 2.0;
  r -= x[1];
  r += 1.0;
  r -= 0.25;
  const double gate = fifth_gate(y, x);
  const T base = ((0.5 * (a * a) + 0.5 * (y[1] * y[1])) + 0.5 * (y[2] * y[2])) + (p[4] * (x[0] * x[0]) + (0.1 * x[1]) * y[0]);
  return (base + (0.001 * (double)(i % 3)) * y[1]) + p[5] * (gate * ((m + 0.1 * n) + r * 0.5));
}
#ifndef MIOC_DERIVE_FY
__device__ void Fy@SIG@, double (*fy)[NY]) {  // fy[2][0] has no e term; all nine entries written
  const double th = tanh(y[0] - x[0]), u = y[2] * x[0];
  fy[0][0] = -p[0] + p[5] * (1.0 - th * th);
  fy[0][1] = 1.0 + p[5] * (0.5 * y[2]);
  fy[0][2] = p[5] * (0.5 * y[1]);
  fy[1][0] = -1.0 + p[5] * (-1.0 / ((6.0 + y[0]) * (2.0 + x[1])));
  fy[1][1] = -p[1];
  fy[1][2] = x[1] + p[5] * (x[0] / (1.0 + u * u));
  fy[2][0] = 0.5 * x[0];
  fy[2][1] = p[5] * (1.0 / (2.0 * sqrt(5.0 + y[1])));
  fy[2][2] = -p[2] + p[5] * ((2.0 * y[2]) * exp(0.5 - y[2] * y[2]));
}
#endif
#ifndef MIOC_DERIVE_FU
__device__ void Fu@SIG@, double (*fu)[NX]) {  // fu[0][1] and fu[2][1] are structural zeros: never written
  const double th = tanh(y[0] - x[0]), u = y[2] * x[0];
  fu[0][0] = p[3] * t - p[5] * (1.0 - th * th);
  fu[1][0] = p[5] * (y[2] / (1.0 + u * u));
  fu[1][1] = y[2] + p[5] * (log(6.0 + y[0]) / ((2.0 + x[1]) * (2.0 + x[1])));
  fu[2][0] = 0.5 * y[0] - p[5] / ((3.0 + x[0]) * (3.0 + x[0]));
}
#endif
#ifndef MIOC_DERIVE_GY
__device__ void Gy@SIG@, double *gy) {
  const double D = 2.0 + x[1], u = 0.1 * y[1] + 0.5 * x[1], tn = tan(u), sn = sin(u), cs = cos(u);
  const double A0 = (1.0 - 1.5 * sqrt(2.0 + y[0])) + (x[1] + 1.0) * pow(2.0 + y[0], x[1]);
  const double A1 = 0.1 * ((1.0 + tn * tn) + (cs * cs - sn * sn));
  gy[0] = ((y[0] - 1.0) + 0.1 * x[1]) + p[5] * (0.5 * A0 / D + 0.2);
  gy[1] = (y[1] + 0.001 * (double)(i % 3)) + p[5] * ((0.5 * A1 / D + 0.1) + 0.0625 * y[2]);
  gy[2] = y[2] + p[5] * ((-0.5 / D + 0.2) + 0.0625 * y[1]);
}
#endif
#ifndef MIOC_DERIVE_GU
__device__ void Gu@SIG@, double *gu) {
  const double D = 2.0 + x[1], u = 0.1 * y[1] + 0.5 * x[1], tn = tan(u), sn = sin(u), cs = cos(u);
  const double B = pow(2.0 + y[0], x[1] + 1.0);
  const double A = ((((tn + sn * cs) + (5.0 - y[2])) + (y[0] + 5.0)) - pow(2.0 + y[0], 1.5)) + B;
  const double Ax1 = 0.5 * ((1.0 + tn * tn) + (cs * cs - sn * sn)) + B * log(2.0 + y[0]);
  gu[0] = (2.0 * p[4]) * x[0] + p[5] * 0.1;
  gu[1] = 0.1 * y[0] + p[5] * ((0.5 * Ax1 / D - (0.5 * A) / (D * D)) - 0.5);
}
#endif
""".replace("@SIG@", _SIG).replace("@TSIG@", _TSIG)

# the copy for check_hooks: the sign of the hand-written Fy's entry fy[0][1] = d f0 / d y1 (about +1) flipped
_FLIP = "  fy[0][1] = 1.0 + p[5] * (0.5 * y[2]);\n"
assert SOURCE.count(_FLIP) == 1
SOURCE_WRONG_FY = SOURCE.replace(_FLIP, "  fy[0][1] = -(1.0 + p[5] * (0.5 * y[2]));\n")


class FifthObj(AbstractODEObjective):
    """The shape of the problem for the host TRM loop (levels, horizon, state0).  The hooks have no host mirror: the
    tests replace eval_f_helper / eval_df_helper by calls of the device program."""

    def __init__(self, nt=48, T0=0.0, T1=0.96):
        super().__init__(T0, T1, nt, V, product_iterator(V), STATE0)
