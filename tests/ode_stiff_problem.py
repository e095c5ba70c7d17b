"""A stiff ODE problem for the tests of the implicit integrators of user-defined device objectives (test_ode_implicit.py,
test_gpu_ode_implicit.py): hook text for mioc.ode_device.ODEProgram and the matching host objective
(mioc.ode.AbstractODEObjective), written with the same parenthesisation, in the pattern of ode_program_problem.py.
ny = 3 states and nx = 2 controls on the product grid [[0,1,2],[0,1]], one parameter, the fast rate kappa = 2000: y0 is
pulled onto y1^2 within 1 / kappa, so an explicit scheme at h = 0.04 (kappa h = 80) blows up while the slow dynamics
need no finer step.  Nonlinear in y (Newton iterates), time dependent, structural zeros in Fy and Fu that the hooks
never write, Gu != 0.

  F  = [ -kappa (y0 - y1^2) + x0,   (-y1 + (x1 / 2) y2) + t / 5,   -0.3 y2 + (x0 / 2) y1 ]
  G  = ((y0 - 1/2)^2 / 2 + y1^2 / 2) + (x0^2 / 20 + (x1 / 10) y2)
  p  = [kappa]
"""
import numpy as np

from mioc.iterators import product_iterator
from mioc.ode import AbstractODEObjective

NY, NX = 3, 2
V = [[0, 1, 2], [0, 1]]
PARAMS = [2000.0]
STATE0 = [0.3, 0.4, -0.2]

_SIG = "(const double *p, int i, double t, const double *y, const double *x"
SOURCE = """
__device__ void F@SIG@, double *f) {
  f[0] = -p[0] * (y[0] - y[1] * y[1]) + x[0];
  f[1] = (-y[1] + (0.5 * x[1]) * y[2]) + 0.2 * t;
  f[2] = -0.3 * y[2] + (0.5 * x[0]) * y[1];
}
__device__ void Fy@SIG@, double (*fy)[NY]) {  // fy[0][2], fy[1][0] and fy[2][0] are structural zeros: never written
  fy[0][0] = -p[0];
  fy[0][1] = p[0] * (2.0 * y[1]);
  fy[1][1] = -1.0;
  fy[1][2] = 0.5 * x[1];
  fy[2][1] = 0.5 * x[0];
  fy[2][2] = -0.3;
}
__device__ void Fu@SIG@, double (*fu)[NX]) {  // three of six entries are non-zero
  fu[0][0] = 1.0;
  fu[1][1] = 0.5 * y[2];
  fu[2][0] = 0.5 * y[1];
}
__device__ double G@SIG@) {
  const double a = y[0] - 0.5;
  return (0.5 * (a * a) + 0.5 * (y[1] * y[1])) + (0.05 * (x[0] * x[0]) + (0.1 * x[1]) * y[2]);
}
__device__ void Gy@SIG@, double *gy) {
  gy[0] = y[0] - 0.5;
  gy[1] = y[1];
  gy[2] = 0.1 * x[1];
}
__device__ void Gu@SIG@, double *gu) {
  gu[0] = 0.1 * x[0];
  gu[1] = 0.1 * y[2];
}
""".replace("@SIG@", _SIG)


class StiffObj(AbstractODEObjective):
    """The host mirror of SOURCE."""

    def __init__(self, nt=24, T0=0.0, T1=0.96):
        super().__init__(T0, T1, nt, V, product_iterator(V), STATE0)
        self.p = np.array(PARAMS, dtype=np.float64)

    def F(self, f, i, y, x):
        p, t = self.p, self.i2t(i)
        f[0] = -p[0] * (y[0] - y[1] * y[1]) + x[0]
        f[1] = (-y[1] + (0.5 * x[1]) * y[2]) + 0.2 * t
        f[2] = -0.3 * y[2] + (0.5 * x[0]) * y[1]

    def Fy(self, fy, i, y, x):
        p = self.p
        fy[0, 0] = -p[0]
        fy[0, 1] = p[0] * (2.0 * y[1])
        fy[1, 1] = -1.0
        fy[1, 2] = 0.5 * x[1]
        fy[2, 1] = 0.5 * x[0]
        fy[2, 2] = -0.3

    def Fu(self, fu, i, y, x):
        fu[0, 0] = 1.0
        fu[1, 1] = 0.5 * y[2]
        fu[2, 0] = 0.5 * y[1]

    def G(self, i, y, x):
        a = y[0] - 0.5
        return (0.5 * (a * a) + 0.5 * (y[1] * y[1])) + (0.05 * (x[0] * x[0]) + (0.1 * x[1]) * y[2])

    def Gy(self, gy, i, y, x):
        gy[0] = y[0] - 0.5
        gy[1] = y[1]
        gy[2] = 0.1 * x[1]

    def Gu(self, gu, i, y, x):
        gu[0] = 0.1 * x[0]
        gu[1] = 0.1 * y[2]


# The non-convergence problem: ny = nx = 1, F = x0 (1e3 + 1e6 y^2) - y, G = y^2 / 2.  With x = 1 the stage equation
# k = F(y_n + theta h k) has no real root at the tests' steps (its discriminant is negative), with x = 0 it is linear.
NOROOT_NY, NOROOT_NX = 1, 1
NOROOT_V = [[0, 1]]
NOROOT_STATE0 = [0.1]
NOROOT_SOURCE = """
__device__ void F@SIG@, double *f) { f[0] = x[0] * (1e3 + 1e6 * (y[0] * y[0])) - y[0]; }
__device__ void Fy@SIG@, double (*fy)[NY]) { fy[0][0] = x[0] * (2e6 * y[0]) - 1.0; }
__device__ void Fu@SIG@, double (*fu)[NX]) { fu[0][0] = 1e3 + 1e6 * (y[0] * y[0]); }
__device__ double G@SIG@) { return 0.5 * (y[0] * y[0]); }
__device__ void Gy@SIG@, double *gy) { gy[0] = y[0]; }
__device__ void Gu@SIG@, double *gu) {}
""".replace("@SIG@", _SIG)


class NoRootObj(AbstractODEObjective):
    """The host mirror of NOROOT_SOURCE."""

    def __init__(self, nt=8, T0=0.0, T1=0.32):
        super().__init__(T0, T1, nt, NOROOT_V, product_iterator(NOROOT_V), NOROOT_STATE0)

    def F(self, f, i, y, x):
        f[0] = x[0] * (1e3 + 1e6 * (y[0] * y[0])) - y[0]

    def Fy(self, fy, i, y, x):
        fy[0, 0] = x[0] * (2e6 * y[0]) - 1.0

    def Fu(self, fu, i, y, x):
        fu[0, 0] = 1e3 + 1e6 * (y[0] * y[0])

    def G(self, i, y, x):
        return 0.5 * (y[0] * y[0])

    def Gy(self, gy, i, y, x):
        gy[0] = y[0]

    def Gu(self, gu, i, y, x):
        pass
