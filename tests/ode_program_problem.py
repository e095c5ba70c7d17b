"""A fourth ODE problem for the tests of user-defined device objectives (test_ode_program.py, test_gpu_ode_program.py):
hook text for mioc.ode_device.ODEProgram and the matching host objective (mioc.ode.AbstractODEObjective), written with
the same parenthesisation.  It exercises what the three built-in examples never do: ny = 3 states and nx = 2 controls
on the product grid [[0,1,2],[0,1]], an F that depends on t, a running cost G that depends on the control (Gu != 0),
an Fy / Fu with structural zeros that the hooks never write, five parameters.  The linear part is damped (the
eigenvalues of the y-Jacobian have real parts about -0.3 .. -0.65 for all controls), so explicit Euler at
tau = 0.01 is well inside its stability region.

  F  = [ -a y0 + y1 + (w t) x0,   -y0 - b y1 + x1 y2,   -c y2 + (x0 / 2) y0 ]
  G  = (y0 - 1)^2 / 2 + y1^2 / 2 + y2^2 / 2 + g x0^2 + (x1 / 10) y0
  p  = [a, b, c, w, g]
"""
import numpy as np

from mioc.iterators import product_iterator
from mioc.ode import AbstractODEObjective

NY, NX = 3, 2
V = [[0, 1, 2], [0, 1]]
PARAMS = [0.5, 0.8, 0.3, 0.2, 0.05]
STATE0 = [0.2, -0.1, 0.3]

_SIG = "(const double *p, int i, double t, const double *y, const double *x"
SOURCE = """
__device__ void F@SIG@, double *f) {
  f[0] = (-p[0] * y[0] + y[1]) + (p[3] * t) * x[0];
  f[1] = (-y[0] - p[1] * y[1]) + x[1] * y[2];
  f[2] = -p[2] * y[2] + (0.5 * x[0]) * y[0];
}
__device__ void Fy@SIG@, double (*fy)[NY]) {  // fy[0][2] and fy[2][1] are structural zeros: never written
  fy[0][0] = -p[0];
  fy[0][1] = 1.0;
  fy[1][0] = -1.0;
  fy[1][1] = -p[1];
  fy[1][2] = x[1];
  fy[2][0] = 0.5 * x[0];
  fy[2][2] = -p[2];
}
__device__ void Fu@SIG@, double (*fu)[NX]) {  // three of six entries are non-zero
  fu[0][0] = p[3] * t;
  fu[1][1] = y[2];
  fu[2][0] = 0.5 * y[0];
}
__device__ double G@SIG@) {
  const double a = y[0] - 1.0;
  return ((0.5 * (a * a) + 0.5 * (y[1] * y[1])) + 0.5 * (y[2] * y[2])) + (p[4] * (x[0] * x[0]) + (0.1 * x[1]) * y[0]);
}
__device__ void Gy@SIG@, double *gy) {
  gy[0] = (y[0] - 1.0) + 0.1 * x[1];
  gy[1] = y[1];
  gy[2] = y[2];
}
__device__ void Gu@SIG@, double *gu) {
  gu[0] = (2.0 * p[4]) * x[0];
  gu[1] = 0.1 * y[0];
}
""".replace("@SIG@", _SIG)


class FourthObj(AbstractODEObjective):
    """The host mirror of SOURCE."""

    def __init__(self, nt=96, T0=0.0, T1=0.96):
        super().__init__(T0, T1, nt, V, product_iterator(V), STATE0)
        self.p = np.array(PARAMS, dtype=np.float64)

    def F(self, f, i, y, x):
        p, t = self.p, self.i2t(i)
        f[0] = (-p[0] * y[0] + y[1]) + (p[3] * t) * x[0]
        f[1] = (-y[0] - p[1] * y[1]) + x[1] * y[2]
        f[2] = -p[2] * y[2] + (0.5 * x[0]) * y[0]

    def Fy(self, fy, i, y, x):
        p = self.p
        fy[0, 0] = -p[0]
        fy[0, 1] = 1.0
        fy[1, 0] = -1.0
        fy[1, 1] = -p[1]
        fy[1, 2] = x[1]
        fy[2, 0] = 0.5 * x[0]
        fy[2, 2] = -p[2]

    def Fu(self, fu, i, y, x):
        fu[0, 0] = self.p[3] * self.i2t(i)
        fu[1, 1] = y[2]
        fu[2, 0] = 0.5 * y[0]

    def G(self, i, y, x):
        a = y[0] - 1.0
        return ((0.5 * (a * a) + 0.5 * (y[1] * y[1])) + 0.5 * (y[2] * y[2])) + \
            (self.p[4] * (x[0] * x[0]) + (0.1 * x[1]) * y[0])

    def Gy(self, gy, i, y, x):
        gy[0] = (y[0] - 1.0) + 0.1 * x[1]
        gy[1] = y[1]
        gy[2] = y[2]

    def Gu(self, gu, i, y, x):
        gu[0] = (2.0 * self.p[4]) * x[0]
        gu[1] = 0.1 * y[0]
