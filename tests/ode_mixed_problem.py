"""A mixed ODE problem for the tests of continuous controls beside the DP (test_mixed_host.py, test_gpu_mixed.py): hook
text for mioc.ode_device.ODEProgram -- templated F and G, the derivative hooks derived (derive="all") -- and the
matching host objective (mioc.ode.AbstractODEObjective with nu = 1), written with the same parenthesisation.

ny = 2, nu = 1 continuous control c = x[0] in [lo, hi], nv = 1 integer control v = x[1] on the levels [0, 1, 2]:
Lotka-Volterra with a harvest whose rate is the product of both controls, so each part's gradient depends on the other,

  F  = [ y0 (1 - y1) - (p0 c) (v y0),   y1 (y0 - 1) - (p1 c) (v y1) ]
  G  = (y0 - 1)^2 / 2 + (y1 - 1)^2 / 2 + p2 c^2
  p  = [p0, p1, p2]

lo = 0; hi = 1 except 0.6 on the first quarter of the horizon, so a pointwise bound is active.

The second program (KA_*) has a known answer, for RK4: G = (c - ct(i))^2 with F depending on v only, so that
J = tau sum (c_i - ct_i)^2 and dJ/dc_i = 2 (c_i - ct_i) up to rounding: a step of size 1 reflects c about ct, a step
of size 1/2 lands on ct.  ct lies outside [0, 1] at the steps i = 5, 11 (mod 16).
"""
import numpy as np

from mioc.iterators import product_iterator
from mioc.ode import AbstractODEObjective

NY, NX, NU = 2, 2, 1
V = [[0, 1, 2]]
PARAMS = [0.4, 0.2, 0.01]
STATE0 = [0.5, 0.7]
T0, T1 = 0.0, 12.0

_TSIG = "(const double *p, int i, double t, const T *y, const T *x"
SOURCE = """
template <class T> __device__ void F@SIG@, T *f) {
  f[0] = y[0] * (1.0 - y[1]) - (p[0] * x[0]) * (x[1] * y[0]);
  f[1] = y[1] * (y[0] - 1.0) - (p[1] * x[0]) * (x[1] * y[1]);
}
template <class T> __device__ T G@SIG@) {
  const T a = y[0] - 1.0, b = y[1] - 1.0;
  return (0.5 * (a * a) + 0.5 * (b * b)) + p[2] * (x[0] * x[0]);
}
""".replace("@SIG@", _TSIG)


def bounds(nt):
    """lo, hi as (nt, nu) arrays: [0, 1], and [0, 0.6] on the first quarter of the horizon."""
    lo = np.zeros((nt, NU))
    hi = np.ones((nt, NU))
    hi[: nt // 4] = 0.6
    return lo, hi


class MixedLVObj(AbstractODEObjective):
    """The host mirror of SOURCE, the derivative hooks by hand."""

    def __init__(self, nt=96):
        lo, hi = bounds(nt)
        super().__init__(T0, T1, nt, V, product_iterator(V), STATE0, nu=NU, umin=lo.T, umax=hi.T)
        self.p = np.array(PARAMS, dtype=np.float64)

    def F(self, f, i, y, x):
        p = self.p
        f[0] = y[0] * (1.0 - y[1]) - (p[0] * x[0]) * (x[1] * y[0])
        f[1] = y[1] * (y[0] - 1.0) - (p[1] * x[0]) * (x[1] * y[1])

    def Fy(self, fy, i, y, x):
        p = self.p
        fy[0, 0] = (1.0 - y[1]) - (p[0] * x[0]) * x[1]
        fy[0, 1] = -y[0]
        fy[1, 0] = y[1]
        fy[1, 1] = (y[0] - 1.0) - (p[1] * x[0]) * x[1]

    def Fu(self, fu, i, y, x):
        p = self.p
        fu[0, 0] = -p[0] * (x[1] * y[0])
        fu[0, 1] = -(p[0] * x[0]) * y[0]
        fu[1, 0] = -p[1] * (x[1] * y[1])
        fu[1, 1] = -(p[1] * x[0]) * y[1]

    def G(self, i, y, x):
        a, b = y[0] - 1.0, y[1] - 1.0
        return (0.5 * (a * a) + 0.5 * (b * b)) + self.p[2] * (x[0] * x[0])

    def Gy(self, gy, i, y, x):
        gy[0] = y[0] - 1.0
        gy[1] = y[1] - 1.0

    def Gu(self, gu, i, y, x):
        gu[0] = (2.0 * self.p[2]) * x[0]
        gu[1] = 0.0


def start(K, nt, seed):
    """K admissible starts (K, nt, nx) from numpy's generator: c uniform within the bounds, v piecewise constant on
    the levels with a jump about every eighth step."""
    rng = np.random.default_rng(seed)
    lo, hi = bounds(nt)
    x = np.empty((K, nt, NX))
    x[:, :, 0] = lo[:, 0] + (hi[:, 0] - lo[:, 0]) * rng.random((K, nt))
    for k in range(K):
        lv = int(rng.integers(3))
        for i in range(nt):
            if i and rng.random() < 0.125:
                lv = int(rng.integers(3))
            x[k, i, 1] = V[0][lv]
    return x


# ---- the known-answer program ----------------------------------------------------------------------------------------
KA_NY, KA_NX, KA_NU = 1, 2, 1
KA_V = [[0, 1, 2]]
KA_STATE0 = [0.25]
KA_SOURCE = """
__device__ double ct_of(int i) {
  if (i % 16 == 5) return 1.02;
  if (i % 16 == 11) return -0.02;
  return 0.5 + 0.03 * (double)((i * 7) % 11 - 5);
}
template <class T> __device__ void F@SIG@, T *f) { f[0] = x[1] - y[0]; }
template <class T> __device__ T G@SIG@) {
  const T d = x[0] - ct_of(i);
  return d * d;
}
""".replace("@SIG@", _TSIG)


def ka_ct(nt):
    """ct_of(i) for i = 0..nt-1, the same doubles as the hook computes."""
    i = np.arange(nt)
    ct = 0.5 + 0.03 * ((i * 7) % 11 - 5).astype(np.float64)
    ct[i % 16 == 5] = 1.02
    ct[i % 16 == 11] = -0.02
    return ct


def ka_start(K, nt, seed):
    """Starts (K, nt, 2) for the known-answer program: c = ct + d with 0.02 <= |d| <= 0.1 where ct is inside [0, 1] (the
    reflection ct - d stays inside), c on the violated bound where ct is outside; v random on the levels."""
    rng = np.random.default_rng(seed)
    ct = ka_ct(nt)
    d = rng.uniform(0.02, 0.1, size=(K, nt)) * rng.choice([-1.0, 1.0], size=(K, nt))
    c = np.clip(np.where((ct > 1.0) | (ct < 0.0), ct, ct + d), 0.0, 1.0)
    v = rng.integers(0, 3, size=(K, nt)).astype(np.float64)
    return np.ascontiguousarray(np.stack([c, v], axis=2))
