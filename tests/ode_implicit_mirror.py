"""Host mirror of the backward Euler / implicit midpoint schemes of user-defined ODE objectives (include/mioc.h,
"Implicit integrators"): a restatement in Python floats, operation for operation in the documented rounding order,
against which test_gpu_ode_implicit.py compares the device kernel and whose gradient, order and failure contract
test_ode_implicit.py pins.  It drives the hooks of a host objective as ode_rk_mirror.py does: `i` = the control interval
and i2t replaced by the stage time.  Test code: the product never imports it.

  grid      tau = (T1 - T0) / nt, h = tau / m, substep n = i*m + j, stage time t_s = (T0 + n*h) + theta*h
  forward   k = F(Y), Y = y_n + (theta h) k by Newton from k = F(y_n): r = F(Y) - k, A = I - (theta h) Fy(Y),
            A delta = r, k += delta, at most NEWTON_MAX times, until |delta_r| <= NEWTON_TOL * max(1, max|k_r|) and k_r
            finite for every r;  y_{n+1} = y_n + h k;  q_{n+1} = q_n + h G(Y);  J = q_{nt*m}
  adjoint   w = 0; per substep backwards at the stored Y: kbar = h w + ((theta h) h) Gy;  (I - (theta h) Fy)' mu = kbar;
            xbar_i += Fu' mu + h Gu;  w += Fy' mu + h Gy
  gradient  df[:, i] = xbar_i / tau
  failure   a substep that does not converge: J and df are NaN
"""
import math

import numpy as np

THETA = {"beuler": 1.0, "midpoint": 0.5}
NEWTON_MAX, NEWTON_TOL = 12, 1e-10
DBL_MAX = 1.7976931348623157e308

# the order tests (CPU and GPU tier): successive error ratios of J under halved h lie in [0.75 * 2^p, 1.35 * 2^p]
ORDER_BANDS = {"beuler": (1.5, 2.7), "midpoint": (3.0, 5.4)}


def _at(obj, t):
    """The hooks of a host objective read the time through i2t: make it the stage time."""
    obj.i2t = lambda i: t


def _div(a, b):
    """The IEEE quotient of two Python floats (Python raises where IEEE returns an infinity or a NaN)."""
    return float(np.float64(a) / np.float64(b))


def solve(A, b):
    """A d = b: the Gaussian elimination of include/mioc.h ("solve"); A (list of rows) and b are overwritten."""
    n = len(b)
    for c in range(n):
        for r in range(c + 1, n):
            if abs(A[r][c]) > abs(A[c][c]):
                for e in range(c, n):
                    A[c][e], A[r][e] = A[r][e], A[c][e]
                b[c], b[r] = b[r], b[c]
        for r in range(c + 1, n):
            f = _div(A[r][c], A[c][c])
            for e in range(c + 1, n):
                A[r][e] = A[r][e] - f * A[c][e]
            b[r] = b[r] - f * b[c]
    d = [0.0] * n
    for r in range(n - 1, -1, -1):
        s = b[r]
        for e in range(r + 1, n):
            s = s - A[r][e] * d[e]
        d[r] = _div(s, A[r][r])
    return d


def theta_eval(obj, x, integrator, substeps, want_df=True, stats=None):
    """J and df (nx, nt; None unless want_df) of the control x (nx, nt) under `integrator` with `substeps`; NaN for both
    where a substep's Newton iteration fails.  stats (a list, optional) receives the Newton updates of every substep."""
    theta, m = THETA[integrator], int(substeps)
    ny, nx, nt = obj.ny, obj.nx, obj.nt
    T0 = obj.T0
    tau = (obj.T1 - obj.T0) / nt
    h = tau / m
    th = theta * h
    thh = th * h
    x = np.asarray(x, dtype=np.float64)
    y = np.array(obj.state0, dtype=np.float64)
    stages = []
    kv, f = np.zeros(ny), np.zeros(ny)
    fy = np.zeros((ny, ny))  # zeroed once per evaluation
    q = 0.0
    try:
        with np.errstate(all="ignore"):
            for i in range(nt):
                xc = x[:, i].copy()
                for j in range(m):
                    n = i * m + j
                    ts = (T0 + float(n) * h) + th
                    _at(obj, ts)
                    obj.F(kv, i, y, xc)
                    conv, it = False, 0
                    while it < NEWTON_MAX and not conv:
                        it += 1
                        Y = np.array([y[r] + th * kv[r] for r in range(ny)])
                        obj.F(f, i, Y, xc)
                        obj.Fy(fy, i, Y, xc)
                        res = [float(f[r] - kv[r]) for r in range(ny)]
                        A = [[(1.0 if r == c else 0.0) - th * float(fy[r, c]) for c in range(ny)] for r in range(ny)]
                        d = solve(A, res)
                        kmax = 1.0
                        for r in range(ny):
                            kv[r] = kv[r] + d[r]
                            a = abs(float(kv[r]))
                            kmax = a if a > kmax else kmax  # fmax: a NaN is dropped
                        tol = NEWTON_TOL * kmax
                        conv = all(abs(d[r]) <= tol and abs(float(kv[r])) <= DBL_MAX for r in range(ny))
                    if stats is not None:
                        stats.append(it)
                    if not conv:
                        return math.nan, (np.full((nx, nt), math.nan) if want_df else None)
                    Y = np.array([y[r] + th * kv[r] for r in range(ny)])
                    stages.append(Y)
                    q = q + h * obj.G(i, Y, xc)
                    for r in range(ny):
                        y[r] = y[r] + h * kv[r]
            J = float(q)
            if not want_df:
                return J, None
            df = np.zeros((nx, nt))
            fu, gy, gu = np.zeros((ny, nx)), np.zeros(ny), np.zeros(nx)  # zeroed once, fy as the forward sweep left it
            w = [0.0] * ny
            for i in range(nt - 1, -1, -1):
                xc = x[:, i].copy()
                xbar = [0.0] * nx
                for j in range(m - 1, -1, -1):
                    n = i * m + j
                    ts = (T0 + float(n) * h) + th
                    Y = stages[n]
                    _at(obj, ts)
                    obj.Fy(fy, i, Y, xc)
                    obj.Gy(gy, i, Y, xc)
                    kb = [h * w[r] + thh * float(gy[r]) for r in range(ny)]
                    A = [[(1.0 if r == c else 0.0) - th * float(fy[c, r]) for c in range(ny)] for r in range(ny)]
                    mu = solve(A, kb)
                    obj.Fu(fu, i, Y, xc)
                    obj.Gu(gu, i, Y, xc)
                    for mm in range(nx):
                        t = float(fu[0, mm]) * mu[0]
                        for r in range(1, ny):
                            t = t + float(fu[r, mm]) * mu[r]
                        xbar[mm] = xbar[mm] + (t + h * float(gu[mm]))
                    for c in range(ny):
                        t = float(fy[0, c]) * mu[0]
                        for r in range(1, ny):
                            t = t + float(fy[r, c]) * mu[r]
                        w[c] = w[c] + (t + h * float(gy[c]))
                for mm in range(nx):
                    df[mm, i] = _div(xbar[mm], tau)
            return J, df
    finally:
        del obj.i2t  # the class's own i2t again
