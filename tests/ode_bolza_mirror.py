"""Host mirror of the three skeletons of user-defined ODE objectives with a terminal cost E, sampled data and the state
output (include/mioc.h: "Hook contract", "Integrators", "Implicit integrators", "Terminal cost, sampled data, state
output"): a restatement in Python floats, operation for operation in the documented rounding order, against which
test_gpu_ode_bolza.py compares the device kernels and whose gradient and known answers test_ode_bolza.py pins.  Test
code: it imports nothing of the product.

A problem is a namespace `hooks` of Python callables that take the extended parameter list p_ext = p + data[c] (c the
control column whose x the hook is given):
  F(p_ext, i, t, y, x, f)   Fy(.., fy)   Fu(.., fu)   Gy(.., gy)   Gu(.., gu)   write their last argument, only the
                            entries that are not structurally zero (the outputs are zeroed once per evaluation);
  G(p_ext, i, t, y, x)      returns the running cost;
  E(p_ext, t, y), Ey(p_ext, t, y, ey)   the terminal cost, or hooks.E = None for a problem without one.

Every function takes p (list), data (nt rows of nd floats, or None), state0, T0, T1 and the control x as (nt, nx) rows
(the device layout) and returns (J, df (nt, nx) or None, Y (nt + 1, ny)).
"""
import math

import numpy as np

TABLEAUX = {
    "heun": ((0.0, 1.0), (0.0, 1.0), (0.5, 0.5)),
    "rk4": ((0.0, 0.5, 0.5, 1.0), (0.0, 0.5, 0.5, 1.0), (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)),
}
THETA = {"beuler": 1.0, "midpoint": 0.5}
NEWTON_MAX, NEWTON_TOL = 12, 1e-10
DBL_MAX = 1.7976931348623157e308


def _pe(p, data, c):
    return list(p) + ([] if data is None else [float(v) for v in data[c]])


def _zeros(*shape):
    if len(shape) == 1:
        return [0.0] * shape[0]
    return [[0.0] * shape[1] for _ in range(shape[0])]


def _div(a, b):
    """The IEEE quotient of two Python floats (Python raises where IEEE returns an infinity or a NaN)."""
    return float(np.float64(a) / np.float64(b))


def euler_eval(hooks, p, data, state0, T0, T1, x, want_df=True):
    """The reference's explicit Euler / trapezoid scheme (kBodyEuler of csrc/mioc_ode_skeleton.h)."""
    x = [[float(v) for v in row] for row in x]
    nt, nx, ny = len(x), len(x[0]), len(state0)
    tau = (T1 - T0) / nt
    y = [float(v) for v in state0]
    Y = [list(y)]
    f = _zeros(ny)
    pe = _pe(p, data, 0)
    xc = x[0]
    fval = 0.5 * hooks.G(pe, 0, T0 + 0.0 * tau, y, xc)
    states = []
    for i in range(nt):
        hooks.F(pe, i, T0 + float(i) * tau, y, xc, f)  # data column i: pe was set with xc
        y = [y[r] + tau * f[r] for r in range(ny)]
        states.append(list(y))
        Y.append(list(y))
        if i < nt - 1:
            xn = x[i + 1]
            pe = _pe(p, data, i + 1)
            fval = fval + hooks.G(pe, i + 1, T0 + float(i + 1) * tau, y, xn)
            xc = xn
        else:
            fval = fval + 0.5 * hooks.G(pe, nt - 1, T0 + float(nt - 1) * tau, y, xc)
    tend = T0 + float(nt) * tau
    J = fval * tau
    if hooks.E is not None:
        J = fval * tau + hooks.E(pe, tend, y)  # data column nt - 1
    if not want_df:
        return J, None, Y
    df = _zeros(nt, nx)
    gy, gu, fy, fu = _zeros(ny), _zeros(nx), _zeros(ny, ny), _zeros(ny, nx)  # zeroed once
    hooks.Gy(pe, nt, tend, y, xc, gy)
    if hooks.E is not None:
        ey = _zeros(ny)
        hooks.Ey(pe, tend, y, ey)
        lam = [(-0.5 * tau) * gy[r] - ey[r] for r in range(ny)]
    else:
        lam = [(-0.5 * tau) * gy[r] for r in range(ny)]
    for i in range(nt - 1, -1, -1):
        t = T0 + float(i) * tau
        s = [float(v) for v in state0] if i == 0 else states[i - 1]
        # pe is column i's: column nt - 1 from the forward sweep, then reloaded with xc below
        hooks.Fu(pe, i, t, s, xc, fu)
        hooks.Gu(pe, i, t, s, xc, gu)
        for m in range(nx):
            acc = fu[0][m] * lam[0]
            for r in range(1, ny):
                acc = acc + fu[r][m] * lam[r]
            df[i][m] = (0.0 - acc) + gu[m]
        if i == 0:
            break
        hooks.Gy(pe, i, t, s, xc, gy)
        hooks.Fy(pe, i, t, s, xc, fy)
        a = _zeros(ny)
        for c in range(ny):
            acc = fy[0][c] * lam[0]
            for r in range(1, ny):
                acc = acc + fy[r][c] * lam[r]
            a[c] = acc
        lam = [lam[c] + tau * (a[c] - gy[c]) for c in range(ny)]
        xc = x[i - 1]
        pe = _pe(p, data, i - 1)
    return J, df, Y


def rk_eval(hooks, p, data, state0, T0, T1, x, integrator, substeps, want_df=True):
    """Heun / classical RK4 with substeps (kBodyRK)."""
    c, a, b = TABLEAUX[integrator]
    S, ms = len(c), int(substeps)
    x = [[float(v) for v in row] for row in x]
    nt, nx, ny = len(x), len(x[0]), len(state0)
    tau = (T1 - T0) / nt
    h = tau / ms
    ch = [cs * h for cs in c]
    ha = [as_ * h for as_ in a]
    hb = [bs * h for bs in b]
    y = [float(v) for v in state0]
    Y = [list(y)]
    states = []
    k = [_zeros(ny) for _ in range(S)]
    g = [0.0] * S
    q = 0.0
    for i in range(nt):
        xc = x[i]
        pe = _pe(p, data, i)
        for j in range(ms):
            n = i * ms + j
            tn = T0 + float(n) * h
            states.append(list(y))
            for s in range(S):
                Ys = list(y) if s == 0 else [y[r] + ha[s] * k[s - 1][r] for r in range(ny)]
                hooks.F(pe, i, tn + ch[s], Ys, xc, k[s])
                g[s] = hooks.G(pe, i, tn + ch[s], Ys, xc)
            for r in range(ny):
                inc = hb[0] * k[0][r]
                for s in range(1, S):
                    inc = inc + hb[s] * k[s][r]
                y[r] = y[r] + inc
            inc = hb[0] * g[0]
            for s in range(1, S):
                inc = inc + hb[s] * g[s]
            q = q + inc
        Y.append(list(y))
    tend = T0 + float(nt * ms) * h
    J = q
    if hooks.E is not None:
        J = q + hooks.E(pe, tend, y)
    if not want_df:
        return J, None, Y
    df = _zeros(nt, nx)
    fy, fu, gy, gu = _zeros(ny, ny), _zeros(ny, nx), _zeros(ny), _zeros(nx)  # zeroed once
    w = _zeros(ny)
    if hooks.E is not None:
        ey = _zeros(ny)
        hooks.Ey(pe, tend, y, ey)
        w = list(ey)
    for i in range(nt - 1, -1, -1):
        xc = x[i]
        pe = _pe(p, data, i)
        xbar = _zeros(nx)
        for j in range(ms - 1, -1, -1):
            n = i * ms + j
            tn = T0 + float(n) * h
            yn = states[n]
            Ys = []
            for s in range(S):  # the stage states again, from the stored y_n
                Ys.append(list(yn) if s == 0 else [yn[r] + ha[s] * k[s - 1][r] for r in range(ny)])
                if s < S - 1:
                    hooks.F(pe, i, tn + ch[s], Ys[s], xc, k[s])
            Ybar, acc = _zeros(ny), _zeros(ny)
            for s in range(S - 1, -1, -1):
                if s == S - 1:
                    kb = [hb[s] * w[r] for r in range(ny)]
                else:
                    kb = [hb[s] * w[r] + ha[s + 1] * Ybar[r] for r in range(ny)]
                hooks.Fy(pe, i, tn + ch[s], Ys[s], xc, fy)
                hooks.Gy(pe, i, tn + ch[s], Ys[s], xc, gy)
                hooks.Fu(pe, i, tn + ch[s], Ys[s], xc, fu)
                hooks.Gu(pe, i, tn + ch[s], Ys[s], xc, gu)
                for cc in range(ny):
                    t = fy[0][cc] * kb[0]
                    for r in range(1, ny):
                        t = t + fy[r][cc] * kb[r]
                    Ybar[cc] = t + hb[s] * gy[cc]
                for m in range(nx):
                    t = fu[0][m] * kb[0]
                    for r in range(1, ny):
                        t = t + fu[r][m] * kb[r]
                    xbar[m] = xbar[m] + (t + hb[s] * gu[m])
                for cc in range(ny):
                    acc[cc] = Ybar[cc] if s == S - 1 else acc[cc] + Ybar[cc]
            for cc in range(ny):
                w[cc] = w[cc] + acc[cc]
        for m in range(nx):
            df[i][m] = _div(xbar[m], tau)
    return J, df, Y


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


def theta_eval(hooks, p, data, state0, T0, T1, x, integrator, substeps, want_df=True):
    """Backward Euler / implicit midpoint with substeps (kBodyTheta); a failed Newton iteration gives NaN."""
    theta, ms = THETA[integrator], int(substeps)
    x = [[float(v) for v in row] for row in x]
    nt, nx, ny = len(x), len(x[0]), len(state0)
    tau = (T1 - T0) / nt
    h = tau / ms
    th = theta * h
    thh = th * h
    y = [float(v) for v in state0]
    Y = [list(y)]
    stages = []
    kv, f = _zeros(ny), _zeros(ny)
    fy = _zeros(ny, ny)  # zeroed once per evaluation
    q = 0.0
    nan_out = (math.nan, [[math.nan] * nx for _ in range(nt)] if want_df else None,
               [[math.nan] * ny for _ in range(nt + 1)])
    for i in range(nt):
        xc = x[i]
        pe = _pe(p, data, i)
        for j in range(ms):
            n = i * ms + j
            ts = (T0 + float(n) * h) + th
            hooks.F(pe, i, ts, y, xc, kv)
            conv, it = False, 0
            while it < NEWTON_MAX and not conv:
                it += 1
                Ys = [y[r] + th * kv[r] for r in range(ny)]
                hooks.F(pe, i, ts, Ys, xc, f)
                hooks.Fy(pe, i, ts, Ys, xc, fy)
                res = [f[r] - kv[r] for r in range(ny)]
                A = [[(1.0 if r == c else 0.0) - th * fy[r][c] for c in range(ny)] for r in range(ny)]
                d = solve(A, res)
                kmax = 1.0
                for r in range(ny):
                    kv[r] = kv[r] + d[r]
                    av = abs(kv[r])
                    kmax = av if av > kmax else kmax
                tol = NEWTON_TOL * kmax
                conv = all(abs(d[r]) <= tol and abs(kv[r]) <= DBL_MAX for r in range(ny))
            if not conv:
                return nan_out
            Ys = [y[r] + th * kv[r] for r in range(ny)]
            stages.append(Ys)
            q = q + h * hooks.G(pe, i, ts, Ys, xc)
            y = [y[r] + h * kv[r] for r in range(ny)]
        Y.append(list(y))
    tend = T0 + float(nt * ms) * h
    J = q
    if hooks.E is not None:
        J = q + hooks.E(pe, tend, y)
    if not want_df:
        return J, None, Y
    df = _zeros(nt, nx)
    fu, gy, gu = _zeros(ny, nx), _zeros(ny), _zeros(nx)  # zeroed once, fy as the forward sweep left it
    w = _zeros(ny)
    if hooks.E is not None:
        ey = _zeros(ny)
        hooks.Ey(pe, tend, y, ey)
        w = list(ey)
    for i in range(nt - 1, -1, -1):
        xc = x[i]
        pe = _pe(p, data, i)
        xbar = _zeros(nx)
        for j in range(ms - 1, -1, -1):
            n = i * ms + j
            ts = (T0 + float(n) * h) + th
            Ys = stages[n]
            hooks.Fy(pe, i, ts, Ys, xc, fy)
            hooks.Gy(pe, i, ts, Ys, xc, gy)
            kb = [h * w[r] + thh * gy[r] for r in range(ny)]
            A = [[(1.0 if r == c else 0.0) - th * fy[c][r] for c in range(ny)] for r in range(ny)]
            mu = solve(A, kb)
            hooks.Fu(pe, i, ts, Ys, xc, fu)
            hooks.Gu(pe, i, ts, Ys, xc, gu)
            for m in range(nx):
                t = fu[0][m] * mu[0]
                for r in range(1, ny):
                    t = t + fu[r][m] * mu[r]
                xbar[m] = xbar[m] + (t + h * gu[m])
            for c in range(ny):
                t = fy[0][c] * mu[0]
                for r in range(1, ny):
                    t = t + fy[r][c] * mu[r]
                w[c] = w[c] + (t + h * gy[c])
        for m in range(nx):
            df[i][m] = _div(xbar[m], tau)
    return J, df, Y


def bolza_eval(hooks, p, data, state0, T0, T1, x, integrator, substeps=1, want_df=True):
    """(J, df (nt, nx) numpy or None, Y (nt + 1, ny) numpy) under any of the five integrators."""
    if integrator == "euler":
        J, df, Y = euler_eval(hooks, p, data, state0, T0, T1, x, want_df)
    elif integrator in TABLEAUX:
        J, df, Y = rk_eval(hooks, p, data, state0, T0, T1, x, integrator, substeps, want_df)
    else:
        J, df, Y = theta_eval(hooks, p, data, state0, T0, T1, x, integrator, substeps, want_df)
    return float(J), (None if df is None else np.array(df, dtype=np.float64)), np.array(Y, dtype=np.float64)
