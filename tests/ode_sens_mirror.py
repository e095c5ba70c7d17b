"""Host mirror of the sensitivities of user-defined ODE objectives (include/mioc.h, "Sensitivities"): the Heun / RK4 body
and the backward Euler / midpoint body of csrc/mioc_ode_skeleton.h with dJ/dparams and dJ/dstate0, restated in Python
floats operation for operation in the documented rounding order.  test_gpu_ode_sens.py compares the device kernels with
it; test_ode_sens.py pins its gradients against differences of its own J and its known answers.  Test code: it imports
the helpers of ode_bolza_mirror.py and nothing of the product.

A problem is a namespace of Python callables as in ode_bolza_mirror.py, with three more that write only the entries
that are not structurally zero (the outputs are zeroed once per evaluation):
  Fp(p_ext, i, t, y, x, fp)   fp[r][e] = dF_r/dp_e      Gp(.., gp)   gp[e] = dG/dp_e      Ep(p_ext, t, y, ep)
for e < NP = len(p) only: the data entries behind the parameters are not differentiated.

``sens_eval`` returns (J, df (nt, nx), Jp (NP,), Jy0 (ny,)); ``sens_eval_scen`` evaluates K restarts of S scenarios,
restart q with scenario q % S's parameters and state0.

WRONG names the wrong versions of the two new update lines that the tests must be able to tell from the right one;
``wrong=<name>`` evaluates that version (J and df are never affected).
"""
import math

import numpy as np

from ode_bolza_mirror import NEWTON_MAX, NEWTON_TOL, DBL_MAX, TABLEAUX, THETA, _div, _pe, _zeros, solve

WRONG = (
    "pbar_reset",        # pbar set to 0.0 at the start of every interval's backward sweep, like xbar
    "gp_unweighted",     # gp added without its (b_s h) / h weight
    "ep_dropped",        # pbar starts from 0.0 although there is a terminal cost
    "fp_transposed",     # fp[e][r] in place of fp[r][e]
    "kbar_wrong_stage",  # Heun / RK4: kbar of the stage handled before; theta: the right-hand side in place of mu
    "w_early",           # Jy0 read before the last substep of the sweep (substep 0) has updated w
    "data_differentiated",  # the data entry d0 carries the tangent of parameter 0
    "scen_div",          # restart q takes the parameters of scenario q / S (sens_eval_scen only)
)


def _pbar_add(pbar, fp, gp, v, wgt, wrong, extra=None):
    """pbar[e] = pbar[e] + (((fp[0][e]*v[0] + fp[1][e]*v[1]) + ...) + wgt*gp[e]); extra: (fd, gd) of the data entry."""
    ny = len(v)
    for e in range(len(pbar)):
        col = [fp[e][r] for r in range(ny)] if wrong == "fp_transposed" else [fp[r][e] for r in range(ny)]
        g = gp[e]
        if extra is not None and e == 0:
            col = [col[r] + extra[0][r] for r in range(ny)]
            g = g + extra[1]
        t = col[0] * v[0]
        for r in range(1, ny):
            t = t + col[r] * v[r]
        pbar[e] = pbar[e] + (t + (g if wrong == "gp_unweighted" else wgt * g))


def _data_terms(hooks, wrong, pe, i, t, Ys, xc, ny):
    if wrong != "data_differentiated":
        return None
    fd = _zeros(ny)
    hooks.Fd(pe, i, t, Ys, xc, fd)
    return fd, hooks.Gd(pe, i, t, Ys, xc)


def _pbar_start(hooks, pe, tend, y, NP, wrong):
    pbar = _zeros(NP)
    if hooks.E is not None and wrong != "ep_dropped":
        ep = _zeros(NP)
        hooks.Ep(pe, tend, y, ep)
        pbar = list(ep)
    return pbar


def rk_sens(hooks, p, data, state0, T0, T1, x, integrator, substeps, wrong=None):
    """Heun / classical RK4 with substeps (kBodyRK with MIOC_SENS)."""
    c, a, b = TABLEAUX[integrator]
    S, ms, NP = len(c), int(substeps), len(p)
    x = [[float(v) for v in row] for row in x]
    nt, nx, ny = len(x), len(x[0]), len(state0)
    tau = (T1 - T0) / nt
    h = tau / ms
    ch = [cs * h for cs in c]
    ha = [as_ * h for as_ in a]
    hb = [bs * h for bs in b]
    y = [float(v) for v in state0]
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
    tend = T0 + float(nt * ms) * h
    J = q
    if hooks.E is not None:
        J = q + hooks.E(pe, tend, y)
    df = _zeros(nt, nx)
    fy, fu, gy, gu = _zeros(ny, ny), _zeros(ny, nx), _zeros(ny), _zeros(nx)  # zeroed once
    w = _zeros(ny)
    if hooks.E is not None:
        ey = _zeros(ny)
        hooks.Ey(pe, tend, y, ey)
        w = list(ey)
    fp, gp = _zeros(ny, NP), _zeros(NP)  # zeroed once
    pbar = _pbar_start(hooks, pe, tend, y, NP, wrong)
    w_before_last = list(w)
    for i in range(nt - 1, -1, -1):
        xc = x[i]
        pe = _pe(p, data, i)
        xbar = _zeros(nx)
        if wrong == "pbar_reset":
            pbar = _zeros(NP)
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
            kb_before = None
            for s in range(S - 1, -1, -1):
                if s == S - 1:
                    kb = [hb[s] * w[r] for r in range(ny)]
                else:
                    kb = [hb[s] * w[r] + ha[s + 1] * Ybar[r] for r in range(ny)]
                hooks.Fy(pe, i, tn + ch[s], Ys[s], xc, fy)
                hooks.Gy(pe, i, tn + ch[s], Ys[s], xc, gy)
                hooks.Fu(pe, i, tn + ch[s], Ys[s], xc, fu)
                hooks.Gu(pe, i, tn + ch[s], Ys[s], xc, gu)
                hooks.Fp(pe, i, tn + ch[s], Ys[s], xc, fp)
                hooks.Gp(pe, i, tn + ch[s], Ys[s], xc, gp)
                v = kb_before if wrong == "kbar_wrong_stage" and kb_before is not None else kb
                _pbar_add(pbar, fp, gp, v, hb[s], wrong, _data_terms(hooks, wrong, pe, i, tn + ch[s], Ys[s], xc, ny))
                kb_before = kb
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
            w_before_last = list(w)
            for cc in range(ny):
                w[cc] = w[cc] + acc[cc]
        for m in range(nx):
            df[i][m] = _div(xbar[m], tau)
    return J, df, pbar, (w_before_last if wrong == "w_early" else list(w))


def theta_sens(hooks, p, data, state0, T0, T1, x, integrator, substeps, wrong=None):
    """Backward Euler / implicit midpoint with substeps (kBodyTheta with MIOC_SENS); a failed Newton iteration gives NaN
    in J and in every entry of df, Jp and Jy0."""
    theta, ms, NP = THETA[integrator], int(substeps), len(p)
    x = [[float(v) for v in row] for row in x]
    nt, nx, ny = len(x), len(x[0]), len(state0)
    tau = (T1 - T0) / nt
    h = tau / ms
    th = theta * h
    thh = th * h
    y = [float(v) for v in state0]
    stages = []
    kv, f = _zeros(ny), _zeros(ny)
    fy = _zeros(ny, ny)  # zeroed once per evaluation
    q = 0.0
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
                return math.nan, [[math.nan] * nx for _ in range(nt)], [math.nan] * NP, [math.nan] * ny
            Ys = [y[r] + th * kv[r] for r in range(ny)]
            stages.append(Ys)
            q = q + h * hooks.G(pe, i, ts, Ys, xc)
            y = [y[r] + h * kv[r] for r in range(ny)]
    tend = T0 + float(nt * ms) * h
    J = q
    if hooks.E is not None:
        J = q + hooks.E(pe, tend, y)
    df = _zeros(nt, nx)
    fu, gy, gu = _zeros(ny, nx), _zeros(ny), _zeros(nx)  # zeroed once, fy as the forward sweep left it
    w = _zeros(ny)
    if hooks.E is not None:
        ey = _zeros(ny)
        hooks.Ey(pe, tend, y, ey)
        w = list(ey)
    fp, gp = _zeros(ny, NP), _zeros(NP)  # zeroed once
    pbar = _pbar_start(hooks, pe, tend, y, NP, wrong)
    w_before_last = list(w)
    for i in range(nt - 1, -1, -1):
        xc = x[i]
        pe = _pe(p, data, i)
        xbar = _zeros(nx)
        if wrong == "pbar_reset":
            pbar = _zeros(NP)
        for j in range(ms - 1, -1, -1):
            n = i * ms + j
            ts = (T0 + float(n) * h) + th
            Ys = stages[n]
            hooks.Fy(pe, i, ts, Ys, xc, fy)
            hooks.Gy(pe, i, ts, Ys, xc, gy)
            kb = [h * w[r] + thh * gy[r] for r in range(ny)]
            rhs = list(kb)
            A = [[(1.0 if r == c else 0.0) - th * fy[c][r] for c in range(ny)] for r in range(ny)]
            mu = solve(A, kb)
            hooks.Fu(pe, i, ts, Ys, xc, fu)
            hooks.Gu(pe, i, ts, Ys, xc, gu)
            hooks.Fp(pe, i, ts, Ys, xc, fp)
            hooks.Gp(pe, i, ts, Ys, xc, gp)
            _pbar_add(pbar, fp, gp, rhs if wrong == "kbar_wrong_stage" else mu, h, wrong,
                      _data_terms(hooks, wrong, pe, i, ts, Ys, xc, ny))
            for m in range(nx):
                t = fu[0][m] * mu[0]
                for r in range(1, ny):
                    t = t + fu[r][m] * mu[r]
                xbar[m] = xbar[m] + (t + h * gu[m])
            w_before_last = list(w)
            for c in range(ny):
                t = fy[0][c] * mu[0]
                for r in range(1, ny):
                    t = t + fy[r][c] * mu[r]
                w[c] = w[c] + (t + h * gy[c])
        for m in range(nx):
            df[i][m] = _div(xbar[m], tau)
    return J, df, pbar, (w_before_last if wrong == "w_early" else list(w))


def sens_eval(hooks, p, data, state0, T0, T1, x, integrator, substeps=1, wrong=None):
    """(J, df (nt, nx), Jp (NP,), Jy0 (ny,)) under Heun, RK4, backward Euler or the midpoint rule."""
    body = rk_sens if integrator in TABLEAUX else theta_sens
    J, df, Jp, Jy0 = body(hooks, [float(v) for v in p], data, state0, T0, T1, x, integrator, substeps, wrong)
    return float(J), np.array(df, dtype=np.float64), np.array(Jp, dtype=np.float64), np.array(Jy0, dtype=np.float64)


def sens_eval_scen(hooks, params, data, state0, T0, T1, x, integrator, substeps=1, wrong=None):
    """K restarts x (K, nt, nx) of S scenarios params (S, NP), state0 (S, ny); data shared.  Restart q is evaluated with
    scenario q % S's values.  Returns (J (K,), df (K, nt, nx), Jp (K, NP), Jy0 (K, ny))."""
    S = len(state0)
    out = []
    for q in range(len(x)):
        sc = (q // S) % S if wrong == "scen_div" else q % S
        out.append(sens_eval(hooks, params[sc], data, state0[sc], T0, T1, x[q], integrator, substeps,
                             None if wrong == "scen_div" else wrong))
    return tuple(np.array([o[n] for o in out]) for n in range(4))
