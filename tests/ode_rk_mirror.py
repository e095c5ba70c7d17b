"""Host mirror of the Heun / RK4 schemes of user-defined ODE objectives (include/mioc.h, "Integrators"): a restatement in
Python floats, operation for operation in the documented rounding order, against which test_gpu_ode_integrators.py
compares the device kernel and whose gradient and order test_ode_integrators.py pins.  It drives the hooks of a host
objective (mioc.ode.AbstractODEObjective, e.g. ode_program_problem.FourthObj) with `i` = the control interval and
i2t replaced by the stage time.  Test code: the product never imports it.

  grid      tau = (T1 - T0) / nt, h = tau / m, substep n = i*m + j, t_n = T0 + n*h, stage time t_n + c_s*h
  forward   Y_1 = y_n, Y_s = y_n + (h a_{s,s-1}) k_{s-1};  k_s = F(Y_s), g_s = G(Y_s)
            y_{n+1} = y_n + sum_s (h b_s) k_s;  q_{n+1} = q_n + sum_s (h b_s) g_s;  J = q_{nt*m}
  adjoint   w = 0; per substep, s = S..1: kbar_s = (h b_s) w + (h a_{s+1,s}) Ybar_{s+1};
            Ybar_s = Fy' kbar_s + (h b_s) Gy;  xbar_i += Fu' kbar_s + (h b_s) Gu;  then w += sum_s Ybar_s
  gradient  df[:, i] = xbar_i / tau
"""
import numpy as np

# name -> (c, sub-diagonal a with a[0] unused, b)
TABLEAUX = {
    "heun": ((0.0, 1.0), (0.0, 1.0), (0.5, 0.5)),
    "rk4": ((0.0, 0.5, 0.5, 1.0), (0.0, 0.5, 0.5, 1.0), (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)),
}

# the order tests (CPU and GPU tier): successive error ratios of J under halved h lie in [0.75 * 2^p, 1.35 * 2^p]
ORDER_BANDS = {"heun": (3.0, 5.4), "rk4": (12.0, 21.6)}


def order_control(nt=24, seed=0):
    """The random grid control (nx, nt) of the order tests, on the fourth problem's levels (3 x 2)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 3, nt), rng.integers(0, 2, nt)]).astype(np.float64)


def _at(obj, t):
    """The hooks of a host objective read the time through i2t: make it the stage time."""
    obj.i2t = lambda i: t


def rk_eval(obj, x, integrator, substeps, want_df=True):
    """J and df (nx, nt; None unless want_df) of the control x (nx, nt) under `integrator` with `substeps`."""
    c, a, b = TABLEAUX[integrator]
    S, m = len(c), int(substeps)
    ny, nx, nt = obj.ny, obj.nx, obj.nt
    T0 = obj.T0
    tau = (obj.T1 - obj.T0) / nt
    h = tau / m
    ch = [cs * h for cs in c]
    ha = [as_ * h for as_ in a]
    hb = [bs * h for bs in b]
    x = np.asarray(x, dtype=np.float64)
    y = np.array(obj.state0, dtype=np.float64)
    states = []
    k = [np.zeros(ny) for _ in range(S)]
    g = [0.0] * S
    q = 0.0
    try:
        for i in range(nt):
            xc = x[:, i].copy()
            for j in range(m):
                n = i * m + j
                tn = T0 + float(n) * h
                states.append(y.copy())
                for s in range(S):
                    Y = y.copy() if s == 0 else np.array([y[r] + ha[s] * k[s - 1][r] for r in range(ny)])
                    _at(obj, tn + ch[s])
                    obj.F(k[s], i, Y, xc)
                    g[s] = obj.G(i, Y, xc)
                for r in range(ny):
                    inc = hb[0] * k[0][r]
                    for s in range(1, S):
                        inc = inc + hb[s] * k[s][r]
                    y[r] = y[r] + inc
                inc = hb[0] * g[0]
                for s in range(1, S):
                    inc = inc + hb[s] * g[s]
                q = q + inc
        J = float(q)
        if not want_df:
            return J, None
        df = np.zeros((nx, nt))
        fy, fu, gy, gu = np.zeros((ny, ny)), np.zeros((ny, nx)), np.zeros(ny), np.zeros(nx)  # zeroed once
        w = np.zeros(ny)
        for i in range(nt - 1, -1, -1):
            xc = x[:, i].copy()
            xbar = np.zeros(nx)
            for j in range(m - 1, -1, -1):
                n = i * m + j
                tn = T0 + float(n) * h
                yn = states[n]
                Ys = []
                for s in range(S):  # the stage states again, from the stored y_n
                    Y = yn.copy() if s == 0 else np.array([yn[r] + ha[s] * k[s - 1][r] for r in range(ny)])
                    Ys.append(Y)
                    if s < S - 1:
                        _at(obj, tn + ch[s])
                        obj.F(k[s], i, Y, xc)
                Ybar = np.zeros(ny)
                acc = np.zeros(ny)
                for s in range(S - 1, -1, -1):
                    if s == S - 1:
                        kb = [hb[s] * w[r] for r in range(ny)]
                    else:
                        kb = [hb[s] * w[r] + ha[s + 1] * Ybar[r] for r in range(ny)]
                    _at(obj, tn + ch[s])
                    obj.Fy(fy, i, Ys[s], xc)
                    obj.Gy(gy, i, Ys[s], xc)
                    obj.Fu(fu, i, Ys[s], xc)
                    obj.Gu(gu, i, Ys[s], xc)
                    for cc in range(ny):
                        t = fy[0, cc] * kb[0]
                        for r in range(1, ny):
                            t = t + fy[r, cc] * kb[r]
                        Ybar[cc] = t + hb[s] * gy[cc]
                    for mm in range(nx):
                        t = fu[0, mm] * kb[0]
                        for r in range(1, ny):
                            t = t + fu[r, mm] * kb[r]
                        xbar[mm] = xbar[mm] + (t + hb[s] * gu[mm])
                    for cc in range(ny):
                        acc[cc] = Ybar[cc] if s == S - 1 else acc[cc] + Ybar[cc]
                for cc in range(ny):
                    w[cc] = w[cc] + acc[cc]
            for mm in range(nx):
                df[mm, i] = xbar[mm] / tau
        return J, df
    finally:
        del obj.i2t  # the class's own i2t again
