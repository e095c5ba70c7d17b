"""The mixed trust-region method: continuous controls beside the DP's integer ones, for ODE objectives.

The reference's objectives carry nu continuous controls with pointwise bounds (obj.nu, obj.umin, obj.umax,
HelpFunctions.jl:136-193) and its README announces an algorithm for them, but it has no code for it.  This module
defines one.  A mixed control x has nx = nu + nv rows per time step, rows 0..nu-1 continuous (c),
rows nu..nx-1 integer (v).  Every outer iteration takes

  1. one projected-gradient step in c with v fixed: a backtracking (Armijo) line search whose R candidate step sizes
     s 2^-j are all evaluated at once -- on the device one fan launch, ONE value-only launch of the ODE kernel for
     all R K candidates, one select launch;
  2. one trust-region step in v with c fixed: the inner loop of multi-trust.jl:108-158 on the compact integer rows,
     exactly as TRM_batch runs it (DP, backtrack with per-restart budgets, pred, J_new, accept / halve / stop).

The loop keeps x (the accepted iterate), v_old (its integer rows) and J_old = J(x).  A restart is *final* once
neither part moves: the DP reports pred <= 0 (its stop flag) and the continuous step before it did not reduce J by
more than ctol max(1, |J|); a continuous step that does move clears the stop flag, so the DP runs again at the new c.
The result is J_old + beta TV_p(v_old).

Two quirks of the reference's TRM (mioc.trm.TRM, TRM_batch) are deliberately NOT carried over, because the line
search needs J_old = J(x) to hold: the gradient is never taken at a rejected trial (it is always taken at the
accepted iterate x), and the value returned has the TV of the accepted v, not of the last trial.  An inner loop that
exhausts kmax without accepting simply repeats in the next outer iteration, as in the reference.

``TRM_mixed_batch`` runs K restarts on the device; ``TRM_mixed`` is the same loop for one restart on the host, through
an objective's eval_f / eval_df and a SubproblemSolver, with the fan, the slope and the selection restated in plain
Python loops with exactly the operations of the kernels (include/mioc.h, "Mixed controls"): given bit-equal J and df
the two agree bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

from .iterators import LevelTable
from .objective import eval_df_, eval_f, eval_f_
from .trm import SubproblemSolver, TRM_parameters, TV_p


class MixedParameters:
    """Parameters of the continuous step: the first step size s0, the Armijo constant c1, the number R of candidate
    step sizes s 2^-j tried at once (1..16), the largest step size smax, and ctol: a step has *moved* if it reduces J
    by more than ctol max(1, |J|)."""

    def __init__(self, s0=1.0, c1=1e-4, R=8, smax=1e6, ctol=1e-9):
        self.s0, self.c1, self.R, self.smax, self.ctol = float(s0), float(c1), int(R), float(smax), float(ctol)
        if int(R) != R or not 1 <= self.R <= 16:
            raise ValueError("R must be an integer in 1..16")
        if not (0.0 < self.c1 < 1.0):
            raise ValueError("need 0 < c1 < 1")
        if not (self.s0 > 0.0 and math.isfinite(self.s0)) or not self.smax >= self.s0:
            raise ValueError("need 0 < s0 <= smax, s0 finite")
        if not self.ctol >= 0.0:
            raise ValueError("ctol must not be negative")

    def __repr__(self):
        return f"MixedParameters(s0={self.s0}, c1={self.c1}, R={self.R}, smax={self.smax}, ctol={self.ctol})"


# ---- the kernels' operations, restated (mioc_mixed_fan_device / mioc_mixed_select_device) -------------------------
def fan_host(x, g, lo, hi, s, R, nu, tau):
    """The R candidates of one restart: x, g (nt, nx) and lo, hi (nt, nu) numpy arrays, s the step size.  Returns
    xfan (R, nt, nx) and slope (R,) with the operations and the summation order of k_mixed_fan."""
    nt, nx = x.shape
    xfan = np.empty((R, nt, nx), dtype=np.float64)
    slope = np.empty(R, dtype=np.float64)
    for j in range(R):
        sj = math.ldexp(s, -j)
        cand = np.array(x, dtype=np.float64, copy=True)
        acc = 0.0
        for i in range(nt):
            for m in range(nu):
                xv, gv, l, h = float(x[i, m]), float(g[i, m]), float(lo[i, m]), float(hi[i, m])
                t = xv - sj * gv
                c = l if t < l else (h if t > h else t)
                cand[i, m] = c
                acc = acc + gv * (xv - c)
        xfan[j] = cand
        slope[j] = tau * acc
    return xfan, slope


class MixedState:
    """One restart's entry of the device state block: s, the final and moved flags, jsel, csteps."""

    def __init__(self, s0):
        self.s, self.final, self.moved, self.jsel, self.csteps = float(s0), False, False, 0, 0


def select_host(st, stop, slope, Jfan, J_old, R, c1, smax, ctol):
    """k_mixed_select for one restart: updates ``st`` and returns (the candidate to copy into x or -1, the DP's stop
    flag, J_old)."""
    if st.final:                                  # 1.
        return -1, stop, J_old
    if stop and not st.moved:                     # 2.
        st.final = True
        return -1, stop, J_old
    jsel = -1                                     # 3.
    for j in range(R):
        sl, Jj = float(slope[j]), float(Jfan[j])
        if sl > 0.0 and Jj <= J_old - c1 * sl:
            jsel = j
            break
    moved = False
    if jsel >= 0:
        Jj, s2 = float(Jfan[jsel]), 2.0 * math.ldexp(st.s, -jsel)
        moved = (J_old - Jj) > ctol * max(1.0, abs(J_old))
        J_old = Jj
        st.s = s2 if s2 < smax else smax
        st.csteps += 1
    else:
        st.s = math.ldexp(st.s, -R)
    st.jsel, st.moved = jsel, moved
    if stop:                                      # 4.
        if moved:
            stop = False
        else:
            st.final = True
    return jsel, stop, J_old


# ---- random continuous starts (HelpFunctions.jl:158-193) ------------------------------------------------------------
def cont_noise(K, nu, nt, seed):
    """The Gaussian noise of rand_start_cont, (K, nu, nt) float64 on the CPU: torch's generator seeded with ``seed``
    (not Julia's MersenneTwister stream; a seed reproduces its starts on any device)."""
    import torch
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    return torch.randn(int(K), int(nu), int(nt), generator=gen, dtype=torch.float64)


def rand_start_cont(K, nt, lo, hi, sigma=100.0, seed=0, device="cpu"):
    """rand_func_cont (HelpFunctions.jl:158-193) for K restarts, in torch: Gaussian noise smoothed by the normalised
    kernel exp(-(i - nt/2)^2 / (2 sigma^2)), i = 1..nt -- the reference's centred window of the full convolution, as one
    fp64 matmul with the kernel's Toeplitz matrix --, each row rescaled to [min lo, max hi] and projected onto the
    pointwise bounds.  lo, hi: (nt, nu).  Returns (K, nt, nu) float64 on ``device``."""
    import torch
    dev = torch.device(device)
    lo = torch.tensor(np.asarray(lo, dtype=np.float64), device=dev)
    hi = torch.tensor(np.asarray(hi, dtype=np.float64), device=dev)
    nt = int(nt)
    if nt < 2 or lo.dim() != 2 or lo.shape[0] != nt or lo.shape != hi.shape:
        raise ValueError("need nt >= 2 and lo, hi of shape (nt, nu)")
    nu = lo.shape[1]
    xi = cont_noise(K, nu, nt, seed).to(dev)
    i = torch.arange(1, nt + 1, dtype=torch.float64, device=dev)
    gauss = torch.exp(-((i - nt / 2) ** 2) / (2 * float(sigma) ** 2))
    gauss = gauss / gauss.sum()
    # conv(xi, gauss)[n] = sum_j xi[j] gauss[n - j]; the window starts at floor((nt - 1) / 2) (0-based)
    s0 = (nt - 1) // 2
    t = torch.arange(nt, device=dev)
    d = s0 + t[:, None] - t[None, :]                       # [t, j]: the kernel index n - j
    toep = torch.where((d >= 0) & (d < nt), gauss[d.clamp(0, nt - 1)], torch.zeros((), dtype=torch.float64, device=dev))
    u = xi @ toep.T                                        # (K, nu, nt)
    mn, mx = u.amin(dim=2, keepdim=True), u.amax(dim=2, keepdim=True)
    lo_r, hi_r = lo.amin(dim=0)[None, :, None], hi.amax(dim=0)[None, :, None]
    u = lo_r + (hi_r - lo_r) * (u - mn) / (mx - mn)
    u = torch.minimum(u, hi.T[None])                       # the projection, HelpFunctions.jl:181-190
    u = torch.maximum(u, lo.T[None])
    return u.transpose(1, 2).contiguous()


# ---- one restart on the host ------------------------------------------------------------------------------------------
def TRM_mixed(obj, par=None, cpar=None, x0=None, solver=None, device=0, stats=None):
    """The mixed trust-region method (module docstring) for one restart, on the host.

    obj: an objective with nu >= 1 continuous rows in front of its integer ones (mioc.ode.AbstractODEObjective(...,
    nu, umin, umax)); J and its gradient come from eval_f / eval_f_ / eval_df_.  par: TRM_parameters, cpar:
    MixedParameters.  x0: the (nx, nt) start, its continuous rows within the bounds and its integer rows on the levels.
    ``solver`` defaults to a SubproblemSolver on HIP device ``device`` for the integer rows' levels.  obj.x holds the
    accepted iterate afterwards.  stats: a dict to receive {"iters": outer iterations whose DP ran, "outer": outer
    iterations, "csteps", "jsel": the candidate chosen per outer iteration (-1 none, None: the restart was final),
    "values": J_old + beta TV_p(v_old) after every outer iteration, "stop_cleared": how often a continuous step
    cleared the DP's stop flag, "final"}.  Returns J_old + beta TV_p(v_old)."""
    par = TRM_parameters() if par is None else par
    cpar = MixedParameters() if cpar is None else cpar
    nu, nx, nt = int(obj.nu), int(obj.nx), int(obj.nt)
    if nu < 1:
        raise ValueError("TRM_mixed needs nu >= 1 continuous controls; for nu == 0 use mioc.TRM")
    if x0 is None:
        raise ValueError("TRM_mixed needs a start x0 (nx, nt)")
    tau = float(obj.tau)
    beta, D0, sigma, p, kmax, maxiter = par.beta, par.Delta0, par.sigma, par.p, par.kmax, par.maxiter
    if kmax < 1:
        raise ValueError("kmax must be at least 1")
    R, c1, smax, ctol = cpar.R, cpar.c1, cpar.smax, cpar.ctol
    if solver is None:
        solver = SubproblemSolver(LevelTable(obj.V, obj.iterator), p, beta, device=device)
    lo, hi = np.ascontiguousarray(obj.umin.T), np.ascontiguousarray(obj.umax.T)  # (nt, nu), the device layout
    x = np.array(np.asarray(x0, dtype=np.float64).T, order="C", copy=True)      # (nt, nx), the caller's x0 is kept
    if x.shape != (nt, nx):
        raise ValueError("x0 must have the shape (nx, nt)")
    if not (np.all(x[:, :nu] >= lo) and np.all(x[:, :nu] <= hi)):
        raise ValueError("the continuous rows of x0 must lie within umin, umax")
    B = int(math.floor(D0 / tau))

    def value(xx):
        return eval_f(obj, np.asfortranarray(xx.T))

    def gradient(xx):
        obj.x[:, :] = xx.T
        eval_f_(obj)
        eval_df_(obj)
        return np.ascontiguousarray(obj.df.T)

    v_old = np.asfortranarray(x[:, nu:].T)  # (nv, nt), the solver's layout
    J_old = value(x)
    st = MixedState(cpar.s0)
    stop = False
    iters = cleared = 0
    jsels, values = [], []
    it = 1
    while it <= maxiter:
        # the continuous step at fixed v
        g = gradient(x)
        searched = not st.final and not (stop and not st.moved)  # rules 1 and 2 read no candidate
        if searched:
            xfan, slope = fan_host(x, g, lo, hi, st.s, R, nu, tau)
            Jfan = [value(xfan[j]) for j in range(R)]
        else:
            xfan = slope = Jfan = None
        had_stop = stop
        j, stop, J_old = select_host(st, stop, slope, Jfan, J_old, R, c1, smax, ctol)
        if j >= 0:
            x[:, :nu] = xfan[j][:, :nu]
        cleared += int(had_stop and not stop)
        jsels.append(st.jsel if searched else None)
        # the trust-region step at fixed c (multi-trust.jl:99-158 on the integer rows)
        g = gradient(x)
        df_v = np.asfortranarray(g[:, nu:].T)
        tv_old = TV_p(v_old, p)
        if not stop:
            iters += 1
            solver.bellman(df_v, v_old, B, tau)
            Dk, k, budget = D0, 1, B
            inner = True
            while inner:
                trial, _phi = solver.backtrack(budget)
                x_trial = x.copy()
                x_trial[:, nu:] = np.asarray(trial).T
                int_val, _tvo, tv_new, _ = solver.pred()
                J_new = value(x_trial)
                pred = int_val + beta * (tv_old - tv_new)
                ared = (J_old - J_new) + beta * (tv_old - tv_new)
                if pred <= 0.0:
                    stop, inner = True, False
                elif ared < sigma * pred:
                    Dk = Dk / 2
                    budget = int(math.floor(Dk / tau))
                else:
                    v_old = np.array(trial, dtype=np.float64, order="F", copy=True)
                    J_old, tv_old = J_new, tv_new
                    inner = False
                k += 1
                if k > kmax:
                    inner = False
        x[:, nu:] = v_old.T
        values.append(J_old + beta * TV_p(v_old, p))
        it += 1
        if st.final or (stop and not st.moved):
            break
    obj.x[:, :] = x.T
    if stats is not None:
        stats.update(iters=iters, outer=it - 1, csteps=st.csteps, jsel=jsels, values=values, stop_cleared=cleared,
                     final=st.final)
    return J_old + beta * TV_p(v_old, p)


# ---- K restarts on the device -----------------------------------------------------------------------------------------
def TRM_mixed_batch(problem, par=None, cpar=None, K=None, x0=None, seed=0, device=0, inner_chunk=2,  # noqa: C901
                    stats=None):
    """The mixed trust-region method (module docstring) for K restarts of a mioc.ode_device.MixedODEProblem, with
    every restart's data and control state on the device.

    x0: a (K, nt, nx) float64 CUDA tensor of starts (continuous rows within the bounds, integer rows on the levels), or
    None for K random starts: rand_start_cont for c and the device's rand_func_int (rand_start_tensor) for v, both from
    ``seed``, joined.  inner_chunk: inner iterations enqueued between two read-backs of the control flags
    (mioc_mixed_poll).  stats: a dict to receive {"polls", "outer", "csteps", "jsel" (the candidate accepted last),
    "flags" (1 final, 2 moved), "s"}.  Returns (values (K,) numpy: J_old + beta TV_p(v_old) per restart, x (K, nt, nx)
    CUDA tensor: the accepted iterates, iterations (K,) numpy: outer iterations in which the restart's DP ran)."""
    import torch

    from .native import Context
    from .ode_device import DeviceODEProblem, MixedODEProblem
    from .trm_batch import _inner_loop
    if isinstance(problem, DeviceODEProblem):
        raise ValueError("a DeviceODEProblem has no continuous controls (nu == 0): use mioc.trm_batch.TRM_batch")
    if not isinstance(problem, MixedODEProblem):
        raise ValueError("TRM_mixed_batch takes a mioc.ode_device.MixedODEProblem")
    par = TRM_parameters() if par is None else par
    cpar = MixedParameters() if cpar is None else cpar
    if x0 is None and K is None:
        raise ValueError("give K restarts or the starts x0")
    mp = problem
    mp.check_restarts(K if x0 is None else x0.shape[0])  # a scenario problem: restart k solves scenario k % S
    nu, nx, nt = mp.nu, mp.program.nx, mp.nt
    nv = nx - nu
    beta, D0, sigma, kmax, maxiter = par.beta, par.Delta0, par.sigma, par.kmax, par.maxiter
    if kmax < 1:
        raise ValueError("kmax must be at least 1")
    R, c1, smax, ctol = cpar.R, cpar.c1, cpar.smax, cpar.ctol
    tau = (mp.T1 - mp.T0) / nt
    B = int(math.floor(D0 / tau))
    dev = torch.device("cuda", device)
    f64 = dict(dtype=torch.float64, device=dev)
    ctx = Context(device)
    try:
        ctx.set_levels(LevelTable(mp.V, mp.iterator))
        ctx.set_cost(par.p, beta)
        lo, hi = torch.tensor(mp.lo, **f64), torch.tensor(mp.hi, **f64)
        if x0 is None:
            K = int(K)
            v = torch.empty(K, nt, nv, **f64)
            torch.cuda.current_stream(dev).synchronize()
            ctx.rand_start_tensor(v, seed)
            ctx.synchronize()
            x = torch.cat([rand_start_cont(K, nt, mp.lo, mp.hi, seed=seed, device=dev), v], dim=2).contiguous()
        else:
            x = x0.to(device=dev, dtype=torch.float64).contiguous().clone()
            if x.dim() != 3 or tuple(x.shape[1:]) != (nt, nx):
                raise ValueError(f"x0 must have the shape (K, {nt}, {nx})")
            if not bool(((x[:, :, :nu] >= lo) & (x[:, :, :nu] <= hi)).all()):
                raise ValueError("the continuous rows of x0 must lie within lo, hi")
        K = x.shape[0]

        def evalf(xx, J, df):
            mp.eval_tensors(ctx, xx, J, df)

        v_old = x[:, :, nu:].contiguous()
        g, x_trial = torch.empty_like(x), x.clone()
        df_v, trial_v, v_cur = (torch.empty_like(v_old) for _ in range(3))
        xfan = torch.empty(R, K, nt, nx, **f64)
        slope, Jfan = torch.empty(R, K, **f64), torch.empty(R, K, **f64)
        J_old, J_new, J_scr, tv_u, int_val, tv_o, tv_new, pred = (torch.empty(K, **f64) for _ in range(8))
        budgets = torch.empty(K, dtype=torch.int32, device=dev)
        state = ctx.trm_state_tensor(K)
        mstate = ctx.mixed_state_tensor(K, cpar.s0)
        torch.cuda.current_stream(dev).synchronize()        # every buffer above before the context's stream
        evalf(x, J_old, None)
        polls, it = 0, 1

        def one_trial():  # of the trust-region step in v, as TRM_batch runs it
            ctx.backtrack_batch_budgets_tensors(budgets, trial_v)
            ctx.rows_copy_tensors(x_trial, nu, trial_v, 0, nv)    # join
            ctx.pred_batch_tensors(int_val, tv_o, tv_new, pred)
            evalf(x_trial, J_new, None)
            ctx.trm_inner_end(state, sigma, kmax, tau, B, int_val, tv_new, J_new, J_old, J_scr, tv_u, budgets, trial_v,
                              v_cur, v_old)
        try:
            while it <= maxiter:
                ctx.trm_attach(None)
                evalf(x, None, g)                                     # the continuous step at fixed v
                ctx.mixed_fan_tensors(R, nu, tau, x, g, lo, hi, mstate, xfan, slope)
                evalf(xfan.view(R * K, nt, nx), Jfan, None)           # all R K candidates in one value-only launch
                ctx.mixed_select_tensors(R, nu, c1, smax, ctol, mstate, state, xfan, slope, Jfan, J_old, x)
                evalf(x, None, g)                                     # the gradient at the moved c
                ctx.rows_copy_tensors(df_v, 0, g, nu, nv)             # split
                ctx.rows_copy_tensors(x_trial, 0, x, 0, nu)           # the trials' continuous rows
                ctx.tv_tensors(v_old, tv_u)                           # TV_old = TV of the accepted v
                ctx.trm_outer_begin(state, tv_u, D0, B, budgets)
                ctx.trm_attach(state)
                ctx.bellman_batch_tensors(df_v, v_old, B, tau)
                n, live = _inner_loop(one_trial, lambda: ctx.mixed_poll(mstate, state), kmax, inner_chunk)
                polls += n
                ctx.trm_attach(None)
                ctx.rows_copy_tensors(x, nu, v_old, 0, nv)            # the accepted v back into x
                it += 1
                if not live:
                    break
        finally:
            ctx.trm_attach(None)
        ctx.tv_tensors(v_old, tv_u)
        ctx.synchronize()
        values = (J_old + beta * tv_u).cpu().numpy()
        iters = ctx.trm_state_arrays(state, K)["iters"].astype(np.int64)
        if stats is not None:
            ms = ctx.mixed_state_arrays(mstate, K)
            stats.update(polls=polls, outer=it - 1, csteps=ms["csteps"], jsel=ms["jsel"], flags=ms["flags"], s=ms["s"])
    finally:
        ctx.close()
    return values, x, iters


__all__ = ["MixedParameters", "MixedState", "TRM_mixed", "TRM_mixed_batch", "fan_host", "select_host",
           "rand_start_cont", "cont_noise"]
