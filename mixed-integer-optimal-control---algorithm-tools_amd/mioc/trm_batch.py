"""Multi-start TRM with every restart's data and its control state on the device.

The control flow is multi-trust.jl:53-170 per restart, run for K restarts in lock step:

  outer iteration   TV_old = TV_p(u), ∇f = eval_df!(u)                       multi-trust.jl:99-103
  inner iteration   bellman_TRM! (first) or eval_u_TRM! at B_new (halved)    :108-114
                    int_val, TV_new                                           :117-126  (mioc_pred_batch_device)
                    J_new = eval_f!(u), pred, ared, stop / halve / accept     :124-158  (mioc_trm_inner_end_device)
  return            J + β·TV_p(u)                                            :169

Device kernels do all O(nt) work: the random starts (mioc_rand_start_device, HelpFunctions.jl:204-225), the ODE
objective and adjoint gradient (mioc_ode_eval_device, ODEObjective.jl:125-184; for a user-defined ODE objective the
kernel compiled from its hooks, mioc.ode_device) or the PDE heat objective's
(mioc_heat_eval_device, PDEObjective.jl:129-199) or the convolution objective's (mioc_conv_eval_device,
example_convolution.jl:128-141), the DP and backtrack with one budget per restart after halving
(mioc_backtrack_batch_budgets_device), pred and TV_p -- and the control itself: Δᵏ, k, the inner / halved / stopped
flags, the decision, obj.x = trial, the accept bookkeeping and the next budgets live in a device state block
(mioc_trm_outer_begin_device / mioc_trm_inner_end_device).  Everything is enqueued on the context's stream; the
host enqueues inner iterations in chunks and reads back two flags (any restart still in its inner loop, any restart
not stopped) once per chunk (mioc_trm_poll) -- with the default chunk of 2 that is one read-back per outer
iteration whenever every inner loop ends within two trials.  Kernels of an inner iteration that no restart needs
return at once (the state's gate word, mioc_trm_attach).  Restarts that left their inner loop are ignored by the
state update, so every restart follows exactly the sequence of the single-restart loop, including its quirks: the
gradient of the next outer iteration is taken at the last trial u (obj.x), accepted or not, and a stop returns
J_old + β·TV_p(u_trial).

``TRM_batch`` knows a problem by its members, not by its type (its docstring lists them): HeatProblem, ConvProblem and
DeviceODEProblem have them, and so can any other object.
"""
from __future__ import annotations

import math

import numpy as np

from .iterators import LevelTable, bounded_sum_iterator
from .native import (MIOC_ODE_DOUBLETANK, MIOC_ODE_FISHING, MIOC_ODE_VANDERPOL, Context)

# the reference's ODE examples: (problem code, default nt, T0, T1) -- example_fishing.jl, example_doubletank.jl,
# example_vanderpol.jl; all three are SOS1 over three binary controls
PROBLEMS = {"fishing": (MIOC_ODE_FISHING, 1200, 0.0, 12.0), "doubletank": (MIOC_ODE_DOUBLETANK, 1000, 0.0, 10.0),
            "vanderpol": (MIOC_ODE_VANDERPOL, 2000, 0.0, 20.0)}


def sos1_levels():
    V = [[0, 1], [0, 1], [0, 1]]
    return LevelTable(V, bounded_sum_iterator(V, 1, 1))


class _ExampleProblem:
    """One of the reference's three ODE examples (PROBLEMS[name]) as a problem of TRM_batch."""
    fixes_nt = False

    def __init__(self, name):
        self.code, self.nt, self.T0, self.T1 = PROBLEMS[name]

    def level_table(self):
        return sos1_levels()

    def setup(self, ctx):
        """Nothing: the example's constants are the kernel's."""

    def eval_tensors(self, ctx, x, J=None, df=None):
        ctx.ode_eval_tensors(self.code, x, self.T0, self.T1, J, df)

    def check_restarts(self, K):
        """Any number of restarts."""


def _inner_loop(trial, poll, kmax, inner_chunk):
    """The inner iterations of one outer iteration: ``trial()`` enqueues one, ``poll()`` synchronises and returns (any
    restart still inside its inner loop, the caller's second flag).  At most kmax trials are enqueued, inner_chunk of
    them between two polls, none after a poll that finds no restart inside.  Returns (polls made, the last poll's
    second flag: True if there was none)."""
    done, polls, flag = 0, 0, True
    while done < kmax:
        chunk = min(inner_chunk, kmax - done)
        for _ in range(chunk):
            trial()
        done += chunk
        inner, flag = poll()  # the one read-back per chunk
        polls += 1
        if not inner:
            break
    return polls, flag


def TRM_batch(problem, par, K=None, x0=None, seed=0, nt=None, device=0, log=None, inner_chunk=2, stats=None):
    """Run TRM (multi-trust.jl:53-170) for K restarts of a problem on the device.

    problem: any object with the members
      nt, T0, T1        the default number of steps and the horizon;
      level_table()     the LevelTable of its controls;
      fixes_nt          False, or the reason why ``nt`` cannot differ from problem.nt (the message raised);
      setup(ctx)        hands its data to the native.Context (may do nothing);
      eval_tensors(ctx, x, J, df)   enqueues J (K,) and / or df (K, nt, nx) at the controls x (K, nt, nx);
      check_restarts(K) ValueError if K restarts cannot be run (may do nothing)
    -- a mioc.heat.HeatProblem (example_heat.jl: 6 x 6 product levels, gradient from mioc_heat_eval_device), a
    mioc.conv.ConvProblem (example_convolution.jl: one control, levels -2..2, gradient from mioc_conv_eval_device), a
    mioc.ode_device.DeviceODEProblem (a user-defined ODE objective: levels from its V and iterator, gradient from its
    compiled hooks) -- or one of the strings "fishing" / "doubletank" / "vanderpol" = _ExampleProblem(name) and
    "convolution" = ConvProblem(nt = nt or 2048).
    x0: a (K, nt, nx) float64 CUDA tensor of starts, or None for K device random starts (rand_func_int with `seed`).
    log: a list to receive (inner iteration, decisions (K,)) after every inner iteration (debugging: one stream
    synchronisation each).  inner_chunk: inner iterations enqueued between two read-backs of the control flags.
    stats: a dict to receive {"polls": read-backs, "outer": outer iterations, "algo": the DP that served the last
    bellman (mioc_last_algo), "diagnostics": its counters (mioc_diagnostics)}.
    Returns (values (K,) numpy: J + β·TV_p(u) per restart, u (K, nt, nx) CUDA tensor: obj.x of each restart,
    iterations (K,) numpy)."""
    import torch
    if isinstance(problem, str):
        from .conv import ConvProblem
        problem = ConvProblem(nt=nt or 2048) if problem == "convolution" else _ExampleProblem(problem)
    problem.check_restarts(K if x0 is None else x0.shape[0])  # a scenario problem: S divides K
    if problem.fixes_nt and nt is not None and int(nt) != problem.nt:
        raise ValueError(problem.fixes_nt)
    T0, T1 = problem.T0, problem.T1
    lt = problem.level_table()
    dev = torch.device("cuda", device)
    ctx = Context(device)
    try:
        problem.setup(ctx)
        ctx.set_levels(lt)
        ctx.set_cost(par.p, par.beta)
        if x0 is None:
            nt = problem.nt if nt is None else int(nt)
            u = torch.empty(int(K), nt, lt.M, dtype=torch.float64, device=dev)
            ctx.rand_start_tensor(u, seed)
        else:
            u = x0.to(device=dev, dtype=torch.float64).contiguous().clone()
        K, nt, _ = u.shape
        tau = (T1 - T0) / nt
        beta, D0, sigma, kmax, maxiter = par.beta, par.Delta0, par.sigma, par.kmax, par.maxiter
        B = int(math.floor(D0 / tau))  # multi-trust.jl:69

        f64 = dict(dtype=torch.float64, device=dev)
        ctx.synchronize()                      # u (random starts) from the context's stream before torch reads it
        u_old = u.clone()
        J_old = torch.empty(K, **f64)
        tv_u = torch.empty(K, **f64)
        J = torch.full((K,), math.inf, **f64)
        df = torch.empty_like(u)
        trial = torch.empty_like(u)
        int_val, tv_o, tv_new, pred = (torch.empty(K, **f64) for _ in range(4))
        J_new = torch.empty(K, **f64)
        dec = torch.empty(K, dtype=torch.int32, device=dev)
        budgets = torch.empty(K, dtype=torch.int32, device=dev)
        state = ctx.trm_state_tensor(K)
        torch.cuda.current_stream(dev).synchronize()  # every buffer above (torch's stream) before the context's stream
        problem.eval_tensors(ctx, u, J_old, None)
        ctx.tv_tensors(u, tv_u)                # TV of the current u; afterwards every trial's TV_new
        ctx.trm_attach(state)
        polls, it = 0, 1

        def one_trial():
            ctx.backtrack_batch_budgets_tensors(budgets, trial)
            ctx.pred_batch_tensors(int_val, tv_o, tv_new, pred)
            problem.eval_tensors(ctx, trial, J_new, None)
            ctx.trm_inner_end(state, sigma, kmax, tau, B, int_val, tv_new, J_new, J_old, J, tv_u, budgets, trial, u,
                              u_old, decision=dec if log is not None else None)
            if log is not None:                                     # debugging: one synchronisation per trial
                st = ctx.trm_state_arrays(state, K)
                d = dec.cpu().numpy().copy()
                log.append((it, st["k"].copy(), st["Dk"].copy(), None, d, d >= 0))
        try:
            while it <= maxiter:
                ctx.trm_outer_begin(state, tv_u, D0, B, budgets)    # TV_old, Δᵏ, k, inner, :99-107
                problem.eval_tensors(ctx, u, None, df)              # ∇f at obj.x = u, :102-103
                ctx.bellman_batch_tensors(df, u_old, B, tau)
                n, active = _inner_loop(one_trial, lambda: ctx.trm_poll(state), kmax, inner_chunk)
                polls += n
                it += 1
                if not active:                                      # every restart stopped, :96
                    break
        finally:
            ctx.trm_attach(None)
        problem.eval_tensors(ctx, u, None, df)                      # final derivative, :166-167
        ctx.synchronize()                                           # the context's results before torch reads them
        values = (J + beta * tv_u).cpu().numpy()                    # J + β·TV_p(u, p), :169
        iters = ctx.trm_state_arrays(state, K)["iters"].astype(np.int64)
        if stats is not None:
            stats.update(polls=polls, outer=it - 1, algo=ctx.last_algo(), diagnostics=ctx.diagnostics())
    finally:
        ctx.close()
    return values, u, iters
