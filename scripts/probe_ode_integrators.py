"""Timing and accuracy of the Heun / RK4 integrators of run-time compiled ODE objectives against the reference's
Euler scheme: python scripts/probe_ode_integrators.py [time|accuracy|trm] [out file].

time      The fishing problem on [0, 12], K = 1024 restarts, per call with J and df and per value-only call:
            * the Euler program at nt = 1200 (the yardstick, measured in the same process);
            * Heun and RK4 at nt = 1200 with 1 substep;
            * RK4 at nt = 300 with 4 substeps (as many substeps as the others have steps);
          by HIP events on the library's stream, ROUNDS rounds alternating between the programs, REP launches per
          round after a warm-up; the spread over the rounds is printed with the medians.  Run it in several processes.
accuracy  Van der Pol on [0, 20] with a fixed random SOS1 control, piecewise constant on 256 intervals: the error of J
          against RK4 with 128 substeps per interval (as nt = 512 with 64 substeps, every control column twice: the same
          substep grid; the problem is autonomous) for the reference scheme at nt = 256 * {1, 4, 16, 64} (columns
          repeated) and for Heun and RK4 at nt = 256 with 1, 2, 4 substeps.
trm       Wall time of TRM_batch on van der Pol, K = 8 starts, beta = 0.1, Delta0 = 0.25, p = Inf, maxiter = 5, kmax = 5
          (the C3 preset's cost): the Euler program at nt = 16384 against RK4 with 4 substeps at nt = 256; one warm-up
          run, then three timed runs of each, alternating.  Start k is the damped control (c = 0.75) everywhere but on
          [2.5 k, 2.5 k + 0.625), where it is c = -1: the same function of time on both grids, and bounded (random
          starts are not: with c = -2 held for long the oscillator's true solution blows up in finite time).
"""
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mixed-integer-optimal-control---algorithm-tools_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mioc  # noqa: E402
from mioc import native  # noqa: E402
from mioc.ode_device import EXAMPLE_PARAMS, EXAMPLE_STATE0, example_problem, example_program  # noqa: E402
from mioc.trm_batch import TRM_batch, sos1_levels  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "time"
out = sys.argv[2] if len(sys.argv) > 2 else None
lines = []

if mode == "time":
    K, REP, ROUNDS = 1024, 10, 7
    T0, T1 = 0.0, 12.0
    y0, par = EXAMPLE_STATE0["fishing"], EXAMPLE_PARAMS["fishing"]
    cases = [("euler nt=1200    ", "euler", 1, 1200), ("heun  nt=1200 m=1", "heun", 1, 1200),
             ("rk4   nt=1200 m=1", "rk4", 1, 1200), ("rk4   nt=300  m=4", "rk4", 4, 300)]
    ctx = native.Context(0)
    ctx.set_levels(sos1_levels())
    progs, xs, Js, dfs = {}, {}, {}, {}
    for name, integ, m, nt in cases:
        progs[name] = example_program("fishing", integ, m)
        if nt not in xs:
            xs[nt] = torch.empty(K, nt, 3, dtype=torch.float64, device="cuda")
            ctx.rand_start_tensor(xs[nt], seed=1)
        Js[name] = torch.empty(K, dtype=torch.float64, device="cuda")
        dfs[name] = torch.empty_like(xs[nt])
    torch.cuda.synchronize()
    st = torch.cuda.ExternalStream(ctx.stream())
    calls = {}
    for name, integ, m, nt in cases:
        calls[name + " J+df"] = (lambda n=name, t=nt: ctx.ode_program_eval_tensors(progs[n], xs[t], T0, T1, y0, par,
                                                                                   Js[n], dfs[n]))
    for name, integ, m, nt in cases:
        calls[name + " J   "] = (lambda n=name, t=nt: ctx.ode_program_eval_tensors(progs[n], xs[t], T0, T1, y0, par,
                                                                                   Js[n], None))
    for fn in calls.values():
        for _ in range(3):
            fn()
    ctx.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, fn in calls.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record(st)
            for _ in range(REP):
                fn()
            ev[1].record(st)
            ctx.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]) / REP)
    finite = all(bool(torch.isfinite(Js[n]).all()) and bool(torch.isfinite(dfs[n]).all()) for n in Js)
    lines.append(f"probe_ode_integrators time: fishing K={K} (HIP events, {ROUNDS} alternating rounds of {REP} launches "
                 f"after 3 warm-up; outputs finite: {finite})")
    base = {k[-5:]: statistics.median(v) for k, v in ms.items() if k.startswith("euler")}
    for name, v in ms.items():
        lines.append(f"  {name}  median {statistics.median(v):8.4f} ms   min {min(v):8.4f}   max {max(v):8.4f}   "
                     f"x{statistics.median(v) / base[name[-5:]]:.3f} of euler")
    for p in progs.values():
        p.close()
    ctx.close()
elif mode == "accuracy":
    NI, T0, T1 = 256, 0.0, 20.0
    y0, par = EXAMPLE_STATE0["vanderpol"], EXAMPLE_PARAMS["vanderpol"]
    rng = np.random.default_rng(1)
    base = np.eye(3)[rng.integers(0, 3, size=NI)]  # (256, 3), SOS1

    def J_of(integ, m, rep):
        x = torch.tensor(np.ascontiguousarray(np.repeat(base, rep, axis=0)[None]), dtype=torch.float64, device="cuda")
        J = torch.empty(1, dtype=torch.float64, device="cuda")
        with example_program("vanderpol", integ, m) as p:
            ctx.ode_program_eval_tensors(p, x, T0, T1, y0, par, J, None)
            ctx.synchronize()
        return J.item()

    ctx = native.Context(0)
    ref = J_of("rk4", 64, 2)
    lines.append(f"probe_ode_integrators accuracy: vanderpol on [0, 20], a random SOS1 control on {NI} intervals (seed 1); "
                 f"J of RK4 with 128 substeps per interval = {ref!r}")
    for rep in (1, 4, 16, 64):
        lines.append(f"  reference Euler / trapezoid  nt = {NI * rep:6d}            |J - ref| = "
                     f"{abs(J_of('euler', 1, rep) - ref):.3e}")
    for integ in ("heun", "rk4"):
        for m in (1, 2, 4):
            lines.append(f"  {integ:4s}                         nt = {NI:6d}, m = {m}     |J - ref| = "
                         f"{abs(J_of(integ, m, 1) - ref):.3e}")
    ctx.close()
elif mode == "trm":
    K = 8
    parm = mioc.TRM_parameters(beta=0.1, Delta0=0.25, p=math.inf, maxiter=5, kmax=5)
    probs = {"euler nt=16384    ": example_problem("vanderpol", nt=16384),
             "rk4   nt=256   m=4": example_problem("vanderpol", nt=256, integrator="rk4", substeps=4)}

    def starts(nt):
        x = torch.zeros(K, nt, 3, dtype=torch.float64, device="cuda")
        x[:, :, 1] = 1.0
        for k in range(K):
            a, b = (4 * k * nt) // 32, ((4 * k + 1) * nt) // 32
            x[k, a:b, 1], x[k, a:b, 0] = 0.0, 1.0
        return x

    x0 = {n: starts(prob.nt) for n, prob in probs.items()}
    wall = {n: [] for n in probs}
    info, failed = {}, {}
    for rnd in range(4):  # round 0 warms up
        for n, prob in probs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                vals, u, iters = TRM_batch(prob, parm, x0=x0[n])
            except native.MiocNativeError as e:  # e.g. a trial whose states overflow: NaN passes the reference's test
                failed[n] = str(e)
                continue
            torch.cuda.synchronize()
            if rnd:
                wall[n].append(time.perf_counter() - t0)
            info[n] = (float(np.min(vals)), float(np.median(vals)), iters.tolist())
    lines.append(f"probe_ode_integrators trm: vanderpol, TRM_batch K={K} beta=0.1 Delta0=0.25 p=Inf maxiter=5 kmax=5 "
                 f"(wall time of the whole call, 3 runs after a warm-up)")
    for n in probs:
        if n in failed:
            lines.append(f"  {n}  failed: {failed[n]}")
            continue
        lines.append(f"  {n}  {min(wall[n]):8.4f} .. {max(wall[n]):8.4f} s   values min {info[n][0]:.6f} median "
                     f"{info[n][1]:.6f}   iterations {info[n][2]}")
    for prob in probs.values():
        prob.program.close()
else:
    sys.exit("mode: time, accuracy or trm")

print("\n".join(lines), flush=True)
if out:
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
