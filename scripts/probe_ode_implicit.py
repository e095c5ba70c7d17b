"""Timing and accuracy of the implicit integrators (backward Euler, implicit midpoint) of run-time compiled ODE
objectives against classical RK4: python scripts/probe_ode_implicit.py [time|accuracy] [out file].

time      The fishing problem on [0, 12], K = 1024 restarts, nt = 1200, per call with J and df and per value-only
          call: backward Euler and the implicit midpoint rule with 1 substep against RK4 with 1 substep (the
          yardstick, measured in the same process), by HIP events on the library's stream, ROUNDS rounds alternating
          between the programs, REP launches per round after a warm-up; the spread over the rounds is printed with the
          medians.  Run it in several processes.
accuracy  The stiff problem of tests/ode_stiff_problem.py (fast rate kappa = 2000) on [0, 0.96], nt = 24 (h = 0.04 / m),
          the control of the order tests: the relative error of J against the implicit midpoint rule at 64 substeps
          with every control column repeated 8 times (512 substeps per interval of the coarse grid) for Heun, RK4,
          backward Euler and the implicit midpoint rule at m = 1, 2, 4 substeps.
"""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mixed-integer-optimal-control---algorithm-tools_amd"), ROOT,
                os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mioc import native  # noqa: E402
from mioc.ode_device import EXAMPLE_PARAMS, EXAMPLE_STATE0, ODEProgram, example_program  # noqa: E402
from mioc.trm_batch import sos1_levels  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "time"
out = sys.argv[2] if len(sys.argv) > 2 else None
lines = []

if mode == "time":
    K, NT, REP, ROUNDS = 1024, 1200, 10, 7
    T0, T1 = 0.0, 12.0
    y0, par = EXAMPLE_STATE0["fishing"], EXAMPLE_PARAMS["fishing"]
    cases = [("rk4      m=1", "rk4"), ("beuler   m=1", "beuler"), ("midpoint m=1", "midpoint")]
    ctx = native.Context(0)
    ctx.set_levels(sos1_levels())
    x = torch.empty(K, NT, 3, dtype=torch.float64, device="cuda")
    ctx.rand_start_tensor(x, seed=1)
    progs = {name: example_program("fishing", integ, 1) for name, integ in cases}
    Js = {name: torch.empty(K, dtype=torch.float64, device="cuda") for name, _ in cases}
    dfs = {name: torch.empty_like(x) for name, _ in cases}
    torch.cuda.synchronize()
    st = torch.cuda.ExternalStream(ctx.stream())
    calls = {}
    for name, _ in cases:
        calls[name + " J+df"] = (lambda n=name: ctx.ode_program_eval_tensors(progs[n], x, T0, T1, y0, par, Js[n], dfs[n]))
    for name, _ in cases:
        calls[name + " J   "] = (lambda n=name: ctx.ode_program_eval_tensors(progs[n], x, T0, T1, y0, par, Js[n], None))
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
    lines.append(f"probe_ode_implicit time: fishing K={K} nt={NT} (HIP events, {ROUNDS} alternating rounds of {REP} "
                 f"launches after 3 warm-up; outputs finite: {finite})")
    base = {k[-5:]: statistics.median(v) for k, v in ms.items() if k.startswith("rk4")}
    for name, v in ms.items():
        lines.append(f"  {name}  median {statistics.median(v):8.4f} ms   min {min(v):8.4f}   max {max(v):8.4f}   "
                     f"x{statistics.median(v) / base[name[-5:]]:.3f} of rk4")
    for p in progs.values():
        p.close()
    ctx.close()
elif mode == "accuracy":
    import ode_stiff_problem as stiff  # noqa: E402
    from ode_rk_mirror import order_control  # noqa: E402
    NT, T1 = 24, 0.96
    base = np.ascontiguousarray(order_control(NT).T)  # (24, 2)

    def J_of(integ, m, rep=1):
        x = torch.tensor(np.ascontiguousarray(np.repeat(base, rep, axis=0)[None]), dtype=torch.float64, device="cuda")
        J = torch.empty(1, dtype=torch.float64, device="cuda")
        with ODEProgram(stiff.SOURCE, stiff.NY, stiff.NX, len(stiff.PARAMS), integrator=integ, substeps=m) as p:
            ctx.ode_program_eval_tensors(p, x, 0.0, T1, stiff.STATE0, stiff.PARAMS, J, None)
            ctx.synchronize()
        return J.item()

    ctx = native.Context(0)
    ref = J_of("midpoint", 64, 8)
    lines.append(f"probe_ode_implicit accuracy: the stiff problem (kappa = 2000) on [0, {T1}], nt = {NT}, h = 0.04 / m; "
                 f"J of the implicit midpoint rule with 512 substeps per interval = {ref!r}")
    for integ in ("heun", "rk4", "beuler", "midpoint"):
        for m in (1, 2, 4):
            J = J_of(integ, m)
            err = abs(J - ref) / abs(ref) if math.isfinite(J) else math.nan
            lines.append(f"  {integ:8s} m = {m}   J = {J!r:24s}   |J - ref| / |ref| = {err:.3e}")
    ctx.close()
else:
    sys.exit("mode: time or accuracy")

print("\n".join(lines), flush=True)
if out:
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
