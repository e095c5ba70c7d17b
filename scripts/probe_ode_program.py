"""Timing of a run-time compiled ODE objective against the built-in kernel: python scripts/probe_ode_program.py [K]
[nt] [out file].

The fishing problem, K restarts (default 1024) of nt steps (default 1200) on [0, 12], per call with J and df:
  * k_ode_eval (mioc_ode_eval_device), the yardstick;
  * the program kernel compiled from EXAMPLE_SOURCES["fishing"] (mioc_ode_program_eval_device);
both by HIP events on the library's stream in the same process, ROUNDS rounds alternating between the two, REP
launches per round after a warm-up; the spread over the rounds is printed with the medians.  Also the J-only calls
(the program kernel stores no forward states then), the wall time of mioc_ode_program_create (the first call loads
hiprtc; then three more), and a bit comparison of the two kernels' outputs.
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mixed-integer-optimal-control---algorithm-tools_amd"), ROOT]

import torch  # noqa: E402

from mioc import native  # noqa: E402
from mioc.ode_device import EXAMPLE_PARAMS, EXAMPLE_STATE0, example_program  # noqa: E402
from mioc.trm_batch import sos1_levels  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
nt = int(sys.argv[2]) if len(sys.argv) > 2 else 1200
out = sys.argv[3] if len(sys.argv) > 3 else None
REP, ROUNDS = 10, 7
T0, T1 = 0.0, 12.0

create_s = []
for _ in range(4):
    t0 = time.perf_counter()
    prog = example_program("fishing")
    create_s.append(time.perf_counter() - t0)
    if len(create_s) < 4:
        prog.close()

ctx = native.Context(0)
ctx.set_levels(sos1_levels())
x = torch.empty(K, nt, 3, dtype=torch.float64, device="cuda")
ctx.rand_start_tensor(x, seed=1)
Jb, Jp = (torch.empty(K, dtype=torch.float64, device="cuda") for _ in range(2))
dfb, dfp = torch.empty_like(x), torch.empty_like(x)
torch.cuda.synchronize()
st = torch.cuda.ExternalStream(ctx.stream())
y0, par = EXAMPLE_STATE0["fishing"], EXAMPLE_PARAMS["fishing"]

calls = {
    "k_ode_eval J+df": lambda: ctx.ode_eval_tensors(native.MIOC_ODE_FISHING, x, T0, T1, Jb, dfb),
    "program    J+df": lambda: ctx.ode_program_eval_tensors(prog, x, T0, T1, y0, par, Jp, dfp),
    "k_ode_eval J   ": lambda: ctx.ode_eval_tensors(native.MIOC_ODE_FISHING, x, T0, T1, Jb, None),
    "program    J   ": lambda: ctx.ode_program_eval_tensors(prog, x, T0, T1, y0, par, Jp, None),
}
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
same = bool(torch.equal(Jb, Jp)) and bool(torch.equal(dfb, dfp))
lines = [f"probe_ode_program: fishing K={K} nt={nt} (HIP events, {ROUNDS} alternating rounds of {REP} launches after 3 "
         f"warm-up; outputs bit-identical: {same})"]
for name, v in ms.items():
    lines.append(f"  {name}  median {statistics.median(v):8.4f} ms   min {min(v):8.4f}   max {max(v):8.4f}")
med = {name: statistics.median(v) for name, v in ms.items()}
lines.append(f"  program / k_ode_eval: J+df {med['program    J+df'] / med['k_ode_eval J+df']:.3f}, "
             f"J only {med['program    J   '] / med['k_ode_eval J   ']:.3f}")
lines.append(f"  mioc_ode_program_create wall time: first {create_s[0]:.3f} s (loads hiprtc), then "
             + ", ".join(f"{s:.3f}" for s in create_s[1:]) + " s")
print("\n".join(lines), flush=True)
if out:
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
prog.close()
ctx.close()
sys.exit(0 if same else 1)
