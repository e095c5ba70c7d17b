"""Cost of a terminal cost, sampled data and the state output of ODE programs (mioc_ode_program_create_bolza):
  python scripts/probe_ode_bolza.py [K] [nt] [out file]          timing; needs the GPU
  python scripts/probe_ode_bolza.py resources [out file]         registers and scratch per integrator; needs no GPU

Timing: the fishing problem, K restarts (default 1024) of nt steps (default 1200) on [0, 12], with Euler and with RK4
(one substep), four programs each:
  plain      EXAMPLE_SOURCES["fishing"], the program as it was;
  terminal   the same text with E = ((y0 - 1)^2 + (y1 - 1)^2) / 2 and Ey;
  ndata = 2  the same text with the tracking target of G and Gy read from two data columns (all ones: the same J);
  states     the plain text compiled with the state output, d_Y given.
Per call with J and df and per value-only call, by HIP events on the library's stream in one process, ROUNDS rounds
alternating between all the calls, REP launches per round after a warm-up; medians with the min-max spread over the
rounds and the ratio to the plain program of the same integrator.

`resources` takes the source text the library assembles (mioc_ode_program_source) for the problem of
tests/ode_bolza_problem.py (ny = 3, nx = 2, NP = 3, ND = 2, terminal cost, state output), hand-written and derived
hooks, and compiles it offline with the library's flags and -Rpass-analysis=kernel-resource-usage for each of the five
integrators; and the fishing text with and without ND = 2, to show what the per-lane parameter copy costs a
hand-written kernel.
"""
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mixed-integer-optimal-control---algorithm-tools_amd")
sys.path[:0] = [PKG, ROOT]

from mioc.ode_device import (EXAMPLE_PARAMS, EXAMPLE_SHAPES, EXAMPLE_SOURCES, EXAMPLE_STATE0, ODEProgram,  # noqa: E402
                             program_source)

FISH = EXAMPLE_SOURCES["fishing"]
FISH_TERMINAL = FISH + """
__device__ double E(const double *p, double t, const double *y) {
  const double a = y[0] - 1.0, b = y[1] - 1.0;
  return 0.5 * (a * a) + 0.5 * (b * b);
}
__device__ void Ey(const double *p, double t, const double *y, double *ey) {
  ey[0] = y[0] - 1.0;
  ey[1] = y[1] - 1.0;
}
"""
FISH_DATA = FISH.replace("y[0] - 1.0", "y[0] - p[NP]").replace("y[1] - 1.0", "y[1] - p[NP + 1]")
assert FISH_DATA.count("p[NP") == 4


def resources(out):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ode_bolza_problem as bp
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lines = ["probe_ode_bolza resources: the assembled source compiled offline for gfx950 (-O3 -ffp-contract=off "
             "-fno-fast-math)"]
    fish = EXAMPLE_SHAPES["fishing"]
    cases = [(f"bolza problem (3, 2, NP 3, ND 2, E, Y) {label}", bp.SOURCE, (bp.NY, bp.NX, bp.NP), derive, bp.ND,
              True, True) for label, derive in (("hand", False), ("AD  ", True))]
    cases += [("fishing plain                             ", FISH, fish, False, 0, False, False),
              ("fishing ND = 2                            ", FISH_DATA, fish, False, 2, False, False),
              ("fishing terminal                          ", FISH_TERMINAL, fish, False, 0, True, False),
              ("fishing states                            ", FISH, fish, False, 0, False, True)]
    for integrator in ("euler", "heun", "rk4", "beuler", "midpoint"):
        for label, text, shape, derive, ndata, terminal, states in cases:
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "prog.hip")
                with open(path, "w") as f:
                    f.write(program_source(text, *shape, integrator, derive="all" if derive else (), ndata=ndata,
                                           terminal=terminal, states=states))
                r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math",
                                    "--cuda-device-only", "-include", "hip/hip_runtime.h",
                                    "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o",
                                    os.path.join(d, "prog.o")], capture_output=True, text=True, check=True)
            at = r.stderr.index("Function Name: mioc_ode_program_kernel")
            got = {k: re.search(r"\b" + k + r"[^:\n]*: (\d+)", r.stderr[at:]).group(1)
                   for k in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy")}
            lines.append(f"  {integrator:8s} {label}  VGPRs {got['VGPRs']:>3s}  AGPRs {got['AGPRs']:>3s}  "
                         f"SGPRs {got['TotalSGPRs']:>3s}  scratch {got['ScratchSize']} B/lane  "
                         f"waves/SIMD {got['Occupancy']}")
    print("\n".join(lines), flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def timing(K, nt, out):
    import torch

    from mioc import native
    from mioc.trm_batch import sos1_levels
    REP, ROUNDS = 10, 7
    T0, T1 = 0.0, 12.0
    shape = EXAMPLE_SHAPES["fishing"]
    y0, par = EXAMPLE_STATE0["fishing"], EXAMPLE_PARAMS["fishing"]
    variants = {"plain   ": (FISH, {}), "terminal": (FISH_TERMINAL, dict(terminal=True)),
                "ndata=2 ": (FISH_DATA, dict(ndata=2)), "states  ": (FISH, dict(states=True))}
    ctx = native.Context(0)
    ctx.set_levels(sos1_levels())
    x = torch.empty(K, nt, 3, dtype=torch.float64, device="cuda")
    ctx.rand_start_tensor(x, seed=1)
    data = torch.ones(nt, 2, dtype=torch.float64, device="cuda")
    Y = torch.empty(K, nt + 1, shape[0], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.ExternalStream(ctx.stream())
    progs, calls, J, df = {}, {}, {}, {}
    for integrator in ("euler", "rk4"):
        for name, (text, kw) in variants.items():
            key = (integrator, name)
            progs[key] = ODEProgram(text, *shape, integrator=integrator, **kw)
            J[key] = torch.empty(K, dtype=torch.float64, device="cuda")
            df[key] = torch.empty_like(x)
            extra = dict(data=data) if "ndata" in kw else dict(Y=Y) if "states" in kw else {}

            def call(want_df, key=key, extra=extra):
                ctx.ode_program_eval_tensors(progs[key], x, T0, T1, y0, par, J[key], df[key] if want_df else None,
                                             **extra)
            calls[key + ("J+df",)] = lambda call=call: call(True)
            calls[key + ("J   ",)] = lambda call=call: call(False)
    torch.cuda.synchronize()
    for fn in calls.values():
        for _ in range(3):
            fn()
    ctx.synchronize()
    ms = {key: [] for key in calls}
    for _ in range(ROUNDS):
        for key, fn in calls.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record(st)
            for _ in range(REP):
                fn()
            ev[1].record(st)
            ctx.synchronize()
            ms[key].append(ev[0].elapsed_time(ev[1]) / REP)
    # the data columns are all ones, the target of the plain text: the same J and df
    same = all(bool(torch.equal(J[i, "ndata=2 "], J[i, "plain   "])) and
               bool(torch.equal(df[i, "ndata=2 "], df[i, "plain   "])) and
               bool(torch.equal(J[i, "states  "], J[i, "plain   "])) for i in ("euler", "rk4"))
    lines = [f"probe_ode_bolza: fishing K={K} nt={nt} (HIP events, {ROUNDS} alternating rounds of {REP} launches after "
             f"3 warm-up; ndata=2 (all ones) and states give the plain program's J and df bits: {same})"]
    med = {key: statistics.median(v) for key, v in ms.items()}
    for (integrator, name, what), v in ms.items():
        ratio = med[integrator, name, what] / med[integrator, "plain   ", what]
        lines.append(f"  {integrator:5s} {name} {what}  median {med[integrator, name, what]:8.4f} ms   "
                     f"min {min(v):8.4f}   max {max(v):8.4f}   / plain {ratio:.3f}")
    print("\n".join(lines), flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for p in progs.values():
        p.close()
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "resources":
        resources(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    sys.exit(timing(int(sys.argv[1]) if len(sys.argv) > 1 else 1024, int(sys.argv[2]) if len(sys.argv) > 2 else 1200,
                    sys.argv[3] if len(sys.argv) > 3 else None))
