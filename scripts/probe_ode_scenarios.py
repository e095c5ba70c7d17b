"""Cost of scenarios for ODE programs (mioc_ode_program_create_scen; include/mioc.h, "Scenarios"):
  python scripts/probe_ode_scenarios.py [K] [nt] [out file]          timing; needs the GPU
  python scripts/probe_ode_scenarios.py resources [out file]         registers and scratch per program; needs no GPU
profiles/ode_scenarios_probe.txt is the two outputs, one after the other, and the lines of the one-column-ahead variant
of the per-scenario data loads, measured by this script while the skeleton had that variant.

Timing: the fishing problem with derived hooks (EXAMPLE_SOURCES_AD), K restarts (default 1024) of nt steps (default
1200) on [0, 12], with Euler and with RK4 (one substep), these programs each:
  scen=0              the program without scenarios, state0 and params by value: the baseline;
  scen=1 S=1          compiled for scenarios, one scenario (every lane loads the same doubles);
  scen=1 S=K          K distinct scenarios (state0 + 0.05 N(0,1), params (1 + 0.05 U(-1,1)));
  nd=2 scen=0         the tracking target of G read from two shared data columns: the baseline of the data lines;
  nd=2 scen=1 S=K     distinct state0 and params, the shared data table (scalar loads);
  nd=2 scen=3 S=K     per-scenario data (1 + 0.05 N(0,1)): every lane loads its own row.
Per call with J and df and per value-only call, by HIP events on the library's stream in one process, ROUNDS rounds
alternating between all the calls, REP launches per round after a warm-up; medians with the min-max spread over the
rounds and the ratio to the baseline of the same integrator (scen=0, or nd=2 scen=0 for the data lines).

`resources` compiles the text the library assembles for each of these programs offline with the library's flags and
-Rpass-analysis=kernel-resource-usage.
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

from mioc.ode_device import (EXAMPLE_PARAMS, EXAMPLE_SHAPES, EXAMPLE_SOURCES_AD, EXAMPLE_STATE0, ODEProgram,  # noqa: E402
                             program_source)

FISH = EXAMPLE_SOURCES_AD["fishing"]
FISH_DATA = FISH.replace("y[0] - 1.0", "y[0] - p[NP]").replace("y[1] - 1.0", "y[1] - p[NP + 1]")
assert FISH_DATA.count("p[NP") == 2
# name: (text, ndata, scenarios, baseline)
PROGRAMS = {"scen=0           ": (FISH, 0, False, None),
            "scen=1           ": (FISH, 0, True, "scen=0           "),
            "nd=2 scen=0      ": (FISH_DATA, 2, False, None),
            "nd=2 scen=1      ": (FISH_DATA, 2, True, "nd=2 scen=0      "),
            "nd=2 scen=3      ": (FISH_DATA, 2, "data", "nd=2 scen=0      ")}
INTEGRATORS = ("euler", "rk4")


def resources(out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lines = ["probe_ode_scenarios resources: the assembled source (fishing, derived hooks) compiled offline for gfx950 "
             "(-O3 -ffp-contract=off -fno-fast-math)"]
    for integrator in INTEGRATORS:
        for name, (text, ndata, scen, _) in PROGRAMS.items():
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "prog.hip")
                with open(path, "w") as f:
                    f.write(program_source(text, *EXAMPLE_SHAPES["fishing"], integrator, derive="all", ndata=ndata,
                                           scenarios=scen))
                r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math",
                                    "--cuda-device-only", "-include", "hip/hip_runtime.h",
                                    "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o",
                                    os.path.join(d, "prog.o")], capture_output=True, text=True, check=True)
            at = r.stderr.index("Function Name: mioc_ode_program_kernel")
            got = {k: re.search(r"\b" + k + r"[^:\n]*: (\d+)", r.stderr[at:]).group(1)
                   for k in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy")}
            lines.append(f"  {integrator:5s} {name}  VGPRs {got['VGPRs']:>3s}  AGPRs {got['AGPRs']:>3s}  "
                         f"SGPRs {got['TotalSGPRs']:>3s}  scratch {got['ScratchSize']} B/lane  "
                         f"waves/SIMD {got['Occupancy']}")
    print("\n".join(lines), flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def timing(K, nt, out):
    import numpy as np
    import torch

    from mioc import native
    from mioc.trm_batch import sos1_levels
    REP, ROUNDS = 10, 7
    T0, T1 = 0.0, 12.0
    shape = EXAMPLE_SHAPES["fishing"]
    y0, par = EXAMPLE_STATE0["fishing"], EXAMPLE_PARAMS["fishing"]
    f64 = dict(dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(1)
    # the scenario arrays, the scenario index fastest: [r][s], [e][s], [c][e][s]
    y0_1 = torch.tensor(np.array(y0, dtype=np.float64)[:, None], **f64)
    par_1 = torch.tensor(np.array(par, dtype=np.float64)[:, None], **f64)
    y0_K = torch.tensor(np.array(y0)[:, None] + 0.05 * rng.standard_normal((shape[0], K)), **f64)
    par_K = torch.tensor(np.array(par, dtype=np.float64)[:, None] * (1.0 + 0.05 * rng.uniform(-1, 1, (shape[2], K))),
                         **f64)
    data = torch.ones(nt, 2, **f64)
    data_K = torch.tensor(1.0 + 0.05 * rng.standard_normal((nt, 2, K)), **f64)
    ctx = native.Context(0)
    ctx.set_levels(sos1_levels())
    x = torch.empty(K, nt, 3, **f64)
    ctx.rand_start_tensor(x, seed=1)
    torch.cuda.synchronize()
    st = torch.cuda.ExternalStream(ctx.stream())
    # line name: (program, S, state0, params, data, baseline line)
    lines_of = {"scen=0            ": ("scen=0           ", 0, None, None, None, None),
                "scen=1 S=1        ": ("scen=1           ", 1, y0_1, par_1, None, "scen=0            "),
                "scen=1 S=K        ": ("scen=1           ", K, y0_K, par_K, None, "scen=0            "),
                "nd=2 scen=0       ": ("nd=2 scen=0      ", 0, None, None, data, None),
                "nd=2 scen=1 S=K   ": ("nd=2 scen=1      ", K, y0_K, par_K, data, "nd=2 scen=0       "),
                "nd=2 scen=3 S=K   ": ("nd=2 scen=3      ", K, y0_K, par_K, data_K, "nd=2 scen=0       ")}
    progs, calls, J, df = {}, {}, {}, {}
    for integrator in INTEGRATORS:
        for name, (text, ndata, scen, _) in PROGRAMS.items():
            progs[integrator, name] = ODEProgram(text, *shape, integrator=integrator, derive="all", ndata=ndata,
                                                 scenarios=scen)
        for line, (pname, S, ys, ps, dd, _) in lines_of.items():
            key = (integrator, line)
            J[key] = torch.empty(K, **f64)
            df[key] = torch.empty_like(x)

            def call(want_df, key=key, prog=progs[integrator, pname], S=S, ys=ys, ps=ps, dd=dd):
                if S:
                    ctx.ode_program_eval_scen_tensors(prog, None, x, T0, T1, S, ys, ps, dd, J[key],
                                                      df[key] if want_df else None)
                else:
                    ctx.ode_program_eval_tensors(prog, x, T0, T1, y0, par, J[key], df[key] if want_df else None,
                                                 data=dd)
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

    def same(i, a, b):
        return bool(torch.equal(J[i, a], J[i, b])) and bool(torch.equal(df[i, a], df[i, b]))
    # one uniform scenario gives the baseline's bits
    ok = all(same(i, "scen=1 S=1        ", "scen=0            ") and
             bool(torch.isfinite(J[i, "nd=2 scen=3 S=K   "]).all()) for i in INTEGRATORS)
    lines = [f"probe_ode_scenarios: fishing, derived hooks, K={K} nt={nt} (HIP events, {ROUNDS} alternating rounds of "
             f"{REP} launches after 3 warm-up; S=1 gives the scen=0 program's J and df bits: {ok})"]
    med = {key: statistics.median(v) for key, v in ms.items()}
    for (integrator, line, what), v in ms.items():
        base = lines_of[line][5] or line
        ratio = med[integrator, line, what] / med[integrator, base, what]
        lines.append(f"  {integrator:5s} {line} {what}  median {med[integrator, line, what]:8.4f} ms   "
                     f"min {min(v):8.4f}   max {max(v):8.4f}   / {base.strip()} {ratio:.3f}")
    print("\n".join(lines), flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for p in progs.values():
        p.close()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "resources":
        resources(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    sys.exit(timing(int(sys.argv[1]) if len(sys.argv) > 1 else 1024, int(sys.argv[2]) if len(sys.argv) > 2 else 1200,
                    sys.argv[3] if len(sys.argv) > 3 else None))
