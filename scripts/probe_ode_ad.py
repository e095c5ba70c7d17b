"""Timing of derived ODE hooks (mioc_ode_program_create_ad) against hand-written ones:
  python scripts/probe_ode_ad.py INTEGRATOR [K] [nt] [out file]     one of euler, rk4, midpoint, ...; needs the GPU
  python scripts/probe_ode_ad.py resources [out file]               registers and scratch of both kernels; needs no GPU

The fishing problem, K restarts (default 1024) of nt steps (default 1200) on [0, 12], one substep:
  * the program of EXAMPLE_SOURCES["fishing"] (six hand-written hooks);
  * the program of EXAMPLE_SOURCES_AD["fishing"] with derive="all" (templated F and G, four generated hooks);
per call with J and df and per value-only call, by HIP events on the library's stream in one process, ROUNDS rounds
alternating between the programs, REP launches per round after a warm-up; the spread over the rounds is printed with
the medians.  Also the wall time of mioc_ode_program_create_ad against mioc_ode_program_create_ex (the first call of
the process loads hiprtc and is reported apart), and whether J is bit-identical and how far df deviates.  One
integrator per process: run it once each for euler, rk4 and midpoint.

`resources` takes the source text the library assembles (head, dual type, text, generated hooks, skeleton:
mioc_ode_program_source) and compiles it offline with the library's flags and -Rpass-analysis=kernel-resource-usage,
for euler, rk4 and midpoint.
"""
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mixed-integer-optimal-control---algorithm-tools_amd")
sys.path[:0] = [PKG, ROOT]

from mioc.ode_device import (EXAMPLE_PARAMS, EXAMPLE_SHAPES, EXAMPLE_SOURCES, EXAMPLE_SOURCES_AD,  # noqa: E402
                             EXAMPLE_STATE0, INTEGRATORS, ODEProgram, program_source)


def resources(out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lines = ["probe_ode_ad resources: fishing (ny, nx) = (2, 3), the assembled source compiled offline for gfx950 "
             "(-O3 -ffp-contract=off -fno-fast-math)"]
    for integrator in ("euler", "rk4", "midpoint"):
        for label, text, derive in (("hand", EXAMPLE_SOURCES["fishing"], ()),
                                    ("AD  ", EXAMPLE_SOURCES_AD["fishing"], "all")):
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "prog.hip")
                with open(path, "w") as f:
                    f.write(program_source(text, *EXAMPLE_SHAPES["fishing"], integrator, derive=derive))
                r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math",
                                    "--cuda-device-only", "-include", "hip/hip_runtime.h",
                                    "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o",
                                    os.path.join(d, "prog.o")], capture_output=True, text=True, check=True)
            got = {k: re.search(r"\b" + k + r"[^:\n]*: (\d+)", r.stderr).group(1)
                   for k in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy")}
            lines.append(f"  {integrator:8s} {label}  VGPRs {got['VGPRs']:>3s}  AGPRs {got['AGPRs']:>3s}  "
                         f"SGPRs {got['TotalSGPRs']:>3s}  scratch {got['ScratchSize']} B/lane  "
                         f"waves/SIMD {got['Occupancy']}")
    print("\n".join(lines), flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def timing(integrator, K, nt, out):
    import torch

    from mioc import native
    from mioc.trm_batch import sos1_levels
    REP, ROUNDS = 10, 7
    T0, T1 = 0.0, 12.0
    shape = EXAMPLE_SHAPES["fishing"]
    create = {"hand": [], "AD": []}
    progs = {}
    for r in range(5):  # the first hand-written create loads hiprtc: reported apart
        for label, text, derive in (("hand", EXAMPLE_SOURCES["fishing"], ()),
                                    ("AD", EXAMPLE_SOURCES_AD["fishing"], "all")):
            t0 = time.perf_counter()
            p = ODEProgram(text, *shape, integrator=integrator, derive=derive)
            create[label].append(time.perf_counter() - t0)
            if r < 4:
                p.close()
            else:
                progs[label] = p
    ctx = native.Context(0)
    ctx.set_levels(sos1_levels())
    x = torch.empty(K, nt, 3, dtype=torch.float64, device="cuda")
    ctx.rand_start_tensor(x, seed=1)
    J = {k: torch.empty(K, dtype=torch.float64, device="cuda") for k in progs}
    df = {k: torch.empty_like(x) for k in progs}
    torch.cuda.synchronize()
    st = torch.cuda.ExternalStream(ctx.stream())
    y0, par = EXAMPLE_STATE0["fishing"], EXAMPLE_PARAMS["fishing"]
    calls = {
        "hand J+df": lambda: ctx.ode_program_eval_tensors(progs["hand"], x, T0, T1, y0, par, J["hand"], df["hand"]),
        "AD   J+df": lambda: ctx.ode_program_eval_tensors(progs["AD"], x, T0, T1, y0, par, J["AD"], df["AD"]),
        "hand J   ": lambda: ctx.ode_program_eval_tensors(progs["hand"], x, T0, T1, y0, par, J["hand"], None),
        "AD   J   ": lambda: ctx.ode_program_eval_tensors(progs["AD"], x, T0, T1, y0, par, J["AD"], None),
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
    same_J = bool(torch.equal(J["hand"], J["AD"]))
    dev = float(((df["AD"] - df["hand"]).abs().amax(dim=(1, 2)) / df["hand"].abs().amax(dim=(1, 2))).max())
    lines = [f"probe_ode_ad: fishing {integrator} K={K} nt={nt} (HIP events, {ROUNDS} alternating rounds of {REP} launches "
             f"after 3 warm-up; J bit-identical: {same_J}; worst |df_AD - df_hand| / max|df| per restart: {dev:.3g})"]
    for name, v in ms.items():
        lines.append(f"  {name}  median {statistics.median(v):8.4f} ms   min {min(v):8.4f}   max {max(v):8.4f}")
    med = {name: statistics.median(v) for name, v in ms.items()}
    lines.append(f"  AD / hand: J+df {med['AD   J+df'] / med['hand J+df']:.3f}, J only {med['AD   J   '] / med['hand J   ']:.3f}")
    lines.append(f"  create wall time: first hand-written {create['hand'][0]:.3f} s (loads hiprtc); then hand-written "
                 + ", ".join(f"{s:.3f}" for s in create["hand"][1:]) + " s; AD "
                 + ", ".join(f"{s:.3f}" for s in create["AD"]) + " s")
    print("\n".join(lines), flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for p in progs.values():
        p.close()
    ctx.close()
    return 0 if same_J and dev <= 1e-12 else 1


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "euler"
    if mode == "resources":
        resources(sys.argv[2] if len(sys.argv) > 2 else None)
        sys.exit(0)
    if mode not in INTEGRATORS:
        sys.exit(f"usage: probe_ode_ad.py resources | {' | '.join(INTEGRATORS)} [K] [nt] [out file]")
    sys.exit(timing(mode, int(sys.argv[2]) if len(sys.argv) > 2 else 1024, int(sys.argv[3]) if len(sys.argv) > 3 else 1200,
                    sys.argv[4] if len(sys.argv) > 4 else None))
