"""What the tests of scenarios share (test_ode_scenarios.py, test_gpu_ode_scenarios.py; include/mioc.h, "Scenarios"):
the scenario draws on tests/ode_bolza_problem.py, the variant of its text without sampled data, and one evaluation of a
scenario program through device arrays that this module lays out itself, independently of mioc.ode_device.

Scenario s is drawn with a fixed seed: state0 = STATE0 + 0.1 N(0, 1), params = PARAMS (1 + 0.2 U(-1, 1)),
data = make_data(nt) + 0.05 N(0, 1).
"""
import math

import numpy as np

import ode_bolza_problem as bp

# The text without sampled data (ndata = 0): the two data columns become the parameters p[3] and p[4], NP = 5.  The
# mirror's hooks read p[bp.NP] and p[bp.NP + 1], which are p[3] and p[4]: the same hooks serve with data = None.
NODATA_SOURCE = bp.SOURCE.replace("p[NP + 1]", "p[4]").replace("p[NP]", "p[3]")
assert "NP" not in NODATA_SOURCE
NODATA_NP = 5
NODATA_PARAMS = bp.PARAMS + [0.75, 0.05]


def draw_scenarios(S, nt, seed=11, nodata=False):
    """(state0 (S, NY), params (S, NP), data (S, nt, ND)) of S scenarios; nodata: params (S, 5), data None."""
    rng = np.random.default_rng(seed)
    state0 = np.array(bp.STATE0) + 0.1 * rng.standard_normal((S, bp.NY))
    base = np.array(NODATA_PARAMS if nodata else bp.PARAMS)
    params = base * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, size=(S, base.size)))
    data = None if nodata else np.array(bp.make_data(nt))[None] + 0.05 * rng.standard_normal((S, nt, bp.ND))
    return np.ascontiguousarray(state0), np.ascontiguousarray(params), data


def uniform_scenarios(S, nt):
    """S copies of the problem's own values."""
    return (np.tile(np.array(bp.STATE0), (S, 1)), np.tile(np.array(bp.PARAMS), (S, 1)),
            np.tile(np.array(bp.make_data(nt))[None], (S, 1, 1)))


def run_scen(ctx, prog, x, T0, T1, state0, params, data, nu=None, want_J=True, want_df=True, want_Y=True,
             fill=math.nan):
    """One evaluation of a scenario program: state0 (S, ny), params (S, nparams), data (S, nt, ndata) for a program
    with per-scenario data, else (nt, ndata) or None.  J (K,), df (K, nt, nx), Y (K, nt + 1, ny) as numpy from device
    buffers prefilled with `fill` (None where not asked for)."""
    import torch
    K, nt, _ = x.shape
    S = state0.shape[0]
    f64 = dict(dtype=torch.float64, device="cuda")
    d_y0 = torch.tensor(np.ascontiguousarray(np.asarray(state0).T), **f64)                    # [r][s]
    d_par = torch.tensor(np.ascontiguousarray(np.asarray(params).T), **f64) if prog.nparams else None  # [e][s]
    if data is None:
        d_data = None
    elif np.ndim(data) == 3:
        d_data = torch.tensor(np.ascontiguousarray(np.asarray(data).transpose(1, 2, 0)), **f64)  # [c][e][s]
    else:
        d_data = torch.tensor(np.asarray(data), **f64)
    dx = torch.tensor(x, **f64)
    J = torch.full((K,), fill, **f64) if want_J else None
    df = torch.full_like(dx, fill) if want_df else None
    Y = torch.full((K, nt + 1, prog.ny), fill, **f64) if want_Y else None
    torch.cuda.synchronize()
    ctx.ode_program_eval_scen_tensors(prog, nu, dx, T0, T1, S, d_y0, d_par, d_data, J, df, Y)
    ctx.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (J, df, Y))
