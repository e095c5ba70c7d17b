"""GPU tier of the one path through the Python layer (the CPU tier: test_ode_program_paths.py).

Every ``Context.ode_program_eval*_tensors`` wrapper calls the library's _sens eval entry; its J, df (and Y) are
bit-identical to a direct call of the older C entry the wrapper used to pick.  K = 70: one full 64-lane block and a
partial one; nt = 3; RK4.  And ``TRM_batch`` knows a problem by its members alone, and closes its context when the
problem raises."""
import ctypes
import math

import numpy as np
import pytest

import mioc
from mioc import native
from mioc.conv import ConvProblem
from mioc.ode_device import EXAMPLE_PARAMS, EXAMPLE_SHAPES, EXAMPLE_SOURCES, EXAMPLE_STATE0, ODEProgram
from mioc.trm_batch import TRM_batch

import ode_bolza_problem as bp
from ode_gpu_support import grid, sos1

pytestmark = pytest.mark.gpu

K, NT, T1 = 70, 3, 0.3
FISH_Y0 = np.array(EXAMPLE_STATE0["fishing"], dtype=np.float64)
FISH_PAR = np.array(EXAMPLE_PARAMS["fishing"], dtype=np.float64)


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def hp(a):
    return ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def rig():
    """One context, the three programs, the controls on the device and a maker of NaN-filled outputs."""
    import torch
    f64 = dict(dtype=torch.float64, device="cuda")
    progs = {
        "fishing": ODEProgram(EXAMPLE_SOURCES["fishing"], *EXAMPLE_SHAPES["fishing"], integrator="rk4"),
        "bolza": ODEProgram(bp.SOURCE, bp.NY, bp.NX, bp.NP, integrator="rk4", ndata=bp.ND, terminal=True, states=True),
        "scen": ODEProgram(EXAMPLE_SOURCES["fishing"], *EXAMPLE_SHAPES["fishing"], integrator="rk4", scenarios=True),
    }
    x3 = torch.tensor(sos1(K, NT, 21), **f64)
    x2 = torch.tensor(grid(K, NT, 22), **f64)

    def outputs(x, ny=None):
        out = [torch.full((K,), math.nan, **f64), torch.full_like(x, math.nan)]
        if ny is not None:
            out.append(torch.full((K, NT + 1, ny), math.nan, **f64))
        torch.cuda.synchronize()
        return out
    with native.Context(0) as ctx:
        yield ctx, progs, x3, x2, outputs
    for p in progs.values():
        p.close()


def _same(ctx, got, want):
    import torch
    ctx.synchronize()
    for a, b in zip(got, want):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


def test_plain_wrapper_is_the_plain_entry(rig):
    ctx, progs, x, _, outputs = rig
    y0, par = FISH_Y0, FISH_PAR
    got, want = outputs(x), outputs(x)
    ctx.ode_program_eval_tensors(progs["fishing"], x, 0.0, T1, y0, par, *got)
    assert ctx.lib.mioc_ode_program_eval_device(ctx.h, progs["fishing"].h, K, vp(x), NT, 0.0, T1, hp(y0), hp(par),
                                                *map(vp, want)) == native.MIOC_OK
    _same(ctx, got, want)


def test_mixed_wrapper_is_the_mixed_entry(rig):
    ctx, progs, x, _, outputs = rig
    y0, par = FISH_Y0, FISH_PAR
    got, want = outputs(x), outputs(x)
    ctx.ode_program_eval_mixed_tensors(progs["fishing"], 1, x, 0.0, T1, y0, par, *got)
    assert ctx.lib.mioc_ode_program_eval_mixed_device(ctx.h, progs["fishing"].h, 1, K, vp(x), NT, 0.0, T1, hp(y0),
                                                      hp(par), *map(vp, want)) == native.MIOC_OK
    _same(ctx, got, want)


def test_data_and_states_are_the_bolza_entry(rig):
    import torch
    ctx, progs, _, x, outputs = rig
    y0, par = np.array(bp.STATE0, dtype=np.float64), np.array(bp.PARAMS, dtype=np.float64)
    data = torch.tensor(bp.make_data(NT), dtype=torch.float64, device="cuda")
    (J, df, Y), want = outputs(x, bp.NY), outputs(x, bp.NY)
    ctx.ode_program_eval_tensors(progs["bolza"], x, 0.0, T1, y0, par, J, df, data=data, Y=Y)
    assert ctx.lib.mioc_ode_program_eval_bolza_device(ctx.h, progs["bolza"].h, 0, K, vp(x), NT, 0.0, T1, hp(y0),
                                                      hp(par), vp(data), *map(vp, want)) == native.MIOC_OK
    _same(ctx, (J, df, Y), want)


def test_scenario_wrapper_is_the_scenario_entry(rig):
    import torch
    ctx, progs, x, _, outputs = rig
    S = 2
    rng = np.random.default_rng(23)
    y0 = np.array(EXAMPLE_STATE0["fishing"])[:, None] * (1.0 + 0.1 * rng.random((2, S)))       # (ny, S)
    par = np.array(EXAMPLE_PARAMS["fishing"])[:, None] * (1.0 + 0.1 * rng.random((12, S)))    # (nparams, S)
    d_y0, d_par = (torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda") for a in (y0, par))
    got, want = outputs(x), outputs(x)
    ctx.ode_program_eval_scen_tensors(progs["scen"], None, x, 0.0, T1, S, d_y0, d_par, None, *got)
    assert ctx.lib.mioc_ode_program_eval_scen_device(ctx.h, progs["scen"].h, 0, K, vp(x), NT, 0.0, T1, S, vp(d_y0),
                                                     vp(d_par), None, *map(vp, want), None) == native.MIOC_OK
    _same(ctx, got, want)


# ---- TRM_batch takes any object with the members it asks for ---------------------------------------------------------
class Wrapped:
    """The members TRM_batch asks of a problem, delegated to a ConvProblem; no type TRM_batch could recognise."""

    def __init__(self, cp):
        self.cp, self.nt, self.T0, self.T1, self.fixes_nt = cp, cp.nt, cp.T0, cp.T1, cp.fixes_nt
        self.level_table, self.setup, self.check_restarts = cp.level_table, cp.setup, cp.check_restarts
        self.calls = 0

    def eval_tensors(self, ctx, x, J=None, df=None):
        self.calls += 1
        self.cp.eval_tensors(ctx, x, J, df)


class Raising(Wrapped):
    def eval_tensors(self, ctx, x, J=None, df=None):
        if self.calls == 1:
            raise RuntimeError("the problem's second evaluation")  # before anything is enqueued for it
        super().eval_tensors(ctx, x, J, df)


# nt = 1 is the smallest mioc_conv_setup accepts: tau = 2, and Delta0 = 4 gives the budget B = 2
PAR = dict(beta=1e-4, Delta0=4.0, p=1, maxiter=2, kmax=2)


def test_trm_batch_takes_a_protocol_object():
    cp = ConvProblem(nt=1)
    par = mioc.TRM_parameters(**PAR)
    w = Wrapped(cp)
    vw, uw, iw = TRM_batch(w, par, K=2, seed=1)
    vc, uc, ic = TRM_batch(cp, par, K=2, seed=1)
    assert w.calls >= 3  # J of the starts, one gradient at least, the final derivative
    # (a restart that accepts no trial within maxiter returns J = Inf, as in the reference: equal on both sides)
    assert np.array_equal(vw, vc) and not np.any(np.isnan(vc)) and np.array_equal(iw, ic)
    assert np.array_equal(uw.cpu().numpy(), uc.cpu().numpy())


def test_trm_batch_closes_its_context_when_the_problem_raises():
    before = set(native._LIVE)
    r = Raising(ConvProblem(nt=1))
    with pytest.raises(RuntimeError, match="second evaluation"):
        TRM_batch(r, mioc.TRM_parameters(**PAR), K=2, seed=1)
    assert r.calls == 1
    assert set(native._LIVE) == before
