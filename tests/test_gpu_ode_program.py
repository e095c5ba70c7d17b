"""GPU tier of user-defined ODE objectives (mioc_ode_program_eval_device, include/mioc.h).

The three built-in problems restated as hook text (mioc.ode_device.EXAMPLE_SOURCES) execute the same IEEE operations
in the same order as k_ode_eval, without contraction, so their J and df are compared with np.array_equal: a
difference is a finding, not a tolerance to widen.  The tests' fourth problem (tests/ode_program_problem.py: ny = 3,
nx = 2, t-dependent F, control-dependent G, structural zeros) is compared with its host mirror at the bar of
test_gpu_ode.py (1e-12 relative for J, 1e-12 of max|df|).  Then the gate of the device TRM control, scratch growth,
program / context lifetimes, and TRM_batch on a DeviceODEProblem."""
import math

import numpy as np
import pytest

import mioc
from mioc import native
from mioc.iterators import LevelTable
from mioc.ode_device import (EXAMPLE_PARAMS, EXAMPLE_SHAPES, EXAMPLE_SOURCES, EXAMPLE_STATE0, DeviceODEProblem,
                             ODEProgram)

import ode_program_problem as fourth
from ode_gpu_support import grid as _grid, program_objective, run_eval as _run, sos1 as _sos1

pytestmark = pytest.mark.gpu

BUILTIN = {"fishing": native.MIOC_ODE_FISHING, "doubletank": native.MIOC_ODE_DOUBLETANK,
           "vanderpol": native.MIOC_ODE_VANDERPOL}


@pytest.fixture(scope="module")
def programs():
    """Every program compiled once per module."""
    progs = {n: ODEProgram(EXAMPLE_SOURCES[n], *EXAMPLE_SHAPES[n]) for n in BUILTIN}
    progs["fourth"] = ODEProgram(fourth.SOURCE, fourth.NY, fourth.NX, len(fourth.PARAMS))
    yield progs
    for p in progs.values():
        p.close()


def _data(name):
    if name == "fourth":
        return fourth.STATE0, fourth.PARAMS
    return EXAMPLE_STATE0[name], EXAMPLE_PARAMS[name]


def _prog_eval(ctx, prog, name, T1):
    y0, par = _data(name)
    return lambda dx, J, df: ctx.ode_program_eval_tensors(prog, dx, 0.0, T1, y0, par, J, df)


@pytest.mark.parametrize("K,nt", [(70, 64), (3, 1), (3, 2)])
@pytest.mark.parametrize("name", list(BUILTIN))
def test_examples_bit_identical_to_builtin(programs, name, K, nt):
    """K = 70: one full block and a partial one of 6 lanes; nt = 1, 2: the loops' edge cases."""
    T1 = 0.01 * nt
    x = _sos1(K, nt, 11 + nt)
    with native.Context(0) as ctx:
        builtin = lambda dx, J, df: ctx.ode_eval_tensors(BUILTIN[name], dx, 0.0, T1, J, df)  # noqa: E731
        program = _prog_eval(ctx, programs[name], name, T1)
        Jb, dfb = _run(ctx, x, builtin)
        Jp, dfp = _run(ctx, x, program)
        assert np.all(np.isfinite(Jb)) and np.all(np.isfinite(dfb))
        assert np.array_equal(Jp, Jb), np.flatnonzero(Jp != Jb)
        assert np.array_equal(dfp, dfb), np.argwhere(dfp != dfb)[:4]
        Jp1, none = _run(ctx, x, program, want_df=False)     # d_df NULL
        assert none is None and np.array_equal(Jp1, Jb)
        none, dfp1 = _run(ctx, x, program, want_J=False)     # d_J NULL
        assert none is None and np.array_equal(dfp1, dfb)


@pytest.fixture(scope="module")
def fourth_reference():
    """The host mirror's J and df for K = 70 controls of the fourth problem (nt = 96, T1 = 0.96), computed once."""
    K, nt = 70, 96
    x = _grid(K, nt, 5)
    obj = fourth.FourthObj(nt=nt, T1=0.96)
    Jh, dfh = np.empty(K), np.empty((K, nt, fourth.NX))
    for k in range(K):
        obj.x[:, :] = x[k].T
        Jh[k] = mioc.eval_f_(obj)
        mioc.eval_df_(obj)
        dfh[k] = obj.df.T
    x.setflags(write=False), Jh.setflags(write=False), dfh.setflags(write=False)
    return x, Jh, dfh


def test_fourth_problem_vs_host_mirror(programs, fourth_reference):
    x, Jh, dfh = fourth_reference
    with native.Context(0) as ctx:
        J, df = _run(ctx, x, _prog_eval(ctx, programs["fourth"], "fourth", 0.96))
    exact = 0
    for k in range(x.shape[0]):
        assert abs(J[k] - Jh[k]) <= 1e-12 * abs(Jh[k]), (k, J[k], Jh[k])
        assert np.max(np.abs(df[k] - dfh[k])) <= 1e-12 * max(1e-300, np.max(np.abs(dfh[k]))), k
        exact += int(J[k] == Jh[k]) + int(np.array_equal(df[k], dfh[k]))
    assert np.all(df[:, :, 1] != 0.0)  # Gu[1] = 0.1 y0 is in every column
    print(f"fourth: {exact} of {2 * x.shape[0]} J / df arrays bit-identical to the host mirror")


def test_gate_closed_leaves_outputs_untouched(programs, fourth_reference):
    x, Jh, dfh = fourth_reference
    x = x[:5]
    with native.Context(0) as ctx:
        ev = _prog_eval(ctx, programs["fourth"], "fourth", 0.96)
        state = ctx.trm_state_tensor(5)      # zero-initialised: the gate word is 0
        ctx.trm_attach(state)
        J, df = _run(ctx, x, ev)
        assert np.all(np.isnan(J)) and np.all(np.isnan(df))
        ctx.trm_attach(None)
        J, df = _run(ctx, x, ev)
        assert np.allclose(J, Jh[:5], rtol=1e-12, atol=0) and np.all(np.isfinite(df))


def test_scratch_growth_equals_fresh_context(programs):
    xs, xl = _grid(4, 16, 1), _grid(130, 96, 2)
    with native.Context(0) as ctx:
        _run(ctx, xs, _prog_eval(ctx, programs["fourth"], "fourth", 0.16))
        J1, df1 = _run(ctx, xl, _prog_eval(ctx, programs["fourth"], "fourth", 0.96))
    with native.Context(0) as ctx:
        J2, df2 = _run(ctx, xl, _prog_eval(ctx, programs["fourth"], "fourth", 0.96))
    assert np.all(np.isfinite(J1)) and np.all(np.isfinite(df1))
    assert np.array_equal(J1, J2) and np.array_equal(df1, df2)


def test_program_and_context_lifetimes(programs):
    xa, xb = _sos1(9, 32, 3), _grid(9, 32, 4)
    with native.Context(0) as c1, native.Context(0) as c2:
        a1 = _prog_eval(c1, programs["fishing"], "fishing", 0.32)
        b1 = _prog_eval(c1, programs["fourth"], "fourth", 0.32)
        ra, rb = _run(c1, xa, a1), _run(c1, xb, b1)
        for _ in range(2):  # two programs alternately in one context: each its own results
            qa, qb = _run(c1, xa, a1), _run(c1, xb, b1)
            assert np.array_equal(qa[0], ra[0]) and np.array_equal(qa[1], ra[1])
            assert np.array_equal(qb[0], rb[0]) and np.array_equal(qb[1], rb[1])
        assert not np.array_equal(ra[0], rb[0])
        # one program in two contexts on device 0
        sb = _run(c2, xb, _prog_eval(c2, programs["fourth"], "fourth", 0.32))
        assert np.array_equal(sb[0], rb[0]) and np.array_equal(sb[1], rb[1])
        Jb, dfb = _run(c2, xa, lambda dx, J, df: c2.ode_eval_tensors(native.MIOC_ODE_FISHING, dx, 0.0, 0.32, J, df))
        assert np.array_equal(ra[0], Jb) and np.array_equal(ra[1], dfb)


def test_eval_argument_checks(programs):
    import torch
    with native.Context(0) as ctx:
        x = torch.tensor(_grid(2, 8, 0), dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):  # nx of the tensor against the program's
            ctx.ode_program_eval_tensors(programs["fishing"], x, 0.0, 1.0, [0.5, 0.7], EXAMPLE_PARAMS["fishing"])
        with pytest.raises(native.MiocNativeError):  # T1 <= T0
            ctx.ode_program_eval_tensors(programs["fourth"], x, 1.0, 1.0, fourth.STATE0, fourth.PARAMS)
        ctx.set_levels(LevelTable([[0, 1]] * 3, mioc.bounded_sum_iterator([[0, 1]] * 3, 1, 1)))
        with pytest.raises(native.MiocNativeError):  # nx against the levels' M
            ctx.ode_program_eval_tensors(programs["fourth"], x, 0.0, 1.0, fourth.STATE0, fourth.PARAMS)


def test_trm_batch_fishing_source_equals_builtin(programs):
    """TRM_batch on the fishing hooks against TRM_batch("fishing"): same x0, K = 12, nt = 240 and the parameters of
    test_gpu_ode.py::test_trm_batch_equals_sequential_trm."""
    import torch
    from mioc.trm_batch import PROBLEMS, TRM_batch
    K, nt = 12, 240
    par = mioc.TRM_parameters(beta=1e-3, Delta0=1.0, p=math.inf, maxiter=6, kmax=5)
    V = [[0, 1]] * 3
    it = mioc.bounded_sum_iterator(V, 1, 1)
    with native.Context(0) as ctx:
        ctx.set_levels(LevelTable(V, it))
        x0 = torch.empty(K, nt, 3, dtype=torch.float64, device="cuda")
        ctx.rand_start_tensor(x0, seed=99)
        ctx.synchronize()
    _, nt_def, T0, T1 = PROBLEMS["fishing"]
    prob = DeviceODEProblem(programs["fishing"], V, it, T0, T1, nt_def, EXAMPLE_STATE0["fishing"],
                            EXAMPLE_PARAMS["fishing"])
    vb, ub, ib = TRM_batch("fishing", par, x0=x0)
    vp, up, ip = TRM_batch(prob, par, x0=x0)
    assert np.array_equal(vp, vb) and np.array_equal(ip, ib) and torch.equal(up, ub)
    assert not torch.equal(ub, x0)  # the runs moved


def test_trm_batch_fourth_problem_equals_sequential_trm(programs):
    import torch
    from mioc.trm_batch import TRM_batch
    K, nt, T1 = 6, 96, 0.96
    par = mioc.TRM_parameters(beta=1e-3, Delta0=0.25, p=1, maxiter=4, kmax=4)
    prob = DeviceODEProblem(programs["fourth"], fourth.V, None, 0.0, T1, nt, fourth.STATE0, fourth.PARAMS)
    with native.Context(0) as ctx:
        ctx.set_levels(LevelTable(fourth.V))
        x0 = torch.empty(K, nt, fourth.NX, dtype=torch.float64, device="cuda")
        ctx.rand_start_tensor(x0, seed=4)
        ctx.synchronize()
        vals, u, iters = TRM_batch(prob, par, x0=x0)
        ub = u.cpu().numpy()
        assert not np.array_equal(ub, x0.cpu().numpy())
        for k in range(K):
            obj = program_objective(fourth.FourthObj(nt=nt, T1=T1), programs["fourth"], ctx, fourth.STATE0,
                                    fourth.PARAMS)
            J = mioc.TRM(obj, par, x0=x0[k].cpu().numpy().T.copy())
            assert J == vals[k], (k, J, vals[k])
            assert np.array_equal(obj.x, ub[k].T), k
    print(f"fourth: iterations per restart {iters.tolist()}")
