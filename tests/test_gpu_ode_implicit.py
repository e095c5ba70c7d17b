"""GPU tier of the implicit integrators of user-defined ODE objectives (backward Euler and the implicit midpoint rule:
mioc_ode_program_create_ex; the scheme, its Newton rule and its rounding order: include/mioc.h, "Implicit integrators").

The device kernel is compared with the host mirror (tests/ode_implicit_mirror.py) on the tests' fourth problem and on
the stiff problem at the bar of test_gpu_ode_program.py (1e-12 relative for J, 1e-12 of max|df|): a miss means the
operation order differs from the documented one.  Then independence of K, the finite-difference criterion and the order
on the device's own numbers, the NaN contract of a restart whose Newton iteration cannot converge, scratch growth, and
TRM_batch against the sequential TRM."""
import numpy as np
import pytest

import mioc
from mioc import native
from mioc.iterators import LevelTable
from mioc.ode_device import DeviceODEProblem, ODEProgram

import ode_program_problem as fourth
import ode_stiff_problem as stiff
from ode_gpu_support import assert_at_bar, grid as _grid, program_objective, run_program
from ode_implicit_mirror import ORDER_BANDS, theta_eval
from ode_rk_mirror import order_control

pytestmark = pytest.mark.gpu

SCHEMES = [("beuler", 1), ("beuler", 3), ("midpoint", 1), ("midpoint", 3)]
PROBLEMS = {"fourth": (fourth, fourth.FourthObj), "stiff": (stiff, stiff.StiffObj)}


@pytest.fixture(scope="module")
def programs():
    """Every program compiled once per module, by (problem, integrator, substeps)."""
    progs = {}

    def get(problem, integrator, substeps):
        key = (problem, integrator, substeps)
        if key not in progs:
            if problem == "noroot":
                progs[key] = ODEProgram(stiff.NOROOT_SOURCE, stiff.NOROOT_NY, stiff.NOROOT_NX, 0, integrator=integrator,
                                        substeps=substeps)
            else:
                mod = PROBLEMS[problem][0]
                progs[key] = ODEProgram(mod.SOURCE, mod.NY, mod.NX, len(mod.PARAMS), integrator=integrator,
                                        substeps=substeps)
        return progs[key]
    yield get
    for p in progs.values():
        p.close()


def _run(ctx, prog, x, T1, state0=fourth.STATE0, params=fourth.PARAMS, **kw):
    """J and df from buffers prefilled with 7.0 (None where not asked for): a NaN in the output is one the kernel
    wrote."""
    return run_program(ctx, prog, x, 0.0, T1, state0, params, fill=7.0, **kw)[:2]


def _run_p(ctx, programs, problem, integrator, substeps, x, T1, **kw):
    mod = PROBLEMS[problem][0]
    return _run(ctx, programs(problem, integrator, substeps), x, T1, state0=mod.STATE0, params=mod.PARAMS, **kw)


def _mirror(problem, x, T1, integrator, substeps):
    K, nt, nx = x.shape
    obj = PROBLEMS[problem][1](nt=nt, T1=T1)
    Jh, dfh = np.empty(K), np.empty((K, nt, nx))
    for k in range(K):
        Jh[k], d = theta_eval(obj, x[k].T, integrator, substeps)
        dfh[k] = d.T
    return Jh, dfh


@pytest.fixture(scope="module")
def x70():
    x = _grid(70, 24, 5)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def device70(programs, x70):
    """The device's J and df of the K = 70 call (nt = 24, T1 = 0.96) per problem and scheme, computed once."""
    out = {}
    with native.Context(0) as ctx:
        for problem in PROBLEMS:
            for integrator, m in SCHEMES:
                out[problem, integrator, m] = _run_p(ctx, programs, problem, integrator, m, x70, 0.96)
    return out


@pytest.mark.parametrize("integrator,substeps", SCHEMES)
@pytest.mark.parametrize("problem", ["fourth", "stiff"])
def test_vs_mirror(programs, x70, device70, problem, integrator, substeps):
    """K = 70: one full block and a partial one of 6 lanes."""
    J, df = device70[problem, integrator, substeps]
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(df))
    Jh, dfh = _mirror(problem, x70, 0.96, integrator, substeps)
    exact = sum(int(J[k] == Jh[k]) + int(np.array_equal(df[k], dfh[k])) for k in range(70))
    print(f"{problem} {integrator} m={substeps}: {exact} of 140 J / df arrays bit-identical to the mirror")
    assert_at_bar((J, df), (Jh, dfh))
    with native.Context(0) as ctx:
        J1, none = _run_p(ctx, programs, problem, integrator, substeps, x70, 0.96, want_df=False)  # no states stored
        assert none is None and np.array_equal(J1, J)
        none, df1 = _run_p(ctx, programs, problem, integrator, substeps, x70, 0.96, want_J=False)  # d_J NULL
        assert none is None and np.array_equal(df1, df)


@pytest.mark.parametrize("nt", [1, 2])
@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_edge_shapes(programs, integrator, substeps, nt):
    x = _grid(3, nt, 20 + nt)
    T1 = 0.04 * nt
    with native.Context(0) as ctx:
        J, df = _run_p(ctx, programs, "fourth", integrator, substeps, x, T1)
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(df))
    assert_at_bar((J, df), _mirror("fourth", x, T1, integrator, substeps))


@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_independent_of_K_and_position(programs, x70, device70, integrator, substeps):
    J, df = device70["stiff", integrator, substeps]
    big = _grid(130, 24, 6)
    big[129], big[64] = x70[0], x70[69]  # the first restart at the far end, the last one at a block's start
    with native.Context(0) as ctx:
        for k in (0, 37, 69):
            J1, df1 = _run_p(ctx, programs, "stiff", integrator, substeps, x70[k:k + 1], 0.96)
            assert J1[0] == J[k] and np.array_equal(df1[0], df[k]), k
        Jb, dfb = _run_p(ctx, programs, "stiff", integrator, substeps, big, 0.96)
    assert Jb[129] == J[0] and np.array_equal(dfb[129], df[0])
    assert Jb[64] == J[69] and np.array_equal(dfb[64], df[69])


@pytest.mark.parametrize("integrator,substeps", [("beuler", 2), ("midpoint", 2)])
@pytest.mark.parametrize("problem,T1", [("fourth", 4.8), ("stiff", 0.96)])
def test_device_gradient_is_exact(programs, problem, T1, integrator, substeps):
    """The criterion of test_ode_integrators.py::test_mirror_gradient_is_exact on the device's own J and df: x and
    x + t h for t = 1e-4, 1e-5, 1e-6 are 4 restarts of one call."""
    nt = 24
    rng = np.random.default_rng(7)
    x = np.full((nt, 2), 0.5)
    h = rng.standard_normal((nt, 2))
    ts = (1e-4, 1e-5, 1e-6)
    X = np.ascontiguousarray(np.stack([x] + [x + t * h for t in ts]))
    with native.Context(0) as ctx:
        J, df = _run_p(ctx, programs, problem, integrator, substeps, X, T1)
    dfh = (T1 / nt) * float(np.sum(df[0] * h))
    errs = [(abs((J[1 + q] - J[0]) / t - dfh), abs(dfh)) for q, t in enumerate(ts)]
    print(errs)
    scale = max(1e-12, errs[0][1])
    assert errs[2][0] <= 1e-4 * scale + 1e-9, errs
    assert errs[1][0] <= errs[0][0] * 0.5 + 1e-9, errs


@pytest.mark.parametrize("integrator", ["beuler", "midpoint"])
def test_device_order(programs, integrator):
    """Errors of the device's J at substeps 1, 2, 4 against its RK4 at 64 substeps: the bands of the CPU tier."""
    x = np.ascontiguousarray(order_control(24).T[None])
    with ODEProgram(fourth.SOURCE, fourth.NY, fourth.NX, len(fourth.PARAMS), integrator="rk4", substeps=64) as rk, \
            native.Context(0) as ctx:
        ref = _run(ctx, rk, x, 0.96, want_df=False)[0][0]
        e = [abs(_run_p(ctx, programs, "fourth", integrator, m, x, 0.96, want_df=False)[0][0] - ref) for m in (1, 2, 4)]
    lo, hi = ORDER_BANDS[integrator]
    print(integrator, e, e[0] / e[1], e[1] / e[2])
    assert lo <= e[0] / e[1] <= hi and lo <= e[1] / e[2] <= hi, e


@pytest.mark.parametrize("integrator,substeps", [("beuler", 1), ("midpoint", 3)])
def test_non_convergence_is_nan_for_that_restart_only(programs, integrator, substeps):
    """K = 66 (a full block and two lanes): even restarts x = 0, odd restarts x = 1, whose stage equation has no real
    root.  The odd ones are NaN throughout, the even ones untouched, and the call itself succeeds."""
    K, nt, T1 = 66, 8, 0.32
    prog = programs("noroot", integrator, substeps)
    x = np.zeros((K, nt, 1))
    x[1::2] = 1.0
    kw = dict(state0=stiff.NOROOT_STATE0, params=[])
    with native.Context(0) as ctx:
        J, df = _run(ctx, prog, x, T1, **kw)  # MIOC_OK: anything else raises
        J0, df0 = _run(ctx, prog, x[:1], T1, **kw)
        Jv, _ = _run(ctx, prog, x, T1, want_df=False, **kw)
        _, dfv = _run(ctx, prog, x, T1, want_J=False, **kw)
    assert np.all(np.isnan(J[1::2])) and np.all(np.isnan(df[1::2]))
    assert np.all(np.isfinite(J[0::2])) and np.all(np.isfinite(df[0::2]))
    for k in range(0, K, 2):
        assert J[k] == J0[0] and np.array_equal(df[k], df0[0]), k
    assert np.array_equal(Jv, J, equal_nan=True) and np.array_equal(dfv, df, equal_nan=True)
    obj = stiff.NoRootObj(nt=nt, T1=T1)
    Jh, dfh = theta_eval(obj, x[0].T, integrator, substeps)
    assert_at_bar((J[:1], df[:1]), (np.array([Jh]), dfh.T[None]))


def test_scratch_growth_equals_fresh_context(programs):
    prog = programs("fourth", "midpoint", 3)
    xs, xl = _grid(4, 16, 1), _grid(130, 96, 2)
    with native.Context(0) as ctx:
        _run(ctx, prog, xs, 0.16)
        J1, df1 = _run(ctx, prog, xl, 0.96)
    with native.Context(0) as ctx:
        J2, df2 = _run(ctx, prog, xl, 0.96)
    assert np.all(np.isfinite(J1)) and np.all(np.isfinite(df1))
    assert np.array_equal(J1, J2) and np.array_equal(df1, df2)


def test_trm_batch_midpoint_equals_sequential_trm(programs):
    """The parameters of test_gpu_ode_integrators.py::test_trm_batch_rk4_equals_sequential_trm with the implicit
    midpoint rule and 2 substeps."""
    import torch
    from mioc.trm_batch import TRM_batch
    K, nt, T1 = 6, 48, 0.96
    prog = programs("fourth", "midpoint", 2)
    par = mioc.TRM_parameters(beta=1e-3, Delta0=0.25, p=1, maxiter=4, kmax=4)
    prob = DeviceODEProblem(prog, fourth.V, None, 0.0, T1, nt, fourth.STATE0, fourth.PARAMS)
    with native.Context(0) as ctx:
        ctx.set_levels(LevelTable(fourth.V))
        x0 = torch.empty(K, nt, fourth.NX, dtype=torch.float64, device="cuda")
        ctx.rand_start_tensor(x0, seed=4)
        ctx.synchronize()
        vals, u, iters = TRM_batch(prob, par, x0=x0)
        ub = u.cpu().numpy()
        assert not np.array_equal(ub, x0.cpu().numpy())
        for k in range(K):
            obj = program_objective(fourth.FourthObj(nt=nt, T1=T1), prog, ctx, fourth.STATE0, fourth.PARAMS)
            J = mioc.TRM(obj, par, x0=x0[k].cpu().numpy().T.copy())
            assert J == vals[k], (k, J, vals[k])
            assert np.array_equal(obj.x, ub[k].T), k
    print(f"midpoint m=2: iterations per restart {iters.tolist()}")
