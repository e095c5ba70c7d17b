"""GPU tier of the Heun / RK4 integrators of user-defined ODE objectives (mioc_ode_program_create_ex; the scheme and
its rounding order: include/mioc.h, "Integrators").

The device kernel is compared with the host mirror (tests/ode_rk_mirror.py) on the tests' fourth problem at the bar of
test_gpu_ode_program.py (1e-12 relative for J, 1e-12 of max|df|): a miss means the operation order differs from the
documented one.  Then independence of K, the finite-difference criterion and the order on the device's own numbers,
the untouched default scheme, scratch growth, and TRM_batch against the sequential TRM."""
import math

import numpy as np
import pytest

import mioc
from mioc import native
from mioc.iterators import LevelTable
from mioc.ode_device import EXAMPLE_PARAMS, EXAMPLE_SHAPES, EXAMPLE_SOURCES, EXAMPLE_STATE0, DeviceODEProblem, ODEProgram

import ode_program_problem as fourth
from ode_gpu_support import assert_at_bar, grid as _grid, program_objective, run_program
from ode_rk_mirror import ORDER_BANDS, order_control, rk_eval

pytestmark = pytest.mark.gpu

SCHEMES = [("heun", 1), ("rk4", 1), ("rk4", 3)]


@pytest.fixture(scope="module")
def programs():
    """Every program of the fourth problem compiled once per module, by (integrator, substeps)."""
    progs = {}

    def get(integrator, substeps):
        key = (integrator, substeps)
        if key not in progs:
            progs[key] = ODEProgram(fourth.SOURCE, fourth.NY, fourth.NX, len(fourth.PARAMS), integrator=integrator,
                                    substeps=substeps)
        return progs[key]
    yield get
    for p in progs.values():
        p.close()


def _run(ctx, prog, x, T1, **kw):
    """J and df of the fourth problem from NaN-prefilled device buffers (None where not asked for)."""
    return run_program(ctx, prog, x, 0.0, T1, fourth.STATE0, fourth.PARAMS, **kw)[:2]


def _mirror(x, T1, integrator, substeps):
    K, nt, _ = x.shape
    obj = fourth.FourthObj(nt=nt, T1=T1)
    Jh, dfh = np.empty(K), np.empty((K, nt, fourth.NX))
    for k in range(K):
        Jh[k], d = rk_eval(obj, x[k].T, integrator, substeps)
        dfh[k] = d.T
    return Jh, dfh


@pytest.fixture(scope="module")
def x70():
    x = _grid(70, 24, 5)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def device70(programs, x70):
    """The device's J and df of the K = 70 call (nt = 24, T1 = 0.96) per scheme, computed once."""
    out = {}
    with native.Context(0) as ctx:
        for integrator, m in SCHEMES:
            out[integrator, m] = _run(ctx, programs(integrator, m), x70, 0.96)
    return out


@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_fourth_problem_vs_mirror(programs, x70, device70, integrator, substeps):
    """K = 70: one full block and a partial one of 6 lanes."""
    J, df = device70[integrator, substeps]
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(df))
    Jh, dfh = _mirror(x70, 0.96, integrator, substeps)
    exact = sum(int(J[k] == Jh[k]) + int(np.array_equal(df[k], dfh[k])) for k in range(70))
    print(f"{integrator} m={substeps}: {exact} of 140 J / df arrays bit-identical to the mirror")
    assert_at_bar((J, df), (Jh, dfh))
    assert np.all(df[:, :, 1] != 0.0)  # Gu[1] = 0.1 y0 is in every column
    with native.Context(0) as ctx:
        J1, none = _run(ctx, programs(integrator, substeps), x70, 0.96, want_df=False)  # d_df NULL: no states stored
        assert none is None and np.array_equal(J1, J)
        none, df1 = _run(ctx, programs(integrator, substeps), x70, 0.96, want_J=False)  # d_J NULL
        assert none is None and np.array_equal(df1, df)


@pytest.mark.parametrize("nt", [1, 2])
@pytest.mark.parametrize("integrator,substeps", [("heun", 1), ("heun", 3), ("rk4", 1), ("rk4", 3)])
def test_edge_shapes(programs, integrator, substeps, nt):
    x = _grid(3, nt, 20 + nt)
    T1 = 0.04 * nt
    with native.Context(0) as ctx:
        J, df = _run(ctx, programs(integrator, substeps), x, T1)
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(df))
    assert_at_bar((J, df), _mirror(x, T1, integrator, substeps))


@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_independent_of_K_and_position(programs, x70, device70, integrator, substeps):
    J, df = device70[integrator, substeps]
    prog = programs(integrator, substeps)
    big = _grid(130, 24, 6)
    big[129], big[64] = x70[0], x70[69]  # the first restart at the far end, the last one at a block's start
    with native.Context(0) as ctx:
        for k in (0, 37, 69):
            J1, df1 = _run(ctx, prog, x70[k:k + 1], 0.96)
            assert J1[0] == J[k] and np.array_equal(df1[0], df[k]), k
        Jb, dfb = _run(ctx, prog, big, 0.96)
    assert Jb[129] == J[0] and np.array_equal(dfb[129], df[0])
    assert Jb[64] == J[69] and np.array_equal(dfb[64], df[69])


def test_device_gradient_is_exact(programs):
    """The criterion of test_ode_oracle.py:28-32 on the device's own J and df (RK4, 2 substeps): x and x + t h for
    t = 1e-4, 1e-5, 1e-6 are 4 restarts of one call."""
    nt, T1 = 24, 4.8
    rng = np.random.default_rng(7)
    x = np.full((nt, fourth.NX), 0.5)
    h = rng.standard_normal((nt, fourth.NX))
    ts = (1e-4, 1e-5, 1e-6)
    X = np.ascontiguousarray(np.stack([x] + [x + t * h for t in ts]))
    with native.Context(0) as ctx:
        J, df = _run(ctx, programs("rk4", 2), X, T1)
    dfh = (T1 / nt) * float(np.sum(df[0] * h))
    errs = [(abs((J[1 + q] - J[0]) / t - dfh), abs(dfh)) for q, t in enumerate(ts)]
    print(errs)
    scale = max(1e-12, errs[0][1])
    assert errs[2][0] <= 1e-4 * scale + 1e-9, errs
    assert errs[1][0] <= errs[0][0] * 0.5 + 1e-9, errs


@pytest.mark.parametrize("integrator", ["heun", "rk4"])
def test_device_order(programs, integrator):
    """Errors of the device's J at substeps 1, 2, 4 against its RK4 at 64 substeps: the bands of the CPU tier."""
    x = np.ascontiguousarray(order_control(24).T[None])
    with native.Context(0) as ctx:
        ref = _run(ctx, programs("rk4", 64), x, 0.96, want_df=False)[0][0]
        e = [abs(_run(ctx, programs(integrator, m), x, 0.96, want_df=False)[0][0] - ref) for m in (1, 2, 4)]
    lo, hi = ORDER_BANDS[integrator]
    print(integrator, e, e[0] / e[1], e[1] / e[2])
    assert lo <= e[0] / e[1] <= hi and lo <= e[1] / e[2] <= hi, e


def test_default_scheme_untouched():
    """A program from _ex(..., EULER, 1) against one from mioc_ode_program_create: the fishing hooks, K = 70, nt = 64."""
    import ctypes

    import torch
    lib = native.load_library()
    name = "fishing"
    rng = np.random.default_rng(75)
    x = torch.tensor(np.eye(3)[rng.integers(0, 3, size=(70, 64))], dtype=torch.float64, device="cuda")
    res = []
    with ODEProgram(EXAMPLE_SOURCES[name], *EXAMPLE_SHAPES[name]) as plain, native.Context(0) as ctx:
        h = ctypes.c_void_p()
        ny, nx, nparams = EXAMPLE_SHAPES[name]
        rc = lib.mioc_ode_program_create_ex(EXAMPLE_SOURCES[name].encode(), ny, nx, nparams,
                                            native.MIOC_ODE_INT_EULER, 1, ctypes.byref(h), None, 0)
        assert rc == native.MIOC_OK and h.value
        y0 = np.array(EXAMPLE_STATE0[name], dtype=np.float64)
        par = np.array(EXAMPLE_PARAMS[name], dtype=np.float64)
        try:
            for handle in (plain.h, h):
                J = torch.full((70,), math.nan, dtype=torch.float64, device="cuda")
                df = torch.full_like(x, math.nan)
                torch.cuda.synchronize()
                rc = lib.mioc_ode_program_eval_device(ctx.h, handle, 70, ctypes.c_void_p(x.data_ptr()), 64, 0.0, 0.64,
                                                      ctypes.c_void_p(y0.ctypes.data), ctypes.c_void_p(par.ctypes.data),
                                                      ctypes.c_void_p(J.data_ptr()), ctypes.c_void_p(df.data_ptr()))
                assert rc == native.MIOC_OK
                ctx.synchronize()
                res.append((J.cpu().numpy(), df.cpu().numpy()))
        finally:
            assert lib.mioc_ode_program_destroy(h) == native.MIOC_OK
    assert np.all(np.isfinite(res[0][0])) and np.all(np.isfinite(res[0][1]))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_scratch_growth_equals_fresh_context(programs):
    prog = programs("rk4", 3)
    xs, xl = _grid(4, 16, 1), _grid(130, 96, 2)
    with native.Context(0) as ctx:
        _run(ctx, prog, xs, 0.16)
        J1, df1 = _run(ctx, prog, xl, 0.96)
    with native.Context(0) as ctx:
        J2, df2 = _run(ctx, prog, xl, 0.96)
    assert np.all(np.isfinite(J1)) and np.all(np.isfinite(df1))
    assert np.array_equal(J1, J2) and np.array_equal(df1, df2)


def test_trm_batch_rk4_equals_sequential_trm(programs):
    """The parameters of test_gpu_ode_program.py::test_trm_batch_fourth_problem_equals_sequential_trm on a coarser
    control grid (nt = 48) with RK4 and 2 substeps."""
    import torch
    from mioc.trm_batch import TRM_batch
    K, nt, T1 = 6, 48, 0.96
    prog = programs("rk4", 2)
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
    print(f"rk4 m=2: iterations per restart {iters.tolist()}")
