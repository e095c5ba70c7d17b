"""GPU tier of the terminal cost, the sampled data and the state output of user-defined ODE objectives
(mioc_ode_program_create_bolza, mioc_ode_program_eval_bolza_device; the contract: include/mioc.h, "Terminal cost,
sampled data, state output").

The device kernels are compared with the host mirror (tests/ode_bolza_mirror.py) on tests/ode_bolza_problem.py at the
bar of test_gpu_ode_program.py (1e-12 relative for J, 1e-12 of the maximum for df and Y): a miss means the operation
order or a data column differs from the documented one.  Then the hand-derived known answer, edge shapes, independence
of K, derived against hand-written hooks, the features switched off, the refusals of the entries, and TRM_batch /
TRM_mixed_batch against the host loops."""
import ctypes
import math
import types

import numpy as np
import pytest

import mioc
from mioc import native
from mioc.iterators import LevelTable
from mioc.ode_device import DeviceODEProblem, MixedODEProblem, ODEProgram, check_hooks
from mioc.trm_mixed import MixedParameters, TRM_mixed, TRM_mixed_batch

import ode_bolza_problem as bp
import ode_program_problem as fourth
from ode_bolza_mirror import bolza_eval
from ode_gpu_support import assert_at_bar as _assert_at_bar, grid as _grid, program_objective, run_program

pytestmark = pytest.mark.gpu

SCHEMES = [("euler", 1), ("heun", 1), ("rk4", 1), ("rk4", 3), ("beuler", 1), ("midpoint", 2)]
T1 = 0.96


@pytest.fixture(scope="module")
def programs():
    """Every program compiled once per module, by (text key, integrator, substeps)."""
    progs = {}
    texts = {"bolza": (bp.SOURCE, bp.NY, bp.NX, bp.NP, dict(ndata=bp.ND, terminal=True, states=True)),
             "known": (bp.KNOWN_SOURCE, 1, 1, 0, dict(ndata=1, terminal=True, states=True)),
             "fourth": (fourth.SOURCE, fourth.NY, fourth.NX, len(fourth.PARAMS), {}),
             "fourth_e0": (fourth.SOURCE + bp.SOURCE_E0, fourth.NY, fourth.NX, len(fourth.PARAMS),
                           dict(terminal=True))}

    def get(key, integrator, substeps=1):
        k = (key, integrator, substeps)
        if k not in progs:
            text, ny, nx, nparams, kw = texts[key]
            progs[k] = ODEProgram(text, ny, nx, nparams, integrator=integrator, substeps=substeps, **kw)
        return progs[k]
    yield get
    for p in progs.values():
        p.close()


def _run(ctx, prog, x, T1, state0, params, data, want_Y=True, **kw):
    """J, df and Y from NaN-prefilled device buffers (None where not asked for)."""
    return run_program(ctx, prog, x, 0.0, T1, state0, params, data=data, want_Y=want_Y, **kw)


def _run_bolza(ctx, prog, x, T1, **kw):
    return _run(ctx, prog, x, T1, bp.STATE0, bp.PARAMS, bp.make_data(x.shape[1]), **kw)


def _mirror(x, T1, integrator, substeps):
    K, nt, _ = x.shape
    data = bp.make_data(nt)
    Jh, dfh, Yh = np.empty(K), np.empty((K, nt, bp.NX)), np.empty((K, nt + 1, bp.NY))
    for k in range(K):
        Jh[k], dfh[k], Yh[k] = bolza_eval(bp.HOOKS, bp.PARAMS, data, bp.STATE0, 0.0, T1, x[k], integrator, substeps)
    return Jh, dfh, Yh


@pytest.fixture(scope="module")
def x70():
    x = _grid(70, 24, 5)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def device70(programs, x70):
    """The device's J, df and Y of the K = 70 call (nt = 24, T1 = 0.96) per scheme, computed once."""
    out = {}
    with native.Context(0) as ctx:
        for integrator, m in SCHEMES:
            out[integrator, m] = _run_bolza(ctx, programs("bolza", integrator, m), x70, T1)
    return out


@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_device_vs_mirror(programs, x70, device70, integrator, substeps):
    """K = 70: one full block and a partial one of 6 lanes."""
    J, df, Y = device70[integrator, substeps]
    _assert_at_bar((J, df, Y), _mirror(x70, T1, integrator, substeps), f"{integrator} m={substeps}")
    assert np.array_equal(Y[:, 0, :], np.tile(bp.STATE0, (70, 1)))
    prog = programs("bolza", integrator, substeps)
    with native.Context(0) as ctx:
        J1, none, Y1 = _run_bolza(ctx, prog, x70, T1, want_df=False)          # d_df NULL
        assert none is None and np.array_equal(J1, J) and np.array_equal(Y1, Y)
        n1, n2, Y2 = _run_bolza(ctx, prog, x70, T1, want_J=False, want_df=False)  # d_J and d_df NULL
        assert n1 is None and n2 is None and np.array_equal(Y2, Y)
        J3, df3, none = _run_bolza(ctx, prog, x70, T1, want_Y=False)           # d_Y NULL
        assert none is None and np.array_equal(J3, J) and np.array_equal(df3, df)


@pytest.mark.parametrize("integrator,substeps", [("euler", 1), ("heun", 1), ("heun", 2), ("beuler", 1),
                                                 ("midpoint", 1), ("rk4", 1), ("rk4", 2)])
def test_known_answer(programs, integrator, substeps):
    """F = d x, G = d x, E = 2 y on the data 1, 2, 4, 8: every value exact, RK4 at the 1e-12 bar (its b weights do not
    sum to 1 in doubles).  K = 3 copies of the one control."""
    kn = bp.KNOWN
    x = np.ascontiguousarray(np.tile(np.array(kn["x"])[None], (3, 1, 1)))
    with native.Context(0) as ctx:
        J, df, Y = _run(ctx, programs("known", integrator, substeps), x, kn["T1"], kn["state0"], [], kn["data"])
    Jx = kn["J_euler"] if integrator == "euler" else kn["J_other"]
    print(integrator, substeps, J.tolist(), df[0, :, 0].tolist(), Y[0, :, 0].tolist())
    for k in range(3):
        if integrator == "rk4":
            assert abs(J[k] - Jx) <= 1e-12 * Jx
            assert np.max(np.abs(df[k, :, 0] - kn["df"])) <= 1e-12 * max(kn["df"])
            assert np.max(np.abs(Y[k, :, 0] - kn["Y"])) <= 1e-12 * max(kn["Y"])
        else:
            assert J[k] == Jx and df[k, :, 0].tolist() == kn["df"] and Y[k, :, 0].tolist() == kn["Y"]


@pytest.mark.parametrize("nt", [1, 2])
@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_edge_shapes(programs, integrator, substeps, nt):
    x = _grid(3, nt, 20 + nt)
    with native.Context(0) as ctx:
        dev = _run_bolza(ctx, programs("bolza", integrator, substeps), x, 0.04 * nt)
    _assert_at_bar(dev, _mirror(x, 0.04 * nt, integrator, substeps), f"{integrator} m={substeps} nt={nt}")


@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_independent_of_K_and_position(programs, x70, device70, integrator, substeps):
    J, df, Y = device70[integrator, substeps]
    prog = programs("bolza", integrator, substeps)
    big = _grid(130, 24, 6)
    big[129], big[64] = x70[0], x70[69]  # the first restart at the far end, the last one at a block's start
    with native.Context(0) as ctx:
        for k in (0, 37, 69):
            J1, df1, Y1 = _run_bolza(ctx, prog, x70[k:k + 1], T1)
            assert J1[0] == J[k] and np.array_equal(df1[0], df[k]) and np.array_equal(Y1[0], Y[k]), k
        Jb, dfb, Yb = _run_bolza(ctx, prog, big, T1)
    assert Jb[129] == J[0] and np.array_equal(dfb[129], df[0]) and np.array_equal(Yb[129], Y[0])
    assert Jb[64] == J[69] and np.array_equal(dfb[64], df[69]) and np.array_equal(Yb[64], Y[69])


@pytest.mark.parametrize("integrator,substeps", [("euler", 1), ("rk4", 2)])
def test_derived_against_hand_written(x70, integrator, substeps):
    import torch
    x = torch.tensor(x70[:5], dtype=torch.float64, device="cuda")
    data = torch.tensor(bp.make_data(24), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with native.Context(0) as ctx:
        args = (bp.NY, bp.NX, bp.NP, x, 0.0, T1, bp.STATE0, bp.PARAMS)
        kw = dict(integrator=integrator, substeps=substeps, ndata=bp.ND, terminal=True, data=data)
        good = check_hooks(ctx, bp.SOURCE, *args, **kw)
        print(good)
        assert good.pop("J_equal") is True
        assert set(good) == {"all", "Fy", "Fu", "Gy", "Gu", "Ey"} and all(v < 1e-12 for v in good.values()), good
        if integrator == "euler":
            return
        bad = check_hooks(ctx, bp.SOURCE_WRONG_EY, *args, **kw)
        print(bad)
        assert bad.pop("J_equal") is True
        assert bad["Ey"] > 1e-3 and bad["all"] > 1e-3
        assert all(bad[n] < 1e-12 for n in ("Fy", "Fu", "Gy", "Gu")), bad


def test_called_hooks_with_data_have_an_exact_gradient():
    """The largest shape (ny = nx = 8, NP = 32, ND = 16), every hook derived, Heun with 2 substeps: the generated hooks
    are compiled as called functions and handed the address of the per-lane p.  The criterion of
    test_device_gradient_is_exact (test_gpu_ode_integrators.py) on the device's own J and df, with E and the data
    in J: x and x + t h for t = 1e-4, 1e-5, 1e-6 are 4 restarts of one call."""
    n, nt, T = 8, 12, 1.2
    rng = np.random.default_rng(7)
    params = (0.1 + 0.02 * np.arange(32)).tolist()
    data = (0.05 + 0.01 * rng.integers(0, 9, size=(nt, 16))).tolist()
    state0 = (0.1 * (1 + np.arange(n) % 3)).tolist()
    x = np.full((nt, n), 0.5)
    h = rng.standard_normal((nt, n))
    ts = (1e-4, 1e-5, 1e-6)
    X = np.ascontiguousarray(np.stack([x] + [x + t * h for t in ts]))
    with ODEProgram(bp.synthetic_source(n, 32, 16), n, n, 32, integrator="heun", substeps=2, derive="all", ndata=16,
                    terminal=True, states=True) as prog, native.Context(0) as ctx:
        assert prog.log.startswith("mioc_ad:") and "compiled as functions" in prog.log
        J, df, Y = _run(ctx, prog, X, T, state0, params, data)
        Jq, _, _ = _run(ctx, prog, X[:1], T, state0, params, [[0.0] * 16] * nt, want_df=False, want_Y=False)
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(df)) and np.array_equal(Y[:, 0, :], np.tile(state0, (4, 1)))
    assert Jq[0] != J[0]  # the data are in J
    dfh = (T / nt) * float(np.sum(df[0] * h))
    errs = [(abs((J[1 + q] - J[0]) / t - dfh), abs(dfh)) for q, t in enumerate(ts)]
    print(errs)
    scale = max(1e-12, errs[0][1])
    assert errs[2][0] <= 1e-4 * scale + 1e-9, errs
    assert errs[1][0] <= errs[0][0] * 0.5 + 1e-9, errs


def _raw(lib, h, ny, nx, nparams):
    """A program handle made through the C entry, in the shape Context.ode_program_eval_tensors takes."""
    return types.SimpleNamespace(h=h, ny=ny, nx=nx, nparams=nparams, ndata=0, states=False)


def test_features_off_is_create_ad(x70):
    """_bolza(ndata = 0, flags = 0) against _create_ad on the fourth problem: bit-equal J and df."""
    lib = native.load_library()
    ny, nx, nparams = fourth.NY, fourth.NX, len(fourth.PARAMS)
    ha, hb = ctypes.c_void_p(), ctypes.c_void_p()
    text = fourth.SOURCE.encode()
    assert lib.mioc_ode_program_create_ad(text, ny, nx, nparams, native.MIOC_ODE_INT_EULER, 1, 0, ctypes.byref(ha),
                                          None, 0) == native.MIOC_OK
    assert lib.mioc_ode_program_create_bolza(text, ny, nx, nparams, 0, native.MIOC_ODE_INT_EULER, 1, 0, 0,
                                             ctypes.byref(hb), None, 0) == native.MIOC_OK
    try:
        with native.Context(0) as ctx:
            res = [_run(ctx, _raw(lib, h, ny, nx, nparams), x70, T1, fourth.STATE0, fourth.PARAMS, None, want_Y=False)
                   for h in (ha, hb)]
    finally:
        assert lib.mioc_ode_program_destroy(ha) == native.MIOC_OK
        assert lib.mioc_ode_program_destroy(hb) == native.MIOC_OK
    assert np.all(np.isfinite(res[0][0])) and np.all(np.isfinite(res[0][1]))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_terminal_with_zero_E_is_the_plain_program(programs, x70):
    with native.Context(0) as ctx:
        plain = _run(ctx, programs("fourth", "heun", 1), x70, T1, fourth.STATE0, fourth.PARAMS, None, want_Y=False)
        e0 = _run(ctx, programs("fourth_e0", "heun", 1), x70, T1, fourth.STATE0, fourth.PARAMS, None, want_Y=False)
    assert np.all(np.isfinite(plain[0])) and np.all(np.isfinite(plain[1]))
    assert np.array_equal(plain[0], e0[0]) and np.array_equal(plain[1], e0[1])


def test_refusals_of_the_device_entries(programs, x70):
    import torch
    lib = native.load_library()
    prog, plain = programs("bolza", "heun", 1), programs("fourth", "heun", 1)
    x = torch.tensor(x70[:4], dtype=torch.float64, device="cuda")
    data = torch.tensor(bp.make_data(24), dtype=torch.float64, device="cuda")
    J = torch.full((4,), math.nan, dtype=torch.float64, device="cuda")
    Y = torch.full((4, 25, 3), math.nan, dtype=torch.float64, device="cuda")
    y0, par = np.array(bp.STATE0), np.array(bp.PARAMS)
    y4, par4 = np.array(fourth.STATE0, dtype=np.float64), np.array(fourth.PARAMS, dtype=np.float64)
    torch.cuda.synchronize()

    def vp(t):
        return ctypes.c_void_p(t.data_ptr())

    def hp(a):
        return ctypes.c_void_p(a.ctypes.data)
    with native.Context(0) as ctx:
        head = (4, vp(x), 24, 0.0, T1)
        # ndata > 0 with d_data NULL
        assert lib.mioc_ode_program_eval_bolza_device(ctx.h, prog.h, 0, *head, hp(y0), hp(par), None, vp(J), None,
                                                      None) == native.MIOC_EINVAL
        # d_Y on a program without MIOC_ODE_STATES
        assert lib.mioc_ode_program_eval_bolza_device(ctx.h, plain.h, 0, *head, hp(y4), hp(par4), None, vp(J), None,
                                                      vp(Y)) == native.MIOC_EINVAL
        # the two existing entries on a program with ndata > 0
        assert lib.mioc_ode_program_eval_device(ctx.h, prog.h, *head, hp(y0), hp(par), vp(J),
                                                None) == native.MIOC_EINVAL
        assert lib.mioc_ode_program_eval_mixed_device(ctx.h, prog.h, 1, *head, hp(y0), hp(par), vp(J),
                                                      None) == native.MIOC_EINVAL
        with pytest.raises(native.MiocNativeError):
            ctx.ode_program_eval_tensors(prog, x, 0.0, T1, bp.STATE0, bp.PARAMS, J)
        with pytest.raises(ValueError):
            ctx.ode_program_eval_tensors(plain, x, 0.0, T1, fourth.STATE0, fourth.PARAMS, J, Y=Y)
        with pytest.raises(ValueError):  # data of another nt
            ctx.ode_program_eval_tensors(prog, x, 0.0, T1, bp.STATE0, bp.PARAMS, J, data=data[:23].contiguous())
        ctx.synchronize()
        assert bool(torch.isnan(J).all()) and bool(torch.isnan(Y).all())  # nothing ran
        # the context stays usable, and so does the mixed check of the new entry
        ctx.ode_program_eval_mixed_tensors(prog, 1, x, 0.0, T1, bp.STATE0, bp.PARAMS, J, data=data, Y=Y)
        ctx.synchronize()
        Jd, _, Yd = _run_bolza(ctx, prog, x70[:4], T1, want_df=False)
        assert np.array_equal(J.cpu().numpy(), Jd) and np.array_equal(Y.cpu().numpy(), Yd)
        # the existing entries on a program with the terminal flag and ndata == 0
        ctx.ode_program_eval_tensors(programs("fourth_e0", "heun", 1), x, 0.0, T1, fourth.STATE0, fourth.PARAMS, J)
        ctx.synchronize()
        assert bool(torch.isfinite(J).all())


def test_trm_batch_equals_sequential_trm(programs):
    import torch
    from mioc.trm_batch import TRM_batch
    K, nt = 6, 48
    prog = programs("bolza", "rk4", 2)
    par = mioc.TRM_parameters(beta=1e-3, Delta0=0.25, p=1, maxiter=4, kmax=4)
    rows = bp.make_data(nt)
    prob = DeviceODEProblem(prog, bp.V, None, 0.0, T1, nt, bp.STATE0, bp.PARAMS, data=rows)
    with pytest.raises(ValueError):
        TRM_batch(prob, par, K=2, nt=nt + 1)
    with native.Context(0) as ctx:
        ctx.set_levels(LevelTable(bp.V))
        x0 = torch.empty(K, nt, bp.NX, dtype=torch.float64, device="cuda")
        ctx.rand_start_tensor(x0, seed=4)
        ctx.synchronize()
        vals, u, iters = TRM_batch(prob, par, x0=x0)
        assert len(prob._device_data) == 1  # uploaded once, kept
        ub = u.cpu().numpy()
        assert not np.array_equal(ub, x0.cpu().numpy())
        data = torch.tensor(rows, dtype=torch.float64, device="cuda")
        for k in range(K):
            obj = program_objective(bp.BolzaObj(nt=nt, T1=T1), prog, ctx, bp.STATE0, bp.PARAMS, data=data,
                                    sync_torch=True)
            J = mioc.TRM(obj, par, x0=x0[k].cpu().numpy().T.copy())
            assert J == vals[k], (k, J, vals[k])
            assert np.array_equal(obj.x, ub[k].T), k
        # the states of the solution: row 0 is state0, and E of the last row is the E inside J
        Y = prob.states(ctx, u).cpu().numpy()
        assert Y.shape == (K, nt + 1, bp.NY) and np.array_equal(Y[:, 0, :], np.tile(bp.STATE0, (K, 1)))
        J = torch.empty(K, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        prob.eval_tensors(ctx, u, J)
        with ODEProgram(bp.SOURCE, bp.NY, bp.NX, bp.NP, integrator="rk4", substeps=2, ndata=bp.ND) as noE:
            q = torch.empty(K, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            ctx.ode_program_eval_tensors(noE, u, 0.0, T1, bp.STATE0, bp.PARAMS, q, data=data)
            ctx.synchronize()
        tau = (T1 - 0.0) / nt
        tend = 0.0 + float(nt * 2) * (tau / 2)
        pe = bp.PARAMS + rows[nt - 1]
        want = [q[k].item() + bp.HOOKS.E(pe, tend, Y[k, nt].tolist()) for k in range(K)]
        print("J = q + E(Y[nt]):", [J[k].item() == want[k] for k in range(K)])
        for k in range(K):  # q of the same text without the terminal flag; the bar of the mirror comparison
            assert abs(J[k].item() - want[k]) <= 1e-12 * abs(want[k]), (k, J[k].item(), want[k])
            assert abs(want[k] - q[k].item()) > 1e-3 * abs(want[k]), "E is a visible part of J"
    print(f"bolza rk4 m=2: iterations per restart {iters.tolist()}")


def test_trm_mixed_batch_equals_host_loop(programs):
    import torch
    K, nt, nu = 4, 32, bp.MIXED_NU
    prog = programs("bolza", "rk4", 2)
    par, cpar = mioc.TRM_parameters(beta=1e-3, Delta0=0.25, p=1, maxiter=4, kmax=4), MixedParameters(R=4)
    rows = bp.make_data(nt)
    prob = MixedODEProblem(prog, nu, bp.MIXED_LO, bp.MIXED_HI, bp.MIXED_V, None, 0.0, T1, nt, bp.STATE0, bp.PARAMS,
                           data=rows)
    rng = np.random.default_rng(3)
    x0 = np.ascontiguousarray(np.stack([rng.uniform(bp.MIXED_LO, bp.MIXED_HI, size=(K, nt)),
                                        rng.integers(0, 2, size=(K, nt)).astype(np.float64)], axis=2))
    stats = {}
    vals, x, iters = TRM_mixed_batch(prob, par, cpar, x0=torch.tensor(x0, dtype=torch.float64, device="cuda"),
                                     stats=stats)
    xb = x.cpu().numpy()
    assert not np.array_equal(xb, x0)
    assert np.all(xb[:, :, 0] >= bp.MIXED_LO) and np.all(xb[:, :, 0] <= bp.MIXED_HI)
    assert np.all(np.isin(xb[:, :, 1], bp.MIXED_V[0]))
    with native.Context(0) as ctx:
        data = torch.tensor(rows, dtype=torch.float64, device="cuda")
        for k in range(K):
            obj = program_objective(bp.BolzaMixedObj(nt=nt, T1=T1), prog, ctx, bp.STATE0, bp.PARAMS, data=data, nu=nu,
                                    sync_torch=True)
            st = {}
            J = TRM_mixed(obj, par, cpar, x0=x0[k].T, stats=st)
            assert J == vals[k], (k, J, vals[k])
            assert np.array_equal(obj.x, xb[k].T), k
            assert st["iters"] == iters[k] and st["csteps"] == stats["csteps"][k], (k, st["iters"], iters[k])
        ctx.set_levels(LevelTable(bp.MIXED_V))
        Y = prob.states(ctx, x).cpu().numpy()
        assert Y.shape == (K, nt + 1, bp.NY) and np.array_equal(Y[:, 0, :], np.tile(bp.STATE0, (K, 1)))
        assert np.all(np.isfinite(Y))
    print(f"bolza mixed: iterations per restart {iters.tolist()}, continuous steps {stats['csteps'].tolist()}")
