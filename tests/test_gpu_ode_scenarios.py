"""GPU tier of scenarios for user-defined ODE objectives (mioc_ode_program_create_scen,
mioc_ode_program_eval_scen_device; the contract: include/mioc.h, "Scenarios"): the lane of restart q solves scenario
q % S with its own state0, parameters and (MIOC_ODE_SCEN_DATA) data rows, and computes bit for bit what the program
without scenarios computes from those values.

The yardstick is the scen = 0 program of the same text in the same process, which test_gpu_ode_bolza.py holds to the
host mirror; six lanes are also held to the mirror (tests/ode_bolza_mirror.py) directly, at the project's bar.  The
problem is tests/ode_bolza_problem.py, the scenario draws are tests/ode_scenario_support.py's."""
import ctypes
import math

import numpy as np
import pytest

import mioc
from mioc import native
from mioc.ode_device import DeviceODEProblem, MixedODEProblem, ODEProgram, best_per_scenario
from mioc.trm_mixed import MixedParameters, TRM_mixed_batch

import ode_bolza_problem as bp
from ode_bolza_mirror import bolza_eval
from ode_gpu_support import assert_at_bar, grid, run_program
from ode_scenario_support import (NODATA_NP, NODATA_SOURCE, draw_scenarios, run_scen, uniform_scenarios)

pytestmark = pytest.mark.gpu

SCHEMES = [("euler", 1), ("heun", 1), ("rk4", 2), ("beuler", 1), ("midpoint", 2)]
T1 = 0.96
TEXTS = {"bolza": (bp.SOURCE, bp.NY, bp.NX, bp.NP, dict(ndata=bp.ND, terminal=True, states=True)),
         "nodata": (NODATA_SOURCE, bp.NY, bp.NX, NODATA_NP, dict(terminal=True, states=True)),
         "known": (bp.KNOWN_SOURCE, 1, 1, 0, dict(ndata=1, terminal=True, states=True))}


@pytest.fixture(scope="module")
def programs():
    """Every program compiled once per module, by (text key, integrator, substeps, scenarios, derive)."""
    progs = {}

    def get(key, integrator, substeps=1, scenarios=False, derive=()):
        k = (key, integrator, substeps, scenarios, derive)
        if k not in progs:
            text, ny, nx, nparams, kw = TEXTS[key]
            progs[k] = ODEProgram(text, ny, nx, nparams, integrator=integrator, substeps=substeps, derive=derive,
                                  scenarios=scenarios, **kw)
        return progs[k]
    yield get
    for p in progs.values():
        p.close()


def _same(got, want):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want))


# ---- 1. uniform scenarios: the program without scenarios, bit for bit ------------------------------------------------
@pytest.mark.parametrize("derive", [(), "all"], ids=["hand", "derived"])
@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_uniform_scenarios_are_the_plain_program(programs, integrator, substeps, derive):
    """K = 130 (two full blocks and two lanes), S = 1, 65 (q % S wraps inside a wave) and 130."""
    K, nt = 130, 8
    x = grid(K, nt, 31)
    with native.Context(0) as ctx:
        base = run_program(ctx, programs("bolza", integrator, substeps, False, derive), x, 0.0, T1, bp.STATE0,
                           bp.PARAMS, data=bp.make_data(nt), want_Y=True)
        assert all(np.all(np.isfinite(a)) for a in base)
        for scenarios in (True, "data"):
            prog = programs("bolza", integrator, substeps, scenarios, derive)
            for S in (1, 65, 130):
                y0, par, data = uniform_scenarios(S, nt)
                got = run_scen(ctx, prog, x, 0.0, T1, y0, par, data if scenarios == "data" else data[0])
                assert _same(got, base), (scenarios, S)


# ---- 2. distinct scenarios ---------------------------------------------------------------------------------------------
S2, K2, NT2 = 67, 134, 12   # S prime, more than one wave, a partial block; two controls per scenario
VARIANTS = {"nodata": ("nodata", True), "shared": ("bolza", True), "data": ("bolza", "data")}


def _inputs2(variant):
    y0, par, data = draw_scenarios(S2, NT2, nodata=variant == "nodata")
    if variant == "shared":
        data = np.array(bp.make_data(NT2))
    return grid(K2, NT2, 41), y0, par, data


@pytest.fixture(scope="module")
def distinct(programs):
    """The scenario program's J, df and Y of the K = 134 call, per (variant, integrator, substeps), computed once."""
    cache = {}

    def get(variant, integrator, substeps):
        key = (variant, integrator, substeps)
        if key not in cache:
            text, scenarios = VARIANTS[variant]
            x, y0, par, data = _inputs2(variant)
            with native.Context(0) as ctx:
                cache[key] = run_scen(ctx, programs(text, integrator, substeps, scenarios), x, 0.0, T1, y0, par, data)
        return cache[key]
    return get


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_distinct_scenarios(programs, distinct, integrator, substeps, variant):
    """Lane q against a K = 1 call of the scen = 0 program with scenario q % 67's values, bit for bit; lanes 0, 63, 64,
    66, 67 and 133 also against the host mirror."""
    J, df, Y = distinct(variant, integrator, substeps)
    x, y0, par, data = _inputs2(variant)
    plain = programs(VARIANTS[variant][0], integrator, substeps, False)

    def rows(s):
        return None if data is None else data if data.ndim == 2 else data[s]
    with native.Context(0) as ctx:
        for q in range(K2):
            s = q % S2
            J1, df1, Y1 = run_program(ctx, plain, x[q:q + 1], 0.0, T1, y0[s], par[s], data=rows(s), want_Y=True)
            assert J1[0] == J[q] and np.array_equal(df1[0], df[q]) and np.array_equal(Y1[0], Y[q]), q
    lanes = [0, 63, 64, 66, 67, 133]
    ref = [bolza_eval(bp.HOOKS, par[q % S2].tolist(), rows(q % S2), y0[q % S2].tolist(), 0.0, T1, x[q], integrator,
                      substeps) for q in lanes]
    assert_at_bar((J[lanes], df[lanes], Y[lanes]), tuple(np.array([r[n] for r in ref]) for n in range(3)),
                  f"{variant} {integrator} m={substeps}")
    assert not np.array_equal(J[:S2], J[S2:])  # the two controls of a scenario differ


# ---- 3. the known answer --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,substeps", [("euler", 1), ("heun", 2), ("beuler", 1), ("midpoint", 1), ("rk4", 1)])
def test_known_answer_with_shifted_state0(programs, integrator, substeps):
    """F = d x, G = d x, E = 2 y (NP = 0: d_params is NULL) from state0 = 0.5, 1.5, -0.25: df is the known one, Y is
    shifted by the difference and J by exactly twice the difference.  All values are dyadic, so every scheme but RK4
    is exact; RK4 at the 1e-12 bar of test_gpu_ode_bolza.py::test_known_answer (its b weights do not sum to 1)."""
    kn, starts = bp.KNOWN, [0.5, 1.5, -0.25]
    x = np.ascontiguousarray(np.tile(np.array(kn["x"])[None], (6, 1, 1)))
    with native.Context(0) as ctx:
        J, df, Y = run_scen(ctx, programs("known", integrator, substeps, True), x, kn["T0"], kn["T1"],
                            np.array(starts)[:, None], np.zeros((3, 0)), np.array(kn["data"]))
    Jx = kn["J_euler"] if integrator == "euler" else kn["J_other"]
    print(integrator, substeps, J.tolist(), Y[:, :, 0].tolist())
    for k in range(6):
        d = starts[k % 3] - kn["state0"][0]
        Jk, Yk = Jx + 2.0 * d, [v + d for v in kn["Y"]]
        if integrator == "rk4":
            assert abs(J[k] - Jk) <= 1e-12 * abs(Jk)
            assert np.max(np.abs(df[k, :, 0] - kn["df"])) <= 1e-12 * max(kn["df"])
            assert np.max(np.abs(Y[k, :, 0] - Yk)) <= 1e-12 * max(abs(v) for v in Yk)
        else:
            assert J[k] == Jk and df[k, :, 0].tolist() == kn["df"] and Y[k, :, 0].tolist() == Yk, k


# ---- 4. isolation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,substeps", [("euler", 1), ("rk4", 2), ("beuler", 1)])
def test_a_nan_parameter_stays_in_its_scenario(programs, integrator, substeps):
    S, K, nt = 8, 24, 10
    y0, par, data = draw_scenarios(S, nt, seed=5)
    x = grid(K, nt, 43)
    prog = programs("bolza", integrator, substeps, "data")
    bad_par = par.copy()
    bad_par[5, 0] = math.nan
    with native.Context(0) as ctx:
        clean = run_scen(ctx, prog, x, 0.0, T1, y0, par, data)
        bad = run_scen(ctx, prog, x, 0.0, T1, y0, bad_par, data)
    assert all(np.all(np.isfinite(a)) for a in clean)
    for k in range(K):
        if k % S == 5:
            assert k in (5, 13, 21) and math.isnan(bad[0][k]) and np.all(np.isnan(bad[1][k])), k
        else:
            assert all(np.array_equal(a[k], b[k]) for a, b in zip(bad, clean)), k


# ---- 5. the refusals of the entries ---------------------------------------------------------------------------------
def test_refusals_of_the_device_entries(programs):
    import torch
    lib = native.load_library()
    K, nt, S = 4, 9, 2
    prog, plain = programs("bolza", "heun", 1, "data"), programs("bolza", "heun", 1, False)
    nodata, known = programs("nodata", "heun", 1, True), programs("known", "heun", 1, True)
    y0, par, data = draw_scenarios(S, nt)
    y0n, parn, _ = draw_scenarios(S, nt, nodata=True)
    f64 = dict(dtype=torch.float64, device="cuda")
    x = torch.tensor(grid(K, nt, 3), **f64)
    x1 = x[:, :, :1].contiguous()
    d_y0, d_par = torch.tensor(np.ascontiguousarray(y0.T), **f64), torch.tensor(np.ascontiguousarray(par.T), **f64)
    d_parn = torch.tensor(np.ascontiguousarray(parn.T), **f64)
    d_data = torch.tensor(np.ascontiguousarray(data.transpose(1, 2, 0)), **f64)
    d_rows = torch.tensor(np.ascontiguousarray(data[0]), **f64)
    d_y1 = torch.tensor([[0.5, 1.5]], **f64)
    d_rows1 = torch.tensor(bp.KNOWN["data"] * 3, **f64)[:nt].contiguous()
    J = torch.full((K,), math.nan, **f64)
    torch.cuda.synchronize()

    def vp(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def hp(a):
        return ctypes.c_void_p(a.ctypes.data)

    with native.Context(0) as ctx:
        def scen(p, S_, Y0, P, D, K_=K, xx=x):
            return lib.mioc_ode_program_eval_scen_device(ctx.h, p.h, 0, K_, vp(xx), nt, 0.0, T1, S_, vp(Y0), vp(P),
                                                         vp(D), vp(J), None, None)

        def refused_then_usable(rc):
            assert rc == native.MIOC_EINVAL
            ctx.synchronize()
            assert bool(torch.isnan(J).all())  # nothing ran
            assert scen(prog, S, d_y0, d_par, d_data) == native.MIOC_OK
            ctx.synchronize()
            assert bool(torch.isfinite(J).all())
            J.fill_(math.nan)
            torch.cuda.synchronize()
        refused_then_usable(scen(prog, 0, d_y0, d_par, d_data))        # S < 1
        refused_then_usable(scen(prog, -1, d_y0, d_par, d_data))
        refused_then_usable(scen(prog, 3, d_y0, d_par, d_data))        # K % S != 0
        refused_then_usable(scen(prog, 8, d_y0, d_par, d_data))        # S > K
        refused_then_usable(scen(prog, S, None, d_par, d_data))        # d_state0 NULL
        refused_then_usable(scen(prog, S, d_y0, None, d_data))         # d_params NULL with nparams > 0
        refused_then_usable(scen(prog, S, d_y0, d_par, None))          # d_data NULL with ndata > 0
        refused_then_usable(scen(plain, S, d_y0, d_par, d_rows))       # a program compiled with scen == 0
        # the three older entries refuse a scenario program
        head = (K, vp(x), nt, 0.0, T1)
        refused_then_usable(lib.mioc_ode_program_eval_device(ctx.h, nodata.h, *head, hp(y0n[0]), hp(parn[0]), vp(J),
                                                             None))
        refused_then_usable(lib.mioc_ode_program_eval_mixed_device(ctx.h, nodata.h, 1, *head, hp(y0n[0]), hp(parn[0]),
                                                                   vp(J), None))
        refused_then_usable(lib.mioc_ode_program_eval_bolza_device(ctx.h, prog.h, 0, *head, hp(y0[0]), hp(par[0]),
                                                                   vp(d_rows), vp(J), None, None))
        with pytest.raises(native.MiocNativeError):
            ctx.ode_program_eval_tensors(prog, x, 0.0, T1, y0[0], par[0], J, data=d_rows)
        with pytest.raises(ValueError):  # the Python entry checks K % S itself
            ctx.ode_program_eval_scen_tensors(prog, None, x, 0.0, T1, 3, d_y0, d_par, d_data, J)
        with pytest.raises(ValueError):  # and the size of each array
            ctx.ode_program_eval_scen_tensors(prog, None, x, 0.0, T1, S, d_y0, d_par, d_rows, J)
        with pytest.raises(ValueError):
            ctx.ode_program_eval_scen_tensors(plain, None, x, 0.0, T1, S, d_y0, d_par, d_rows, J)
        ctx.synchronize()
        assert bool(torch.isnan(J).all())
        # accepted: d_params NULL with nparams == 0, shared data with scen = 1, the mixed check (nu = 1)
        assert scen(known, S, d_y1, None, d_rows1, xx=x1) == native.MIOC_OK
        assert scen(nodata, S, d_y0, d_parn, None) == native.MIOC_OK
        ctx.ode_program_eval_scen_tensors(prog, 1, x, 0.0, T1, S, d_y0, d_par, d_data, J)
        ctx.synchronize()
        assert bool(torch.isfinite(J).all())


# ---- 6. TRM_batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,substeps", [("euler", 1), ("rk4", 2)])
def test_trm_batch_restart_k_solves_scenario_k_mod_S(programs, integrator, substeps):
    import torch
    from mioc.trm_batch import TRM_batch
    S, K, nt = 3, 6, 48
    y0, par, data = draw_scenarios(S, nt, seed=7)
    par_trm = mioc.TRM_parameters(beta=1e-3, Delta0=0.25, p=1, maxiter=4, kmax=4)
    prob = DeviceODEProblem(programs("bolza", integrator, substeps, "data"), bp.V, None, 0.0, T1, nt, y0, par, data=data)
    assert prob.S == S
    x0 = torch.tensor(grid(K, nt, 9), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        TRM_batch(prob, par_trm, x0=x0[:4])
    vals, u, iters = TRM_batch(prob, par_trm, x0=x0)
    assert len(prob._device_data) == 1  # uploaded once, kept
    ub = u.cpu().numpy()
    assert not np.array_equal(ub, x0.cpu().numpy()) and np.all(np.isfinite(vals))
    plain = programs("bolza", integrator, substeps, False)
    for s in range(S):
        one = DeviceODEProblem(plain, bp.V, None, 0.0, T1, nt, y0[s], par[s], data=data[s])
        pick = [s, s + S]
        v1, u1, it1 = TRM_batch(one, par_trm, x0=x0[pick])
        assert np.array_equal(v1, vals[pick]), (s, v1, vals[pick])
        assert np.array_equal(u1.cpu().numpy(), ub[pick]) and np.array_equal(it1, iters[pick]), s
    best = best_per_scenario(vals, S)
    assert all(best[s] % S == s and vals[best[s]] == min(vals[s], vals[s + S]) for s in range(S))
    print(f"{integrator} m={substeps}: iterations per restart {iters.tolist()}, best per scenario {best.tolist()}")


# ---- 7. TRM_mixed_batch: the fan's j*K + k mapping --------------------------------------------------------------------
def test_trm_mixed_batch_restart_k_solves_scenario_k_mod_S(programs):
    import torch
    S, K, nt, nu = 2, 4, 32, bp.MIXED_NU
    y0, par, data = draw_scenarios(S, nt, seed=8)
    par_trm, cpar = mioc.TRM_parameters(beta=1e-3, Delta0=0.25, p=1, maxiter=4, kmax=4), MixedParameters(R=4)
    prob = MixedODEProblem(programs("bolza", "rk4", 2, "data"), nu, bp.MIXED_LO, bp.MIXED_HI, bp.MIXED_V, None, 0.0, T1,
                           nt, y0, par, data=data)
    rng = np.random.default_rng(3)
    x0 = np.ascontiguousarray(np.stack([rng.uniform(bp.MIXED_LO, bp.MIXED_HI, size=(K, nt)),
                                        rng.integers(0, 2, size=(K, nt)).astype(np.float64)], axis=2))
    x0 = torch.tensor(x0, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        TRM_mixed_batch(prob, par_trm, cpar, x0=x0[:3])
    stats = {}
    vals, x, iters = TRM_mixed_batch(prob, par_trm, cpar, x0=x0, stats=stats)
    xb = x.cpu().numpy()
    assert not np.array_equal(xb, x0.cpu().numpy()) and np.all(np.isfinite(vals))
    assert int(np.sum(stats["csteps"])) > 0  # candidates of the fan were accepted
    plain = programs("bolza", "rk4", 2, False)
    for s in range(S):
        one = MixedODEProblem(plain, nu, bp.MIXED_LO, bp.MIXED_HI, bp.MIXED_V, None, 0.0, T1, nt, y0[s], par[s],
                              data=data[s])
        pick, st = [s, s + S], {}
        v1, x1, it1 = TRM_mixed_batch(one, par_trm, cpar, x0=x0[pick], stats=st)
        assert np.array_equal(v1, vals[pick]), (s, v1, vals[pick])
        assert np.array_equal(x1.cpu().numpy(), xb[pick]) and np.array_equal(it1, iters[pick]), s
        assert np.array_equal(st["csteps"], stats["csteps"][pick]) and np.array_equal(st["jsel"], stats["jsel"][pick])
    print(f"mixed: iterations per restart {iters.tolist()}, continuous steps {stats['csteps'].tolist()}")


# ---- 8. states() -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,substeps", [("euler", 1), ("rk4", 2)])
def test_states_of_a_scenario_problem(programs, distinct, integrator, substeps):
    import torch
    x, y0, par, data = _inputs2("data")
    prob = DeviceODEProblem(programs("bolza", integrator, substeps, "data"), bp.V, None, 0.0, T1, NT2, y0, par, data=data)
    dx = torch.tensor(x, dtype=torch.float64, device="cuda")
    with native.Context(0) as ctx:
        Y = prob.states(ctx, dx).cpu().numpy()
        J = torch.empty(K2, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        prob.eval_tensors(ctx, dx, J)
        ctx.synchronize()
        with pytest.raises(ValueError):  # K % S != 0
            prob.eval_tensors(ctx, dx[:100].contiguous(), J[:100])
    assert Y.shape == (K2, NT2 + 1, bp.NY)
    assert np.array_equal(Y[:, 0, :], y0[np.arange(K2) % S2])  # row 0: each restart's scenario state0
    Jd, _, Yd = distinct("data", integrator, substeps)
    assert np.array_equal(Y, Yd) and np.array_equal(J.cpu().numpy(), Jd)
