"""GPU tier of the sensitivities of user-defined ODE objectives (mioc_ode_program_create_sens,
mioc_ode_program_eval_sens_device; the contract: include/mioc.h, "Sensitivities").

The device kernels are compared with the host mirror (tests/ode_sens_mirror.py) on tests/ode_sens_problem.py at the bar
of ode_gpu_support.assert_at_bar: 1e-12 relative for J, 1e-12 of the row maximum for df, Jp and Jy0.  Then the
hand-derived known answer, edge shapes, independence of K, every combination of outputs, the program without
sensitivities, derived against hand-written hooks, scenarios, the mixed entry, a failed Newton iteration, the gate, the
refusals of the entries and check_hooks."""
import ctypes
import itertools

import numpy as np
import pytest

from mioc import native
from mioc.iterators import LevelTable
from mioc.ode_device import DeviceODEProblem, MixedODEProblem, ODEProgram, check_hooks

import ode_sens_problem as sp
import ode_stiff_problem as stiff
from ode_gpu_support import assert_at_bar, grid, run_program
from ode_sens_mirror import sens_eval

pytestmark = pytest.mark.gpu

SCHEMES = [("heun", 1), ("rk4", 1), ("rk4", 3), ("beuler", 1), ("midpoint", 2)]
T1 = 0.96
SENTINEL = -7.25  # what every output buffer is filled with, and the rows around it


@pytest.fixture(scope="module")
def programs():
    """Every program compiled once per module, by (text key, integrator, substeps, sensitivities, scenarios, derive)."""
    progs = {}
    texts = {"sens": (sp.SOURCE, sp.NY, sp.NX, sp.NP, dict(ndata=sp.ND, terminal=True, states=True)),
             "known": (sp.KNOWN_SOURCE, 1, 1, 2, dict(terminal=True))}

    def get(key, integrator, substeps=1, sens=True, scenarios=False, derive=()):
        k = (key, integrator, substeps, sens, scenarios, derive)
        if k not in progs:
            text, ny, nx, nparams, kw = texts[key]
            progs[k] = ODEProgram(text, ny, nx, nparams, integrator=integrator, substeps=substeps, derive=derive,
                                  scenarios=scenarios, sensitivities=sens, **kw)
        return progs[k]
    yield get
    for p in progs.values():
        p.close()


def _framed(K, width):
    """A (K + 2, width) device buffer full of the sentinel and its K middle rows, which an evaluation is given."""
    import torch
    whole = torch.full((K + 2, width), SENTINEL, dtype=torch.float64, device="cuda")
    return whole, whole[1:K + 1]


def _frame_intact(whole):
    return bool((whole[0] == SENTINEL).all()) and bool((whole[-1] == SENTINEL).all())


def run_sens(ctx, prog, x, T1, state0, params, data, want="J df Jp Jy0", nu=None, scen=None):
    """One evaluation: {name: numpy array} of the outputs named in `want`.  All four buffers exist, full of the sentinel
    and each between two sentinel rows; the call is handed those named in `want` and NULL for the others, and afterwards
    the rows around every buffer and the whole of a buffer that was not handed over must still hold the sentinel.
    scen = (S, state0 (S, ny), params (S, nparams)): the scenario entry."""
    import torch
    K, nt, nx = x.shape
    f64 = dict(dtype=torch.float64, device="cuda")
    dx = torch.tensor(x, **f64)
    dd = None if data is None else torch.tensor(data, **f64)
    widths = {"J": 1, "df": nt * nx, "Jp": prog.nparams, "Jy0": prog.ny, "Y": (nt + 1) * prog.ny}
    bufs = {n: _framed(K, widths[n]) for n in ("J", "df", "Jp", "Jy0") if widths[n]}
    arg = {n: (bufs[n][1] if n in want.split() else None) for n in widths}
    torch.cuda.synchronize()
    if scen is not None:
        S, y0s, pars = scen
        ctx.ode_program_eval_scen_tensors(prog, nu, dx, 0.0, T1, S, torch.tensor(np.ascontiguousarray(y0s.T), **f64),
                                          torch.tensor(np.ascontiguousarray(pars.T), **f64), dd, arg["J"], arg["df"],
                                          arg["Y"], arg["Jp"], arg["Jy0"])
    elif nu is None:
        ctx.ode_program_eval_tensors(prog, dx, 0.0, T1, state0, params, arg["J"], arg["df"], data=dd, Y=arg["Y"],
                                     Jp=arg["Jp"], Jy0=arg["Jy0"])
    else:
        ctx.ode_program_eval_mixed_tensors(prog, nu, dx, 0.0, T1, state0, params, arg["J"], arg["df"], data=dd,
                                           Y=arg["Y"], Jp=arg["Jp"], Jy0=arg["Jy0"])
    ctx.synchronize()
    shapes = {"J": (K,), "df": (K, nt, nx), "Jp": (K, prog.nparams), "Jy0": (K, prog.ny), "Y": (K, nt + 1, prog.ny)}
    for n, (whole, _) in bufs.items():
        assert _frame_intact(whole), f"{n}: a row outside the K rows was written"
        assert arg[n] is not None or bool((whole == SENTINEL).all()), f"{n}: written although it was not handed over"
    return {n: bufs[n][1].cpu().numpy().reshape(shapes[n]) for n in want.split()}


def _run_problem(ctx, prog, x, T1, **kw):
    return run_sens(ctx, prog, x, T1, sp.STATE0, sp.PARAMS, sp.make_data(x.shape[1]), **kw)


def _mirror(x, T1, integrator, substeps, state0=None, params=None):
    """{J, df, Jp, Jy0} of the mirror; state0 / params: per restart (K, ny) / (K, NP), else the problem's."""
    K, nt, _ = x.shape
    data = sp.make_data(nt)
    out = [sens_eval(sp.HOOKS, sp.PARAMS if params is None else params[k], data,
                     sp.STATE0 if state0 is None else state0[k], 0.0, T1, x[k], integrator, substeps) for k in range(K)]
    return {n: np.array([o[j] for o in out]) for j, n in enumerate(("J", "df", "Jp", "Jy0"))}


def assert_sens_at_bar(dev, ref, label):
    """assert_at_bar for J and df, and its bar for Jp and Jy0: 1e-12 of the row maximum; every figure printed first."""
    assert_at_bar((dev["J"], dev["df"]), (ref["J"], ref["df"]), label)
    worst = {}
    for n in ("Jp", "Jy0"):
        a, b = dev[n], ref[n]
        assert np.all(np.isfinite(a)), (label, n)
        worst[n] = max(np.max(np.abs(a[k] - b[k])) / max(1e-300, np.max(np.abs(b[k]))) for k in range(b.shape[0]))
    exact = sum(int(np.array_equal(dev[n][k], ref[n][k])) for n in worst for k in range(ref["J"].shape[0]))
    print(f"{label}: {exact} of {2 * ref['J'].shape[0]} Jp / Jy0 rows bit-identical to the mirror; worst errors relative "
          f"to the row maximum " + ", ".join(f"{n} {w:.3e}" for n, w in worst.items()))
    assert all(w <= 1e-12 for w in worst.values()), (label, worst)


def _same(a, b, names="J df Jp Jy0"):
    return all(np.array_equal(a[n], b[n], equal_nan=True) for n in names.split())


@pytest.fixture(scope="module")
def x70():
    x = grid(70, 24, 5)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def device70(programs, x70):
    """The device's J, df, Jp and Jy0 of the K = 70 call (nt = 24, T1 = 0.96) per scheme, computed once."""
    out = {}
    with native.Context(0) as ctx:
        for integrator, m in SCHEMES:
            out[integrator, m] = _run_problem(ctx, programs("sens", integrator, m), x70, T1)
    return out


# ---- 1. the device against the mirror ---------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_device_vs_mirror(x70, device70, integrator, substeps):
    """K = 70: one full block and a partial one of 6 lanes."""
    assert_sens_at_bar(device70[integrator, substeps], _mirror(x70, T1, integrator, substeps),
                       f"{integrator} m={substeps}")


@pytest.mark.parametrize("nt", [1, 2])
@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_edge_shapes(programs, integrator, substeps, nt):
    x = grid(3, nt, 20 + nt)
    with native.Context(0) as ctx:
        dev = _run_problem(ctx, programs("sens", integrator, substeps), x, 0.04 * nt)
    assert_sens_at_bar(dev, _mirror(x, 0.04 * nt, integrator, substeps), f"{integrator} m={substeps} nt={nt}")


@pytest.mark.parametrize("integrator,substeps", [("heun", 1), ("heun", 2), ("beuler", 1), ("midpoint", 1),
                                                 ("midpoint", 2), ("rk4", 1), ("rk4", 2)])
def test_known_answer(programs, integrator, substeps):
    """F = p0 x, G = p1 y, E = 2 y, derived by hand in ode_sens_problem.py: every value exact, RK4 at the 1e-12 bar
    (its b weights do not sum to 1 in doubles).  K = 3 copies of the one control."""
    kn, want = sp.KNOWN, sp.known(integrator)
    x = np.ascontiguousarray(np.tile(np.array(kn["x"])[None], (3, 1, 1)))
    with native.Context(0) as ctx:
        d = run_sens(ctx, programs("known", integrator, substeps), x, kn["T1"], kn["state0"], kn["params"], None)
    print(integrator, substeps, d["J"].tolist(), d["df"][0, :, 0].tolist(), d["Jp"][0].tolist(), d["Jy0"][0].tolist())
    for k in range(3):
        got = (d["df"][k, :, 0], d["Jp"][k], d["Jy0"][k])
        if integrator == "rk4":
            assert abs(d["J"][k] - want["J"]) <= 1e-12 * want["J"]
            for a, n in zip(got, ("df", "Jp", "Jy0")):
                assert np.max(np.abs(a - want[n])) <= 1e-12 * max(want[n]), (k, n)
        else:
            assert d["J"][k] == want["J"] and all(a.tolist() == want[n] for a, n in zip(got, ("df", "Jp", "Jy0"))), k


# ---- 2. independence of K and of the lane ------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_independent_of_K_and_position(programs, x70, device70, integrator, substeps):
    """K = 1, 64 (one full block), 65 (one lane in the second block), and restarts moved into K = 130."""
    dev = device70[integrator, substeps]
    prog = programs("sens", integrator, substeps)
    big = grid(130, 24, 6)
    big[129], big[64] = x70[0], x70[69]  # the first restart at the far end, the last one at a block's start
    with native.Context(0) as ctx:
        for k in (0, 37, 69):
            one = _run_problem(ctx, prog, x70[k:k + 1], T1)
            assert all(np.array_equal(one[n][0], dev[n][k]) for n in dev), k
        for K in (64, 65):
            part = _run_problem(ctx, prog, np.ascontiguousarray(x70[:K]), T1)
            assert all(np.array_equal(part[n], dev[n][:K]) for n in dev), K
        b = _run_problem(ctx, prog, big, T1)
    assert all(np.array_equal(b[n][129], dev[n][0]) and np.array_equal(b[n][64], dev[n][69]) for n in dev)


# ---- 3. every combination of outputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,substeps", [("rk4", 3), ("midpoint", 2)])
def test_every_combination_of_outputs(programs, x70, device70, integrator, substeps):
    """d_J, d_df, d_Jp, d_Jy0 each NULL or not: 16 calls.  Each output is that of the all-outputs call bit for bit, a
    buffer that was not handed over keeps its sentinel and the rows handed over sit between sentinel rows (run_sens).
    df in particular does not change when d_Jp is added, and the sweep runs for d_Jy0 alone."""
    full = device70[integrator, substeps]
    prog = programs("sens", integrator, substeps)
    with native.Context(0) as ctx:
        for mask in itertools.product((False, True), repeat=4):
            want = " ".join(n for n, m in zip(("J", "df", "Jp", "Jy0"), mask) if m)
            got = _run_problem(ctx, prog, x70, T1, want=want)
            assert sorted(got) == sorted(want.split())
            assert all(np.array_equal(got[n], full[n]) for n in got), want


# ---- 4. a program that is not asked for sensitivities is the program it was --------------------------------------------
@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_both_pointers_null_is_the_program_without_sensitivities(programs, x70, device70, integrator, substeps):
    """J, df and Y of the sens program through the older entry (no d_Jp, no d_Jy0) against the program compiled with
    sens = 0 from the same text, bit for bit; and df of the all-outputs call is that df too."""
    data = sp.make_data(24)
    with native.Context(0) as ctx:
        plain = run_program(ctx, programs("sens", integrator, substeps, False), x70, 0.0, T1, sp.STATE0, sp.PARAMS,
                            data=data, want_Y=True)
        for sens in (True, "p", "y0"):
            got = run_program(ctx, programs("sens", integrator, substeps, sens), x70, 0.0, T1, sp.STATE0, sp.PARAMS,
                              data=data, want_Y=True)
            assert all(np.array_equal(a, b) for a, b in zip(got, plain)), sens
    assert all(np.all(np.isfinite(a)) for a in plain)
    dev = device70[integrator, substeps]
    assert np.array_equal(dev["J"], plain[0]) and np.array_equal(dev["df"], plain[1])


def test_one_part_alone(programs, x70, device70):
    """sensitivities="p" and "y0": each program returns its part, bit-equal to the program with both."""
    with native.Context(0) as ctx:
        for integrator, m in (("heun", 1), ("beuler", 1)):
            dev = device70[integrator, m]
            p = _run_problem(ctx, programs("sens", integrator, m, "p"), x70, T1, want="J df Jp")
            y = _run_problem(ctx, programs("sens", integrator, m, "y0"), x70, T1, want="J df Jy0")
            assert _same(p, dev, "J df Jp") and _same(y, dev, "J df Jy0"), integrator


# ---- 5. derived hooks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,substeps", [("rk4", 3), ("midpoint", 2)])
def test_derived_against_hand_written(programs, x70, device70, integrator, substeps):
    """Everything derived ("all+p") and the three p hooks alone: J bit for bit (F, G, E with P = double are the same
    expressions), df, Jp and Jy0 at the bar against the hand-written hooks."""
    hand = device70[integrator, substeps]
    with native.Context(0) as ctx:
        for derive in ("all+p", ("Fp", "Gp", "Ep")):
            got = _run_problem(ctx, programs("sens", integrator, substeps, True, False, derive), x70, T1)
            assert np.array_equal(got["J"], hand["J"])
            assert_sens_at_bar(got, hand, f"{integrator} m={substeps} derive={derive}")
            if derive != "all+p":  # Fy, Fu, Gy, Gu, Ey by hand: the adjoint is the same, bit for bit
                assert np.array_equal(got["df"], hand["df"]) and np.array_equal(got["Jy0"], hand["Jy0"])


def test_check_hooks_names_a_sign_flipped_Gp(x70):
    import torch
    x = torch.tensor(x70[:5], dtype=torch.float64, device="cuda")
    data = torch.tensor(sp.make_data(24), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p_hooks = ("Fp", "Gp", "Ep", "all+p")
    with native.Context(0) as ctx:
        args = (sp.NY, sp.NX, sp.NP, x, 0.0, T1, sp.STATE0, sp.PARAMS)
        kw = dict(integrator="rk4", substeps=2, ndata=sp.ND, terminal=True, data=data, sensitivities=True)
        bad = check_hooks(ctx, sp.SOURCE_WRONG_GP, *args, **kw)
        print(bad)
        assert bad.pop("J_equal") is True
        assert set(bad) == {"all", "Fy", "Fu", "Gy", "Gu", "Ey"} | set(p_hooks)
        assert bad["Gp"] > 1e-3 and bad["all+p"] > 1e-3
        assert all(v < 1e-12 for n, v in bad.items() if n not in ("Gp", "all+p")), bad


# ---- 6. scenarios ----------------------------------------------------------------------------------------------------------
def _scenarios(S, seed=11):
    rng = np.random.default_rng(seed)
    state0 = np.array(sp.STATE0) + 0.1 * rng.standard_normal((S, sp.NY))
    params = np.array(sp.PARAMS) * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, size=(S, sp.NP)))
    return np.ascontiguousarray(state0), np.ascontiguousarray(params)


@pytest.mark.parametrize("S,K", [(3, 6), (64, 128)])
@pytest.mark.parametrize("integrator,substeps", [("rk4", 3), ("midpoint", 2)])
def test_scenarios(programs, integrator, substeps, S, K):
    """Restart q's rows are the derivatives in scenario q % S's own values: bit for bit what the sens program without
    scenarios gives on that scenario's parameters and state0 (the two restarts of a scenario in one call), and S = 3
    at the bar against the mirror."""
    nt = 8
    x = grid(K, nt, 31)
    y0s, pars = _scenarios(S)
    data = sp.make_data(nt)
    with native.Context(0) as ctx:
        got = run_sens(ctx, programs("sens", integrator, substeps, True, True), x, T1, None, None, data,
                       scen=(S, y0s, pars))
        for s in range(S):
            pick = list(range(s, K, S))
            one = run_sens(ctx, programs("sens", integrator, substeps), np.ascontiguousarray(x[pick]), T1, y0s[s],
                           pars[s], data)
            assert all(np.array_equal(one[n], got[n][pick]) for n in one), s
        if S == 3:
            prob = DeviceODEProblem(programs("sens", integrator, substeps, True, True), sp.V, None, 0.0, T1, nt, y0s, pars,
                                    data=data)
            import torch
            Jp, Jy0 = prob.sensitivities(ctx, torch.tensor(x, dtype=torch.float64, device="cuda"))
            assert np.array_equal(Jp.cpu().numpy(), got["Jp"]) and np.array_equal(Jy0.cpu().numpy(), got["Jy0"])
    assert not np.array_equal(got["Jp"][:S], got["Jp"][S:2 * S])  # the two controls of a scenario differ
    if S == 3:
        q = np.arange(K) % S
        assert_sens_at_bar(got, _mirror(x, T1, integrator, substeps, y0s[q], pars[q]), f"S=3 {integrator}")


# ---- 7. the mixed entry and the problems' sensitivities() -----------------------------------------------------------------
def test_mixed_entry_and_problem_methods(programs, x70, device70):
    """nu = 1 with the levels of the one integer control: the same kernel, so the rows of the plain entry bit for bit;
    DeviceODEProblem / MixedODEProblem.sensitivities return them, None for a part the program lacks."""
    import torch
    dev = device70["rk4", 3]
    prog = programs("sens", "rk4", 3)
    dx = torch.tensor(x70, dtype=torch.float64, device="cuda")
    data = sp.make_data(24)
    with native.Context(0) as ctx:
        ctx.set_levels(LevelTable(sp.V[1:]))
        got = _run_problem(ctx, prog, x70, T1, nu=1)
        assert _same(got, dev)
        with pytest.raises(native.MiocNativeError):  # nu = 0 against the levels of one control
            _run_problem(ctx, prog, x70, T1)
        mixed = MixedODEProblem(prog, 1, 0.0, 2.0, sp.V[1:], None, 0.0, T1, 24, sp.STATE0, sp.PARAMS, data=data)
        Jp, Jy0 = mixed.sensitivities(ctx, dx)
        assert np.array_equal(Jp.cpu().numpy(), dev["Jp"]) and np.array_equal(Jy0.cpu().numpy(), dev["Jy0"])
    with native.Context(0) as ctx:
        for sens, has in (("p", (True, False)), ("y0", (False, True)), (True, (True, True))):
            prob = DeviceODEProblem(programs("sens", "rk4", 3, sens), sp.V, None, 0.0, T1, 24, sp.STATE0, sp.PARAMS,
                                    data=data)
            out = prob.sensitivities(ctx, dx)
            assert tuple(o is not None for o in out) == has
            assert out[0] is None or (out[0].is_cuda and np.array_equal(out[0].cpu().numpy(), dev["Jp"]))
            assert out[1] is None or (out[1].is_cuda and np.array_equal(out[1].cpu().numpy(), dev["Jy0"]))
        plain = DeviceODEProblem(programs("sens", "rk4", 3, False), sp.V, None, 0.0, T1, 24, sp.STATE0, sp.PARAMS,
                                 data=data)
        with pytest.raises(ValueError):
            plain.sensitivities(ctx, dx)


# ---- 8. a failed Newton iteration ----------------------------------------------------------------------------------------
# ode_stiff_problem's problem without a root, its constant 1e3 as the one parameter: F = x0 (p0 + 1e6 y^2) - y
NOROOT_SOURCE = stiff.NOROOT_SOURCE.replace("1e3", "p[0]") + """
__device__ void Fp(const double *p, int i, double t, const double *y, const double *x, double (*fp)[NP]) { fp[0][0] = x[0]; }
__device__ void Gp(const double *p, int i, double t, const double *y, const double *x, double *gp) {}
"""
assert stiff.NOROOT_SOURCE.count("1e3") == 2  # in F and in Fu


@pytest.mark.parametrize("integrator", ["beuler", "midpoint"])
def test_failed_newton_gives_nan_rows_and_leaves_the_neighbours(integrator):
    """Restart 2 of 5 has x = 1 everywhere (no real root: its Newton iteration fails), the others four small distinct
    controls, x = 2e-6 (k + 1), with which y' = x (1e3 + 1e6 y^2) - y stays tame: its J, df, Jp and Jy0 rows are NaN,
    the neighbours' rows are those of the call without it."""
    nt, T = 8, 0.32
    x = np.ones((5, nt, 1)) * (2e-6 * (1.0 + np.arange(5)))[:, None, None]
    x[2] = 1.0
    with ODEProgram(NOROOT_SOURCE, 1, 1, 1, integrator=integrator, sensitivities=True) as prog, \
            native.Context(0) as ctx:
        got = run_sens(ctx, prog, x, T, stiff.NOROOT_STATE0, [1e3], None)
        rest = run_sens(ctx, prog, np.ascontiguousarray(x[[0, 1, 3, 4]]), T, stiff.NOROOT_STATE0, [1e3], None)
    for n in got:
        assert np.all(np.isnan(got[n][2])), n
        assert np.array_equal(got[n][[0, 1, 3, 4]], rest[n]) and np.all(np.isfinite(rest[n])), n
    assert np.all(rest["Jy0"] != 0.0) and np.all(rest["Jp"] != 0.0)
    assert len(set(rest["J"].tolist())) == 4


# ---- 9. the gate and the refusals -----------------------------------------------------------------------------------------
def test_a_closed_gate_leaves_the_outputs_untouched(programs, x70, device70):
    import torch
    prog = programs("sens", "heun", 1)
    f64 = dict(dtype=torch.float64, device="cuda")
    dx, data = torch.tensor(x70, **f64), torch.tensor(sp.make_data(24), **f64)
    Jp, Jy0 = torch.full((70, sp.NP), SENTINEL, **f64), torch.full((70, sp.NY), SENTINEL, **f64)
    torch.cuda.synchronize()
    with native.Context(0) as ctx:
        ctx.trm_attach(ctx.trm_state_tensor(70))  # zero-initialised: the gate word is 0
        ctx.ode_program_eval_tensors(prog, dx, 0.0, T1, sp.STATE0, sp.PARAMS, data=data, Jp=Jp, Jy0=Jy0)
        ctx.synchronize()
        assert bool((Jp == SENTINEL).all()) and bool((Jy0 == SENTINEL).all())
        ctx.trm_attach(None)
        ctx.ode_program_eval_tensors(prog, dx, 0.0, T1, sp.STATE0, sp.PARAMS, data=data, Jp=Jp, Jy0=Jy0)
        ctx.synchronize()
    dev = device70["heun", 1]
    assert np.array_equal(Jp.cpu().numpy(), dev["Jp"]) and np.array_equal(Jy0.cpu().numpy(), dev["Jy0"])


def test_refusals_of_the_eval_entry(programs, x70, device70):
    import torch
    lib = native.load_library()
    K, nt, S = 4, 24, 2
    both, only_p, only_y = (programs("sens", "heun", 1, s) for s in (True, "p", "y0"))
    plain, scen = programs("sens", "heun", 1, False), programs("sens", "heun", 1, True, True)
    f64 = dict(dtype=torch.float64, device="cuda")
    x, data = torch.tensor(x70[:K], **f64), torch.tensor(sp.make_data(nt), **f64)
    y0s, pars = _scenarios(S)
    d_y0, d_par = torch.tensor(np.ascontiguousarray(y0s.T), **f64), torch.tensor(np.ascontiguousarray(pars.T), **f64)
    J = torch.full((K,), SENTINEL, **f64)
    Jp, Jy0 = torch.full((K, sp.NP), SENTINEL, **f64), torch.full((K, sp.NY), SENTINEL, **f64)
    y0, par = np.array(sp.STATE0), np.array(sp.PARAMS)
    torch.cuda.synchronize()

    def vp(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def hp(a):
        return ctypes.c_void_p(a.ctypes.data)

    with native.Context(0) as ctx:
        def sens(p, S_, Y0, P, D, jp, jy0, K_=K):
            return lib.mioc_ode_program_eval_sens_device(ctx.h, p.h, 0, K_, vp(x), nt, 0.0, T1, S_, Y0, P, vp(D), vp(J),
                                                         None, None, vp(jp), vp(jy0))

        def refused_then_usable(rc):
            assert rc == native.MIOC_EINVAL
            ctx.synchronize()
            assert all(bool((t == SENTINEL).all()) for t in (J, Jp, Jy0))  # nothing ran
            assert sens(both, 0, hp(y0), hp(par), data, Jp, Jy0) == native.MIOC_OK
            ctx.synchronize()
            assert np.array_equal(Jp.cpu().numpy(), device70["heun", 1]["Jp"][:K])
            assert np.array_equal(Jy0.cpu().numpy(), device70["heun", 1]["Jy0"][:K])
            for t in (J, Jp, Jy0):
                t.fill_(SENTINEL)
            torch.cuda.synchronize()
        refused_then_usable(sens(only_y, 0, hp(y0), hp(par), data, Jp, None))       # d_Jp without MIOC_ODE_SENS_P
        refused_then_usable(sens(only_p, 0, hp(y0), hp(par), data, None, Jy0))      # d_Jy0 without MIOC_ODE_SENS_Y0
        refused_then_usable(sens(plain, 0, hp(y0), hp(par), data, Jp, None))        # a program compiled with sens == 0
        refused_then_usable(sens(plain, 0, hp(y0), hp(par), data, None, Jy0))
        refused_then_usable(sens(both, S, vp(d_y0), vp(d_par), data, Jp, Jy0))      # S >= 1 on a program without scenarios
        refused_then_usable(sens(scen, 0, hp(y0), hp(par), data, Jp, Jy0))          # S == 0 on a scenario program
        refused_then_usable(sens(scen, -1, vp(d_y0), vp(d_par), data, Jp, Jy0))
        refused_then_usable(sens(scen, 3, vp(d_y0), vp(d_par), data, Jp, Jy0))      # K % S != 0
        refused_then_usable(sens(both, 0, hp(y0), hp(par), None, Jp, Jy0))          # the checks of _eval_bolza_device
        refused_then_usable(sens(both, 0, None, hp(par), data, Jp, Jy0))
        refused_then_usable(sens(both, 0, hp(y0), hp(par), data, Jp, Jy0, K_=0))
        for p, kw in ((only_y, dict(Jp=Jp)), (only_p, dict(Jy0=Jy0)), (plain, dict(Jp=Jp)),
                      (both, dict(Jp=Jp[:3].contiguous())), (both, dict(Jy0=Jy0.cpu()))):
            with pytest.raises(ValueError):
                ctx.ode_program_eval_tensors(p, x, 0.0, T1, sp.STATE0, sp.PARAMS, data=data, **kw)
        ctx.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in (J, Jp, Jy0))
        # accepted: a scenario program with S matching, and a sens program through the entries without sensitivities
        assert sens(scen, S, vp(d_y0), vp(d_par), data, Jp, Jy0) == native.MIOC_OK
        assert lib.mioc_ode_program_eval_scen_device(ctx.h, scen.h, 0, K, vp(x), nt, 0.0, T1, S, vp(d_y0), vp(d_par),
                                                     vp(data), vp(J), None, None) == native.MIOC_OK
        assert lib.mioc_ode_program_eval_bolza_device(ctx.h, both.h, 0, K, vp(x), nt, 0.0, T1, hp(y0), hp(par), vp(data),
                                                      vp(J), None, None) == native.MIOC_OK
        ctx.synchronize()
        assert np.array_equal(J.cpu().numpy(), device70["heun", 1]["J"][:K])
        assert bool(torch.isfinite(Jp).all()) and bool(torch.isfinite(Jy0).all())
