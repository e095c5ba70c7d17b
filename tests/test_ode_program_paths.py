"""CPU tier of the one path through mioc.ode_device: whatever the keyword arguments, ``ODEProgram`` and
``program_source`` call the library's _sens entries, and the text they hand to the compiler is, byte for byte, what
the narrowest older entry of the C ABI assembles for the same case; and the two problem classes keep the types and
shapes of their inputs, without and with scenarios.  The device tier is test_gpu_ode_program_paths.py."""
import ctypes

import numpy as np
import pytest

from mioc import native
from mioc.ode_device import (EXAMPLE_SHAPES, EXAMPLE_SOURCES, EXAMPLE_SOURCES_AD, EXAMPLE_SOURCES_AD_P, INTEGRATORS,
                             DeviceODEProblem, MixedODEProblem, ODEProgram, program_source)

SHAPE = EXAMPLE_SHAPES["fishing"]
FISH, FISH_AD, FISH_AD_P = EXAMPLE_SOURCES["fishing"], EXAMPLE_SOURCES_AD["fishing"], EXAMPLE_SOURCES_AD_P["fishing"]
# the fishing hooks with a terminal cost by hand, for terminal=True
FISH_E = FISH + """
__device__ double E(const double *p, double t, const double *y) { return 0.5 * (y[0] * y[0]); }
__device__ void Ey(const double *p, double t, const double *y, double *ey) { ey[0] = y[0]; ey[1] = 0.0; }
"""
ALL = native.MIOC_ODE_DERIVE_ALL
ALL_P = ALL | native.MIOC_ODE_DERIVE_FP | native.MIOC_ODE_DERIVE_GP
BOTH = native.MIOC_ODE_TERMINAL | native.MIOC_ODE_STATES

# (id, source, keyword arguments, the same for the C entry: ndata, derive mask, flags, scen (None: the plain entry),
#  sens (None: not the _sens entry))
CASES = [
    ("euler", FISH, {}, 0, 0, 0, None, None),
    ("rk4x2", FISH, dict(integrator="rk4", substeps=2), 0, 0, 0, None, None),
    ("midpoint", FISH, dict(integrator="midpoint"), 0, 0, 0, None, None),
    ("derive_all", FISH_AD, dict(derive="all"), 0, ALL, 0, None, None),
    ("terminal_data_states", FISH_E, dict(terminal=True, ndata=2, states=True), 2, 0, BOTH, None, None),
    ("scenarios", FISH, dict(integrator="rk4", scenarios=True), 0, 0, 0, native.MIOC_ODE_SCEN, None),
    ("scenarios_data", FISH, dict(scenarios="data", ndata=1), 1, 0, 0,
     native.MIOC_ODE_SCEN | native.MIOC_ODE_SCEN_DATA, None),
    ("sens_all_p_heun", FISH_AD_P, dict(integrator="heun", sensitivities=True, derive="all+p"), 0, ALL_P, 0, 0,
     native.MIOC_ODE_SENS_P | native.MIOC_ODE_SENS_Y0),
]
IDS = [c[0] for c in CASES]


def legacy_source(source, kw, ndata, mask, flags, scen, sens, noinline):
    """The text of the narrowest older entry that can express the case, called directly."""
    lib = native.load_library()
    head = (source.encode(), *SHAPE, ndata, INTEGRATORS[kw.get("integrator", "euler")], kw.get("substeps", 1), mask,
            flags)
    if sens is not None:
        entry, args = lib.mioc_ode_program_source_sens, head + (scen, sens, noinline)
    elif scen is not None:
        entry, args = lib.mioc_ode_program_source_scen, head + (scen, noinline)
    else:
        entry, args = lib.mioc_ode_program_source, head + (noinline,)
    need = entry(*args, None, 0)
    assert need > len(source)
    buf = ctypes.create_string_buffer(need + 1)
    assert entry(*args, buf, need + 1) == need
    return buf.value.decode()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_program_source_is_the_legacy_entrys_text(case):
    """Nothing is compiled: the assembler alone."""
    _, source, kw, *c_args = case
    for noinline in (0, 1):
        assert program_source(source, *SHAPE, noinline=bool(noinline), **kw) == legacy_source(source, kw, *c_args,
                                                                                             noinline)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_compiled_program_reports_the_legacy_entrys_text(case):
    """The program compiles through the one create call and reports the text of the older entry; a derived case also
    that of its second compile."""
    _, source, kw, *c_args = case
    with ODEProgram(source, *SHAPE, **kw) as prog:
        assert prog.h
        assert prog.source_text() == legacy_source(source, kw, *c_args, 0) == program_source(source, *SHAPE, **kw)
        if kw.get("derive"):
            assert prog.source_text(noinline=True) == legacy_source(source, kw, *c_args, 1) \
                == program_source(source, *SHAPE, noinline=True, **kw)
        assert (prog.ndata, prog.terminal, prog.states) == (c_args[0], bool(c_args[2] & 1), bool(c_args[2] & 2))
        assert (prog.scenarios, prog.sens) == (c_args[3] or 0, c_args[4] or 0)
        assert sum({"Fy": 1, "Fu": 2, "Gy": 4, "Gu": 8, "Ey": 16, "Fp": 32, "Gp": 64, "Ep": 128}[n]
                   for n in prog.derive) == c_args[1]


# ---- the two problem classes: a program stands in by its shape, nothing is compiled ----------------------------------
class _Prog:
    ny, nx, nparams, ndata = 2, 3, 4, 2

    def __init__(self, scenarios):
        self.scenarios = scenarios


NT = 5
V3, Y0, PAR = [[0, 1], [0, 1, 2], [0, 1]], [0.5, 0.7], [1.0, 2.0, 3.0, 4.0]
ROWS = np.arange(NT * 2, dtype=np.float64).reshape(NT, 2)


def _problem(mixed, prog, state0, params, data):
    if mixed:
        return MixedODEProblem(prog, 1, 0.0, 2.0, V3[1:], None, 0.0, 1.0, NT, state0, params, data=data)
    return DeviceODEProblem(prog, V3, None, 0.0, 1.0, NT, state0, params, data=data)


@pytest.mark.parametrize("mixed", [False, True], ids=["device", "mixed"])
def test_inputs_without_scenarios(mixed):
    pr = _problem(mixed, _Prog(0), tuple(Y0), np.array(PAR), ROWS.tolist())
    assert type(pr.state0) is list and type(pr.params) is list and pr.state0 == Y0 and pr.params == PAR
    assert all(type(v) is float for v in pr.state0 + pr.params)
    assert isinstance(pr.data, np.ndarray) and pr.data.dtype == np.float64 and pr.data.shape == (NT, 2)
    assert np.array_equal(pr.data, ROWS) and pr.data is not ROWS
    assert pr.S == 1 and pr._device_data == {}
    assert pr.nu == (1 if mixed else 0) and pr.nt == NT and (pr.T0, pr.T1) == (0.0, 1.0)
    assert isinstance(pr, MixedODEProblem) == mixed and isinstance(pr, DeviceODEProblem) == (not mixed)
    with pytest.raises(ValueError):
        pr.device_layouts()
    for K in (1, 7, None):
        pr.check_restarts(K)  # no scenarios: any K
    for bad in ((np.tile(Y0, (3, 1)), PAR, ROWS), (Y0, np.tile(PAR, (3, 1)), ROWS), (Y0, PAR, np.tile(ROWS, (3, 1, 1))),
                (Y0[:1], PAR, ROWS), (Y0, PAR[:3], ROWS), (Y0, PAR, ROWS[:4]), (Y0, PAR, None)):
        with pytest.raises(ValueError):  # per scenario needs a scenario program; wrong sizes; data missing
            _problem(mixed, _Prog(0), *bad)


@pytest.mark.parametrize("mixed", [False, True], ids=["device", "mixed"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("per_data", [False, True], ids=["shared_data", "data_per_scenario"])
def test_inputs_with_scenarios(mixed, S, per_data):
    rng = np.random.default_rng(S)
    y0, par, data = rng.standard_normal((S, 2)), rng.standard_normal((S, 4)), rng.standard_normal((S, NT, 2))
    prog = _Prog(3 if per_data else 1)
    pr = _problem(mixed, prog, y0, par, data if per_data else ROWS)
    assert pr.S == S
    for a, shape, src in ((pr.state0, (S, 2), y0), (pr.params, (S, 4), par),
                          (pr.data, (S, NT, 2) if per_data else (NT, 2), data if per_data else ROWS)):
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == shape and a.flags["C_CONTIGUOUS"]
        assert np.array_equal(a, src) and a is not src
    lay = pr.device_layouts()
    assert sorted(lay) == ["data", "params", "state0"]
    assert lay["state0"].shape == (2, S) and lay["params"].shape == (4, S)
    assert lay["data"].shape == ((NT, 2, S) if per_data else (NT, 2))
    assert all(a.flags["C_CONTIGUOUS"] and a.dtype == np.float64 for a in lay.values())
    assert np.array_equal(lay["state0"], y0.T) and np.array_equal(lay["params"], par.T)
    assert np.array_equal(lay["data"], data.transpose(1, 2, 0) if per_data else ROWS)
    # one input per scenario, the others shared: broadcast to S
    pr = _problem(mixed, prog, Y0, par, ROWS)
    assert pr.S == S and pr.state0.shape == (S, 2) and np.array_equal(pr.state0, np.tile(Y0, (S, 1)))
    assert pr.data.shape == ((S, NT, 2) if per_data else (NT, 2))
    # nothing per scenario: S = 1, the same types
    pr = _problem(mixed, prog, Y0, PAR, ROWS)
    assert pr.S == 1 and pr.state0.shape == (1, 2) and pr.params.shape == (1, 4)
    assert pr.data.shape == ((1, NT, 2) if per_data else (NT, 2))
    assert pr.device_layouts()["state0"].shape == (2, 1)


@pytest.mark.parametrize("mixed", [False, True], ids=["device", "mixed"])
def test_scenario_mismatches(mixed):
    rng = np.random.default_rng(7)
    y0, par, data = rng.standard_normal((3, 2)), rng.standard_normal((3, 4)), rng.standard_normal((3, NT, 2))
    for bad in ((y0[:2], par, data), (y0, par[:2], data), (y0, par, data[:2]), (y0[:2], par[:1], ROWS)):
        with pytest.raises(ValueError):  # the numbers of scenarios disagree
            _problem(mixed, _Prog(3), *bad)
    with pytest.raises(ValueError):  # data per scenario need scenarios="data"
        _problem(mixed, _Prog(1), y0, par, data)
    pr = _problem(mixed, _Prog(3), y0, par, data)
    for K in (1, 2, 4, 7, 0, None):
        with pytest.raises(ValueError, match="scenarios"):  # K is no multiple of S = 3
            pr.check_restarts(K)
    for K in (3, 6, 72):
        pr.check_restarts(K)
