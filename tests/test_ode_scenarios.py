"""CPU tier of scenarios for user-defined ODE objectives (mioc_ode_program_create_scen, _source_scen; include/mioc.h,
"Scenarios"): a program without scenarios is assembled byte for byte as before, bad arguments are refused, every
integrator compiles for gfx950 with both scenario variants, and the Python layer infers S, broadcasts, refuses wrong
shapes and K % S != 0 and lays the arrays out with the scenario index fastest.  The device tier is
test_gpu_ode_scenarios.py."""
import ctypes

import numpy as np
import pytest

from mioc import native
from mioc.ode_device import (EXAMPLE_SHAPES, EXAMPLE_SOURCES, DeviceODEProblem, MixedODEProblem, ODEProgram,
                             best_per_scenario, program_source)

import ode_bolza_problem as bp
from ode_scenario_support import NODATA_NP, NODATA_SOURCE, draw_scenarios

INT = {"euler": native.MIOC_ODE_INT_EULER, "heun": native.MIOC_ODE_INT_HEUN, "rk4": native.MIOC_ODE_INT_RK4,
       "beuler": native.MIOC_ODE_INT_BEULER, "midpoint": native.MIOC_ODE_INT_MIDPOINT}
SCHEMES = [("euler", 1), ("heun", 1), ("rk4", 2), ("beuler", 1), ("midpoint", 2)]
BOTH = native.MIOC_ODE_TERMINAL | native.MIOC_ODE_STATES
CAP = 1 << 18


def _source(text, shape, ndata, integrator, substeps, derive, flags, scen=None, noinline=0):
    """(return value, text) of mioc_ode_program_source (scen None) or mioc_ode_program_source_scen."""
    lib = native.load_library()
    buf = ctypes.create_string_buffer(CAP)
    head = (text.encode(), *shape, ndata, integrator, substeps, derive, flags)
    if scen is None:
        n = lib.mioc_ode_program_source(*head, noinline, buf, CAP)
    else:
        n = lib.mioc_ode_program_source_scen(*head, scen, noinline, buf, CAP)
    return n, buf.value


def _create_scen(text, shape, ndata, integrator, substeps, derive, flags, scen):
    lib = native.load_library()
    h, log = ctypes.c_void_p(), ctypes.create_string_buffer(1 << 16)
    rc = lib.mioc_ode_program_create_scen(text.encode(), *shape, ndata, integrator, substeps, derive, flags, scen,
                                          ctypes.byref(h), log, 1 << 16)
    return lib, rc, h, log.value.decode()


FISH = (EXAMPLE_SOURCES["fishing"], EXAMPLE_SHAPES["fishing"], 0, 0)
BOLZA = (bp.SOURCE, (bp.NY, bp.NX, bp.NP), bp.ND, BOTH)


@pytest.mark.parametrize("case", [FISH, BOLZA], ids=["fishing", "bolza"])
@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_source_scen_0_is_source(case, integrator, substeps):
    text, shape, ndata, flags = case
    for derive in ((0,) if case is FISH else (0, native.MIOC_ODE_DERIVE_ALL | native.MIOC_ODE_DERIVE_EY)):
        for noinline in (0, 1):
            n0, t0 = _source(text, shape, ndata, INT[integrator], substeps, derive, flags, None, noinline)
            n1, t1 = _source(text, shape, ndata, INT[integrator], substeps, derive, flags, 0, noinline)
            assert n0 == n1 == len(t0) > len(text) and t0 == t1
            assert b"MIOC_SCEN 1" not in t0 and b"MIOC_SCEN_DATA 1" not in t0


def test_source_scen_head_and_kernel_arguments():
    """The two defines stand behind MIOC_STATES, and only the ones asked for."""
    args = (bp.SOURCE, (bp.NY, bp.NX, bp.NP), bp.ND, INT["rk4"], 2, 0, BOTH)
    _, t1 = _source(*args, native.MIOC_ODE_SCEN)
    _, t3 = _source(*args, native.MIOC_ODE_SCEN | native.MIOC_ODE_SCEN_DATA)
    assert t1[:t1.index(b"#line 1")].endswith(b"#define MIOC_STATES 1\n#define MIOC_SCEN 1\n")
    assert t3[:t3.index(b"#line 1")].endswith(b"#define MIOC_STATES 1\n#define MIOC_SCEN 1\n#define MIOC_SCEN_DATA 1\n")
    _, t0 = _source(*args, 0)
    assert t0[t0.index(b"#line 1"):] == t1[t1.index(b"#line 1"):] == t3[t3.index(b"#line 1"):]  # only the head differs


def test_create_scen_0_is_create_bolza():
    shape = (bp.NY, bp.NX, bp.NP)
    lib, rc, h, log = _create_scen(bp.SOURCE, shape, bp.ND, INT["heun"], 2, 0, BOTH, 0)
    assert rc == native.MIOC_OK and h.value, log
    assert lib.mioc_ode_program_destroy(h) == native.MIOC_OK
    with ODEProgram(bp.SOURCE, *shape, integrator="heun", substeps=2, ndata=bp.ND, terminal=True, states=True) as p:
        assert p.scenarios == 0
        assert p.source_text().encode() == _source(bp.SOURCE, shape, bp.ND, INT["heun"], 2, 0, BOTH, 0)[1]
    # the Python class goes through _create_scen only for a scenario program, and its text says so
    with ODEProgram(bp.SOURCE, *shape, integrator="heun", substeps=2, ndata=bp.ND, terminal=True, states=True,
                    scenarios="data") as p:
        assert p.scenarios == 3
        assert p.source_text().encode() == _source(bp.SOURCE, shape, bp.ND, INT["heun"], 2, 0, BOTH, 3)[1]
        assert p.source_text() == program_source(bp.SOURCE, *shape, "heun", 2, ndata=bp.ND, terminal=True, states=True,
                                                 scenarios="data")


@pytest.mark.parametrize("ndata,scen", [(2, 4), (2, 7), (2, -1), (2, 2), (0, 2), (0, 3)])
def test_scen_refusals(ndata, scen):
    """scen bits outside 3, MIOC_ODE_SCEN_DATA alone, MIOC_ODE_SCEN_DATA with ndata == 0: both entries alike."""
    shape = (bp.NY, bp.NX, bp.NP if ndata else NODATA_NP)
    text = bp.SOURCE if ndata else NODATA_SOURCE
    lib, rc, h, _ = _create_scen(text, shape, ndata, INT["euler"], 1, 0, BOTH, scen)
    assert rc == native.MIOC_EINVAL and not h.value
    n, t = _source(text, shape, ndata, INT["euler"], 1, 0, BOTH, scen)
    assert n == native.MIOC_EINVAL and t == b""
    # the same arguments with an accepted scen are accepted: nothing else was wrong
    assert _source(text, shape, ndata, INT["euler"], 1, 0, BOTH, 1)[0] > 0


def test_python_scenarios_argument():
    shape = (bp.NY, bp.NX, NODATA_NP)
    with pytest.raises(ValueError):
        ODEProgram(NODATA_SOURCE, *shape, terminal=True, scenarios="data")  # needs ndata > 0
    with pytest.raises(ValueError):
        ODEProgram(NODATA_SOURCE, *shape, terminal=True, scenarios="params")
    with pytest.raises(ValueError):
        program_source(NODATA_SOURCE, *shape, terminal=True, scenarios=2)


@pytest.mark.parametrize("derive", [(), "all"], ids=["hand", "derived"])
@pytest.mark.parametrize("scenarios", [True, "data"], ids=["scen1", "scen3"])
@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_scenario_programs_compile(integrator, substeps, scenarios, derive):
    with ODEProgram(bp.SOURCE, bp.NY, bp.NX, bp.NP, integrator=integrator, substeps=substeps, derive=derive,
                    ndata=bp.ND, terminal=True, states=True, scenarios=scenarios) as p:
        assert p.h and p.log == ""  # no warnings either
        assert p.scenarios == (3 if scenarios == "data" else 1)
    if scenarios is True:  # and without data: the per-lane parameter copy exists for the scenarios alone
        with ODEProgram(NODATA_SOURCE, bp.NY, bp.NX, NODATA_NP, integrator=integrator, substeps=substeps,
                        derive=derive, terminal=True, scenarios=True) as p:
            assert p.h and p.log == ""


def test_known_text_without_parameters_compiles():
    with ODEProgram(bp.KNOWN_SOURCE, 1, 1, 0, ndata=1, terminal=True, states=True, scenarios=True) as p:
        assert p.h and p.log == ""


# ---- the Python layer: a program stands in by its shape, nothing is compiled ------------------------------------------
class _Prog:
    ny, nx, nparams, ndata = bp.NY, bp.NX, bp.NP, bp.ND

    def __init__(self, scenarios):
        self.scenarios = scenarios


NT = 9


def _problem(prog, state0, params, data, mixed=False):
    if mixed:
        return MixedODEProblem(prog, bp.MIXED_NU, bp.MIXED_LO, bp.MIXED_HI, bp.MIXED_V, None, 0.0, 0.9, NT, state0,
                               params, data=data)
    return DeviceODEProblem(prog, bp.V, None, 0.0, 0.9, NT, state0, params, data=data)


@pytest.mark.parametrize("mixed", [False, True], ids=["device", "mixed"])
def test_S_inference_broadcast_and_layouts(mixed):
    y0, par, data = draw_scenarios(5, NT)
    rows = np.array(bp.make_data(NT))
    # every input per scenario
    pr = _problem(_Prog(3), y0, par, data, mixed)
    assert pr.S == 5
    lay = pr.device_layouts()
    assert lay["state0"].shape == (bp.NY, 5) and lay["params"].shape == (bp.NP, 5)
    assert lay["data"].shape == (NT, bp.ND, 5)
    assert all(a.flags["C_CONTIGUOUS"] and a.dtype == np.float64 for a in lay.values())
    for s in range(5):  # entry [r*S + s], [e*S + s], [(c*ND + e)*S + s] of the flat arrays
        assert [lay["state0"].ravel()[r * 5 + s] for r in range(bp.NY)] == y0[s].tolist()
        assert [lay["params"].ravel()[e * 5 + s] for e in range(bp.NP)] == par[s].tolist()
        for c in range(NT):
            assert [lay["data"].ravel()[(c * bp.ND + e) * 5 + s] for e in range(bp.ND)] == data[s, c].tolist()
    # one input per scenario, the others broadcast
    pr = _problem(_Prog(3), bp.STATE0, par, rows, mixed)
    assert pr.S == 5 and pr.state0.shape == (5, bp.NY) and pr.data.shape == (5, NT, bp.ND)
    assert np.array_equal(pr.device_layouts()["state0"], np.tile(np.array(bp.STATE0)[:, None], (1, 5)))
    assert np.array_equal(pr.device_layouts()["data"], np.tile(rows[:, :, None], (1, 1, 5)))
    # nothing per scenario: S = 1
    pr = _problem(_Prog(1), bp.STATE0, bp.PARAMS, rows, mixed)
    assert pr.S == 1 and pr.device_layouts()["data"].shape == (NT, bp.ND)
    assert pr.device_layouts()["state0"].shape == (bp.NY, 1)
    # shared data of a program with scen = 1 stay the (nt, ndata) table
    pr = _problem(_Prog(1), y0, par, rows, mixed)
    assert pr.S == 5 and np.array_equal(pr.device_layouts()["data"], rows)
    # a program without scenarios: what it was, S reads 1
    pr = _problem(_Prog(0), bp.STATE0, bp.PARAMS, rows, mixed)
    assert pr.S == 1 and pr.state0 == bp.STATE0 and pr.params == bp.PARAMS
    with pytest.raises(ValueError):
        pr.device_layouts()


@pytest.mark.parametrize("mixed", [False, True], ids=["device", "mixed"])
def test_shape_errors(mixed):
    y0, par, data = draw_scenarios(5, NT)
    rows = np.array(bp.make_data(NT))
    bad = [(y0[:, :2], par, data),            # state0 of the wrong width
           (y0[0, :2], par, data),
           (y0, par[:, :2], data),            # params of the wrong width
           (y0, par, data[:, :NT - 1]),       # data of another nt
           (y0, par, data[:, :, :1]),         # data of another ndata
           (y0, par, None),                   # data missing
           (y0[:4], par, data),               # the sizes disagree
           (y0, par[:3], rows),
           (y0, par, data[:2]),
           (y0[None], par, data)]             # one dimension too many
    for a in bad:
        with pytest.raises(ValueError):
            _problem(_Prog(3), *a, mixed)
    with pytest.raises(ValueError):           # per-scenario data need scenarios="data"
        _problem(_Prog(1), y0, par, data, mixed)
    with pytest.raises(ValueError):           # and a program without scenarios takes one state0
        _problem(_Prog(0), y0, bp.PARAMS, rows, mixed)
    _problem(_Prog(3), y0, par, data, mixed)  # the good one


def test_K_must_be_a_multiple_of_S():
    """Before a context is made, so without a GPU."""
    from mioc.trm_batch import TRM_batch
    from mioc.trm_mixed import TRM_mixed_batch
    import mioc
    y0, par, data = draw_scenarios(3, NT)
    par_trm = mioc.TRM_parameters(beta=1e-3, Delta0=0.25, p=1, maxiter=2, kmax=2)
    pr = _problem(_Prog(3), y0, par, data)
    for K in (1, 2, 4, 7):
        with pytest.raises(ValueError, match="scenarios"):
            TRM_batch(pr, par_trm, K=K)
        with pytest.raises(ValueError, match="scenarios"):
            TRM_batch(pr, par_trm, x0=np.zeros((K, NT, bp.NX)))
        with pytest.raises(ValueError, match="scenarios"):
            pr.check_restarts(K)
    pr.check_restarts(3), pr.check_restarts(6)
    mp = _problem(_Prog(3), y0, par, data, mixed=True)
    with pytest.raises(ValueError, match="scenarios"):
        TRM_mixed_batch(mp, par_trm, K=4)
    with pytest.raises(ValueError, match="scenarios"):
        TRM_mixed_batch(mp, par_trm, x0=np.zeros((5, NT, bp.NX)))
    _problem(_Prog(0), bp.STATE0, bp.PARAMS, np.array(bp.make_data(NT))).check_restarts(7)  # no scenarios: any K


def test_best_per_scenario():
    v = [3.0, 1.0, 2.0, 0.5, 5.0, 1.0, 0.5, np.nan, 4.0]
    assert best_per_scenario(v, 3).tolist() == [3, 1, 5]      # the first at a tie (3 and 6), a NaN never wins
    assert best_per_scenario(v, 1).tolist() == [3]
    assert best_per_scenario(v, 9).tolist() == list(range(9))
    for S in (0, 2, 4):
        with pytest.raises(ValueError):
            best_per_scenario(v, S)
