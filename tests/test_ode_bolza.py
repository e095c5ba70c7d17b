"""CPU tier of the terminal cost, the sampled data and the state output of user-defined ODE objectives
(mioc_ode_program_create_bolza; include/mioc.h, "Terminal cost, sampled data, state output"): the programs compile for
gfx950 without a GPU, bad arguments are refused, and the host mirror (tests/ode_bolza_mirror.py), against which the
device is compared in test_gpu_ode_bolza.py, has an exact gradient (the criterion of test_ode_integrators.py) and
gives the hand-derived known answer bit for bit."""
import ctypes

import numpy as np
import pytest

from mioc import native
from mioc.ode_device import MiocCompileError, DeviceODEProblem, MixedODEProblem, ODEProgram, derive_names

import ode_bolza_problem as bp
from ode_bolza_mirror import bolza_eval

INT = {"euler": native.MIOC_ODE_INT_EULER, "heun": native.MIOC_ODE_INT_HEUN, "rk4": native.MIOC_ODE_INT_RK4,
       "beuler": native.MIOC_ODE_INT_BEULER, "midpoint": native.MIOC_ODE_INT_MIDPOINT}
SCHEMES = [("euler", 1), ("heun", 1), ("rk4", 3), ("beuler", 1), ("midpoint", 2)]
BOTH = native.MIOC_ODE_TERMINAL | native.MIOC_ODE_STATES


def _create(text, ny, nx, nparams, ndata, integrator, substeps, derive, flags):
    lib = native.load_library()
    h = ctypes.c_void_p()
    log = ctypes.create_string_buffer(1 << 16)
    rc = lib.mioc_ode_program_create_bolza(text.encode(), ny, nx, nparams, ndata, integrator, substeps, derive, flags,
                                           ctypes.byref(h), log, 1 << 16)
    return lib, rc, h, log.value.decode()


@pytest.mark.parametrize("derive", [(), "all"], ids=["hand", "derived"])
@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_problem_compiles(integrator, substeps, derive):
    with ODEProgram(bp.SOURCE, bp.NY, bp.NX, bp.NP, integrator=integrator, substeps=substeps, derive=derive,
                    ndata=bp.ND, terminal=True, states=True) as p:
        assert p.h and p.log == ""  # no warnings either
        assert (p.ndata, p.terminal, p.states) == (bp.ND, True, True)
        assert p.derive == (("Fy", "Fu", "Gy", "Gu", "Ey") if derive else ())
    with ODEProgram(bp.SOURCE_XFREE, bp.NY, bp.NX, bp.NP, integrator=integrator, substeps=substeps, derive=derive,
                    ndata=bp.ND, terminal=True) as p:
        assert p.h and p.log == ""


@pytest.mark.parametrize("integrator,substeps", [("euler", 1), ("heun", 2), ("rk4", 64), ("beuler", 2),
                                                 ("midpoint", 64)])
def test_largest_shape_compiles(integrator, substeps):
    """ny = nx = 8, NP = 32, ND = 16, every hook derived: every scheme but Euler falls back to called hooks, which are
    handed the address of the per-lane p (run on the device in test_gpu_ode_bolza.py)."""
    lib, rc, h, log = _create(bp.synthetic_source(8, 32, 16), 8, 8, 32, 16, INT[integrator], substeps,
                              native.MIOC_ODE_DERIVE_ALL | native.MIOC_ODE_DERIVE_EY, BOTH)
    assert rc == native.MIOC_OK, log
    print(integrator, repr(log))
    assert lib.mioc_ode_program_destroy(h) == native.MIOC_OK


@pytest.mark.parametrize("ndata,derive,flags", [(-1, 0, 0), (17, 0, 0), (2, 0, 4), (2, 0, -1), (2, 0, 8 | BOTH),
                                                (2, native.MIOC_ODE_DERIVE_EY, 0),
                                                (2, native.MIOC_ODE_DERIVE_EY, native.MIOC_ODE_STATES),
                                                (2, 32, BOTH)])
def test_create_refusals(ndata, derive, flags):
    lib, rc, h, log = _create(bp.SOURCE, bp.NY, bp.NX, bp.NP, ndata, native.MIOC_ODE_INT_EULER, 1, derive, flags)
    assert rc == native.MIOC_EINVAL and not h.value


def test_create_accepts_the_limits():
    for ndata in (0, 16):  # data that no hook reads
        text = bp.SOURCE.replace("p[NP + 1]", "0.25").replace("p[NP]", "0.5")
        lib, rc, h, log = _create(text, bp.NY, bp.NX, bp.NP, ndata, native.MIOC_ODE_INT_HEUN, 2,
                                  native.MIOC_ODE_DERIVE_EY, BOTH)
        assert rc == native.MIOC_OK and h.value, log
        assert lib.mioc_ode_program_destroy(h) == native.MIOC_OK


def test_terminal_without_E_is_a_compile_error_in_the_hooks():
    text = bp.SOURCE.replace("__device__ T E(", "__device__ T E_missing(")
    lib, rc, h, log = _create(text, bp.NY, bp.NX, bp.NP, bp.ND, native.MIOC_ODE_INT_RK4, 1, 0,
                              native.MIOC_ODE_TERMINAL)
    assert rc == native.MIOC_ECOMPILE and not h.value
    assert "hooks:" in log and "'E'" in log, log
    with pytest.raises(MiocCompileError) as ei:
        ODEProgram(text, bp.NY, bp.NX, bp.NP, ndata=bp.ND, terminal=True)
    assert "hooks:" in ei.value.log


def test_python_arguments():
    args = (bp.SOURCE, bp.NY, bp.NX, bp.NP)
    for kw in (dict(ndata=-1), dict(ndata=17), dict(ndata=1.5), dict(ndata=bp.ND, derive=("Ey",)),
               dict(ndata=bp.ND, derive=("Ey",), states=True), dict(ndata=bp.ND, terminal=True, derive=("Ez",))):
        with pytest.raises(ValueError):
            ODEProgram(*args, **kw)
    assert derive_names("all") == ("Fy", "Fu", "Gy", "Gu")
    assert derive_names("all", terminal=True) == ("Fy", "Fu", "Gy", "Gu", "Ey")
    assert derive_names(("Ey", "Fu"), terminal=True) == ("Fu", "Ey")
    with ODEProgram(*args, ndata=bp.ND, terminal=True, derive=("Ey",)) as prog:
        assert prog.derive == ("Ey",)
        data = bp.make_data(12)
        prob = DeviceODEProblem(prog, bp.V, None, 0.0, 0.48, 12, bp.STATE0, bp.PARAMS, data=data)
        assert prob.data.shape == (12, bp.ND)
        for bad in (None, bp.make_data(11), [[0.0] * 3] * 12):
            with pytest.raises(ValueError):
                DeviceODEProblem(prog, bp.V, None, 0.0, 0.48, 12, bp.STATE0, bp.PARAMS, data=bad)
            with pytest.raises(ValueError):
                MixedODEProblem(prog, 1, 0.0, 2.0, bp.V[1:], None, 0.0, 0.48, 12, bp.STATE0, bp.PARAMS, data=bad)
        mp = MixedODEProblem(prog, 1, 0.0, 2.0, bp.V[1:], None, 0.0, 0.48, 12, bp.STATE0, bp.PARAMS, data=data)
        assert mp.data.shape == (12, bp.ND)
    with ODEProgram(bp.KNOWN_SOURCE.replace("p[0]", "2.0"), 1, 1, 0, terminal=True) as prog:  # no data
        with pytest.raises(ValueError):
            DeviceODEProblem(prog, [[0, 1]], None, 0.0, 1.0, 4, [0.5], data=[[1.0]] * 4)
        assert DeviceODEProblem(prog, [[0, 1]], None, 0.0, 1.0, 4, [0.5]).data is None


@pytest.mark.parametrize("integrator,substeps", [("heun", 1), ("rk4", 1), ("rk4", 3), ("beuler", 1), ("midpoint", 1),
                                                 ("euler", 1)])
def test_mirror_gradient_is_exact(integrator, substeps):
    """The criterion of test_ode_integrators.py:131-135 at x = .5 and a Gaussian direction over all columns, with the
    terminal cost and the data in J.  Euler on the variant whose G does not depend on x: the reference's Euler
    gradient is not the exact derivative of its trapezoid J otherwise (its Gu term carries the weight of an interior
    column at both ends and pairs x_i with y_i), which is the reference's scheme and no matter of this feature."""
    nt, T1 = 12, 2.4
    hooks = bp.HOOKS_XFREE if integrator == "euler" else bp.HOOKS
    data = bp.make_data(nt)
    rng = np.random.default_rng(7)
    x = np.full((nt, bp.NX), 0.5)
    h = rng.standard_normal((nt, bp.NX))

    def ev(xx, want_df):
        return bolza_eval(hooks, bp.PARAMS, data, bp.STATE0, 0.0, T1, xx, integrator, substeps, want_df)
    J, df, Y = ev(x, True)
    assert Y.shape == (nt + 1, bp.NY) and np.array_equal(Y[0], bp.STATE0)
    dfh = (T1 / nt) * float(np.sum(df * h))
    errs = [(abs((ev(x + t * h, False)[0] - J) / t - dfh), abs(dfh)) for t in (1e-4, 1e-5, 1e-6)]
    print(errs)
    scale = max(1e-12, errs[0][1])
    assert errs[2][0] <= 1e-4 * scale + 1e-9, errs
    assert errs[1][0] <= errs[0][0] * 0.5 + 1e-9, errs


@pytest.mark.parametrize("integrator,substeps", [("euler", 1), ("heun", 1), ("heun", 2), ("beuler", 1),
                                                 ("midpoint", 1)])
def test_mirror_known_answer(integrator, substeps):
    """Exact in doubles, derived by hand: F = d x, G = d x, E = 2 y on data 1, 2, 4, 8.  Euler's trapezoid picks the
    data columns 0, 1, 2, 3, 3; a wrong column rule changes J."""
    kn = bp.KNOWN
    J, df, Y = bolza_eval(bp.KNOWN_HOOKS, [], kn["data"], kn["state0"], kn["T0"], kn["T1"], kn["x"], integrator,
                          substeps)
    assert Y[:, 0].tolist() == kn["Y"]
    assert df[:, 0].tolist() == kn["df"]
    assert J == (kn["J_euler"] if integrator == "euler" else kn["J_other"])
