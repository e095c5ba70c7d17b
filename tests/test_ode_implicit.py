"""CPU tier of the implicit integrators of user-defined ODE objectives (backward Euler and the implicit midpoint rule:
mioc_ode_program_create_ex, include/mioc.h, "Implicit integrators"): the programs compile for gfx950 without a GPU; bad
integrator codes and substep counts are refused; and the host mirror of the scheme (tests/ode_implicit_mirror.py),
against which the device is compared in test_gpu_ode_implicit.py, has an exact gradient (the criterion of
test_ode_integrators.py), the scheme's order, survives the stiffness that breaks RK4, and fails loudly (NaN) where the
stage equation has no root."""
import ctypes
import math

import numpy as np
import pytest

from mioc import native
from mioc.ode_device import EXAMPLE_SHAPES, EXAMPLE_SOURCES, ODEProgram, example_problem, example_program

import ode_program_problem as fourth
import ode_stiff_problem as stiff
from ode_implicit_mirror import ORDER_BANDS, theta_eval
from ode_rk_mirror import order_control, rk_eval
from test_ode_integrators import _synthetic

SCHEMES = ["beuler", "midpoint"]


def _create_ex(text, ny, nx, nparams, integrator, substeps):
    lib = native.load_library()
    h = ctypes.c_void_p()
    log = ctypes.create_string_buffer(4096)
    rc = lib.mioc_ode_program_create_ex(text, ny, nx, nparams, integrator, substeps, ctypes.byref(h), log, 4096)
    return lib, rc, h, log


CASES = [(n, EXAMPLE_SOURCES[n]) + EXAMPLE_SHAPES[n] for n in ("fishing", "doubletank", "vanderpol")] + \
    [("fourth", fourth.SOURCE, fourth.NY, fourth.NX, len(fourth.PARAMS)),
     ("stiff", stiff.SOURCE, stiff.NY, stiff.NX, len(stiff.PARAMS))]


@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("integrator", SCHEMES)
@pytest.mark.parametrize("name,text,ny,nx,nparams", CASES, ids=[c[0] for c in CASES])
def test_create_ex_compiles(name, text, ny, nx, nparams, integrator, substeps):
    """Fails before the implicit schemes exist: the Python names raise ValueError."""
    with ODEProgram(text, ny, nx, nparams, integrator=integrator, substeps=substeps) as p:
        assert p.h and p.log == ""  # no warnings either
        assert (p.integrator, p.substeps) == (integrator, substeps)


@pytest.mark.parametrize("integrator", SCHEMES)
def test_create_ex_compiles_the_largest_shape(integrator):
    code = {"beuler": native.MIOC_ODE_INT_BEULER, "midpoint": native.MIOC_ODE_INT_MIDPOINT}[integrator]
    lib, rc, h, log = _create_ex(_synthetic(8).encode(), 8, 8, 0, code, 64)
    assert rc == native.MIOC_OK, log.value.decode()
    assert h.value and log.value == b""
    assert lib.mioc_ode_program_destroy(h) == native.MIOC_OK


def test_codes():
    assert (native.MIOC_ODE_INT_BEULER, native.MIOC_ODE_INT_MIDPOINT) == (16, 17)
    assert (native.MIOC_ODE_NEWTON_MAX, native.MIOC_ODE_NEWTON_TOL) == (12, 1e-10)


@pytest.mark.parametrize("integrator,substeps", [(3, 1), (15, 1), (18, 1), (native.MIOC_ODE_INT_BEULER, 0),
                                                 (native.MIOC_ODE_INT_MIDPOINT, 65)])
def test_create_ex_refusals(integrator, substeps):
    lib, rc, h, log = _create_ex(fourth.SOURCE.encode(), fourth.NY, fourth.NX, len(fourth.PARAMS), integrator, substeps)
    assert rc == native.MIOC_EINVAL and not h.value


def test_python_arguments():
    args = (fourth.SOURCE, fourth.NY, fourth.NX, len(fourth.PARAMS))
    for kw in (dict(integrator="beuler", substeps=0), dict(integrator="midpoint", substeps=65),
               dict(integrator="midpoint", substeps=1.5), dict(integrator="theta")):
        with pytest.raises(ValueError):
            ODEProgram(*args, **kw)
    with ODEProgram(*args, integrator="midpoint", substeps=3) as p:
        assert (p.integrator, p.substeps) == ("midpoint", 3) and p.h
    with example_program("fishing", integrator="beuler", substeps=2) as p:
        assert (p.integrator, p.substeps, p.ny, p.nx) == ("beuler", 2, 2, 3)
    prob = example_problem("vanderpol", nt=256, integrator="beuler", substeps=2)
    assert (prob.nt, prob.program.integrator, prob.program.substeps) == (256, "beuler", 2)
    prob.program.close()


PROBLEMS = {"fourth": (fourth.FourthObj, fourth.NX, 4.8), "stiff": (stiff.StiffObj, stiff.NX, 0.96)}


@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("integrator", SCHEMES)
@pytest.mark.parametrize("problem", ["fourth", "stiff"])
def test_mirror_gradient_is_exact(problem, integrator, substeps):
    """The criterion of test_ode_integrators.py::test_mirror_gradient_is_exact, unchanged, at x = .5 and a Gaussian
    direction over all columns: df is the derivative of the scheme's own J."""
    nt = 24
    cls, nx, T1 = PROBLEMS[problem]
    obj = cls(nt=nt, T1=T1)
    rng = np.random.default_rng(7)
    x = np.full((nx, nt), 0.5)
    h = rng.standard_normal((nx, nt))
    stats = []
    J, df = theta_eval(obj, x, integrator, substeps, stats=stats)
    assert math.isfinite(J) and np.all(np.isfinite(df))
    dfh = obj.tau * float(np.sum(df * h))
    errs = [(abs((theta_eval(obj, x + t * h, integrator, substeps, want_df=False)[0] - J) / t - dfh), abs(dfh))
            for t in (1e-4, 1e-5, 1e-6)]
    print(errs, "Newton updates per substep:", min(stats), "..", max(stats))
    scale = max(1e-12, errs[0][1])
    assert errs[2][0] <= 1e-4 * scale + 1e-9, errs
    assert errs[1][0] <= errs[0][0] * 0.5 + 1e-9, errs


@pytest.mark.parametrize("integrator", SCHEMES)
def test_mirror_order(integrator):
    """Errors of J at substeps 1, 2, 4 against RK4 at 64 substeps fall by 2^p per halving of h (p = 1, 2)."""
    nt = 24
    obj = fourth.FourthObj(nt=nt, T1=0.96)
    x = order_control(nt)
    ref = rk_eval(obj, x, "rk4", 64, want_df=False)[0]
    e = [abs(theta_eval(obj, x, integrator, m, want_df=False)[0] - ref) for m in (1, 2, 4)]
    lo, hi = ORDER_BANDS[integrator]
    print(integrator, e, e[0] / e[1], e[1] / e[2])
    assert lo <= e[0] / e[1] <= hi and lo <= e[1] / e[2] <= hi, e


def test_stiffness():
    """kappa h = 80: one implicit substep per control interval is within 5e-4 relative of the converged value (implicit
    midpoint at 512 substeps); RK4 with one substep leaves its stability region and blows up."""
    nt = 24
    obj = stiff.StiffObj(nt=nt, T1=0.96)
    x = order_control(nt)
    Jstar = theta_eval(obj, x, "midpoint", 512, want_df=False)[0]
    assert math.isfinite(Jstar)
    for integrator in SCHEMES:
        stats = []
        J = theta_eval(obj, x, integrator, 1, want_df=False, stats=stats)[0]
        print(integrator, J, Jstar, abs(J - Jstar) / abs(Jstar), "Newton updates", min(stats), "..", max(stats))
        assert max(stats) > 1  # nonlinear in y: Newton iterates
        assert abs(J - Jstar) <= 5e-4 * abs(Jstar), (integrator, J, Jstar)
    with np.errstate(all="ignore"):
        Jrk = rk_eval(obj, x, "rk4", 1, want_df=False)[0]
    print("rk4 m=1:", Jrk)
    assert not math.isfinite(Jrk) or abs(Jrk) > 1e6


@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("integrator", SCHEMES)
def test_non_convergence_is_nan(integrator, substeps):
    """F = x (1e3 + 1e6 y^2) - y: with x = 1 the stage equation has no real root, so Newton cannot converge."""
    nt = 8
    obj = stiff.NoRootObj(nt=nt, T1=0.32)
    last = np.zeros((1, nt))
    last[0, nt - 1] = 1.0
    for x in (np.ones((1, nt)), last):
        J, df = theta_eval(obj, x, integrator, substeps)
        assert math.isnan(J) and df.shape == (1, nt) and np.all(np.isnan(df))
        assert math.isnan(theta_eval(obj, x, integrator, substeps, want_df=False)[0])
    J, df = theta_eval(obj, np.zeros((1, nt)), integrator, substeps)
    assert math.isfinite(J) and np.all(np.isfinite(df))
