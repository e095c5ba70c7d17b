"""CPU tier of the Heun / RK4 integrators of user-defined ODE objectives (mioc_ode_program_create_ex, include/mioc.h,
"Integrators"): the programs compile for gfx950 without a GPU; bad integrators and substep counts are refused; and
the host mirror of the scheme (tests/ode_rk_mirror.py), against which the device is compared in
test_gpu_ode_integrators.py, has an exact gradient (the criterion of test_ode_oracle.py) and the scheme's order."""
import ctypes

import numpy as np
import pytest

from mioc import native
from mioc.ode_device import EXAMPLE_SHAPES, EXAMPLE_SOURCES, ODEProgram, example_program

import ode_program_problem as fourth
from ode_rk_mirror import ORDER_BANDS, order_control, rk_eval

INT = {"euler": native.MIOC_ODE_INT_EULER, "heun": native.MIOC_ODE_INT_HEUN, "rk4": native.MIOC_ODE_INT_RK4}


def _create_ex(text, ny, nx, nparams, integrator, substeps):
    lib = native.load_library()
    h = ctypes.c_void_p()
    log = ctypes.create_string_buffer(4096)
    rc = lib.mioc_ode_program_create_ex(text, ny, nx, nparams, integrator, substeps, ctypes.byref(h), log, 4096)
    return lib, rc, h, log


CASES = [(n, EXAMPLE_SOURCES[n]) + EXAMPLE_SHAPES[n] for n in ("fishing", "doubletank", "vanderpol")] + \
    [("fourth", fourth.SOURCE, fourth.NY, fourth.NX, len(fourth.PARAMS))]


@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("integrator", ["heun", "rk4"])
@pytest.mark.parametrize("name,text,ny,nx,nparams", CASES, ids=[c[0] for c in CASES])
def test_create_ex_compiles(name, text, ny, nx, nparams, integrator, substeps):
    lib, rc, h, log = _create_ex(text.encode(), ny, nx, nparams, INT[integrator], substeps)
    assert rc == native.MIOC_OK, log.value.decode()
    assert h.value and log.value == b""  # no warnings either
    assert lib.mioc_ode_program_destroy(h) == native.MIOC_OK


def _synthetic(n):
    """Hook text of a dense linear-quadratic problem with ny = nx = n: every entry of fy and fu is written."""
    sig = "(const double *p, int i, double t, const double *y, const double *x"
    return f"""
__device__ void F{sig}, double *f) {{
  for (int r = 0; r < {n}; ++r) {{
    double a = -y[r] + t * x[r];
    for (int c = 0; c < {n}; ++c) a = a + (0.01 * (r + 1)) * (y[c] * x[(r + c) % {n}]);
    f[r] = a;
  }}
}}
__device__ void Fy{sig}, double (*fy)[NY]) {{
  for (int r = 0; r < {n}; ++r)
    for (int c = 0; c < {n}; ++c) fy[r][c] = (r == c ? -1.0 : 0.0) + (0.01 * (r + 1)) * x[(r + c) % {n}];
}}
__device__ void Fu{sig}, double (*fu)[NX]) {{
  for (int r = 0; r < {n}; ++r)
    for (int m = 0; m < {n}; ++m) fu[r][m] = (r == m ? t : 0.0) + (0.01 * (r + 1)) * y[(m - r + {n}) % {n}];
}}
__device__ double G{sig}) {{
  double g = 0.0;
  for (int r = 0; r < {n}; ++r) g = g + (0.5 * (y[r] * y[r]) + 0.1 * (x[r] * y[r]));
  return g;
}}
__device__ void Gy{sig}, double *gy) {{
  for (int r = 0; r < {n}; ++r) gy[r] = y[r] + 0.1 * x[r];
}}
__device__ void Gu{sig}, double *gu) {{
  for (int r = 0; r < {n}; ++r) gu[r] = 0.1 * y[r];
}}
"""


def test_create_ex_compiles_the_largest_shape():
    lib, rc, h, log = _create_ex(_synthetic(8).encode(), 8, 8, 0, native.MIOC_ODE_INT_RK4, 64)
    assert rc == native.MIOC_OK, log.value.decode()
    assert lib.mioc_ode_program_destroy(h) == native.MIOC_OK


@pytest.mark.parametrize("integrator,substeps", [(-1, 1), (3, 1), (native.MIOC_ODE_INT_RK4, 0),
                                                 (native.MIOC_ODE_INT_HEUN, 65), (native.MIOC_ODE_INT_EULER, 2)])
def test_create_ex_refusals(integrator, substeps):
    lib, rc, h, log = _create_ex(fourth.SOURCE.encode(), fourth.NY, fourth.NX, len(fourth.PARAMS), integrator, substeps)
    assert rc == native.MIOC_EINVAL and not h.value


def test_create_ex_euler_is_create():
    lib, rc, h, log = _create_ex(fourth.SOURCE.encode(), fourth.NY, fourth.NX, len(fourth.PARAMS),
                                 native.MIOC_ODE_INT_EULER, 1)
    assert rc == native.MIOC_OK and h.value, log.value.decode()
    assert lib.mioc_ode_program_destroy(h) == native.MIOC_OK


def test_python_arguments():
    args = (fourth.SOURCE, fourth.NY, fourth.NX, len(fourth.PARAMS))
    for kw in (dict(integrator="rk5"), dict(integrator="rk4", substeps=0), dict(integrator="rk4", substeps=65),
               dict(integrator="heun", substeps=1.5), dict(integrator="euler", substeps=2), dict(substeps=2)):
        with pytest.raises(ValueError):
            ODEProgram(*args, **kw)
    with ODEProgram(*args) as p:
        assert (p.integrator, p.substeps) == ("euler", 1)
    with ODEProgram(*args, integrator="rk4", substeps=3) as p:
        assert (p.integrator, p.substeps) == ("rk4", 3) and p.h
    with example_program("vanderpol", integrator="heun", substeps=2) as p:
        assert (p.integrator, p.substeps, p.ny, p.nx) == ("heun", 2, 2, 3)


def test_example_problem_takes_the_scheme_and_a_coarse_grid():
    from mioc.ode_device import example_problem
    from mioc.trm_batch import PROBLEMS
    prob = example_problem("vanderpol", nt=256, integrator="rk4", substeps=4)
    assert (prob.nt, prob.program.integrator, prob.program.substeps) == (256, "rk4", 4)
    prob.program.close()
    prob = example_problem("fishing")
    assert (prob.nt, prob.program.integrator, prob.program.substeps) == (PROBLEMS["fishing"][1], "euler", 1)
    prob.program.close()


@pytest.mark.parametrize("integrator,substeps", [("heun", 1), ("rk4", 1), ("rk4", 3)])
def test_mirror_gradient_is_exact(integrator, substeps):
    """The criterion of test_ode_oracle.py:28-32 at x = .5 and a Gaussian direction over all columns: no end-column
    corrections, df is the derivative of the scheme's own J."""
    nt = 24
    obj = fourth.FourthObj(nt=nt, T1=4.8)
    rng = np.random.default_rng(7)
    x = np.full((fourth.NX, nt), 0.5)
    h = rng.standard_normal((fourth.NX, nt))
    J, df = rk_eval(obj, x, integrator, substeps)
    dfh = obj.tau * float(np.sum(df * h))
    errs = [(abs((rk_eval(obj, x + t * h, integrator, substeps, want_df=False)[0] - J) / t - dfh), abs(dfh))
            for t in (1e-4, 1e-5, 1e-6)]
    print(errs)
    scale = max(1e-12, errs[0][1])
    assert errs[2][0] <= 1e-4 * scale + 1e-9, errs
    assert errs[1][0] <= errs[0][0] * 0.5 + 1e-9, errs


@pytest.mark.parametrize("integrator", ["heun", "rk4"])
def test_mirror_order(integrator):
    """Errors of J at substeps 1, 2, 4 against RK4 at 64 substeps fall by 2^p per halving of h (p = 2, 4)."""
    nt = 24
    obj = fourth.FourthObj(nt=nt, T1=0.96)
    x = order_control(nt)
    ref = rk_eval(obj, x, "rk4", 64, want_df=False)[0]
    e = [abs(rk_eval(obj, x, integrator, m, want_df=False)[0] - ref) for m in (1, 2, 4)]
    lo, hi = ORDER_BANDS[integrator]
    print(integrator, e, e[0] / e[1], e[1] / e[2])
    assert lo <= e[0] / e[1] <= hi and lo <= e[1] / e[2] <= hi, e
