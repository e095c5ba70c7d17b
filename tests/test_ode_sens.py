"""CPU tier of the sensitivities of user-defined ODE objectives (mioc_ode_program_create_sens, _source_sens;
include/mioc.h, "Sensitivities"): the host mirror (tests/ode_sens_mirror.py), against which the device is compared in
test_gpu_ode_sens.py, has exact gradients in the parameters and in state0 (the criterion of
test_ode_bolza.py::test_mirror_gradient_is_exact), each of its named wrong versions misses that criterion, and it gives
the hand-derived known answer; a program without sensitivities is assembled from the text it always had; bad arguments
are refused; the programs compile for gfx950 without a GPU."""
import ctypes

import numpy as np
import pytest

from mioc import native
from mioc.ode_device import (MiocCompileError, DeviceODEProblem, ODEProgram, derive_names, program_source,
                             sensitivity_bits, EXAMPLE_SHAPES, EXAMPLE_SOURCES_AD_P)

import ode_bolza_problem as bp
import ode_sens_problem as sp
from ode_bolza_mirror import bolza_eval
from ode_sens_mirror import WRONG, sens_eval, sens_eval_scen

INT = {"euler": native.MIOC_ODE_INT_EULER, "heun": native.MIOC_ODE_INT_HEUN, "rk4": native.MIOC_ODE_INT_RK4,
       "beuler": native.MIOC_ODE_INT_BEULER, "midpoint": native.MIOC_ODE_INT_MIDPOINT}
SCHEMES = [("heun", 1), ("rk4", 1), ("rk4", 3), ("beuler", 1), ("midpoint", 2)]
BOTH = native.MIOC_ODE_TERMINAL | native.MIOC_ODE_STATES
P_BITS = native.MIOC_ODE_DERIVE_FP | native.MIOC_ODE_DERIVE_GP | native.MIOC_ODE_DERIVE_EP
EVERY = native.MIOC_ODE_DERIVE_ALL | native.MIOC_ODE_DERIVE_EY | P_BITS
NT, T1 = 12, 2.4


# ---- 1. the mirror's gradients against differences of its own J --------------------------------------------------------
def _meets_the_bar(J_of, J, slope):
    """The criterion of test_mirror_gradient_is_exact: J_of(t) is J at the point moved by t along the direction, slope
    the claimed directional derivative."""
    errs = [(abs((J_of(t) - J) / t - slope), abs(slope)) for t in (1e-4, 1e-5, 1e-6)]
    scale = max(1e-12, errs[0][1])
    return errs[2][0] <= 1e-4 * scale + 1e-9 and errs[1][0] <= errs[0][0] * 0.5 + 1e-9, errs


def _direction_check(integrator, substeps, part, wrong=None):
    """One restart of the test problem and a Gaussian direction: (dp, 0) for part "p", (0, dy) for part "y0", so that
    each gradient is held on its own and the two slopes cannot cancel.  A forward difference is itself off by
    t d'Hd / 2, about 0.8 t on this problem whatever the slope is, so the bar at t = 1e-6 can only be met along a
    direction whose slope is not a near-cancellation: the seed is one whose directions make an angle of less than 80
    degrees with the gradients, which the test asserts for the right version."""
    rng = np.random.default_rng(1)
    x = np.stack([rng.integers(0, 3, size=NT), rng.integers(0, 2, size=NT)], axis=1).astype(np.float64)
    dp, dy = rng.standard_normal(sp.NP), rng.standard_normal(sp.NY)
    dp, dy = dp * (part == "p"), dy * (part == "y0")
    data = sp.make_data(NT)
    p0, y0 = np.array(sp.PARAMS), np.array(sp.STATE0)

    def ev(p, y, wrong=None):
        return sens_eval(sp.HOOKS, p.tolist(), data, y.tolist(), 0.0, T1, x, integrator, substeps, wrong)
    J, _, Jp, Jy0 = ev(p0, y0, wrong)
    assert J == ev(p0, y0)[0]  # a wrong version changes neither J nor df
    slope = float(Jp @ dp + Jy0 @ dy)
    if wrong is None:
        g, d = (Jp, dp) if part == "p" else (Jy0, dy)
        assert abs(slope) >= np.cos(np.radians(80.0)) * np.linalg.norm(g) * np.linalg.norm(d), (slope, g, d)
    return _meets_the_bar(lambda t: ev(p0 + t * dp, y0 + t * dy)[0], J, slope)


def _scenario_check(integrator, substeps, part, wrong=None):
    """S = 2 scenarios, K = 4 restarts: restart 1 (scenario 1 = 1 % 2, not 0 = 1 / 2) in a direction of its own
    scenario's parameters (part "p") or state0 (part "y0")."""
    rng = np.random.default_rng(1)
    S, K, q = 2, 4, 1
    x = np.stack([rng.integers(0, 3, size=(K, NT)), rng.integers(0, 2, size=(K, NT))], axis=2).astype(np.float64)
    params = np.array(sp.PARAMS) * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, size=(S, sp.NP)))
    state0 = np.array(sp.STATE0) + 0.1 * rng.standard_normal((S, sp.NY))
    dp, dy = rng.standard_normal(sp.NP), rng.standard_normal(sp.NY)
    dp, dy = dp * (part == "p"), dy * (part == "y0")
    data = sp.make_data(NT)

    def ev(t, wrong=None):
        P, Y0 = params.copy(), state0.copy()
        P[q % S] += t * dp
        Y0[q % S] += t * dy
        return sens_eval_scen(sp.HOOKS, P, data, Y0, 0.0, T1, x, integrator, substeps, wrong)
    J, _, Jp, Jy0 = ev(0.0, wrong)
    Jr = ev(0.0)[0][q]
    slope = float(Jp[q] @ dp + Jy0[q] @ dy)
    return _meets_the_bar(lambda t: ev(t)[0][q], Jr, slope)


@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_mirror_sensitivities_are_exact(integrator, substeps):
    for check in (_direction_check, _scenario_check):
        for part in ("p", "y0"):
            ok, errs = check(integrator, substeps, part)
            print(check.__name__, part, errs)
            assert ok, (check.__name__, part, errs)


@pytest.mark.parametrize("wrong", WRONG)
@pytest.mark.parametrize("integrator,substeps", SCHEMES)
def test_every_wrong_version_misses_the_bar(integrator, substeps, wrong):
    check = _scenario_check if wrong == "scen_div" else _direction_check
    ok, errs = check(integrator, substeps, "y0" if wrong == "w_early" else "p", wrong)
    print(wrong, errs)
    assert not ok, (wrong, errs)


def test_mirror_J_and_df_are_the_bolza_mirrors():
    """With ND = 1 the problem is not ode_bolza_problem's, but the bodies are ode_bolza_mirror's: J and df bit for bit
    on the shared hooks."""
    x = np.full((NT, sp.NX), 1.0)
    for integrator, m in SCHEMES:
        J, df, _, _ = sens_eval(sp.HOOKS, sp.PARAMS, sp.make_data(NT), sp.STATE0, 0.0, T1, x, integrator, m)
        Jb, dfb, _ = bolza_eval(sp.HOOKS, sp.PARAMS, sp.make_data(NT), sp.STATE0, 0.0, T1, x, integrator, m)
        assert J == Jb and np.array_equal(df, dfb), integrator


# ---- 2. the known answer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,substeps", [("heun", 1), ("heun", 2), ("beuler", 1), ("midpoint", 1),
                                                 ("midpoint", 2), ("rk4", 1), ("rk4", 2)])
def test_mirror_known_answer(integrator, substeps):
    """F = p0 x, G = p1 y, E = 2 y: derived by hand in ode_sens_problem.py; every value dyadic, so exact in doubles but
    for RK4, whose b weights do not sum to 1 (the 1e-12 bar of test_gpu_ode_bolza.py::test_known_answer)."""
    kn, want = sp.KNOWN, sp.known(integrator)
    J, df, Jp, Jy0 = sens_eval(sp.KNOWN_HOOKS, kn["params"], None, kn["state0"], kn["T0"], kn["T1"], kn["x"], integrator,
                               substeps)
    print(integrator, substeps, J, df[:, 0].tolist(), Jp.tolist(), Jy0.tolist())
    if integrator == "rk4":
        assert abs(J - want["J"]) <= 1e-12 * want["J"]
        for got, ref in ((df[:, 0], want["df"]), (Jp, want["Jp"]), (Jy0, want["Jy0"])):
            assert np.max(np.abs(got - ref)) <= 1e-12 * max(ref)
    else:
        assert J == want["J"] and df[:, 0].tolist() == want["df"]
        assert Jp.tolist() == want["Jp"] and Jy0.tolist() == want["Jy0"]


# ---- 3. the C entries ------------------------------------------------------------------------------------------------
def _source(entry, *args):
    lib = native.load_library()
    fn = getattr(lib, entry)
    need = fn(*args, None, 0)
    if need < 0:
        return need
    buf = ctypes.create_string_buffer(need + 1)
    assert fn(*args, buf, need + 1) == need
    return buf.value


def test_sens_0_is_source_scen_byte_for_byte():
    """Every integrator, three derive masks, the features off and on, both compiles' texts: 150 pairs, of which the
    15 that _source_scen refuses (Ey derived without a terminal cost) are refused alike."""
    texts = 0
    for integrator in INT.values():
        for derive in (0, native.MIOC_ODE_DERIVE_ALL, native.MIOC_ODE_DERIVE_FU | native.MIOC_ODE_DERIVE_EY):
            for ndata, flags, scen in ((0, 0, 0), (0, native.MIOC_ODE_TERMINAL, 0), (1, BOTH, 0), (1, BOTH, 1),
                                       (1, BOTH, 3)):
                for noinline in (0, 1):
                    m = 1 if integrator == native.MIOC_ODE_INT_EULER else 3
                    head = (sp.SOURCE.encode(), sp.NY, sp.NX, sp.NP, ndata, integrator, m, derive, flags, scen)
                    a = _source("mioc_ode_program_source_scen", *head, noinline)
                    b = _source("mioc_ode_program_source_sens", *head, 0, noinline)
                    assert a == b
                    if isinstance(a, bytes):
                        assert b"MIOC_SENS " not in a.split(b'#line 1 "hooks"')[0]
                        texts += 1
                    else:
                        assert a == native.MIOC_EINVAL and flags == 0 and derive & native.MIOC_ODE_DERIVE_EY
    assert texts == 150 - 10


def test_the_head_of_a_sens_program():
    args = (sp.SOURCE, sp.NY, sp.NX, sp.NP, "rk4", 2)
    plain = program_source(*args, derive="all", ndata=sp.ND, terminal=True, states=True, scenarios=True)
    for sens, value in (("p", 1), ("y0", 2), (True, 3)):
        text = program_source(*args, derive="all", ndata=sp.ND, terminal=True, states=True, scenarios=True,
                              sensitivities=sens)
        assert text == plain.replace("#define MIOC_SCEN 1\n", f"#define MIOC_SCEN 1\n#define MIOC_SENS {value}\n")
    text = program_source(*args, derive="all+p", ndata=sp.ND, terminal=True, sensitivities=True)
    head = text.split('#line 1 "mioc_ad"')[0]
    assert head.endswith("#define MIOC_SENS 3\n" + "".join(f"#define MIOC_DERIVE_{n} 1\n" for n in
                                                         ("FY", "FU", "GY", "GU", "EY", "FP", "GP", "EP")))
    assert program_source(*args, derive="all+p", ndata=sp.ND, terminal=True, sensitivities=True,
                          noinline=True).startswith("#define MIOC_AD_NOINLINE 1\n")


def _create(text, ny, nx, nparams, ndata, integrator, substeps, derive, flags, scen, sens):
    lib = native.load_library()
    h = ctypes.c_void_p()
    log = ctypes.create_string_buffer(1 << 16)
    rc = lib.mioc_ode_program_create_sens(text.encode(), ny, nx, nparams, ndata, integrator, substeps, derive, flags, scen,
                                          sens, ctypes.byref(h), log, 1 << 16)
    return lib, rc, h, log.value.decode()


HEUN = native.MIOC_ODE_INT_HEUN
REFUSED = {
    "sens bit 4": dict(sens=4), "sens 7": dict(sens=7), "sens negative": dict(sens=-1),
    "Euler p": dict(integrator=native.MIOC_ODE_INT_EULER, sens=1),
    "Euler y0": dict(integrator=native.MIOC_ODE_INT_EULER, sens=2),
    "SENS_P without parameters": dict(nparams=0, sens=1),
    "SENS_P with ny * nparams = 66": dict(nparams=22, sens=3),
    "DERIVE_FP without SENS_P": dict(derive=native.MIOC_ODE_DERIVE_FP, sens=2),
    "DERIVE_GP without sens": dict(derive=native.MIOC_ODE_DERIVE_GP, sens=0),
    "DERIVE_EP without SENS_P": dict(derive=native.MIOC_ODE_DERIVE_EP, sens=2),
    "DERIVE_EP without a terminal cost": dict(derive=native.MIOC_ODE_DERIVE_EP, flags=native.MIOC_ODE_STATES, sens=1),
    "derive bit 256": dict(derive=256, sens=3),
    "a case of _create_scen": dict(scen=2, sens=3),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refusals_of_create_and_source(case):
    kw = dict(ny=sp.NY, nx=sp.NX, nparams=sp.NP, ndata=sp.ND, integrator=HEUN, substeps=1, derive=0, flags=BOTH, scen=0,
              sens=3)
    kw.update(REFUSED[case])
    lib, rc, h, log = _create(sp.SOURCE, **kw)
    assert rc == native.MIOC_EINVAL and not h.value
    order = ("ny", "nx", "nparams", "ndata", "integrator", "substeps", "derive", "flags", "scen", "sens")
    assert _source("mioc_ode_program_source_sens", sp.SOURCE.encode(), *(kw[n] for n in order), 0) == native.MIOC_EINVAL


def test_create_accepts_the_limits():
    assert native.MIOC_ODE_DERIVE_ALL == 15
    # ny * nparams = 64 both ways: 2 x 32 here and 8 x 8 below; dJ/dstate0 alone needs no parameters
    text = "\n".join(l for l in sp.KNOWN_SOURCE.splitlines() if " Fp(" not in l and " Gp(" not in l and " Ep(" not in l)
    for nparams, sens, src in ((32, 3, sp.KNOWN_SOURCE), (0, 2, text.replace("p[0]", "2.0").replace("p[1]", "4.0"))):
        lib, rc, h, log = _create(src, 2, 1, nparams, 0, HEUN, 1, 0, native.MIOC_ODE_TERMINAL, 0, sens)
        assert rc == native.MIOC_OK and h.value, log
        assert lib.mioc_ode_program_destroy(h) == native.MIOC_OK


def test_python_arguments():
    args = (sp.SOURCE, sp.NY, sp.NX, sp.NP)
    assert [sensitivity_bits(s) for s in (False, None, "p", "y0", True)] == [0, 0, 1, 2, 3]
    for kw in (dict(sensitivities="x"), dict(sensitivities=True, integrator="euler"), dict(derive=("Fp",)),
               dict(derive="all+p"), dict(derive=("Gp",), sensitivities="y0"), dict(derive="all+p", sensitivities="y0"),
               dict(derive=("Ep",), sensitivities=True), dict(derive="all+q", sensitivities=True)):
        with pytest.raises(ValueError):
            ODEProgram(*args, ndata=sp.ND, **kw)
    # "all" stays the y and u hooks whether or not sensitivities are on; "all+p" adds the p hooks
    assert derive_names("all", terminal=True, sens_p=True) == ("Fy", "Fu", "Gy", "Gu", "Ey")
    assert derive_names("all", sens_p=True) == ("Fy", "Fu", "Gy", "Gu")
    assert derive_names("all+p", sens_p=True) == ("Fy", "Fu", "Gy", "Gu", "Fp", "Gp")
    assert derive_names("all+p", terminal=True, sens_p=True) == ("Fy", "Fu", "Gy", "Gu", "Ey", "Fp", "Gp", "Ep")
    assert derive_names(("Ep", "Fu"), terminal=True, sens_p=True) == ("Fu", "Ep")
    with ODEProgram(*args, ndata=sp.ND, terminal=True) as prog:
        assert prog.sens == 0
        prob = DeviceODEProblem(prog, sp.V, None, 0.0, 0.48, 12, sp.STATE0, sp.PARAMS, data=sp.make_data(12))
        with pytest.raises(ValueError):
            prob.sensitivities(None, None)  # a program without the flag: refused before anything is touched


# ---- 4. the programs compile for gfx950 --------------------------------------------------------------------------------
MASKS = [(), "all", "all+p", ("Fp", "Gp", "Ep"), ("Fy", "Gp"), ("Gu", "Ey", "Fp")] + [(n,) for n in
                                                                                      ("Fy", "Fu", "Gy", "Gu", "Ey", "Fp",
                                                                                       "Gp", "Ep")]


@pytest.mark.parametrize("derive", MASKS, ids=lambda d: d if isinstance(d, str) else "+".join(d) or "hand")
def test_problem_compiles_with_every_mask(derive):
    """One text under its #ifndef guards: by hand, everything derived, and every hook derived on its own."""
    with ODEProgram(sp.SOURCE, sp.NY, sp.NX, sp.NP, integrator="heun", derive=derive, ndata=sp.ND, terminal=True,
                    states=True, sensitivities=True) as p:
        assert p.h and p.log == ""  # no warnings either
        assert p.sens == 3 and p.derive == derive_names(derive, True, True)


@pytest.mark.parametrize("sens", ["p", "y0", True, False])
@pytest.mark.parametrize("integrator,substeps", SCHEMES[1:])
def test_problem_compiles_under_every_scheme(integrator, substeps, sens):
    for derive in ((), "all+p" if sens in ("p", True) else "all"):
        for scenarios in (False, True):
            with ODEProgram(sp.SOURCE, sp.NY, sp.NX, sp.NP, integrator=integrator, substeps=substeps, derive=derive,
                            ndata=sp.ND, terminal=True, scenarios=scenarios, sensitivities=sens) as p:
                assert p.h and p.log == "" and p.sens == sensitivity_bits(sens)
    with ODEProgram(sp.KNOWN_SOURCE, 1, 1, 2, integrator=integrator, substeps=substeps, terminal=True, states=True,
                    sensitivities=sens) as p:
        assert p.h and p.log == ""


@pytest.mark.parametrize("integrator,substeps", [("heun", 2), ("rk4", 64), ("beuler", 2), ("midpoint", 64)])
def test_largest_square_shape_compiles(integrator, substeps):
    """ny = nx = nparams = 8 (fp is 8 x 8), every hook derived."""
    lib, rc, h, log = _create(sp.synthetic_source(8, 8), 8, 8, 8, 0, INT[integrator], substeps, EVERY, BOTH, 0, 3)
    assert rc == native.MIOC_OK, log
    print(integrator, repr(log.splitlines()[:1]))
    assert lib.mioc_ode_program_destroy(h) == native.MIOC_OK


def test_the_fishing_example_with_two_types_compiles():
    with ODEProgram(EXAMPLE_SOURCES_AD_P["fishing"], *EXAMPLE_SHAPES["fishing"], integrator="rk4", derive="all+p",
                    sensitivities=True) as p:
        assert p.h and p.derive == ("Fy", "Fu", "Gy", "Gu", "Fp", "Gp")
        print(repr(p.log.splitlines()[:1]))


def test_a_hand_written_Fp_beside_DERIVE_FP_is_a_compile_error():
    text = sp.SOURCE.replace("#ifndef MIOC_DERIVE_FP", "#ifndef MIOC_DERIVE_FP_not_asked")
    lib, rc, h, log = _create(text, sp.NY, sp.NX, sp.NP, sp.ND, HEUN, 1, native.MIOC_ODE_DERIVE_FP, BOTH, 0, 1)
    assert rc == native.MIOC_ECOMPILE and not h.value
    assert "redefinition of 'Fp'" in log, log
    with pytest.raises(MiocCompileError):
        ODEProgram(text, sp.NY, sp.NX, sp.NP, integrator="heun", derive=("Fp",), ndata=sp.ND, terminal=True,
                   sensitivities="p")


def test_a_one_type_F_cannot_be_derived_in_the_parameters():
    lib, rc, h, log = _create(bp.SOURCE + "\n__device__ void Gp(const double *p, int i, double t, const double *y, "
                              "const double *x, double *gp) {}\n__device__ void Ep(const double *p, double t, const "
                              "double *y, double *ep) {}\n", bp.NY, bp.NX, bp.NP, bp.ND, HEUN, 1,
                              native.MIOC_ODE_DERIVE_FP, BOTH, 0, 1)
    assert rc == native.MIOC_ECOMPILE and not h.value and "mioc_ad_hooks:" in log, log
