"""CPU tier of user-defined ODE objectives (mioc_ode_program_create / _destroy, include/mioc.h): the hook text is
compiled for gfx950 without a GPU; compile errors carry the hooks' own line numbers; argument limits; and the host
mirror of the tests' fourth problem (tests/ode_program_problem.py), against which the device is compared in
test_gpu_ode_program.py, pinned by finite differences the way test_ode_oracle.py pins the oracle."""
import ctypes

import numpy as np
import pytest

import mioc
from mioc import native
from mioc.ode_device import EXAMPLE_SHAPES, EXAMPLE_SOURCES, MiocCompileError, ODEProgram

import ode_program_problem as fourth


def _create(text, ny, nx, nparams, log_cap=4096, out=True):
    lib = native.load_library()
    h = ctypes.c_void_p()
    log = None
    if log_cap is not None:  # prefilled, with 8 guard bytes behind log_cap
        log = ctypes.create_string_buffer(log_cap + 8)
        log.raw = b"\xff" * (log_cap + 8)
    rc = lib.mioc_ode_program_create(text, ny, nx, nparams, ctypes.byref(h) if out else None, log,
                                     0 if log_cap is None else log_cap)
    return lib, rc, h, log


CASES = [(n, EXAMPLE_SOURCES[n]) + EXAMPLE_SHAPES[n] for n in ("fishing", "doubletank", "vanderpol")] + \
    [("fourth", fourth.SOURCE, fourth.NY, fourth.NX, len(fourth.PARAMS))]


@pytest.mark.parametrize("name,text,ny,nx,nparams", CASES, ids=[c[0] for c in CASES])
def test_create_and_destroy(name, text, ny, nx, nparams):
    lib, rc, h, log = _create(text.encode(), ny, nx, nparams)
    assert rc == native.MIOC_OK, log.value.decode()
    assert h.value
    assert lib.mioc_ode_program_destroy(h) == native.MIOC_OK


def test_compile_error_carries_the_hooks_line_number():
    text = EXAMPLE_SOURCES["fishing"].lstrip("\n").split("\n")
    text[2] = "this is not HIP;"  # line 3 of the text
    lib, rc, h, log = _create("\n".join(text).encode(), 2, 3, 12)
    assert rc == native.MIOC_ECOMPILE and not h.value
    assert "hooks:3" in log.value.decode(), log.value.decode()
    with pytest.raises(MiocCompileError) as e:
        ODEProgram("\n".join(text), 2, 3, 12)
    assert "hooks:3" in e.value.log and e.value.code == native.MIOC_ECOMPILE


def test_missing_hook_is_a_compile_error():
    text = EXAMPLE_SOURCES["fishing"]
    cut = text.index("__device__ void Gu")
    lib, rc, h, log = _create(text[:cut].encode(), 2, 3, 12)
    assert rc == native.MIOC_ECOMPILE and not h.value
    assert len(log.value) > 0 and b"Gu" in log.value


def test_log_is_truncated_and_terminated():
    lib, rc, h, full = _create(b"int a = ;\nint b = ;\nint c = ;\n", 2, 3, 0)
    assert rc == native.MIOC_ECOMPILE and len(full.value) > 64
    cap = 24
    lib, rc, h, log = _create(b"int a = ;\nint b = ;\nint c = ;\n", 2, 3, 0, log_cap=cap)
    assert rc == native.MIOC_ECOMPILE
    raw = log.raw
    assert raw[cap - 1] == 0 and b"\x00" not in raw[:cap - 1]      # cap - 1 characters, then the terminator
    assert raw[:cap - 1] == full.value[:cap - 1]
    assert raw[cap:] == b"\xff" * (len(raw) - cap)                 # nothing written past log_cap
    lib, rc, h, log = _create(b"int a = ;\n", 2, 3, 0, log_cap=None)  # a NULL log
    assert rc == native.MIOC_ECOMPILE


@pytest.mark.parametrize("ny,nx,nparams", [(0, 3, 0), (9, 3, 0), (2, 9, 0), (2, 0, 0), (2, 3, 33), (2, 3, -1)])
def test_limits(ny, nx, nparams):
    lib, rc, h, log = _create(EXAMPLE_SOURCES["fishing"].encode(), ny, nx, nparams)
    assert rc == native.MIOC_EINVAL and not h.value


def test_null_arguments_and_oversize_source():
    lib, rc, h, log = _create(None, 2, 3, 12)
    assert rc == native.MIOC_EINVAL and not h.value
    lib, rc, h, log = _create(EXAMPLE_SOURCES["fishing"].encode(), 2, 3, 12, out=False)
    assert rc == native.MIOC_EINVAL
    lib, rc, h, log = _create(b" " * ((1 << 20) + 1), 2, 3, 12)
    assert rc == native.MIOC_EINVAL and not h.value
    assert lib.mioc_ode_program_destroy(None) == native.MIOC_EINVAL
    with pytest.raises(native.MiocNativeError):
        ODEProgram(EXAMPLE_SOURCES["fishing"], 9, 3, 12)


INTEGRATORS = {"euler": (native.MIOC_ODE_INT_EULER, ""), "heun": (native.MIOC_ODE_INT_HEUN, "#define NS 2\n"),
               "rk4": (native.MIOC_ODE_INT_RK4, "#define NS 4\n"), "beuler": (native.MIOC_ODE_INT_BEULER, "#define TH 1.0\n"),
               "midpoint": (native.MIOC_ODE_INT_MIDPOINT, "#define TH 0.5\n")}
MARKERS = ['#line 1 "mioc_ad"', '#line 1 "hooks"\n', '\n#line 1 "mioc_ad_hooks"', '\n#line 1 "mioc_ode_program_skeleton"']


def _source(text, ny, nx, nparams, ndata=0, integrator=native.MIOC_ODE_INT_EULER, substeps=1, derive=0, flags=0,
            noinline=0, cap=1 << 18):
    """mioc_ode_program_source into a prefilled buffer with 8 guard bytes behind cap: (return value, buffer)."""
    lib = native.load_library()
    buf = ctypes.create_string_buffer(cap + 8)
    buf.raw = b"\xff" * (cap + 8)
    return lib.mioc_ode_program_source(text, ny, nx, nparams, ndata, integrator, substeps, derive, flags, noinline, buf,
                                       cap), buf


@pytest.mark.parametrize("derive", [0, native.MIOC_ODE_DERIVE_ALL])
@pytest.mark.parametrize("integrator", list(INTEGRATORS))
def test_source_has_the_hooks_verbatim_and_the_documented_order(integrator, derive):
    """include/mioc.h, "Derived hooks": the head, the dual type under mioc_ad, the caller's text under hooks, the
    generated hooks under mioc_ad_hooks, the skeleton; the two mioc_ad parts only with derive != 0."""
    code, head = INTEGRATORS[integrator]
    hooks = fourth.SOURCE.encode()
    n, buf = _source(hooks, fourth.NY, fourth.NX, len(fourth.PARAMS), integrator=code, derive=derive)
    text = buf.value
    assert n == len(text) > len(hooks)
    assert text.startswith(f"#define NY {fourth.NY}\n#define NX {fourth.NX}\n#define NP {len(fourth.PARAMS)}\n{head}"
                           .encode() + (b"#define MIOC_DERIVE_FY 1\n" if derive else b'#line 1 "hooks"\n'))
    at = [text.find(m.encode()) for m in MARKERS]
    present = [a for a, m in zip(at, MARKERS) if derive or "mioc_ad" not in m]
    assert all(a >= 0 for a in present) and present == sorted(present), at
    assert all(text.count(m.encode()) == (1 if derive or "mioc_ad" not in m else 0) for m in MARKERS)
    assert text[at[1] + len(MARKERS[1]):].startswith(hooks + b"\n#line 1 ")    # verbatim, directly behind its marker
    for once in (b"struct Par {", b"*gate == 0", b"pe[e] = P.p[e]", b"+ E(p, tend, y)", b"#define MIOC_DATA_ARG ,"):
        assert text.count(once) == 1, once                                     # what every integrator shares: once
    n1, buf1 = _source(hooks, fourth.NY, fourth.NX, len(fourth.PARAMS), integrator=code, derive=derive, noinline=1)
    assert buf1.value == b"#define MIOC_AD_NOINLINE 1\n" + text and n1 == len(buf1.value)


def test_source_of_a_plain_program_names_no_feature():
    for integrator, (code, _) in INTEGRATORS.items():
        n, buf = _source(fourth.SOURCE.encode(), fourth.NY, fourth.NX, len(fourth.PARAMS), integrator=code)
        for word in (b"mioc_ad", b"MIOC_TERMINAL 1", b"MIOC_STATES 1", b"MIOC_DERIVE_", b"NOINLINE 1"):
            assert n > 0 and word not in buf.value, (integrator, word)
        # ND: only the skeleton's own default, "#ifndef ND / #define ND 0"; nothing in front of the skeleton defines it
        assert buf.value.count(b"#define ND") == 1 and b"#ifndef ND\n#define ND 0\n#endif\n" in buf.value
        assert b"#define ND" not in buf.value[:buf.value.index(MARKERS[3].encode())]
    both = native.MIOC_ODE_TERMINAL | native.MIOC_ODE_STATES
    n, buf = _source(fourth.SOURCE.encode(), fourth.NY, fourth.NX, len(fourth.PARAMS), ndata=3, flags=both)
    head = buf.value[:buf.value.index(b"#line 1")]
    assert head.endswith(b"#define ND 3\n#define MIOC_TERMINAL 1\n#define MIOC_STATES 1\n")


def test_source_is_truncated_and_terminated():
    args = (fourth.SOURCE.encode(), fourth.NY, fourth.NX, len(fourth.PARAMS))
    need, full = _source(*args)
    assert need == len(full.value)
    for cap in (need + 1, need, 24, 1):
        n, buf = _source(*args, cap=cap)
        raw = buf.raw
        assert n == need                                               # the length needed, whatever fits
        assert raw[:cap] == full.value[:cap - 1] + b"\x00"             # cap - 1 characters, then the terminator
        assert raw[cap:] == b"\xff" * 8                                # nothing written past the capacity
    lib = native.load_library()
    assert lib.mioc_ode_program_source(*args, 0, native.MIOC_ODE_INT_EULER, 1, 0, 0, 0, None, 0) == need  # a NULL buffer


BOLZA_REFUSALS = [dict(ndata=17), dict(ndata=-1), dict(flags=4), dict(derive=32), dict(derive=native.MIOC_ODE_DERIVE_EY),
                  dict(integrator=3), dict(substeps=2), dict(integrator=native.MIOC_ODE_INT_RK4, substeps=65),
                  dict(integrator=native.MIOC_ODE_INT_HEUN, substeps=0)]


@pytest.mark.parametrize("kw", [dict(zip(("ny", "nx", "nparams"), c)) for c in
                                [(0, 3, 0), (9, 3, 0), (2, 9, 0), (2, 0, 0), (2, 3, 33), (2, 3, -1)]] + BOLZA_REFUSALS,
                         ids=str)
def test_source_fails_where_create_fails_its_argument_checks(kw):
    """The cases of test_limits and the refusals of mioc_ode_program_create_bolza: both entries return MIOC_EINVAL."""
    a = dict(ny=2, nx=3, nparams=12, ndata=0, integrator=native.MIOC_ODE_INT_EULER, substeps=1, derive=0, flags=0)
    a.update(kw)
    text = EXAMPLE_SOURCES["fishing"].encode()
    lib, h, log = native.load_library(), ctypes.c_void_p(), ctypes.create_string_buffer(256)
    rc = lib.mioc_ode_program_create_bolza(text, a["ny"], a["nx"], a["nparams"], a["ndata"], a["integrator"],
                                           a["substeps"], a["derive"], a["flags"], ctypes.byref(h), log, 256)
    n, buf = _source(text, **a)
    assert rc == native.MIOC_EINVAL and not h.value
    assert n == native.MIOC_EINVAL and buf.value == b""
    assert _source(None, 2, 3, 12)[0] == native.MIOC_EINVAL
    assert _source(b" " * ((1 << 20) + 1), 2, 3, 12)[0] == native.MIOC_EINVAL
    assert _source(b" " * (1 << 20), 2, 3, 12, cap=16)[0] > (1 << 20)


def test_python_source_text():
    """ODEProgram.source_text and program_source return the entry's text."""
    from mioc.ode_device import program_source
    shape = (fourth.NY, fourth.NX, len(fourth.PARAMS))
    want = _source(fourth.SOURCE.encode(), *shape, integrator=native.MIOC_ODE_INT_RK4, substeps=2)[1].value.decode()
    assert program_source(fourth.SOURCE, *shape, integrator="rk4", substeps=2) == want
    with ODEProgram(fourth.SOURCE, *shape, integrator="rk4", substeps=2) as prog:
        assert prog.source_text() == want
        assert prog.source_text(noinline=True) == "#define MIOC_AD_NOINLINE 1\n" + want
    with pytest.raises(native.MiocNativeError):
        program_source(fourth.SOURCE, 9, 2, 5)


def _fd(obj, x, h, t):
    """fd_check of oracle/ode_oracle.py (the reference's test_df) on a host objective."""
    obj.x[:, :] = x
    J = mioc.eval_f_(obj)
    mioc.eval_df_(obj)
    dfh = obj.tau * float(np.sum(obj.df * h))
    return (mioc.eval_f(obj, x + t * h) - J) / t, dfh


def test_fourth_problem_mirror_finite_differences():
    """The criterion of test_ode_oracle.py:28-32 on the fourth problem's host mirror, at x = .5 as there.

    The reference's gradient adds Gu(i, y_i, x_i) with weight 1 at every step (ODEObjective.jl:177-183), while its
    trapezoid cost (:130-146) weighs G(0, y_0, x_0) with 1/2 and evaluates the last control column twice:
    G(nt-1, y_{nt-1}, x_{nt-1}) + G(nt-1, y_nt, x_{nt-1}) / 2.  So with Gu != 0 the reference's df differs from the
    derivative of its own eval_f in the first and the last column, by exactly
        tau * (-Gu(0, y_0, x_0) / 2) . h_0   and   tau * (+Gu(nt-1, y_nt, x_{nt-1}) / 2) . h_{nt-1};
    every other column is exact.  The mirror keeps the reference's formula.  Checked both ways: a direction h that is
    zero in those two columns against the plain criterion, and a direction over all columns against the criterion
    with the two terms above added."""
    nt = 96
    obj = fourth.FourthObj(nt=nt)
    rng = np.random.default_rng(7)
    x = np.full((fourth.NX, nt), 0.5)
    h_all = rng.standard_normal((fourth.NX, nt))
    h_in = h_all.copy()
    h_in[:, 0] = h_in[:, nt - 1] = 0.0
    obj.x[:, :] = x
    mioc.eval_f_(obj)  # caches the states
    gu0, gue = np.zeros(fourth.NX), np.zeros(fourth.NX)
    obj.Gu(gu0, 0, obj.state0, x[:, 0])
    obj.Gu(gue, nt - 1, obj.state[:, nt - 1].copy(), x[:, nt - 1])
    for h, ends in ((h_in, 0.0), (h_all, obj.tau * (-0.5 * gu0 @ h_all[:, 0] + 0.5 * gue @ h_all[:, nt - 1]))):
        errs = []
        for t in (1e-4, 1e-5, 1e-6):
            fd, dfh = _fd(obj, x, h, t)
            errs.append((abs(fd - (dfh + ends)), abs(dfh)))
        print(errs)
        scale = max(1e-12, errs[0][1])
        assert errs[2][0] <= 1e-4 * scale + 1e-9, errs
        assert errs[1][0] <= errs[0][0] * 0.5 + 1e-9, errs
    assert abs(ends) > 1e-3 * scale  # the end terms are far above the criterion: Gu is exercised
