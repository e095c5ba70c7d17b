"""User-defined ODE objectives on the device: the six hooks of an AbstractODEObjective as HIP source text.

The reference's extension point is the objective (julia_opt/ODEObjective.jl:243-248: F!, Fy!, Fu!, G, Gy!, Gu!).
``ODEProgram`` hands the hooks to ``libmioc.so`` as text; the library compiles them into its explicit-Euler / adjoint
sweep for gfx950 at run time and ``Context.ode_program_eval_tensors`` runs that kernel.  The
hook contract (signatures, the step index each hook sees, zeroing, rounding order) is in ``include/mioc.h``.
``ODEProgram(..., integrator="heun" | "rk4", substeps=m)`` compiles the hooks into a Heun / classical RK4 sweep with m
substeps per control interval instead: the states are integrated as accurately as needed
while nt, and with it the DP, follows how finely the control should switch.  ``integrator="beuler" | "midpoint"`` are
backward Euler and the implicit midpoint rule for stiff dynamics: Newton's method per substep on the device, the
gradient by the implicit function theorem; a restart whose Newton iteration fails returns NaN for J and its df row.
``ODEProgram(..., derive="all" | ("Fy", "Gy", ...))`` takes F and G as templates over the scalar type and has the
library generate the named derivative hooks by forward-mode AD (include/mioc.h, "Derived
hooks"); ``check_hooks`` uses that to tell which hand-written derivative hook is wrong.
``ODEProgram(..., ndata=n, terminal=True, states=True)`` (include/mioc.h, "Terminal
cost, sampled data, state output") adds n columns of sampled data behind the parameters (``p[NP + e]``, the row of the
hook's control column), a terminal cost ``E`` with ``Ey`` (derivable: ``derive`` takes "Ey"), and the states at the
control-grid points as an output (``DeviceODEProblem.states``).
``ODEProgram(..., scenarios=True | "data")`` (include/mioc.h, "Scenarios") lets the
restarts of one call solve different problems: ``DeviceODEProblem`` / ``MixedODEProblem`` then take S initial states
and parameter vectors (with "data" also S data tables), and restart k of ``TRM_batch`` / ``TRM_mixed_batch`` solves
scenario k % S; ``best_per_scenario`` picks each scenario's best restart.
``ODEProgram(..., sensitivities=True | "p" | "y0")`` (include/mioc.h, "Sensitivities")
makes dJ/dparams and dJ/dstate0 outputs of an evaluation for every integrator but "euler": the text then also defines
``Fp``, ``Gp`` (and ``Ep``), or ``derive`` names them; ``DeviceODEProblem.sensitivities`` returns them.
Whatever is asked for, Python always calls the library's ``_sens`` entries (create, source, eval): every older entry
of the C ABI forwards to them with the arguments it lacks zero, so the compiler sees the same text.

``EXAMPLE_SOURCES`` restates the three built-in problems as hook text, term for term as ``Hooks<...>`` of
csrc/mioc_ode.hip has them, so each reproduces mioc_ode_eval_device bit for bit; they double as templates.  Parameter
order as in mioc_ode_eval_device without the trailing y0, which is ``state0`` here (``EXAMPLE_PARAMS``,
``EXAMPLE_STATE0``: the examples' constants).
"""
from __future__ import annotations

import atexit
import ctypes
import sys
import weakref

from .native import (MIOC_ECOMPILE, MIOC_ODE_DERIVE_EP, MIOC_ODE_DERIVE_EY, MIOC_ODE_DERIVE_FP, MIOC_ODE_DERIVE_FU,
                     MIOC_ODE_DERIVE_FY, MIOC_ODE_DERIVE_GP, MIOC_ODE_DERIVE_GU, MIOC_ODE_DERIVE_GY, MIOC_ODE_SENS_P,
                     MIOC_ODE_SENS_Y0, MIOC_ODE_INT_BEULER, MIOC_ODE_INT_EULER, MIOC_ODE_INT_HEUN, MIOC_ODE_INT_MIDPOINT,
                     MIOC_ODE_INT_RK4, MIOC_ODE_SCEN, MIOC_ODE_SCEN_DATA, MIOC_ODE_STATES, MIOC_ODE_TERMINAL, MIOC_OK,
                     MiocNativeError, load_library)


class MiocCompileError(MiocNativeError):
    """The hook source did not compile; ``log`` is the compiler's output (the hooks' own line numbers: hooks:N)."""

    def __init__(self, code, log):
        super().__init__(code, "the ODE hooks did not compile:\n" + log)
        self.log = log


_LIVE = weakref.WeakSet()  # programs not yet closed


@atexit.register
def _close_live_programs():
    """Destroy the programs still open while the HIP runtime is alive (see native._close_live_contexts; this handler
    is registered later, so it runs first: a program is unloaded before the contexts that ran it are destroyed)."""
    for p in list(_LIVE):
        try:
            p.close()
        except Exception:
            pass


INTEGRATORS = {"euler": MIOC_ODE_INT_EULER, "heun": MIOC_ODE_INT_HEUN, "rk4": MIOC_ODE_INT_RK4,
               "beuler": MIOC_ODE_INT_BEULER, "midpoint": MIOC_ODE_INT_MIDPOINT}
MAX_SUBSTEPS = 64
MAX_NDATA = 16
# every derivable hook and its bit: E* only with a terminal cost, *p only with sensitivities in the parameters
DERIVE_BITS_EVERY = {"Fy": MIOC_ODE_DERIVE_FY, "Fu": MIOC_ODE_DERIVE_FU, "Gy": MIOC_ODE_DERIVE_GY,
                     "Gu": MIOC_ODE_DERIVE_GU, "Ey": MIOC_ODE_DERIVE_EY, "Fp": MIOC_ODE_DERIVE_FP,
                     "Gp": MIOC_ODE_DERIVE_GP, "Ep": MIOC_ODE_DERIVE_EP}


def sensitivity_bits(sensitivities):
    """``sensitivities`` (False, True, "p" or "y0") as the sens argument of the library's create entry."""
    if sensitivities is False or sensitivities is None:
        return 0
    if sensitivities is True:
        return MIOC_ODE_SENS_P | MIOC_ODE_SENS_Y0
    if isinstance(sensitivities, str) and sensitivities in ("p", "y0"):
        return MIOC_ODE_SENS_P if sensitivities == "p" else MIOC_ODE_SENS_Y0
    raise ValueError(f'sensitivities must be False, True, "p" or "y0", not {sensitivities!r}')


def derive_names(derive, terminal=False, sens_p=False):
    """``derive`` ("all", "all+p" or an iterable of hook names) as a tuple of names in the order Fy, Fu, Gy, Gu(, Ey:
    only a program with a terminal cost has it, and "all" includes it there)(, Fp, Gp: only a program with
    sensitivities in the parameters has them, ``sens_p``; then Ep with a terminal cost).  "all" stays the y and u hooks
    whether or not sensitivities are on; "all+p" adds Fp, Gp (and Ep) and needs ``sens_p``."""
    bits = [n for n in DERIVE_BITS_EVERY if (terminal or n[0] != "E") and (sens_p or n[1] != "p")]
    plain = tuple(n for n in bits if n[1] != "p")
    if isinstance(derive, str):
        if derive == "all+p" and not sens_p:
            raise ValueError('derive "all+p" needs sensitivities in the parameters (sensitivities=True or "p")')
        if derive not in ("all", "all+p"):
            raise ValueError(f'derive must be "all", "all+p" or an iterable of {list(bits)}, not {derive!r}')
        return plain if derive == "all" else tuple(bits)
    names = set(derive)
    if names & {"Ey", "Ep"} and not terminal:
        raise ValueError('derive "Ey" / "Ep" needs terminal=True')
    if names & {"Fp", "Gp", "Ep"} and not sens_p:
        raise ValueError('derive "Fp" / "Gp" / "Ep" needs sensitivities in the parameters (sensitivities=True or "p")')
    unknown = sorted(str(n) for n in names if n not in bits)
    if unknown:
        raise ValueError(f"derive names must be among {list(bits)}, not {unknown}")
    return tuple(n for n in bits if n in names)


def scenario_bits(scenarios, ndata=0):
    """``scenarios`` (False, True or "data") as the scen argument of the library's create entry."""
    if scenarios is False or scenarios is None:
        return 0
    if scenarios is True:
        return MIOC_ODE_SCEN
    if isinstance(scenarios, str) and scenarios == "data":
        if not ndata:
            raise ValueError('scenarios="data" needs ndata > 0')
        return MIOC_ODE_SCEN | MIOC_ODE_SCEN_DATA
    raise ValueError(f'scenarios must be False, True or "data", not {scenarios!r}')


def _program_args(source, ny, nx, nparams, integrator, substeps, derive, ndata, terminal, states, scen, sens):
    """(the derive names, the arguments that the library's _create_sens and _source_sens entries share): ``derive`` as
    derive_names takes it, ``scen`` and ``sens`` as scenario_bits and sensitivity_bits return them."""
    names = derive_names(derive, terminal, bool(sens & MIOC_ODE_SENS_P))
    mask = sum(DERIVE_BITS_EVERY[n] for n in names)
    flags = (MIOC_ODE_TERMINAL if terminal else 0) | (MIOC_ODE_STATES if states else 0)
    text = source.encode() if isinstance(source, str) else source
    return names, (text, int(ny), int(nx), int(nparams), int(ndata), INTEGRATORS[integrator], int(substeps), mask,
                   flags, scen, sens)


def _source_text(args, noinline):
    """The text the library assembles for _program_args' ``args``: the entry is asked for the size, then the text."""
    entry, args = load_library().mioc_ode_program_source_sens, args + (int(bool(noinline)),)
    need = entry(*args, None, 0)
    if need < 0:
        raise MiocNativeError(need, "the library's program source entry: bad arguments")
    buf = ctypes.create_string_buffer(need + 1)
    entry(*args, buf, need + 1)
    return buf.value.decode()


def program_source(source, ny, nx, nparams, integrator="euler", substeps=1, derive=(), ndata=0, terminal=False,
                   states=False, noinline=False, scenarios=False, sensitivities=False):
    """The text the library hands to the compiler for ``ODEProgram(source, ny, ...)``, as a str; nothing is compiled
    (the library's _source_sens entry, which every older source entry forwards to).  noinline: the text of the second
    compile of derived hooks (include/mioc.h)."""
    return _source_text(_program_args(source, ny, nx, nparams, integrator, substeps, derive, ndata, terminal, states,
                                      scenario_bits(scenarios, ndata), sensitivity_bits(sensitivities))[1], noinline)


class ODEProgram:
    """Six hooks (HIP source text) compiled for gfx950: ny states, nx controls, nparams parameters.  Needs no GPU to
    compile; one program serves any number of contexts.  ``close()`` destroys it (also ``with ODEProgram(...) as p``).

    ``integrator``: "euler" (the reference's explicit Euler / trapezoid scheme, the default), "heun", "rk4", or the
    implicit "beuler" (backward Euler) and "midpoint" (implicit midpoint rule) for stiff dynamics; all but "euler"
    with ``substeps`` steps inside every control interval and the exact gradient of their discrete J (include/mioc.h,
    "Integrators" and "Implicit integrators"); the program carries both, every evaluation uses them.

    ``derive``: "all" or an iterable of "Fy", "Fu", "Gy", "Gu" -- the hooks the library generates by forward-mode AD
    from F and G, which the text then defines as templates over the scalar type (include/mioc.h, "Derived hooks");
    the text defines the others.  ``ODEProgram.derive`` is the tuple of names; empty: all six hooks are the text's.

    ``ndata``: columns of sampled data (0..16); a hook then finds the data row of its control column in
    ``p[NP] .. p[NP + ndata - 1]`` and every evaluation takes ``data``, an (nt, ndata) tensor.  ``terminal``: the text
    also defines the terminal cost ``E(p, t, y)`` and ``Ey`` (or ``derive`` names "Ey"; "all" then includes it).
    ``states``: evaluations can return the states at the control-grid points (``Y``).  All three: include/mioc.h,
    "Terminal cost, sampled data, state output"; none asked for: the program is what it was without them.

    ``scenarios``: True compiles the program for S scenarios per call, each with its own state0 and parameters; "data"
    (needs ndata > 0) also with its own data table.  Restart k then solves scenario k % S (include/mioc.h,
    "Scenarios"); such a program is evaluated through a DeviceODEProblem / MixedODEProblem or
    Context.ode_program_eval_scen_tensors.  ``ODEProgram.scenarios`` is the C entry's scen argument (0, 1 or 3).

    ``sensitivities``: True compiles the program so that an evaluation can return dJ/dparams and dJ/dstate0 ("p" /
    "y0": one of them; include/mioc.h, "Sensitivities"); not with "euler".  With the parameter part the text also
    defines ``Fp``, ``Gp`` and, with ``terminal``, ``Ep``, or ``derive`` names them: F, G, E are then templates over
    the state type and the parameter type.  ``derive="all"`` stays the y and u hooks; ``"all+p"`` adds Fp, Gp (and
    Ep).  ``ODEProgram.sens`` is the C entry's sens argument (0..3)."""

    LOG_CAP = 1 << 16

    def __init__(self, source, ny, nx, nparams, integrator="euler", substeps=1, derive=(), ndata=0, terminal=False,
                 states=False, scenarios=False, sensitivities=False):
        self.h = None
        self.terminal, self.states = bool(terminal), bool(states)
        if int(ndata) != ndata or not 0 <= ndata <= MAX_NDATA:
            raise ValueError(f"ndata must be an integer in 0..{MAX_NDATA}, not {ndata!r}")
        self.ndata = int(ndata)
        self.scenarios = scenario_bits(scenarios, self.ndata)
        self.sens = sensitivity_bits(sensitivities)
        if integrator not in INTEGRATORS:
            raise ValueError(f"integrator must be one of {sorted(INTEGRATORS)}, not {integrator!r}")
        if int(substeps) != substeps or not 1 <= substeps <= MAX_SUBSTEPS:
            raise ValueError(f"substeps must be an integer in 1..{MAX_SUBSTEPS}, not {substeps!r}")
        if integrator == "euler" and substeps != 1:
            raise ValueError("the reference's Euler scheme defines no substeps: use heun, rk4, beuler or midpoint")
        if integrator == "euler" and self.sens:
            raise ValueError("the reference's Euler scheme has no sensitivities: its df is not the derivative of its J; "
                             "use heun, rk4, beuler or midpoint")
        self.integrator, self.substeps = integrator, int(substeps)
        self.lib = load_library()
        self.ny, self.nx, self.nparams = int(ny), int(nx), int(nparams)
        self.derive, self._args = _program_args(source, ny, nx, nparams, integrator, substeps, derive, self.ndata,
                                                self.terminal, self.states, self.scenarios, self.sens)
        h = ctypes.c_void_p()
        log = ctypes.create_string_buffer(self.LOG_CAP)
        rc = self.lib.mioc_ode_program_create_sens(*self._args, ctypes.byref(h), log, self.LOG_CAP)
        self.log = log.value.decode(errors="replace")
        if rc == MIOC_ECOMPILE:
            raise MiocCompileError(rc, self.log)
        if rc != MIOC_OK:
            raise MiocNativeError(rc, self.log or "the library's program create entry: bad ny / nx / nparams / source "
                                                  "(1 <= ny, nx <= 8, 0 <= nparams <= 32, 0 <= ndata <= 16, at most 1 MiB "
                                                  "of text)")
        self.h = h
        _LIVE.add(self)

    def source_text(self, noinline=False):
        """The text this program was compiled from; noinline: that of the second compile."""
        return _source_text(self._args, noinline)

    def close(self):
        if self.h:
            h, self.h = self.h, None
            _LIVE.discard(self)
            self.lib.mioc_ode_program_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self, _finalizing=sys.is_finalizing):
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class _ODEProblem:
    """What DeviceODEProblem (nu = 0) and MixedODEProblem (nu >= 1 continuous controls in front) share: the program,
    the levels V of the integer controls and their iterator, [T0, T1], nt, the inputs state0 / params / data, and
    everything that evaluates them.  It has the members mioc.trm_batch.TRM_batch asks of a problem."""

    def __init__(self, program, nu, V, iterator, T0, T1, nt, state0, params, data):
        import numpy as np
        self.program, self.nu = program, int(nu)
        self.V = [list(v) for v in V]
        self.iterator = iterator
        self.T0, self.T1, self.nt = float(T0), float(T1), int(nt)
        self._device_data = {}  # per device used: {"state0", "params", "data"} as tensors; None: passed from the host
        if not self.T1 > self.T0 or self.nt < 1:
            raise ValueError("need T1 > T0 and nt >= 1")
        scen, nd = getattr(program, "scenarios", 0), getattr(program, "ndata", 0)
        if (data is None) != (nd == 0):
            raise ValueError(f"the program reads {nd} columns of sampled data: give data of shape (nt, {nd})" if nd else
                             "the program reads no sampled data")
        sizes = {}

        def take(name, a, shape, may_lead):
            a = np.array(a, dtype=np.float64, order="C", copy=True)
            if a.shape == shape:
                return a
            if may_lead and a.ndim == len(shape) + 1 and a.shape[1:] == shape and a.shape[0] >= 1:
                sizes[name] = a.shape[0]
                return a
            lead = f" or (S,) + {shape}" if may_lead else ""
            raise ValueError(f"{name} must have the shape {shape}{lead}, not {a.shape}" +
                             ("" if scen else ": inputs per scenario need a program compiled with scenarios"))
        y0 = take("state0", state0, (program.ny,), bool(scen))
        par = take("params", np.zeros(0) if program.nparams == 0 and np.size(params) == 0 and np.ndim(params) < 2
                   else params, (program.nparams,), bool(scen))
        dat = None if data is None else take("data", data, (self.nt, nd), bool(scen & MIOC_ODE_SCEN_DATA))
        if len(set(sizes.values())) > 1:
            raise ValueError(f"the numbers of scenarios disagree: {sizes}")
        self._scen, self._S = bool(scen), next(iter(sizes.values()), 1)
        if scen:  # (S, ny), (S, nparams) and, per scenario, (S, nt, ndata): an input without the leading size is shared
            y0, par = (np.array(np.broadcast_to(a, (self._S,) + a.shape[-1:]), order="C", copy=True) for a in (y0, par))
            if dat is not None and scen & MIOC_ODE_SCEN_DATA:
                dat = np.array(np.broadcast_to(dat, (self._S, self.nt, nd)), order="C", copy=True)
        self.state0, self.params, self.data = (y0, par, dat) if scen else (y0.tolist(), par.tolist(), dat)

    def _eval(self, ctx, x, J=None, df=None, Y=None, Jp=None, Jy0=None):
        """One evaluation at the controls x (K, nt, nx) on ctx, into the outputs given.  The problem's arrays are
        uploaded to the device of x at the first use there and kept; with scenarios restart k solves scenario k % S."""
        self.check_restarts(x.shape[0])
        if self.data is not None and x.shape[1] != self.nt:
            raise ValueError(f"the problem's data fix nt = {self.nt}; x has {x.shape[1]} steps")
        key = str(x.device)
        if key not in self._device_data:
            import torch
            lay = self.device_layouts() if self._scen else {"state0": None, "params": None, "data": self.data}
            self._device_data[key] = {n: None if a is None else torch.tensor(a, dtype=torch.float64, device=x.device)
                                      for n, a in lay.items()}
            torch.cuda.current_stream(x.device).synchronize()  # the upload before the context's stream reads it
        d = self._device_data[key]
        host = (x, self.T0, self.T1, self.state0, self.params, J, df, d["data"], Y, Jp, Jy0)
        if self._scen:
            ctx.ode_program_eval_scen_tensors(self.program, self.nu, x, self.T0, self.T1, self._S, d["state0"],
                                              d["params"], d["data"], J, df, Y, Jp, Jy0)
        elif self.nu:
            ctx.ode_program_eval_mixed_tensors(self.program, self.nu, *host)
        else:
            ctx.ode_program_eval_tensors(self.program, *host)

    def eval_tensors(self, ctx, x, J=None, df=None):
        """J (K,) and df (K, nt, nx) at the controls x, each optional; enqueued on ctx."""
        self._eval(ctx, x, J, df)

    def states(self, ctx, x):
        """The states (K, nt + 1, ny) of the controls x (K, nt, nx) at the control-grid points t_i = T0 + i tau; row 0
        is state0 (with scenarios: that of scenario k % S).  The program must have been compiled with states=True.
        Synchronises the context."""
        import torch
        Y = torch.empty(x.shape[0], x.shape[1] + 1, self.program.ny, dtype=torch.float64, device=x.device)
        torch.cuda.current_stream(x.device).synchronize()
        self._eval(ctx, x, Y=Y)
        ctx.synchronize()
        return Y

    def sensitivities(self, ctx, x):
        """(Jp (K, nparams), Jy0 (K, ny)): dJ/dparams and dJ/dstate0 at the controls x (K, nt, nx), as CUDA tensors;
        a part the program was not compiled for comes back as None (with scenarios: restart k's derivatives in
        scenario k % S's own values).  ValueError for a program without sensitivities.  Synchronises the context."""
        import torch
        prog = self.program
        sens = int(getattr(prog, "sens", 0))
        if not sens:
            raise ValueError("the program was not compiled with sensitivities")
        K = x.shape[0]
        Jp = torch.empty(K, prog.nparams, dtype=torch.float64, device=x.device) if sens & MIOC_ODE_SENS_P else None
        Jy0 = torch.empty(K, prog.ny, dtype=torch.float64, device=x.device) if sens & MIOC_ODE_SENS_Y0 else None
        torch.cuda.current_stream(x.device).synchronize()
        self._eval(ctx, x, Jp=Jp, Jy0=Jy0)
        ctx.synchronize()
        return Jp, Jy0

    @property
    def S(self):
        """The number of scenarios (1 for a program without them)."""
        return self._S

    def device_layouts(self):
        """The numpy arrays a scenario problem uploads, the scenario index fastest (include/mioc.h, "Scenarios"):
        {"state0": (ny, S), "params": (nparams, S), "data": (nt, ndata), (nt, ndata, S) per scenario, or None}."""
        import numpy as np
        if not self._scen:
            raise ValueError("the program was not compiled with scenarios")
        data = self.data
        if data is not None and data.ndim == 3:
            data = np.ascontiguousarray(data.transpose(1, 2, 0))
        return {"state0": np.ascontiguousarray(self.state0.T), "params": np.ascontiguousarray(self.params.T),
                "data": data}

    def check_restarts(self, K):
        """ValueError unless K restarts divide evenly among the problem's scenarios."""
        if self._scen and (K is None or int(K) < 1 or int(K) % self._S):
            raise ValueError(f"K = {K} restarts do not divide among the problem's S = {self._S} scenarios: K % S != 0")

    # the rest of what TRM_batch asks of a problem
    def level_table(self):
        from .iterators import LevelTable
        return LevelTable(self.V, self.iterator)

    @property
    def fixes_nt(self):
        """False, or why a caller cannot choose nt."""
        return "the problem's sampled data fix nt" if self.data is not None else False

    def setup(self, ctx):
        """Nothing: the arrays are uploaded at the first evaluation."""


class DeviceODEProblem(_ODEProblem):
    """An ODE-constrained problem for TRM_batch: a compiled ``ODEProgram`` with the data the Julia objective holds --
    the levels V and their iterator (None: the product grid), [T0, T1], the default number of steps nt, state0 and
    the parameters; ``data``: the (nt, ndata) samples of a program with ndata > 0, which fix nt (uploaded once per
    device and kept).

    For a program compiled with ``scenarios``, state0 is (ny,) or (S, ny), params (nparams,) or (S, nparams) and, with
    scenarios="data", data (nt, ndata) or (S, nt, ndata): ``S`` is the common leading size (1 if there is none), an
    input without it is shared by all scenarios, and restart k of a call solves scenario k % S.  The problem then keeps
    state0 (S, ny), params (S, nparams) and data as numpy arrays; ``device_layouts()`` are the arrays uploaded."""

    def __init__(self, program, V, iterator, T0, T1, nt, state0, params=(), data=None):
        super().__init__(program, 0, V, iterator, T0, T1, nt, state0, params, data)
        if len(self.V) != program.nx:
            raise ValueError("V must have one entry per control: the program's nx")


class MixedODEProblem(_ODEProblem):
    """An ODE-constrained problem with mixed controls for mioc.trm_mixed.TRM_mixed_batch: a compiled ``ODEProgram``
    whose first ``nu`` controls are continuous with the pointwise bounds ``lo`` <= ``hi`` (scalars, (nu,) or (nt, nu);
    kept as (nt, nu) numpy arrays, the device layout) and whose other nx - nu controls take the levels V with their
    iterator (None: the product grid); then [T0, T1], the number of steps nt, state0, the parameters and ``data``, the
    (nt, ndata) samples of a program with ndata > 0 (uploaded once per device and kept)."""

    def __init__(self, program, nu, lo, hi, V, iterator, T0, T1, nt, state0, params=(), data=None):
        import numpy as np
        if int(nu) != nu or not 1 <= nu < program.nx:
            raise ValueError(f"nu must be an integer in 1..{program.nx - 1} (nu = 0: DeviceODEProblem), not {nu!r}")
        super().__init__(program, nu, V, iterator, T0, T1, nt, state0, params, data)
        if len(self.V) != program.nx - self.nu:
            raise ValueError("V must have one entry per integer control: the program's nx - nu")

        def bound(b, name):
            b = np.asarray(b, dtype=np.float64)
            if b.ndim > 2 or (b.ndim == 1 and b.shape != (self.nu,)) or (b.ndim == 2 and b.shape != (self.nt, self.nu)):
                raise ValueError(f"{name} must be a scalar or have the shape (nu,) or (nt, nu)")
            return np.array(np.broadcast_to(b, (self.nt, self.nu)), order="C", copy=True)
        self.lo, self.hi = bound(lo, "lo"), bound(hi, "hi")
        if not np.all(self.lo <= self.hi):  # also refuses a NaN bound
            raise ValueError("need lo <= hi everywhere")


def best_per_scenario(values, S):
    """The index of the best restart of each scenario: values (K,) of K = S*m restarts, restart k having solved
    scenario k % S, gives an (S,) int array whose entry s is the k with the smallest value among k % S == s (the first
    such k at a tie; a NaN never wins against a number)."""
    import numpy as np
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    S = int(S)
    if S < 1 or v.size == 0 or v.size % S:
        raise ValueError(f"{v.size} values do not divide among {S} scenarios")
    v = np.where(np.isnan(v), np.inf, v).reshape(-1, S)
    return np.argmin(v, axis=0) * S + np.arange(S)


_SIG = "(const double *p, int i, double t, const double *y, const double *x"

EXAMPLE_SOURCES = {
    # Lotka-Volterra fishing (example_fishing.jl:14-92): p = alpha, beta, gamma, delta, c1, c2, v1[3], v2[3]
    "fishing": """
__device__ double fish_s1(const double *p, const double *x) { return ((0.0 + x[0] * p[6]) + x[1] * p[7]) + x[2] * p[8]; }
__device__ double fish_s2(const double *p, const double *x) { return ((0.0 + x[0] * p[9]) + x[1] * p[10]) + x[2] * p[11]; }
__device__ void F@SIG@, double *f) {
  f[0] = y[0] * ((p[0] - p[1] * y[1]) - p[4] * fish_s1(p, x));
  f[1] = y[1] * ((-p[2] + p[3] * y[0]) - p[5] * fish_s2(p, x));
}
__device__ void Fy@SIG@, double (*fy)[NY]) {
  fy[0][0] = (p[0] - p[1] * y[1]) - p[4] * fish_s1(p, x);
  fy[0][1] = y[0] * -p[1];
  fy[1][0] = y[1] * p[3];
  fy[1][1] = (-p[2] + p[3] * y[0]) - p[5] * fish_s2(p, x);
}
__device__ void Fu@SIG@, double (*fu)[NX]) {
  for (int m = 0; m < 3; ++m) {
    fu[0][m] = (y[0] * -p[4]) * p[6 + m];
    fu[1][m] = (y[1] * -p[5]) * p[9 + m];
  }
}
__device__ double G@SIG@) {
  const double a = y[0] - 1.0, b = y[1] - 1.0;
  return 0.5 * (a * a) + 0.5 * (b * b);
}
__device__ void Gy@SIG@, double *gy) {
  gy[0] = y[0] - 1.0;
  gy[1] = y[1] - 1.0;
}
__device__ void Gu@SIG@, double *gu) {}
""",
    # double tank multimode (example_doubletank.jl:14-82): p = k1, k2, c[3]
    "doubletank": """
__device__ double tank_cx(const double *p, const double *x) { return ((0.0 + p[2] * x[0]) + p[3] * x[1]) + p[4] * x[2]; }
__device__ void F@SIG@, double *f) {
  f[0] = tank_cx(p, x) - sqrt(y[0]);
  f[1] = sqrt(y[0]) - sqrt(y[1]);
}
__device__ void Fy@SIG@, double (*fy)[NY]) {
  fy[0][0] = -1.0 / (2.0 * sqrt(y[0]));
  fy[0][1] = 0.0;
  fy[1][0] = 1.0 / (2.0 * sqrt(y[0]));
  fy[1][1] = -1.0 / (2.0 * sqrt(y[1]));
}
__device__ void Fu@SIG@, double (*fu)[NX]) {
  for (int m = 0; m < 3; ++m) {
    fu[0][m] = p[2 + m];
    fu[1][m] = 0.0;
  }
}
__device__ double G@SIG@) {
  const double d = y[1] - p[1];
  return p[0] * (d * d);
}
__device__ void Gy@SIG@, double *gy) {
  gy[0] = 0.0;
  gy[1] = (2.0 * p[0]) * (y[1] - p[1]);
}
__device__ void Gu@SIG@, double *gu) {}
""",
    # Van der Pol oscillator, binary variant (example_vanderpol.jl:14-81): p = c[3]
    "vanderpol": """
__device__ double vdp_cx(const double *p, const double *x) { return ((0.0 + p[0] * x[0]) + p[1] * x[1]) + p[2] * x[2]; }
__device__ void F@SIG@, double *f) {
  f[0] = y[1];
  f[1] = ((1.0 - y[0] * y[0]) * y[1]) * vdp_cx(p, x) - y[0];
}
__device__ void Fy@SIG@, double (*fy)[NY]) {
  const double s = vdp_cx(p, x);
  fy[0][0] = 0.0;
  fy[0][1] = 1.0;
  fy[1][0] = ((-2.0 * y[0]) * y[1]) * s - 1.0;
  fy[1][1] = (1.0 - y[0] * y[0]) * s;
}
__device__ void Fu@SIG@, double (*fu)[NX]) {
  for (int m = 0; m < 3; ++m) {
    fu[0][m] = 0.0;
    fu[1][m] = (p[m] * (1.0 - y[0] * y[0])) * y[1];
  }
}
__device__ double G@SIG@) { return y[0] * y[0] + y[1] * y[1]; }
__device__ void Gy@SIG@, double *gy) {
  gy[0] = 2.0 * y[0];
  gy[1] = 2.0 * y[1];
}
__device__ void Gu@SIG@, double *gu) {}
""",
}
EXAMPLE_SOURCES = {k: v.replace("@SIG@", _SIG) for k, v in EXAMPLE_SOURCES.items()}

# The same three problems for derive="all": F and G as templates over the scalar type, their helpers, and nothing
# else.  F and G keep the parenthesisation above, so with T = double they are the same expressions (the same J bits).
_TSIG = "(const double *p, int i, double t, const T *y, const T *x"

EXAMPLE_SOURCES_AD = {
    "fishing": """
template <class T> __device__ T fish_s1(const double *p, const T *x) { return ((0.0 + x[0] * p[6]) + x[1] * p[7]) + x[2] * p[8]; }
template <class T> __device__ T fish_s2(const double *p, const T *x) { return ((0.0 + x[0] * p[9]) + x[1] * p[10]) + x[2] * p[11]; }
template <class T> __device__ void F@SIG@, T *f) {
  f[0] = y[0] * ((p[0] - p[1] * y[1]) - p[4] * fish_s1(p, x));
  f[1] = y[1] * ((-p[2] + p[3] * y[0]) - p[5] * fish_s2(p, x));
}
template <class T> __device__ T G@SIG@) {
  const T a = y[0] - 1.0, b = y[1] - 1.0;
  return 0.5 * (a * a) + 0.5 * (b * b);
}
""",
    "doubletank": """
template <class T> __device__ T tank_cx(const double *p, const T *x) { return ((0.0 + p[2] * x[0]) + p[3] * x[1]) + p[4] * x[2]; }
template <class T> __device__ void F@SIG@, T *f) {
  f[0] = tank_cx(p, x) - sqrt(y[0]);
  f[1] = sqrt(y[0]) - sqrt(y[1]);
}
template <class T> __device__ T G@SIG@) {
  const T d = y[1] - p[1];
  return p[0] * (d * d);
}
""",
    "vanderpol": """
template <class T> __device__ T vdp_cx(const double *p, const T *x) { return ((0.0 + p[0] * x[0]) + p[1] * x[1]) + p[2] * x[2]; }
template <class T> __device__ void F@SIG@, T *f) {
  f[0] = y[1];
  f[1] = ((1.0 - y[0] * y[0]) * y[1]) * vdp_cx(p, x) - y[0];
}
template <class T> __device__ T G@SIG@) { return y[0] * y[0] + y[1] * y[1]; }
""",
}
EXAMPLE_SOURCES_AD = {k: v.replace("@SIG@", _TSIG) for k, v in EXAMPLE_SOURCES_AD.items()}

# Fishing for derive="all+p" (sensitivities in the parameters): F and G as templates over the state type T and the
# parameter type P, so that Fp and Gp are generated too.  The same parenthesisation: with T = P = double the same bits.
_TPSIG = "(const P *p, int i, double t, const T *y, const T *x"
EXAMPLE_SOURCES_AD_P = {
    "fishing": """
template <class T, class P> __device__ T fish_s1(const P *p, const T *x) { return ((0.0 + x[0] * p[6]) + x[1] * p[7]) + x[2] * p[8]; }
template <class T, class P> __device__ T fish_s2(const P *p, const T *x) { return ((0.0 + x[0] * p[9]) + x[1] * p[10]) + x[2] * p[11]; }
template <class T, class P> __device__ void F@SIG@, T *f) {
  f[0] = y[0] * ((p[0] - p[1] * y[1]) - p[4] * fish_s1<T, P>(p, x));
  f[1] = y[1] * ((-p[2] + p[3] * y[0]) - p[5] * fish_s2<T, P>(p, x));
}
template <class T, class P> __device__ T G@SIG@) {
  const T a = y[0] - 1.0, b = y[1] - 1.0;
  return 0.5 * (a * a) + 0.5 * (b * b);
}
""".replace("@SIG@", _TPSIG),
}

# the examples' constants (example_fishing.jl, example_doubletank.jl, example_vanderpol.jl) and shapes
EXAMPLE_PARAMS = {"fishing": [1, 1, 1, 1, 1, 1, 0.2, 0.4, 0.01, 0.1, 0.2, 0.1], "doubletank": [2, 3, 1, 0.5, 2],
                  "vanderpol": [-1, 0.75, -2]}
EXAMPLE_STATE0 = {"fishing": [0.5, 0.7], "doubletank": [2, 2], "vanderpol": [1, 0]}
EXAMPLE_SHAPES = {k: (2, 3, len(v)) for k, v in EXAMPLE_PARAMS.items()}  # (ny, nx, nparams)


def example_program(name, integrator="euler", substeps=1, ad=False):
    """ODEProgram of a built-in example's hook text; ``ad``: of its F and G alone (EXAMPLE_SOURCES_AD), the four
    derivative hooks generated (derive="all")."""
    if ad:
        return ODEProgram(EXAMPLE_SOURCES_AD[name], *EXAMPLE_SHAPES[name], integrator=integrator, substeps=substeps,
                          derive="all")
    return ODEProgram(EXAMPLE_SOURCES[name], *EXAMPLE_SHAPES[name], integrator=integrator, substeps=substeps)


def check_hooks(ctx, source, ny, nx, nparams, x, T0, T1, state0, params, integrator="euler", substeps=1, ndata=0,
                terminal=False, data=None, sensitivities=False):
    """Which hand-written derivative hook is wrong?  The program-level counterpart of the reference's test_Fy! /
    test_Fu! (ODEObjective.jl:186-241), without finite differences.

    ``source`` defines F and G as templates over the scalar type and each of Fy, Fu, Gy, Gu by hand under its guard
    (``#ifndef MIOC_DERIVE_FY`` ... ``#endif``, include/mioc.h "Derived hooks").  It is compiled six times: all hooks
    by hand (derive = 0), all four derived, and each one derived with the other three by hand; J and df are evaluated
    at the controls ``x``, a (K, nt, nx) float64 CUDA tensor, on ``ctx``.  Returns a dict:
      "J_equal"   J is bit-equal across the six programs (F and G are the same in all);
      "Fy", "Fu", "Gy", "Gu"   max|df(that hook derived) - df(all by hand)| / max|df(all derived)|: replacing a correct
                  hand-written hook by the derived one changes df by rounding only, a wrong one by its error;
      "all"       the same for all four derived against all by hand.
    A wrong hook shows in its own entry and in "all" alone.  The programs are closed before returning.
    ``terminal``: the text also defines E as a template and Ey by hand under ``#ifndef MIOC_DERIVE_EY``; there is one
    more program and the key "Ey".  ``ndata``, ``data``: the (nt, ndata) float64 CUDA tensor of a text with data.
    ``sensitivities`` (True or "p"; not with "euler"): the text defines F, G (and E) as templates over the state type
    and the parameter type and Fp, Gp (and Ep) by hand under ``#ifndef MIOC_DERIVE_FP`` etc.; every program is
    compiled with the sensitivities and there is one more program per p hook and the program "all+p" (everything
    derived).  The keys "Fp", "Gp", "Ep" and "all+p" compare Jp = dJ/dparams in place of df:
    max|Jp(derived) - Jp(all by hand)| / max|Jp(all+p)|; a wrong y or u hook also shows in "all+p"."""
    import torch
    sens_p = bool(sensitivity_bits(sensitivities) & MIOC_ODE_SENS_P)
    if sensitivities and not sens_p:
        raise ValueError('check_hooks compares the parameter hooks: sensitivities must be True or "p"')
    names = derive_names("all+p" if sens_p else "all", terminal, sens_p)
    masks = [("hand", ()), ("all", "all")] + ([("all+p", "all+p")] if sens_p else []) + [(n, (n,)) for n in names]
    res = {}
    for key, derive in masks:
        with ODEProgram(source, ny, nx, nparams, integrator=integrator, substeps=substeps, derive=derive, ndata=ndata,
                        terminal=terminal, sensitivities=sensitivities) as prog:
            J = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
            df = torch.empty_like(x)
            Jp = torch.empty(x.shape[0], nparams, dtype=torch.float64, device=x.device) if sens_p else None
            torch.cuda.current_stream(x.device).synchronize()
            ctx.ode_program_eval_tensors(prog, x, T0, T1, state0, params, J, df, data=data, Jp=Jp)
            ctx.synchronize()
            res[key] = (J, df, Jp)
    J0, df0, Jp0 = res["hand"]
    scale = float(res["all"][1].abs().max())
    out = {"J_equal": all(bool(torch.equal(r[0], J0)) for r in res.values())}
    for key, _ in masks[1:]:
        if key in ("Fp", "Gp", "Ep", "all+p"):
            out[key] = float((res[key][2] - Jp0).abs().max()) / float(res["all+p"][2].abs().max())
        else:
            out[key] = float((res[key][1] - df0).abs().max()) / scale
    return out


def example_problem(name, program=None, nt=None, integrator="euler", substeps=1, ad=False):
    """DeviceODEProblem of a built-in example (SOS1 over three binary controls, the example's horizon; nt: the
    example's unless given -- with heun / rk4 / beuler / midpoint and substeps the control grid can be much coarser
    than the example's).
    Without ``program``, one is compiled with ``integrator`` and ``substeps``, with ``ad`` from F and G alone."""
    from .iterators import bounded_sum_iterator
    from .trm_batch import PROBLEMS
    _, nt_def, T0, T1 = PROBLEMS[name]
    V = [[0, 1], [0, 1], [0, 1]]
    return DeviceODEProblem(program or example_program(name, integrator, substeps, ad), V, bounded_sum_iterator(V, 1, 1),
                            T0, T1, nt_def if nt is None else nt, EXAMPLE_STATE0[name], EXAMPLE_PARAMS[name])
