"""ctypes binding of ``libmioc.so`` (the C ABI declared in ``include/mioc.h``).

This is the product path.  There is no CPU fallback: if the HIP library is missing or no GPU is
visible, every entry point raises ``MiocNativeError``.
"""
from __future__ import annotations

import atexit
import collections
import ctypes
import math
import os
import sys
import weakref

import numpy as np

from .iterators import LevelTable

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libmioc.so")

MIOC_OK = 0
MIOC_EINVAL = -1
MIOC_EINEXACT = -2
MIOC_ENOMEM = -3
MIOC_EHIP = -4
MIOC_EINFEASIBLE = -5
MIOC_ESTATE = -6
MIOC_ENONFINITE = -7
MIOC_ECOMPILE = -8

MIOC_P_INF, MIOC_P_ONE, MIOC_P_INTLUT, MIOC_P_TABLE = 0, 1, 2, 3
MIOC_OPT_ALGO, MIOC_OPT_TIMING, MIOC_OPT_PERSIST, MIOC_OPT_PRED_FMA = 1, 2, 3, 4
MIOC_OPT_SPIN_LIMIT, MIOC_OPT_SDT_BUFFERS, MIOC_OPT_FSEP_SEGMENTS, MIOC_OPT_PINF_WALK = 5, 6, 7, 8
MIOC_OPT_SDT_ROW_OWNER = 10
MIOC_ALGO_AUTO, MIOC_ALGO_GENERIC, MIOC_ALGO_PINF, MIOC_ALGO_PYRAMID, MIOC_ALGO_SEPARABLE = 0, 1, 2, 3, 4
MIOC_ALGO_FUSED, MIOC_ALGO_FUSED_SEPARABLE = 5, 6
MIOC_ODE_FISHING, MIOC_ODE_DOUBLETANK, MIOC_ODE_VANDERPOL = 1, 2, 3
MIOC_ODE_INT_EULER, MIOC_ODE_INT_HEUN, MIOC_ODE_INT_RK4 = 0, 1, 2
MIOC_ODE_INT_BEULER, MIOC_ODE_INT_MIDPOINT = 16, 17  # the implicit schemes start at 16
MIOC_ODE_NEWTON_MAX, MIOC_ODE_NEWTON_TOL = 12, 1e-10
MIOC_ODE_DERIVE_FY, MIOC_ODE_DERIVE_FU, MIOC_ODE_DERIVE_GY, MIOC_ODE_DERIVE_GU, MIOC_ODE_DERIVE_ALL = 1, 2, 4, 8, 15
MIOC_ODE_TERMINAL, MIOC_ODE_STATES, MIOC_ODE_DERIVE_EY = 1, 2, 16  # flags of _create_bolza; the derive bit of Ey
MIOC_ODE_SCEN, MIOC_ODE_SCEN_DATA = 1, 2  # scen of _create_scen: state0 and params per scenario; the data rows as well
MIOC_ODE_SENS_P, MIOC_ODE_SENS_Y0 = 1, 2  # sens of _create_sens: dJ/dparams, dJ/dstate0
MIOC_ODE_DERIVE_FP, MIOC_ODE_DERIVE_GP, MIOC_ODE_DERIVE_EP = 32, 64, 128  # derive bits of Fp, Gp, Ep (with SENS_P)

EXPORTED = [
    "mioc_version", "mioc_create", "mioc_destroy", "mioc_last_error", "mioc_set_option", "mioc_set_levels",
    "mioc_set_cost", "mioc_bellman", "mioc_backtrack", "mioc_bellman_batch_device",
    "mioc_backtrack_batch_device", "mioc_synchronize", "mioc_stream", "mioc_kernel_stats",
    "mioc_reset_stats", "mioc_last_algo", "mioc_last_sdt_driver", "mioc_diagnostics", "mioc_get_argmin_table",
    "mioc_get_pinf_tables", "mioc_get_ranks_device",
    "mioc_pred", "mioc_pred_batch_device", "mioc_tv_device", "mioc_trm_decide_device", "mioc_batch_multi",
    "mioc_ode_eval_device", "mioc_rand_start_device", "mioc_backtrack_batch_budgets_device",
    "mioc_heat_setup", "mioc_heat_eval_device", "mioc_heat_eval",
    "mioc_conv_setup", "mioc_conv_eval_device", "mioc_conv_eval", "mioc_conv_tiles_per_wave",
    "mioc_trm_state_bytes", "mioc_trm_attach", "mioc_trm_outer_begin_device", "mioc_trm_inner_end_device",
    "mioc_trm_poll",
    "mioc_ode_program_create", "mioc_ode_program_destroy", "mioc_ode_program_eval_device",
    "mioc_ode_program_create_ex", "mioc_ode_program_create_ad",
    "mioc_ode_program_create_bolza", "mioc_ode_program_source", "mioc_ode_program_eval_bolza_device",
    "mioc_ode_program_eval_mixed_device", "mioc_rows_copy_device", "mioc_mixed_state_bytes", "mioc_mixed_fan_device",
    "mioc_mixed_select_device", "mioc_mixed_poll",
    "mioc_ode_program_create_scen", "mioc_ode_program_source_scen", "mioc_ode_program_eval_scen_device",
    "mioc_ode_program_create_sens", "mioc_ode_program_source_sens", "mioc_ode_program_eval_sens_device",
]

MIXED_FAN_TERMS = 2048  # slope terms per LDS chunk of mioc_mixed_fan_device (kMixedChunk)


def mixed_fan_chunk(nu):
    """Slope terms (elements of the continuous rows) that mioc_mixed_fan_device folds per LDS chunk: an even number of
    time steps of nu terms each, at most MIXED_FAN_TERMS."""
    return ((MIXED_FAN_TERMS // int(nu)) & ~1) * int(nu)


# one step of the p = Inf collapse's tables (Context.pinf_tables): R (RP,), kmin, k2 (BWP,) float64, kfirst (BWP,)
# int32, kabs float, and the sizes BW <= BWP, RP
PinfTables = collections.namedtuple("PinfTables", "R kmin k2 kfirst kabs BW BWP RP")


class MiocNativeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mioc error {code}: {msg}")
        self.code = code


class InexactError(MiocNativeError):
    """Non-integral |ν - u_old| -- the reference's InexactError (HelpFunctions.jl:37,57)."""


_lib = None


def load_library(path=None):
    """Load libmioc.so; raise loudly if it is missing (no silent fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("MIOC_LIB") or LIB_PATH
    if not os.path.exists(p):
        raise MiocNativeError(MIOC_EHIP, f"HIP library not built: {p} (run __graft_entry__.build())")
    # One HIP runtime per process: torch ships its own libamdhip64.so (soname libamdhip64.so.7).
    # Loading torch first makes the dynamic linker bind libmioc's DT_NEEDED libamdhip64.so.7 to that
    # same runtime, so torch tensors / torch.distributed and libmioc share devices and streams.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(p)
    vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    sig = {
        "mioc_version": (ctypes.c_char_p, []),
        "mioc_create": (i32, [i32, ctypes.POINTER(vp)]),
        "mioc_destroy": (i32, [vp]),
        "mioc_last_error": (ctypes.c_char_p, [vp]),
        "mioc_set_option": (i32, [vp, i32, i64]),
        "mioc_set_levels": (i32, [vp, i64, vp, vp, i64, vp]),
        "mioc_set_cost": (i32, [vp, i32, i64, dbl, i64, vp]),
        "mioc_bellman": (i32, [vp, vp, vp, i64, i64, i64, dbl]),
        "mioc_backtrack": (i32, [vp, i64, vp, ctypes.POINTER(dbl), vp]),
        "mioc_bellman_batch_device": (i32, [vp, i64, vp, vp, i64, i64, i64, dbl]),
        "mioc_backtrack_batch_device": (i32, [vp, i64, vp, vp, vp]),
        "mioc_synchronize": (i32, [vp]),
        "mioc_stream": (vp, [vp]),
        "mioc_kernel_stats": (i32, [vp, i32, ctypes.POINTER(dbl), ctypes.POINTER(i64),
                                    ctypes.POINTER(ctypes.c_char_p)]),
        "mioc_reset_stats": (i32, [vp]),
        "mioc_last_algo": (i32, [vp]),
        "mioc_last_sdt_driver": (i32, [vp]),
        "mioc_diagnostics": (i32, [vp, vp, i32]),
        "mioc_get_argmin_table": (i32, [vp, i64, i64, vp]),
        "mioc_get_pinf_tables": (i32, [vp, i64, i64, vp, vp, vp, vp, vp, vp]),
        "mioc_get_ranks_device": (i32, [vp, vp]),
        "mioc_pred": (i32, [vp, ctypes.POINTER(dbl), ctypes.POINTER(dbl), ctypes.POINTER(dbl),
                            ctypes.POINTER(dbl)]),
        "mioc_pred_batch_device": (i32, [vp, vp, vp, vp, vp]),
        "mioc_tv_device": (i32, [vp, i64, vp, i64, i64, vp]),
        "mioc_trm_decide_device": (i32, [vp, i64, vp, vp, vp, vp, vp, dbl, vp, vp]),
        "mioc_batch_multi": (i32, [vp, i32, i64, vp, vp, i64, i64, i64, dbl, i64, vp, vp, vp]),
        "mioc_ode_eval_device": (i32, [vp, i32, i64, vp, i64, i64, dbl, dbl, vp, i32, vp, vp]),
        "mioc_rand_start_device": (i32, [vp, i64, i64, i64, ctypes.c_uint64, vp]),
        "mioc_backtrack_batch_budgets_device": (i32, [vp, vp, vp, vp, vp]),
        "mioc_heat_setup": (i32, [vp, i64, i64, i64, dbl, dbl, dbl, vp, vp, vp, vp, vp]),
        "mioc_heat_eval_device": (i32, [vp, i64, vp, vp, vp]),
        "mioc_heat_eval": (i32, [vp, i64, vp, vp, vp]),
        "mioc_conv_setup": (i32, [vp, i64, dbl, dbl, vp, vp]),
        "mioc_conv_eval_device": (i32, [vp, i64, vp, vp, vp]),
        "mioc_conv_eval": (i32, [vp, i64, vp, vp, vp]),
        "mioc_conv_tiles_per_wave": (i32, [i64, i64]),
        "mioc_trm_state_bytes": (i64, [i64]),
        "mioc_trm_attach": (i32, [vp, vp]),
        "mioc_trm_outer_begin_device": (i32, [vp, i64, vp, vp, dbl, i64, vp]),
        "mioc_trm_inner_end_device": (i32, [vp, i64, vp, dbl, i64, dbl, i64, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp,
                                            vp, vp]),
        "mioc_trm_poll": (i32, [vp, vp, vp]),
        "mioc_ode_program_create": (i32, [ctypes.c_char_p, i32, i32, i32, ctypes.POINTER(vp), ctypes.c_char_p, i64]),
        "mioc_ode_program_create_ex": (i32, [ctypes.c_char_p, i32, i32, i32, i32, i32, ctypes.POINTER(vp),
                                             ctypes.c_char_p, i64]),
        "mioc_ode_program_create_ad": (i32, [ctypes.c_char_p, i32, i32, i32, i32, i32, i32, ctypes.POINTER(vp),
                                             ctypes.c_char_p, i64]),
        "mioc_ode_program_create_bolza": (i32, [ctypes.c_char_p, i32, i32, i32, i32, i32, i32, i32, i32,
                                                ctypes.POINTER(vp), ctypes.c_char_p, i64]),
        "mioc_ode_program_source": (i64, [ctypes.c_char_p, i32, i32, i32, i32, i32, i32, i32, i32, i32, ctypes.c_char_p,
                                          i64]),
        "mioc_ode_program_create_scen": (i32, [ctypes.c_char_p, i32, i32, i32, i32, i32, i32, i32, i32, i32,
                                               ctypes.POINTER(vp), ctypes.c_char_p, i64]),
        "mioc_ode_program_source_scen": (i64, [ctypes.c_char_p, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32,
                                               ctypes.c_char_p, i64]),
        "mioc_ode_program_eval_scen_device": (i32, [vp, vp, i64, i64, vp, i64, dbl, dbl, i64, vp, vp, vp, vp, vp, vp]),
        "mioc_ode_program_create_sens": (i32, [ctypes.c_char_p, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32,
                                               ctypes.POINTER(vp), ctypes.c_char_p, i64]),
        "mioc_ode_program_source_sens": (i64, [ctypes.c_char_p, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32,
                                               ctypes.c_char_p, i64]),
        "mioc_ode_program_eval_sens_device": (i32, [vp, vp, i64, i64, vp, i64, dbl, dbl, i64, vp, vp, vp, vp, vp, vp,
                                                    vp, vp]),
        "mioc_ode_program_destroy": (i32, [vp]),
        "mioc_ode_program_eval_bolza_device": (i32, [vp, vp, i64, i64, vp, i64, dbl, dbl, vp, vp, vp, vp, vp, vp]),
        "mioc_ode_program_eval_device": (i32, [vp, vp, i64, vp, i64, dbl, dbl, vp, vp, vp, vp]),
        "mioc_ode_program_eval_mixed_device": (i32, [vp, vp, i64, i64, vp, i64, dbl, dbl, vp, vp, vp, vp]),
        "mioc_rows_copy_device": (i32, [vp, i64, i64, vp, i64, i64, vp, i64, i64, i64]),
        "mioc_mixed_state_bytes": (i64, [i64]),
        "mioc_mixed_fan_device": (i32, [vp, i64, i64, i64, i64, i64, dbl, vp, vp, vp, vp, vp, vp, vp]),
        "mioc_mixed_select_device": (i32, [vp, i64, i64, i64, i64, i64, dbl, dbl, dbl, vp, vp, vp, vp, vp, vp, vp]),
        "mioc_mixed_poll": (i32, [vp, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def ptr(t):
    """The device address of a tensor as a ``c_void_p``; None stays None (a NULL pointer)."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def check_tensor(name, t, n=None, dtype="float64", dim=None, on=None, optional=False):
    """ValueError unless t is a contiguous CUDA tensor of torch.<dtype> -- with n entries (n given), of shape
    (K, nt, nx) (dim=3), on the device of the tensor ``on`` (given); optional: None passes."""
    if t is None and optional:
        return
    if (t is None or not t.is_cuda or not t.is_contiguous() or str(t.dtype) != "torch." + dtype or
            (dim is not None and t.dim() != dim) or (n is not None and t.numel() != n) or
            (on is not None and t.device != on.device)):
        raise ValueError(f"{name} must be a contiguous {dtype} CUDA tensor" +
                         (" of shape (K, nt, nx)" if dim == 3 else "") +
                         (f" with {n} entries" if n is not None else "") +
                         (" on the device of x" if on is not None else ""))


def cost_spec(p, L=None, levels=None):
    """Map the reference's ``p`` (Int, Float64 or Inf; multi-trust.jl:28) to (p_kind, p_int, table).

    p = Inf and p = 1 are exact on the device.  For other p the weight (sum |d|^p)^(1/p) uses
    Julia's own ``^`` in the reference; here the host supplies it (computed with Python's pow unless a
    caller passes Julia's values) -- parity for p not in {1, Inf} is unpinned.
    """
    if p == math.inf:
        return MIOC_P_INF, 1, None
    if float(p) == 1.0:
        return MIOC_P_ONE, 1, None
    if float(p) == int(p) and 2 <= int(p) <= 8:
        pi = int(p)
        maxkey = sum(int(max(v) - min(v)) ** pi for v in levels.nu)
        return MIOC_P_INTLUT, pi, np.array([float(s) ** (1.0 / pi) for s in range(maxkey + 1)])
    if not p > 0:
        raise ValueError("Only positive integer valued `p` are accepted!")
    nv = levels.nuval
    d = np.abs(nv[:, None, :] - nv[None, :, :]) ** float(p)
    return MIOC_P_TABLE, 1, np.ascontiguousarray((d.sum(axis=2) ** (1.0 / float(p))).reshape(-1))


_LIVE = weakref.WeakSet()  # contexts not yet closed


@atexit.register
def _close_live_contexts():
    """Destroy every context still open while the HIP runtime is alive: atexit handlers run before the C
    runtime's exit() tears down libamdhip64's static state, whereas a __del__ reached during interpreter
    finalisation (or from a garbage cycle collected then) can run after it ('What's weak' 5)."""
    for c in list(_LIVE):
        try:
            c.close()
        except Exception:
            pass


class Context:
    """One device context: levels + cost + the resident DP (fronts / argmin table / class tables).

    Close it explicitly (``close()`` or ``with Context(0) as ctx:``); contexts left open are closed by an atexit
    handler, never from ``__del__`` during interpreter shutdown."""

    def __init__(self, device=0):
        self.h = None
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.mioc_create(int(device), ctypes.byref(h))
        if rc != MIOC_OK:
            raise MiocNativeError(rc, f"mioc_create(device={device}) failed (no visible HIP device?)")
        self.h = h
        self.device = int(device)
        self.levels = None
        self.M = None
        self.nt = None
        self.B = None
        _LIVE.add(self)

    def close(self):
        if self.h:
            h, self.h = self.h, None
            _LIVE.discard(self)
            self.lib.mioc_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self, _finalizing=sys.is_finalizing):
        # an unreferenced context is destroyed while the program runs; at shutdown the atexit handler has
        # already closed it, and a HIP call from a finaliser that runs after the runtime's teardown is unsafe
        # (the default argument keeps the check usable after the sys module is torn down)
        if _finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != MIOC_OK:
            msg = self.lib.mioc_last_error(self.h).decode()
            if rc == MIOC_EINEXACT:
                raise InexactError(rc, msg)
            raise MiocNativeError(rc, msg)

    def set_option(self, option, value):
        self._check(self.lib.mioc_set_option(self.h, option, int(value)))

    def set_levels(self, levels: LevelTable):
        self.levels = levels
        self.M = levels.M
        self._check(self.lib.mioc_set_levels(self.h, levels.M, _p(levels.counts), _p(levels.values),
                                             levels.L, _p(levels.tuples)))

    def set_cost(self, p, beta, table=None, p_int=None, p_kind=None):
        if p_kind is None:
            p_kind, p_int, tab = cost_spec(p, levels=self.levels)
            if table is not None:
                tab = np.ascontiguousarray(table, dtype=np.float64)
        else:
            tab = None if table is None else np.ascontiguousarray(table, dtype=np.float64)
            p_int = p_int or 1
        self._tab = tab
        self._check(self.lib.mioc_set_cost(self.h, p_kind, int(p_int), float(beta),
                                           0 if tab is None else tab.size,
                                           None if tab is None else _p(tab)))

    # -- host-buffer API (Julia-style: ∇f and u_old are nx x nt, column-major) --------------
    def bellman(self, df, u_old, B, dt):
        df = np.asfortranarray(df, dtype=np.float64)
        u_old = np.asfortranarray(u_old, dtype=np.float64)
        if df.shape != u_old.shape:
            raise ValueError("df and u_old must have the same shape (nx, nt)")
        nx, nt = df.shape
        self._check(self.lib.mioc_bellman(self.h, _p(df), _p(u_old), nx, nt, int(B), float(dt)))
        self.nt, self.B = nt, int(B)  # after success: a rejected call leaves the previous DP (and its sizes) in place

    def backtrack(self, B_use=None):
        if self.nt is None:  # no DP yet: let the library report the state error (MIOC_ESTATE)
            dummy = np.zeros(1, dtype=np.float64)
            self._check(self.lib.mioc_backtrack(self.h, 0 if B_use is None else int(B_use), _p(dummy),
                                                None, None))
        B_use = self.B if B_use is None else int(B_use)
        u = np.zeros((self.M, self.nt), dtype=np.float64, order="F")
        ps = ctypes.c_double(0.0)
        sw = np.zeros(self.nt, dtype=np.uint8)
        self._check(self.lib.mioc_backtrack(self.h, B_use, _p(u), ctypes.byref(ps), _p(sw)))
        return u, ps.value, sw.astype(bool)

    # -- device-resident batch API (pointers are device addresses, e.g. torch .data_ptr()) ----
    def bellman_batch_device(self, K, df_ptr, uold_ptr, nx, nt, B, dt):
        self._check(self.lib.mioc_bellman_batch_device(self.h, int(K), ctypes.c_void_p(df_ptr),
                                                       ctypes.c_void_p(uold_ptr), int(nx), int(nt), int(B),
                                                       float(dt)))
        self.nt, self.B = nt, int(B)

    def backtrack_batch_device(self, B_use, u_ptr, phi_ptr=0, status_ptr=0):
        self._check(self.lib.mioc_backtrack_batch_device(self.h, int(B_use), ctypes.c_void_p(u_ptr),
                                                         ctypes.c_void_p(phi_ptr or None),
                                                         ctypes.c_void_p(status_ptr or None)))

    # -- the same, from torch tensors (shape/contiguity checked: the raw-pointer API cannot check) --
    def bellman_batch_tensors(self, df, u_old, B, dt):
        """df, u_old: float64 CUDA tensors of shape (K, nt, nx), C-contiguous (each subproblem's nx x nt
        column-major block, the layout of mioc_bellman_batch_device)."""
        check_tensor("df", df, dim=3)
        check_tensor("u_old", u_old, dim=3)
        if tuple(df.shape) != tuple(u_old.shape):
            raise ValueError("df and u_old must have the same shape (K, nt, nx)")
        K, nt, nx = df.shape
        self.bellman_batch_device(K, df.data_ptr(), u_old.data_ptr(), nx, nt, B, dt)

    def backtrack_batch_tensors(self, B_use, u, phi=None, status=None):
        """u: float64 CUDA tensor (K, nt, nx), contiguous; phi: (K,) float64; status: (K,) int32."""
        check_tensor("u", u, dim=3)
        check_tensor("phi", phi, u.shape[0], optional=True)
        check_tensor("status", status, u.shape[0], "int32", optional=True)
        self.backtrack_batch_device(B_use, u.data_ptr(), 0 if phi is None else phi.data_ptr(),
                                    0 if status is None else status.data_ptr())

    def backtrack_batch_budgets_tensors(self, budgets, u, phi=None, status=None):
        """eval_u_TRM! with one budget per subproblem: budgets (K,) int32 CUDA tensor (each <= B); u (K, nt, nx)
        float64 CUDA tensor; phi, status optional (mioc_backtrack_batch_budgets_device)."""
        check_tensor("u", u, dim=3)
        check_tensor("budgets", budgets, u.shape[0], "int32")
        check_tensor("phi", phi, u.shape[0], optional=True)
        check_tensor("status", status, u.shape[0], "int32", optional=True)
        self._check(self.lib.mioc_backtrack_batch_budgets_device(self.h, ptr(budgets), ptr(u), ptr(phi), ptr(status)))

    def ranks_tensor(self, out):
        """Level ranks (iterator order) of the last backtrack into `out`, an int32 CUDA tensor (K, nt)."""
        check_tensor("out", out, dtype="int32")
        self._check(self.lib.mioc_get_ranks_device(self.h, ptr(out)))

    # -- trust-region quantities of the last backtrack (multi-trust.jl:117-158) -------------------
    def pred(self):
        """(int_val, TV_p(u_old), TV_p(u), pred) of the last single-subproblem backtrack, on the device."""
        out = [ctypes.c_double(0.0) for _ in range(4)]
        self._check(self.lib.mioc_pred(self.h, *[ctypes.byref(x) for x in out]))
        return tuple(x.value for x in out)

    def pred_batch_tensors(self, int_val=None, tv_old=None, tv_new=None, pred=None):
        """Per-subproblem int_val / TV_p(u_old) / TV_p(u) / pred of the last batch backtrack into (K,) float64
        CUDA tensors (each optional); enqueued on the context's stream."""
        for name, t in (("int_val", int_val), ("tv_old", tv_old), ("tv_new", tv_new), ("pred", pred)):
            check_tensor(name, t, optional=True)
        self._check(self.lib.mioc_pred_batch_device(self.h, ptr(int_val), ptr(tv_old), ptr(tv_new), ptr(pred)))

    def tv_tensors(self, u, out):
        """TV_p of controls u (K, nt, nx) float64 CUDA tensor into out (K,) float64; enqueued."""
        check_tensor("u", u, dim=3)
        K, nt, nx = u.shape
        check_tensor("out", out, K)
        self._check(self.lib.mioc_tv_device(self.h, K, ptr(u), nx, nt, ptr(out)))

    # ---- device-resident TRM control (multi-trust.jl:92-163; include/mioc.h) ----------------------------------
    def trm_state_tensor(self, K):
        """A zero-initialised device state block for K restarts (uint8 CUDA tensor)."""
        import torch
        n = int(self.lib.mioc_trm_state_bytes(int(K)))
        if n < 0:
            raise ValueError("K must be in [1, 4096]")
        return torch.zeros(n, dtype=torch.uint8, device=f"cuda:{self.device}")

    def trm_attach(self, state):
        """Gate the inner-loop kernels by the state's gate word (None detaches)."""
        self._check(self.lib.mioc_trm_attach(self.h, ptr(state)))

    def trm_outer_begin(self, state, tv_u, D0, B, budgets):
        K = tv_u.numel()
        self._check(self.lib.mioc_trm_outer_begin_device(self.h, K, ptr(state), ptr(tv_u), float(D0), int(B),
                                                          ptr(budgets)))

    def trm_inner_end(self, state, sigma, kmax, tau, B, int_val, tv_new, J_new, J_old, J, tv_u, budgets, trial, u,
                      u_old, decision=None):
        K = J.numel()
        self._check(self.lib.mioc_trm_inner_end_device(
            self.h, K, ptr(state), float(sigma), int(kmax), float(tau), int(B), ptr(int_val), ptr(tv_new), ptr(J_new),
            ptr(J_old), ptr(J), ptr(tv_u), ptr(budgets), ptr(decision), u[0].numel(), ptr(trial), ptr(u), ptr(u_old)))

    def trm_state_arrays(self, state, K):
        """The state block on the host: Δᵏ, TV_old, k, flags (1 inner, 2 halved, 4 stopped), outer iterations."""
        self.synchronize()
        b = state.cpu().numpy()
        o = 16
        out = {}
        for name, dt in (("Dk", np.float64), ("tv_old", np.float64), ("k", np.int32), ("flags", np.int32),
                         ("iters", np.int32)):
            n = K * np.dtype(dt).itemsize
            out[name] = b[o:o + n].view(dt).copy()
            o += n
        return out

    def trm_poll(self, state):
        """Synchronise once; (any restart inside its inner loop, any restart not stopped)."""
        out = np.zeros(2, dtype=np.int32)
        self._check(self.lib.mioc_trm_poll(self.h, ptr(state), _p(out)))
        return bool(out[0]), bool(out[1])

    def trm_decide_tensors(self, J_old, J_new, tv_old, tv_new, pred, sigma, decision, ared=None):
        """multi-trust.jl:127-158 per subproblem: decision (K,) int32 = 2 stop / 1 halve / 0 accept."""
        ts = (J_old, J_new, tv_old, tv_new, pred)
        K = decision.numel()
        for name, t in zip(("J_old", "J_new", "tv_old", "tv_new", "pred"), ts):
            check_tensor(name, t, K)
        check_tensor("ared", ared, K, optional=True)
        check_tensor("decision", decision, dtype="int32")
        self._check(self.lib.mioc_trm_decide_device(self.h, K, *[ptr(t) for t in ts], float(sigma), ptr(ared),
                                                    ptr(decision)))

    @staticmethod
    def _check_eval(x, J, df):
        """The checks every objective's evaluation makes: x (K, nt, nx), and J (K,) and df like x if given."""
        check_tensor("x", x, dim=3)
        check_tensor("J", J, x.shape[0], optional=True)
        check_tensor("df", df, x.numel(), optional=True)
        return x.shape

    def ode_eval_tensors(self, problem, x, T0, T1, J=None, df=None, params=None):
        """eval_f! / eval_df! of an ODE example for K controls x (K, nt, 3) float64 CUDA tensor: J (K,) and df
        (K, nt, 3) float64 CUDA tensors (each optional); enqueued (mioc_ode_eval_device)."""
        K, nt, nx = self._check_eval(x, J, df)
        par = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
        self._check(self.lib.mioc_ode_eval_device(
            self.h, int(problem), K, ptr(x), nx, nt, float(T0), float(T1),
            None if par is None else _p(par), 0 if par is None else par.size, ptr(J), ptr(df)))

    def _ode_program_eval(self, prog, nu, nu_min, x, T0, T1, S, state0, params, data, J, df, Y, Jp, Jy0):
        """The body of ode_program_eval_tensors, ode_program_eval_mixed_tensors (S = 0: state0 and params are host
        values) and ode_program_eval_scen_tensors (S >= 1: they are device arrays): the checks, then the one call of the
        library's _sens eval entry, which is every older eval entry with the arguments it lacks zero."""
        K, nt, nx = self._check_eval(x, J, df)
        if nx != prog.nx:
            raise ValueError(f"x has {nx} controls, the program {prog.nx}")
        if int(nu) != nu or not nu_min <= nu < nx:
            raise ValueError(f"nu must be an integer in {nu_min}..{nx - 1}, not {nu!r}")
        scen, sens, nd = int(getattr(prog, "scenarios", 0)), int(getattr(prog, "sens", 0)), getattr(prog, "ndata", 0)
        if Y is not None and not getattr(prog, "states", False):
            raise ValueError("the program was not compiled with states=True")
        for name, t, bit in (("Jp", Jp, MIOC_ODE_SENS_P), ("Jy0", Jy0, MIOC_ODE_SENS_Y0)):
            if t is not None and not sens & bit:
                raise ValueError(f"the program was not compiled with the sensitivities that {name} asks for")
        for name, t, n in (("J", J, K), ("df", df, x.numel()), ("Y", Y, K * (nt + 1) * prog.ny),
                           ("data", data, nt * nd * (S if S and scen & MIOC_ODE_SCEN_DATA else 1)),
                           ("Jp", Jp, K * prog.nparams), ("Jy0", Jy0, K * prog.ny)):
            check_tensor(name, t, n, on=x, optional=True)
        if S:  # the arrays of S scenarios, on the device
            if not scen:
                raise ValueError("the program was not compiled with scenarios")
            if K % S:
                raise ValueError(f"the number of controls, {K}, must be a multiple of the {S} scenarios")
            if data is None and nd:
                raise ValueError("the program reads sampled data: data missing")
            check_tensor("state0", state0, prog.ny * S, on=x)
            check_tensor("params", params, prog.nparams * S, on=x, optional=not prog.nparams)
            y0, par = ptr(state0), ptr(params)
        else:      # one state0 and one parameter vector, host values (a scenario program is refused by the library)
            h_y0 = np.ascontiguousarray(state0, dtype=np.float64).reshape(-1)
            h_par = np.ascontiguousarray(() if params is None else params, dtype=np.float64).reshape(-1)
            if h_y0.size != prog.ny or h_par.size != prog.nparams:
                raise ValueError(f"the program takes {prog.ny} initial states and {prog.nparams} parameters")
            y0, par = _p(h_y0), _p(h_par) if h_par.size else None
        if not prog.h:
            raise ValueError("the ODE program is closed")
        self._check(self.lib.mioc_ode_program_eval_sens_device(
            self.h, prog.h, int(nu), K, ptr(x), nt, float(T0), float(T1), S, y0, par, ptr(data), ptr(J), ptr(df),
            ptr(Y), ptr(Jp), ptr(Jy0)))

    def ode_program_eval_tensors(self, prog, x, T0, T1, state0, params, J=None, df=None, data=None, Y=None, Jp=None,
                                 Jy0=None):
        """eval_f! / eval_df! of a user-defined ODE objective (mioc.ode_device.ODEProgram) for K controls x
        (K, nt, nx) float64 CUDA tensor: J (K,) and df (K, nt, nx) float64 CUDA tensors (each optional); state0 (ny)
        and params (nparams) host values; enqueued (the library's _sens eval entry with nu = 0 and S = 0, which is what
        its plain and _bolza entries forward to).  data: the (nt, ndata) float64 CUDA tensor of a program with sampled
        data; Y: a (K, nt + 1, ny) float64 CUDA tensor to receive the states at the control-grid points (a program
        compiled with states=True).  Jp (K, nparams), Jy0 (K, ny): float64 CUDA tensors to receive dJ/dparams and
        dJ/dstate0 (a program compiled with sensitivities; include/mioc.h, "Sensitivities")."""
        self._ode_program_eval(prog, 0, 0, x, T0, T1, 0, state0, params, data, J, df, Y, Jp, Jy0)

    def ode_program_eval_scen_tensors(self, prog, nu, x, T0, T1, S, state0, params, data=None, J=None, df=None, Y=None,
                                      Jp=None, Jy0=None):
        """ode_program_eval_tensors (nu None or 0) / ode_program_eval_mixed_tensors (nu >= 1) for a program compiled
        with scenarios (include/mioc.h, "Scenarios"): restart k of the K controls x solves scenario k % S.  state0
        (ny, S), params (nparams, S; None with nparams == 0) and data ((nt, ndata), or (nt, ndata, S) for a program
        with per-scenario data) are contiguous float64 CUDA tensors, the scenario index fastest; enqueued
        (the library's _sens eval entry with S >= 1, which is what its _scen entry forwards to).
        Jp (K, nparams), Jy0 (K, ny): restart k's derivatives in scenario k % S's own parameters and state0."""
        if int(S) < 1:
            raise ValueError(f"need S >= 1 scenarios, not {S!r}")
        self._ode_program_eval(prog, nu or 0, 0, x, T0, T1, int(S), state0, params, data, J, df, Y, Jp, Jy0)

    # ---- mixed controls: the continuous step beside the DP (include/mioc.h, "Mixed controls") -----------------
    def ode_program_eval_mixed_tensors(self, prog, nu, x, T0, T1, state0, params, J=None, df=None, data=None, Y=None,
                                       Jp=None, Jy0=None):
        """ode_program_eval_tensors for a mixed control: the first nu >= 1 of the program's nx controls are continuous,
        the levels describe the other nx - nu; x may hold the K*R candidates of a fan
        (the library's _sens eval entry with S = 0, which is what its _mixed entry forwards to; that entry's refusal of
        nu < 1 is made here)."""
        self._ode_program_eval(prog, nu, 1, x, T0, T1, 0, state0, params, data, J, df, Y, Jp, Jy0)

    def rows_copy_tensors(self, dst, dst_row0, src, src_row0, nrows):
        """dst[:, :, dst_row0:dst_row0 + nrows] = src[:, :, src_row0:src_row0 + nrows] for float64 CUDA tensors
        (K, nt, dst_nx) and (K, nt, src_nx); dst may be src with disjoint rows.  Enqueued, gated by trm_attach
        (mioc_rows_copy_device); the row ranges are checked by the library."""
        check_tensor("dst", dst, dim=3)
        check_tensor("src", src, dim=3)
        if tuple(dst.shape[:2]) != tuple(src.shape[:2]):
            raise ValueError("dst and src must agree in K and nt")
        K, nt, dnx = dst.shape
        self._check(self.lib.mioc_rows_copy_device(self.h, K, nt, ptr(dst), dnx, int(dst_row0), ptr(src), src.shape[2],
                                                   int(src_row0), int(nrows)))

    def mixed_state_tensor(self, K, s0):
        """A device state block of the continuous step for K restarts (uint8 CUDA tensor): zeroed, the step sizes s0."""
        import torch
        n = int(self.lib.mioc_mixed_state_bytes(int(K)))
        if n < 0:
            raise ValueError("K must be in [1, 4096]")
        if not (s0 > 0 and math.isfinite(s0)):
            raise ValueError("s0 must be positive and finite")
        b = np.zeros(n, dtype=np.uint8)
        b[16:16 + 8 * int(K)].view(np.float64)[:] = float(s0)
        return torch.from_numpy(b).to(f"cuda:{self.device}")

    def _mixed_check(self, K, R, nu, nx, nt, mstate, f64, what):
        if not 1 <= int(R) <= 16:
            raise ValueError("R must be in 1..16")
        if not 1 <= int(nu) <= nx:
            raise ValueError(f"nu must be in 1..{nx}")
        check_tensor("mstate (of mixed_state_tensor(K, s0))", mstate, int(self.lib.mioc_mixed_state_bytes(K)), "uint8")
        for name, t, n in f64:
            check_tensor(f"{what}: {name}", t, n)

    def mixed_fan_tensors(self, R, nu, tau, x, df, lo, hi, mstate, xfan, slope):
        """The R line-search candidates of every restart: x, df (K, nt, nx), lo, hi (nt, nu), xfan (R, K, nt, nx),
        slope (R, K) float64 CUDA tensors; enqueued (mioc_mixed_fan_device)."""
        if x.dim() != 3:
            raise ValueError("x must have the shape (K, nt, nx)")
        K, nt, nx = x.shape
        self._mixed_check(K, R, nu, nx, nt, mstate,
                          (("x", x, K * nt * nx), ("df", df, K * nt * nx), ("lo", lo, nt * nu), ("hi", hi, nt * nu),
                           ("xfan", xfan, R * K * nt * nx), ("slope", slope, R * K)), "mixed_fan")
        self._check(self.lib.mioc_mixed_fan_device(self.h, K, int(R), int(nu), nx, nt, float(tau), ptr(x), ptr(df),
                                                   ptr(lo), ptr(hi), ptr(mstate), ptr(xfan), ptr(slope)))

    def mixed_select_tensors(self, R, nu, c1, smax, ctol, mstate, trm_state, xfan, slope, Jfan, J_old, x):
        """Per restart the first candidate that passes the Armijo test, the step-size update and the finality rule
        (mioc_mixed_select_device): xfan (R, K, nt, nx), slope, Jfan (R, K), J_old (K,), x (K, nt, nx); trm_state the
        block of trm_state_tensor(K).  Enqueued."""
        if x.dim() != 3:
            raise ValueError("x must have the shape (K, nt, nx)")
        K, nt, nx = x.shape
        self._mixed_check(K, R, nu, nx, nt, mstate,
                          (("x", x, K * nt * nx), ("xfan", xfan, R * K * nt * nx), ("slope", slope, R * K),
                           ("Jfan", Jfan, R * K), ("J_old", J_old, K)), "mixed_select")
        check_tensor("trm_state (of trm_state_tensor(K))", trm_state, int(self.lib.mioc_trm_state_bytes(K)), "uint8")
        self._check(self.lib.mioc_mixed_select_device(self.h, K, int(R), int(nu), nx, nt, float(c1), float(smax),
                                                      float(ctol), ptr(mstate), ptr(trm_state), ptr(xfan), ptr(slope),
                                                      ptr(Jfan), ptr(J_old), ptr(x)))

    def mixed_poll(self, mstate, trm_state):
        """Synchronise once; (any restart inside its inner loop, any restart that can still move)
        (mioc_mixed_poll)."""
        out = np.zeros(2, dtype=np.int32)
        self._check(self.lib.mioc_mixed_poll(self.h, ptr(mstate), ptr(trm_state), _p(out)))
        return bool(out[0]), bool(out[1])

    def mixed_state_arrays(self, mstate, K):
        """The mixed state block on the host: s, flags (1 final, 2 moved), jsel, csteps."""
        self.synchronize()
        b = mstate.cpu().numpy()
        o = 16
        out = {}
        for name, dt in (("s", np.float64), ("flags", np.int32), ("jsel", np.int32), ("csteps", np.int32)):
            n = K * np.dtype(dt).itemsize
            out[name] = b[o:o + n].view(dt).copy()
            o += n
        return out

    def heat_setup(self, M_invA, M_invF, mass, state0, yd, T0, T1, gamma):
        """Hand the heat objective's matrices to the device (mioc_heat_setup; example_heat.jl:101-115): M_invA, mass
        (N, N), M_invF (N, nx), state0 (N,), yd (N, nt+1) as numpy arrays; nt = yd.shape[1] - 1."""
        f = lambda a: np.asfortranarray(a, dtype=np.float64)  # noqa: E731  (column-major, Julia's layout)
        A, F, Mm, y0, Yd = f(M_invA), f(M_invF), f(mass), f(state0), f(yd)
        N, nx = F.shape
        nt = Yd.shape[1] - 1
        if A.shape != (N, N) or Mm.shape != (N, N) or y0.shape != (N,) or Yd.shape[0] != N:
            raise ValueError("heat matrices: M_invA, mass (N, N); M_invF (N, nx); state0 (N,); yd (N, nt+1)")
        self._check(self.lib.mioc_heat_setup(self.h, N, nx, nt, float(T0), float(T1), float(gamma),
                                             _p(A), _p(F), _p(Mm), _p(y0), _p(Yd)))
        self.heat_shape = (N, nx, nt)

    def heat_eval_tensors(self, x, J=None, df=None):
        """eval_f / eval_df of the heat objective for K controls x (K, nt, nx) float64 CUDA tensor into J (K,) and
        df (K, nt, nx) float64 CUDA tensors (each optional); enqueued (mioc_heat_eval_device)."""
        K, nt, nx = self._check_eval(x, J, df)
        if getattr(self, "heat_shape", None) is None or self.heat_shape[1:] != (nx, nt):
            raise ValueError("x does not match the (nx, nt) given to heat_setup")
        self._check(self.lib.mioc_heat_eval_device(self.h, K, ptr(x), ptr(J), ptr(df)))

    def heat_eval(self, xs):
        """Host entry (mioc_heat_eval): xs (K, nx, nt) numpy controls (Julia's per-restart layout) -> J (K,),
        df (K, nx, nt)."""
        x = np.ascontiguousarray(np.asarray(xs, dtype=np.float64).transpose(0, 2, 1))  # K x (nx x nt col-major)
        K, nt, nx = x.shape
        if getattr(self, "heat_shape", None) is None or self.heat_shape[1:] != (nx, nt):
            raise ValueError("xs does not match the (nx, nt) given to heat_setup")
        J = np.empty(K)
        df = np.empty_like(x)
        self._check(self.lib.mioc_heat_eval(self.h, K, _p(x), _p(J), _p(df)))
        return J, df.transpose(0, 2, 1)

    def conv_setup(self, kappa, fvec, T0, T1):
        """Hand the convolution objective's data to the device (mioc_conv_setup; example_convolution.jl:67,47):
        kappa = K[2:nt+1, 1] (nt,) and fvec (nt+1,) as numpy arrays; nt = kappa.size."""
        kap = np.ascontiguousarray(kappa, dtype=np.float64)
        fv = np.ascontiguousarray(fvec, dtype=np.float64)
        if kap.ndim != 1 or fv.shape != (kap.size + 1,):
            raise ValueError("convolution data: kappa (nt,), fvec (nt+1,)")
        nt = kap.size
        self._check(self.lib.mioc_conv_setup(self.h, nt, float(T0), float(T1), _p(kap), _p(fv)))
        self.conv_shape = (1, nt)

    def conv_eval_tensors(self, x, J=None, df=None):
        """eval_f / eval_df of the convolution objective for K controls x (K, nt, 1) float64 CUDA tensor into J (K,)
        and df (K, nt, 1) float64 CUDA tensors (each optional; without df the call stops after J); enqueued
        (mioc_conv_eval_device)."""
        K, nt, nx = self._check_eval(x, J, df)
        if getattr(self, "conv_shape", None) is None or self.conv_shape != (nx, nt):
            raise ValueError("x does not match the (nx = 1, nt) given to conv_setup")
        self._check(self.lib.mioc_conv_eval_device(self.h, K, ptr(x), ptr(J), ptr(df)))

    def conv_tiles_per_wave(self, nt, K):
        """1 or 2: the column tiles per wave of the product kernel that K restarts at nt run
        (mioc_conv_tiles_per_wave)."""
        n = self.lib.mioc_conv_tiles_per_wave(int(nt), int(K))
        if n not in (1, 2):
            raise ValueError("nt or K out of range")
        return n

    def conv_eval(self, xs):
        """Host entry (mioc_conv_eval): xs (K, 1, nt) numpy controls (Julia's per-restart layout) -> J (K,),
        df (K, 1, nt)."""
        x = np.ascontiguousarray(np.asarray(xs, dtype=np.float64).transpose(0, 2, 1))  # K x (nx x nt col-major)
        K, nt, nx = x.shape
        if getattr(self, "conv_shape", None) is None or self.conv_shape != (nx, nt):
            raise ValueError("xs does not match the (nx = 1, nt) given to conv_setup")
        J = np.empty(K)
        df = np.empty_like(x)
        self._check(self.lib.mioc_conv_eval(self.h, K, _p(x), _p(J), _p(df)))
        return J, df.transpose(0, 2, 1)

    def rand_start_tensor(self, out, seed, jumps=-1):
        """rand_func_int (HelpFunctions.jl:204-225) for K restarts into out, a (K, nt, M) float64 CUDA tensor;
        jumps < 0: floor(nt / 10).  Enqueued (mioc_rand_start_device)."""
        check_tensor("out", out, dim=3)
        K, nt, M = out.shape
        if M != self.M:
            raise ValueError("out's last dimension must be the levels' M")
        self._check(self.lib.mioc_rand_start_device(self.h, K, nt, int(jumps), ctypes.c_uint64(int(seed)), ptr(out)))

    def synchronize(self):
        self._check(self.lib.mioc_synchronize(self.h))

    def stream(self):
        return self.lib.mioc_stream(self.h)

    def kernel_stats(self, which=0):
        ms = ctypes.c_double(0)
        n = ctypes.c_int64(0)
        name = ctypes.c_char_p()
        self._check(self.lib.mioc_kernel_stats(self.h, int(which), ctypes.byref(ms), ctypes.byref(n),
                                               ctypes.byref(name)))
        return ms.value, n.value, (name.value or b"").decode()

    def reset_stats(self):
        self._check(self.lib.mioc_reset_stats(self.h))

    def last_algo(self):
        return self.lib.mioc_last_algo(self.h)

    def last_sdt_driver(self):
        """The driver of the last separable DP: 0 per-step launches, 1 k_sdt_run, 2 the one-row k_sdt_run1."""
        return self.lib.mioc_last_sdt_driver(self.h)

    def argmin_table(self, step, k=0):
        """U of step `step` in the reference layout: int32 (B+1, Lgrid), rank of the minimising source
        (mioc_get_argmin_table; cells with Φ = +Inf are -1 below b̃ and unspecified above)."""
        lg = int(np.prod(self.levels.counts))
        out = np.empty((lg, self.B + 1), dtype=np.int32)
        self._check(self.lib.mioc_get_argmin_table(self.h, int(k), int(step), _p(out)))
        return out.T

    def pinf_tables(self, step, k=0):
        """The p=Inf collapse's device rows of step `step` (0 <= step < nt) of subproblem k, as they are
        (mioc_get_pinf_tables): a PinfTables of R[0..RP), kmin, k2, kfirst[0..BWP), kabs and (BW, BWP, RP)."""
        sizes = np.zeros(3, dtype=np.int64)
        self._check(self.lib.mioc_get_pinf_tables(self.h, int(k), int(step), None, None, None, None, None, _p(sizes)))
        BW, BWP, RP = (int(x) for x in sizes)
        R = np.empty(RP, dtype=np.float64)
        kmin, k2 = np.empty(BWP, dtype=np.float64), np.empty(BWP, dtype=np.float64)
        kfirst = np.empty(BWP, dtype=np.int32)
        kabs = np.zeros(1, dtype=np.float64)
        self._check(self.lib.mioc_get_pinf_tables(self.h, int(k), int(step), _p(R), _p(kmin), _p(k2), _p(kfirst),
                                                  _p(kabs), None))
        return PinfTables(R, kmin, k2, kfirst, float(kabs[0]), BW, BWP, RP)

    def diagnostics(self):
        """[value-collision targets scanned, multi-level targets scanned, p=Inf walk fallbacks or U-table walk
        run-ahead rounds, errors,
        hash-overflow rows, targets whose value was not found, values flagged colliding (persistent / segmented DPs
        redone), occupancy, fused separable row segments, p=Inf segmented walk: subproblems walked serially]
        (include/mioc.h)."""
        out = np.zeros(10, dtype=np.int64)
        self._check(self.lib.mioc_diagnostics(self.h, _p(out), 10))
        return out.tolist()


def batch_multi(ctxs, df, u_old, B, dt, B_use=None):
    """mioc_batch_multi: K subproblems (host float64 arrays of shape (K, nt, nx), C-contiguous) split over the
    contexts (one per device, levels and cost set), each block solved from its own host thread.
    Returns (u (K, nt, nx), phi_star (K,), status (K,))."""
    df = np.ascontiguousarray(df, dtype=np.float64)
    u_old = np.ascontiguousarray(u_old, dtype=np.float64)
    if df.ndim != 3 or df.shape != u_old.shape:
        raise ValueError("df and u_old must have the same shape (K, nt, nx)")
    K, nt, nx = df.shape
    u = np.empty_like(df)
    phi = np.empty(K, dtype=np.float64)
    st = np.empty(K, dtype=np.int32)
    arr = (ctypes.c_void_p * len(ctxs))(*[c.h.value for c in ctxs])
    lib = ctxs[0].lib
    rc = lib.mioc_batch_multi(arr, len(ctxs), K, _p(df), _p(u_old), nx, nt, int(B), float(dt),
                              int(B if B_use is None else B_use), _p(u), _p(phi), _p(st))
    ctxs[0]._check(rc)
    return u, phi, st


def pyramid_eligible(levels: LevelTable):
    """Mirror of the library's L1-ball pyramid domain test (mioc_set_levels)."""
    if levels.L != int(np.prod(levels.counts)) or not (2 <= levels.M <= 6) or levels.L > 4096:
        return False
    if int(levels.counts[0]) not in (4, 8) or levels.L // int(levels.counts[0]) > 512:
        return False
    strides = np.cumprod(np.concatenate([[1], levels.counts[:-1]]))
    if not np.array_equal(((levels.tuples - 1) * strides).sum(axis=1), np.arange(levels.L)):
        return False
    return all(list(v) == list(range(v[0], v[0] + len(v))) for v in levels.nu)


def fused_eligible(L, B):
    """Mirror of the library's fused small-state domain (mioc_fused.hip fused_supported): L <= 64 levels, at
    most 192 (64-row block, target) tasks per step, and front + per-step tables within one CU's 160 KiB LDS."""
    if not (1 <= L <= 64) or B < 0:
        return False
    LP = next(x for x in (4, 8, 16, 24, 32, 36, 48, 64) if L <= x)
    R = B + 1
    nrb = (R + 63) // 64
    if nrb * L > 8 * 24:
        return False
    o = (R * (LP + 2) * 8 + 15) // 16 * 16 + 2 * L * LP * 8 + 2 * LP * 4 + 2 * 8 * 24 * 2
    return (o + 15) // 16 * 16 + 16 + L * 8 * 8 <= 160 * 1024


def fused_separable_eligible(levels: LevelTable, B):
    """Mirror of the library's fused separable domain (p = 1 and beta > 0 are checked by the library): a 2-D
    product grid of consecutive integer levels of shape 6x6, 4x4, 8x8 or 8x4, both fronts in one CU's LDS."""
    if levels.M != 2 or not (0 <= B < 512) or levels.L != int(np.prod(levels.counts)):
        return False
    n0, n1 = int(levels.counts[0]), int(levels.counts[1])
    if (n0, n1) not in ((6, 6), (4, 4), (8, 8), (8, 4)):
        return False
    FS = (n0 * n1 + 1) | 1  # two fronts of (B+1) rows + the per-step K table (double-buffered) in 160 KiB of LDS
    if 2 * (((B + 1) * FS * 8 + 15) // 16 * 16) + 2 * n0 * n1 * (n0 + n1 - 1) * 8 > 160 * 1024:
        return False
    strides = np.cumprod(np.concatenate([[1], levels.counts[:-1]]))
    if not np.array_equal(((levels.tuples - 1) * strides).sum(axis=1), np.arange(levels.L)):
        return False
    return all(list(v) == list(range(v[0], v[0] + len(v))) for v in levels.nu)


def separable_eligible(levels: LevelTable):
    """Mirror of the library's separable-transform domain (p = 1 and beta > 0 are checked by the library):
    the pyramid domain restricted to 8^3 and 8^4 grids."""
    return pyramid_eligible(levels) and levels.M in (3, 4) and all(int(c) == 8 for c in levels.counts)
