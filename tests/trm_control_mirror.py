"""Plain-Python restatement of the device-resident TRM control (csrc/mioc_trm.hip: k_trm_outer_begin, k_trm_inner_end,
k_trm_copy), written from multi-trust.jl:92-163 as mirrored in mioc/trm.py and from the contract in include/mioc.h
("Device-resident TRM control").  No GPU, no torch.

One Python float operation per reference operation, in the reference's order:
  pred = int_val + beta * (tvo - tvn)              multi-trust.jl:126
  ared = (J_old - J_new) + beta * (tvo - tvn)      :128
  pred <= 0 -> stop;  ared < sigma * pred -> halve;  else accept      :130, :140  (a NaN fails both tests: accept)
  Dk / 2                                           :142
  int(math.floor(Dk / tau))                        :109
mioc_trm.hip is built without floating-point contraction, so the device's values are these bit for bit.

A control state is a dict of numpy arrays Dk, tv_old (float64), k, flags, iters (int32), one entry per restart; the
functions update it (and J_old, J, tv_u, budgets) in place, as the kernels do.  tests/test_trm_control.py anchors this
file to the host loop mioc.TRM; tests/test_gpu_trm_control.py then judges the kernels by it.
"""
import math

import numpy as np

INNER, HALVED, STOP, COPY_U, COPY_UOLD = 1, 2, 4, 8, 16   # the flag bits (TRM_* of mioc_internal.h)
ACCEPT, HALVE, STOPPED, NOT_IN_LOOP = 0, 1, 2, -1          # decisions (mioc_trm_inner_end_device)
FIELDS = (("Dk", np.float64), ("tv_old", np.float64), ("k", np.int32), ("flags", np.int32), ("iters", np.int32))


def new_state(K):
    """The zero-initialised state of K restarts."""
    return {name: np.zeros(K, dtype=dt) for name, dt in FIELDS}


def copy_state(state):
    return {name: state[name].copy() for name, _ in FIELDS}


def outer_begin_host(state, tv_u, D0, B):
    """The start of an outer iteration (multi-trust.jl:99-107): TV_old = TV_p(u), Δᵏ = Δ⁰, k = 1, and every restart
    that has not stopped enters its inner loop with the full budget.  Returns (budgets, None, (gate, any_active,
    any_copy)): every restart's budget is B; there is no decision."""
    K = len(state["flags"])
    any_active = 0
    for r in range(K):
        f = int(state["flags"][r])
        active = not f & STOP
        state["tv_old"][r] = tv_u[r]
        state["Dk"][r] = D0
        state["k"][r] = 1
        state["flags"][r] = INNER if active else STOP
        if active:
            state["iters"][r] += 1
            any_active = 1
    return np.full(K, B, dtype=np.int32), None, (any_active, any_active, 0)


def inner_end_host(state, beta, sigma, kmax, tau, B, int_val, tv_new, J_new, J_old, J, tv_u, budgets):
    """The end of an inner iteration (multi-trust.jl:117-158) for every restart inside its inner loop; the others
    keep everything but lose their copy bits.  J_old, J, tv_u and budgets (the budgets of the trial just made) are
    updated in place.  Returns (budgets, decision, (gate, any_active, any_copy))."""
    K = len(state["flags"])
    decision = np.full(K, NOT_IN_LOOP, dtype=np.int32)
    gate = any_active = any_copy = 0
    for r in range(K):
        f = int(state["flags"][r]) & ~(COPY_U | COPY_UOLD)
        if f & INNER:
            tvo, tvn = float(state["tv_old"][r]), float(tv_new[r])
            pred = float(int_val[r]) + beta * (tvo - tvn)
            ared = (float(J_old[r]) - float(J_new[r])) + beta * (tvo - tvn)
            f |= COPY_U                       # obj.x = the trial, accepted or not
            tv_u[r] = tv_new[r]
            if pred <= 0:                     # stop: J = J_old
                d = STOPPED
                J[r] = J_old[r]
                f = (f | STOP) & ~INNER
            elif ared < sigma * pred:         # bad step: halve Δᵏ
                d = HALVE
                state["Dk"][r] = float(state["Dk"][r]) / 2
                f |= HALVED
            else:                             # good step: accept
                d = ACCEPT
                f |= COPY_UOLD
                J_old[r] = J_new[r]
                J[r] = J_new[r]
                state["tv_old"][r] = tv_new[r]
                f &= ~INNER
            decision[r] = d
            k = int(state["k"][r]) + 1
            state["k"][r] = k
            if k > kmax:
                f &= ~INNER
            budgets[r] = int(math.floor(float(state["Dk"][r]) / tau)) if f & HALVED else B
            any_copy = 1
        state["flags"][r] = f
        gate |= 1 if f & INNER else 0
        any_active |= 0 if f & STOP else 1
    return budgets, decision, (gate, any_active, any_copy)


def copy_host(flags, trial, u, u_old):
    """k_trm_copy: the trial into u (COPY_U) and into u_old (COPY_UOLD), restart by restart, in place."""
    for r in range(len(flags)):
        if int(flags[r]) & COPY_U:
            u[r] = trial[r]
        if int(flags[r]) & COPY_UOLD:
            u_old[r] = trial[r]


def state_bytes(K):
    """mioc_trm_state_bytes: three words in a 16-byte header, then K entries of each field."""
    return 16 + K * sum(np.dtype(dt).itemsize for _, dt in FIELDS)


def pack_state(state, words=(0, 0, 0)):
    """The device state block (uint8 numpy array) of a state and the words (gate, any_active, any_copy)."""
    K = len(state["flags"])
    b = np.zeros(state_bytes(K), dtype=np.uint8)
    b[:12].view(np.int32)[:] = words
    o = 16
    for name, dt in FIELDS:
        n = K * np.dtype(dt).itemsize
        b[o:o + n].view(dt)[:] = state[name]
        o += n
    return b


def unpack_state(block, K):
    """(state, (gate, any_active, any_copy)) of a device state block read back as a uint8 numpy array."""
    b = np.ascontiguousarray(block, dtype=np.uint8)
    assert b.size == state_bytes(K), (b.size, K)
    state, o = {}, 16
    for name, dt in FIELDS:
        n = K * np.dtype(dt).itemsize
        state[name] = b[o:o + n].view(dt).copy()
        o += n
    return state, tuple(int(w) for w in b[:12].view(np.int32))


def bits(a):
    """A float64 array as its bit patterns, so that NaN == NaN and 0.0 != -0.0 under np.array_equal."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
