"""CPU tier of the device TRM control's restatement (tests/trm_control_mirror.py): it is anchored to the host loop
mioc.TRM (multi-trust.jl:53-170) here, never to the kernels it judges in tests/test_gpu_trm_control.py.

mioc.TRM runs on a scripted solver and a scripted objective that need no device: the solver's pred returns the
script's (int_val, TV_new), the objective's eval_f_helper its J_new, and the solver records every budget it is asked
for and, from the caller's frame, the (outer iteration, k, Δᵏ) of every trial.  The restatement runs all scripts as
one batch, driven exactly as TRM_batch drives the device: outer_begin, then up to kmax times inner_end in chunks, a
poll of the two words after each chunk.  Equal, script by script and bit for bit: the returned J + β·TV, the budgets
asked for, the number of outer iterations, and (Δᵏ, k) at every trial.  Every trial is a control of its own, so the
copy bits are anchored too: obj.x at the end and the u_old handed to every bellman_TRM! equal what copy_host leaves.
"""
import math
import sys
from collections import Counter

import numpy as np
import pytest

import mioc
from mioc.objective import AbstractObjectiveLazy

import trm_control_mirror as tm

BETA, SIGMA, D0, TAU, KMAX, MAXITER = 0.25, 0.5, 1.0, 0.1, 6, 4
NAN = math.nan


class Script:
    """J and TV of the start, then one (int_val, TV_new, J_new) per trial; `i` is the trial being made."""

    def __init__(self, J0, tv0, trials):
        self.J0, self.tv0, self.trials, self.i = float(J0), float(tv0), [tuple(map(float, t)) for t in trials], -1


def trial_control(i):
    """The control of a script's trial i: no two alike, none like the start."""
    return np.array([i + 1.0, -(i + 1.0)])


class ScriptedSolver:
    """The solver= of mioc.TRM: no DP, the script's numbers and a control of its own per trial; records the budgets,
    the u_old of every bellman_TRM! and the loop's own k and Δᵏ."""

    def __init__(self, script):
        self.s, self.budgets, self.trace, self.u_olds = script, [], [], []

    def bellman(self, df, u_old, B, dt):
        self.u_olds.append(np.array(u_old).ravel())

    def backtrack(self, B_use):
        self.budgets.append(int(B_use))
        return trial_control(self.s.i + 1).reshape(1, 2), 0.0

    def pred(self):
        loop = sys._getframe(1)                       # mioc.TRM calls solver.pred() itself: its locals are the loop's
        assert loop.f_code.co_name == "TRM"
        self.trace.append((loop.f_locals["it"], loop.f_locals["k"], loop.f_locals["Dk"]))
        self.s.i += 1
        iv, tvn, _ = self.s.trials[self.s.i]
        return iv, NAN, tvn, NAN


class ScriptedObj(AbstractObjectiveLazy):
    def __init__(self, script, tau):
        self.s, self.nt, self.nx, self.tau, self.V, self.iterator = script, 2, 1, tau, [[0, 1]], None
        self._init_fields(1, 2)

    def eval_f_helper(self, x, cache):
        return self.s.J0 if self.s.i < 0 else self.s.trials[self.s.i][2]

    def eval_df_helper(self):
        pass


def run_host(script, D0=D0, tau=TAU, kmax=KMAX, maxiter=MAXITER):
    """mioc.TRM on one script: (value, budgets, outer iterations, [(it, k, Δᵏ) per trial], obj.x at the end, the
    u_old of every bellman_TRM!)."""
    script.i = -1
    obj, solver = ScriptedObj(script, tau), ScriptedSolver(script)
    par = mioc.TRM_parameters(beta=BETA, p=1, Delta0=D0, sigma=SIGMA, kmax=kmax, maxiter=maxiter)
    x0 = np.array([[0.0, script.tv0]])                # TV_p(x0, 1) = |tv0 - 0| = tv0 exactly
    value = mioc.TRM(obj, par, x0=x0, solver=solver)
    # one eval_df! per outer iteration and a last one
    return value, solver.budgets, obj.df_evals - 1, solver.trace, obj.x.ravel().copy(), solver.u_olds


def run_mirror(scripts, D0=D0, tau=TAU, kmax=KMAX, maxiter=MAXITER, inner_chunk=2, count=None):
    """The restatement on all scripts as one batch, as TRM_batch drives the device.  Per script the same tuple as
    run_host.  count: a Counter to receive the coverage."""
    K = len(scripts)
    B = int(math.floor(D0 / tau))
    state = tm.new_state(K)
    J_old = np.array([s.J0 for s in scripts])
    tv_u = np.array([s.tv0 for s in scripts])
    J = np.full(K, math.inf)
    u = np.array([[0.0, s.tv0] for s in scripts])
    u_old = u.copy()
    nxt = [0] * K
    asked, trace, u_olds = [[] for _ in range(K)], [[] for _ in range(K)], [[] for _ in range(K)]
    it = 1
    while it <= maxiter:
        budgets, _, words = tm.outer_begin_host(state, tv_u, D0, B)
        for r in np.flatnonzero(state["flags"] & tm.INNER):   # bellman_TRM! of the restarts in this outer iteration
            u_olds[r].append(u_old[r].copy())
        done = 0
        while done < kmax:
            for _ in range(min(inner_chunk, kmax - done)):
                iv, tvn, Jn = np.full(K, NAN), np.full(K, NAN), np.full(K, NAN)   # ignored outside the inner loop
                trial = np.full((K, 2), NAN)
                for r in range(K):
                    if state["flags"][r] & tm.INNER:
                        iv[r], tvn[r], Jn[r] = scripts[r].trials[nxt[r]]
                        trial[r] = trial_control(nxt[r])
                        nxt[r] += 1
                        asked[r].append(int(budgets[r]))
                        trace[r].append((it, int(state["k"][r]), float(state["Dk"][r])))
                k_before = state["k"].copy()
                budgets, dec, words = tm.inner_end_host(state, BETA, SIGMA, kmax, tau, B, iv, tvn, Jn, J_old, J, tv_u,
                                                        budgets)
                tm.copy_host(state["flags"], trial, u, u_old)
                done += 1
                if count is not None:
                    for r in np.flatnonzero(dec >= 0):
                        count["k=%d d=%d" % (k_before[r], dec[r])] += 1
                        count["stop in outer 1" if it == 1 else "stop in a later outer"] += int(dec[r] == tm.STOPPED)
                        count["NaN int_val"] += int(math.isnan(iv[r]))
                        count["NaN TV_new"] += int(math.isnan(tvn[r]))
                        count["NaN J_new"] += int(math.isnan(Jn[r]))
                        count["budget 0 next"] += int(dec[r] == tm.HALVE and budgets[r] == 0)
                        count["left the loop halved at kmax"] += int(dec[r] == tm.HALVE and k_before[r] == kmax)
            inner, active = words[0], words[1]        # the poll
            if not inner:
                break
        it += 1
        if not active:
            break
    values = [float(J[r]) + BETA * float(tv_u[r]) for r in range(K)]
    return [(values[r], asked[r], int(state["iters"][r]), trace[r], u[r], u_olds[r]) for r in range(K)]


# trials of a constant TV: pred = int_val, ared = J_old - J_new
def _accept(J_old):
    return (1.0, 2.0, J_old - 1.0)


def _halve(J_old):
    return (1.0, 2.0, J_old)


def _stop(J_old):
    return (-1.0, 2.0, J_old)


def constructed_scripts():
    """Every decision at every k in 1..KMAX, in the first outer iteration and in the second: k - 1 halvings, then the
    decision; stops behind it."""
    out = []
    for later in (False, True):
        for k in range(1, KMAX + 1):
            for make in (_accept, _halve, _stop):
                J_old, trials = 5.0, []
                if later:
                    trials.append(_accept(J_old))
                    J_old -= 1.0
                trials += [_halve(J_old)] * (k - 1) + [make(J_old)]
                if make is _accept:
                    J_old -= 1.0
                trials += [_stop(J_old)] * (KMAX * MAXITER - len(trials))
                out.append(Script(5.0, 2.0, trials))
    return out


def random_scripts(n, seed):
    out = []
    rng = np.random.default_rng(seed)
    for _ in range(n):
        J0, trials = float(rng.normal() * 3), []
        for i in range(KMAX * MAXITER):
            c = rng.random()
            iv = -abs(rng.normal()) if c < 0.06 else 0.0 if c < 0.08 else -0.0 if c < 0.10 else NAN if c < 0.13 \
                else rng.uniform(0.0, 2.0)
            tvn = NAN if rng.random() < 0.03 else float(rng.integers(0, 6))
            Jn = NAN if rng.random() < 0.03 else J0 - 0.4 * i + rng.normal()
            trials.append((iv, tvn, Jn))
        out.append(Script(J0, float(rng.integers(0, 6)), trials))
    return out


def _same(host, mirror):
    (hv, hb, hi, ht, hx, ho), (mv, mb, mi, mt, mx, mo) = host, mirror
    return bool(np.array_equal(tm.bits([hv]), tm.bits([mv]))) and hb == mb and hi == mi and ht == mt and \
        np.array_equal(tm.bits(hx), tm.bits(mx)) and len(ho) == len(mo) and \
        all(np.array_equal(tm.bits(a), tm.bits(b)) for a, b in zip(ho, mo))


@pytest.mark.parametrize("inner_chunk", [1, 2, KMAX])
def test_restatement_equals_host_loop(inner_chunk):
    scripts = constructed_scripts() + random_scripts(300, seed=20)
    count = Counter()
    mirror = run_mirror(scripts, inner_chunk=inner_chunk, count=count)
    for r, s in enumerate(scripts):
        host = run_host(s)
        assert _same(host, mirror[r]), (r, host, mirror[r])
    print("coverage:", dict(sorted(count.items())))
    for k in range(1, KMAX + 1):
        for d in (tm.ACCEPT, tm.HALVE, tm.STOPPED):
            assert count["k=%d d=%d" % (k, d)] >= 2, (k, d)
    for what in ("stop in outer 1", "stop in a later outer", "NaN int_val", "NaN TV_new", "NaN J_new",
                 "budget 0 next", "left the loop halved at kmax"):
        assert count[what] >= 1, what
    assert any(0 in m[1] for m in mirror)             # a trial was made with budget 0
    assert {m[2] for m in mirror} == set(range(1, MAXITER + 1))


def test_floor_cases():
    """B = floor(Δ⁰/Δt) and B_new = floor(Δᵏ/Δt): an exact integer quotient, a quotient one ulp below an integer,
    and 0."""
    halvings = Script(5.0, 2.0, [_halve(5.0)] * 5)
    for run in (lambda s, **kw: run_host(s, **kw), lambda s, **kw: run_mirror([s], **kw)[0]):
        _, budgets, _, trace = run(halvings, D0=1.0, tau=0.1, kmax=5, maxiter=1)[:4]
        assert budgets == [10, 5, 2, 1, 0]            # 1 / 0.1 = 10 and 0.5 / 0.1 = 5 exactly; 0.0625 / 0.1 < 1
        assert [t[2] for t in trace] == [1.0, 0.5, 0.25, 0.125, 0.0625]
        assert 0.3 / 0.1 < 3.0 and 0.6 / 0.1 < 6.0    # 2.9999999999999996 and 5.999999999999999
        _, budgets, _, trace = run(halvings, D0=0.6, tau=0.1, kmax=2, maxiter=1)[:4]
        assert budgets == [5, 2] and trace[1][2] == 0.3


def test_state_block_round_trip():
    rng = np.random.default_rng(1)
    K = 7
    st = {"Dk": rng.random(K), "tv_old": rng.random(K), "k": rng.integers(1, 9, K).astype(np.int32),
          "flags": rng.integers(0, 32, K).astype(np.int32), "iters": rng.integers(0, 9, K).astype(np.int32)}
    block = tm.pack_state(st, (1, 0, 1))
    assert block.size == 16 + 28 * K                  # include/mioc.h, mioc_trm_state_bytes
    back, words = tm.unpack_state(block, K)
    assert words == (1, 0, 1) and all(np.array_equal(back[n], st[n]) for n in st)
