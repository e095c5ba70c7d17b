"""CPU tier of the mixed trust-region method (mioc.trm_mixed): the host loop TRM_mixed on the mixed
Lotka-Volterra problem of tests/ode_mixed_problem.py with the CPU oracle as subproblem solver, the plain-Python
restatements of the fan and select kernels on hand-made inputs, rand_start_cont against np.convolve, argument checks,
and the compile of the mixed program (hiprtc needs no GPU)."""
import math

import numpy as np
import pytest

import mioc
from mioc.iterators import LevelTable
from mioc.trm_mixed import (MixedParameters, MixedState, TRM_mixed, TRM_mixed_batch, cont_noise, fan_host,
                            rand_start_cont, select_host)

import ode_mixed_problem as mixed


class OracleSolver:
    """Test double (the pattern of tests/test_host.py): the CPU oracle behind the SubproblemSolver interface."""

    def __init__(self, levels, p, beta):
        from oracle.oracle import OracleC, Levels, P_INF, P_ONE
        self.oc = OracleC()
        self.lv = Levels(levels.nu, [tuple(t) for t in levels.tuples])
        self.pk = P_INF if p == math.inf else P_ONE
        self.beta = beta

    def bellman(self, df, u_old, B, dt):
        self.df, self.dt = np.array(df, copy=True), dt
        self.uo = np.array(u_old, order="F", copy=True)
        self.B = B
        self.phi, self.U = self.oc.bellman(self.lv, df, u_old, B, self.pk, self.beta, dt)

    def backtrack(self, B_use):
        self.u, phi = self.oc.backtrack(self.lv, self.uo, self.phi, self.U, self.B, B_use)
        return self.u, phi

    def pred(self):
        from oracle.oracle import pred_py, tv_p_kind
        to, tn = tv_p_kind(self.uo, self.pk), tv_p_kind(self.u, self.pk)
        iv, pr = pred_py(self.df, self.uo, self.u, self.dt, self.beta, to, tn)
        return iv, to, tn, pr


# the parameters of the end-to-end runs, here and in test_gpu_mixed.py (which asserts what this seed gives)
E2E = dict(K=6, nt=96, seed=3, par=dict(beta=0.8, Delta0=2.0, p=1, maxiter=6, kmax=3),
           cpar=dict(s0=4.0, R=4, ctol=1e-9))


def run_mirror(obj, x0, par, cpar, solver):
    stats = {}
    val = TRM_mixed(obj, par, cpar, x0=x0, solver=solver, stats=stats)
    return val, stats


def assert_not_vacuous(rows, K):
    """rows: per restart (csteps, the jsel of every outer iteration, v changed, stop flags cleared)."""
    js = [j for r in rows for j in r[1] if j is not None]
    assert all(r[0] >= 1 for r in rows), "an accepted continuous step in every restart"
    assert any(j >= 1 for j in js) and any(j == 0 for j in js), "candidates j = 0 and j >= 1 both chosen"
    assert 2 * sum(bool(r[2]) for r in rows) >= K, "v changed in at least half of the restarts"
    assert any(r[3] >= 1 for r in rows), "a continuous step cleared a DP's stop flag"


def test_e2e_seed_is_not_vacuous_on_host():
    """The seed of test_gpu_mixed.py's end-to-end comparison, chosen here: the host objective and the CPU oracle take
    the path that the GPU test asserts for the device program."""
    K, nt = E2E["K"], E2E["nt"]
    par, cpar = mioc.TRM_parameters(**E2E["par"]), MixedParameters(**E2E["cpar"])
    x0 = mixed.start(K, nt, E2E["seed"])
    rows = []
    for k in range(K):
        obj = mixed.MixedLVObj(nt=nt)
        _, st = run_mirror(obj, x0[k].T, par, cpar, OracleSolver(LevelTable(obj.V, obj.iterator), par.p, par.beta))
        rows.append((st["csteps"], st["jsel"], not np.array_equal(obj.x[mixed.NU:], x0[k, :, mixed.NU:].T),
                     st["stop_cleared"]))
    assert_not_vacuous(rows, K)


def test_trm_mixed_host_runs_to_finality():
    nt = 48
    obj = mixed.MixedLVObj(nt=nt)
    par = mioc.TRM_parameters(beta=2e-3, Delta0=1.0, p=1, maxiter=150, kmax=6)
    cpar = MixedParameters(s0=4.0, R=8, ctol=1e-5)
    x0 = mixed.start(1, nt, 11)[0].T
    J0 = mioc.eval_f(obj, np.asfortranarray(x0)) + par.beta * mioc.TV_p(x0[mixed.NU:], par.p)
    solver = OracleSolver(LevelTable(obj.V, obj.iterator), par.p, par.beta)
    val, st = run_mirror(obj, x0, par, cpar, solver)
    lo, hi = mixed.bounds(nt)
    c, v = obj.x[:mixed.NU], obj.x[mixed.NU:]
    assert np.all(c >= lo.T) and np.all(c <= hi.T)
    assert np.all(np.isin(v, mixed.V[0]))
    assert not np.array_equal(obj.x, x0) and st["csteps"] >= 1 and st["iters"] >= 1
    vals = [J0] + st["values"]
    # each part's step is accepted on a decrease computed in floating point ((J_old - J_new) + beta (TV_old - TV_new)
    # > 0, or the Armijo test); J_old + beta TV is rounded once more, so two ulps are allowed
    for a, b in zip(vals, vals[1:]):
        assert b <= a * (1 + 2 * 2.0 ** -52), (a, b)
    assert val == vals[-1] and val < J0
    assert st["final"] or st["outer"] < par.maxiter     # ended by finality (or by "no part can move"), not by maxiter
    assert st["outer"] < par.maxiter
    print(f"host mixed TRM: {J0:.6f} -> {val:.6f} in {st['outer']} outer iterations, {st['csteps']} continuous steps")


def test_fan_host_hand_made():
    x = np.array([[0.5, 2.0], [0.9, 1.0], [0.1, 0.0]])
    g = np.array([[1.0, 7.0], [-1.0, 7.0], [0.25, 7.0]])
    lo, hi = np.zeros((3, 1)), np.ones((3, 1))
    xfan, slope = fan_host(x, g, lo, hi, 1.0, 3, 1, 0.5)
    # j = 0, s = 1: 0.5 - 1 -> lo; 0.9 + 1 -> hi; 0.1 - 0.25 -> lo.  The integer column is copied.
    assert np.array_equal(xfan[0], [[0.0, 2.0], [1.0, 1.0], [0.0, 0.0]])
    assert slope[0] == 0.5 * (((0.0 + 1.0 * 0.5) + -1.0 * (0.9 - 1.0)) + 0.25 * 0.1)
    # j = 1, s = 1/2: 0.5 - 0.5 = 0 (interior, on lo); 0.9 + 0.5 -> hi; 0.1 - 0.125 -> lo
    assert np.array_equal(xfan[1][:, 0], [0.0, 1.0, 0.0])
    # j = 2, s = 1/4: 0.25 interior; 1.15 -> hi; 0.0375 interior
    assert np.array_equal(xfan[2][:, 0], [0.25, 1.0, 0.1 - 0.25 * 0.25])
    xn = x.copy()
    xn[1, 0] = math.nan
    xf, sl = fan_host(xn, g, lo, hi, 1.0, 1, 1, 0.5)
    assert math.isnan(xf[0][1, 0]) and math.isnan(sl[0])    # a NaN stays a NaN


def _sel(st, stop, slope, Jfan, J_old=10.0, R=3, c1=0.5, smax=6.0, ctol=1e-3):
    return select_host(st, stop, np.array(slope, dtype=float), np.array(Jfan, dtype=float), J_old, R, c1, smax, ctol)


def test_select_host_branches():
    # first accepted j: j = 0 fails Armijo (9.6 > 10 - 0.5), j = 1 passes (9.0 <= 10 - 0.25), j = 2 would too
    st = MixedState(2.0)
    assert _sel(st, False, [1.0, 0.5, 0.25], [9.6, 9.0, 8.0]) == (1, False, 9.0)
    assert (st.s, st.jsel, st.csteps, st.moved, st.final) == (2.0, 1, 1, True, False)   # s = min(2 * 2/2, 6)
    # the step update is capped by smax
    st = MixedState(4.0)
    assert _sel(st, False, [1.0, 1.0, 1.0], [9.0, 0.0, 0.0])[0] == 0 and st.s == 6.0
    # none accepted: s * 2^-R, jsel = -1, not moved
    st = MixedState(2.0)
    assert _sel(st, False, [1.0, 0.5, 0.25], [9.9, 9.9, 9.9]) == (-1, False, 10.0)
    assert (st.s, st.jsel, st.csteps, st.moved, st.final) == (0.25, -1, 0, False, False)
    # a NaN Jfan is skipped, a NaN slope too; slope == 0 is never accepted whatever J is
    st = MixedState(2.0)
    assert _sel(st, False, [1.0, math.nan, 0.25], [math.nan, 0.0, 9.0])[0] == 2
    st = MixedState(2.0)
    assert _sel(st, False, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])[0] == -1
    # accepted but not moved: the reduction is below ctol max(1, |J_old|)
    st = MixedState(2.0)
    assert _sel(st, False, [1e-3, 1.0, 1.0], [9.995, 0.0, 0.0], c1=1e-4) == (0, False, 9.995)
    assert st.moved is False and st.csteps == 1


def test_select_host_finality():
    # 1. a final restart is left alone
    st = MixedState(2.0)
    st.final = True
    assert _sel(st, True, [1.0] * 3, [0.0] * 3) == (-1, True, 10.0) and (st.s, st.csteps) == (2.0, 0)
    # 2. STOP and not moved in the previous call: final without a line search
    st = MixedState(2.0)
    assert _sel(st, True, [1.0] * 3, [0.0] * 3) == (-1, True, 10.0)
    assert st.final and (st.s, st.csteps) == (2.0, 0)
    # 4. STOP, moved before, moves again: the stop flag is cleared
    st = MixedState(2.0)
    st.moved = True
    assert _sel(st, True, [1.0] * 3, [0.0] * 3) == (0, False, 0.0) and not st.final and st.moved
    # 4. STOP, moved before, no candidate now: final
    st = MixedState(2.0)
    st.moved = True
    assert _sel(st, True, [1.0] * 3, [9.9] * 3) == (-1, True, 10.0) and st.final and not st.moved
    # 4. STOP, moved before, accepted below ctol: final, but the step is kept
    st = MixedState(2.0)
    st.moved = True
    assert _sel(st, True, [1e-3, 1.0, 1.0], [9.995, 0.0, 0.0], c1=1e-4) == (0, True, 9.995) and st.final


def test_rand_start_cont_matches_convolution():
    """Bound: every smoothed value is a sum of nt <= 64 products of O(1) noise with kernel weights that sum to 1; the
    matmul may add them in another order than np.convolve, an error of about nt 2^-53 relative to the values' scale;
    with a hundredfold margin 1e-12."""
    K, nt, nu, sigma, seed = 3, 64, 2, 9.0, 5
    lo = np.stack([np.zeros(nt), np.full(nt, -1.0)], axis=1)
    hi = np.stack([np.ones(nt), np.full(nt, 2.0)], axis=1)
    hi[:16, 0] = 0.6
    lo[40:, 1] = 0.5
    u = rand_start_cont(K, nt, lo, hi, sigma=sigma, seed=seed, device="cpu").numpy()
    assert u.shape == (K, nt, nu) and np.all(u >= lo) and np.all(u <= hi)
    xi = cont_noise(K, nu, nt, seed).numpy()
    gauss = np.array([math.exp(-((i - nt / 2) ** 2) / (2 * sigma ** 2)) for i in range(1, nt + 1)])
    gauss = gauss / gauss.sum()
    clipped = 0
    for k in range(K):
        for m in range(nu):
            full = np.convolve(xi[k, m], gauss)
            s = int(math.floor((len(full) - nt) / 2) + 1)           # HelpFunctions.jl:169, 1-based
            w = full[s - 1:s - 1 + nt]
            r = lo[:, m].min() + (hi[:, m].max() - lo[:, m].min()) * (w - w.min()) / (w.max() - w.min())
            clipped += int(np.sum((r > hi[:, m]) | (r < lo[:, m])))
            r = np.maximum(np.minimum(r, hi[:, m]), lo[:, m])
            assert np.max(np.abs(u[k, :, m] - r)) <= 1e-12 * (hi[:, m].max() - lo[:, m].min()), (k, m)
    assert clipped > 0      # the pointwise projection was needed
    assert np.array_equal(u, rand_start_cont(K, nt, lo, hi, sigma=sigma, seed=seed).numpy())
    assert not np.array_equal(u, rand_start_cont(K, nt, lo, hi, sigma=sigma, seed=seed + 1).numpy())


def test_argument_checks():
    for bad in (dict(R=0), dict(R=17), dict(R=2.5), dict(c1=0.0), dict(c1=1.0), dict(s0=0.0), dict(s0=math.inf),
                dict(s0=2.0, smax=1.0), dict(ctol=-1.0)):
        with pytest.raises(ValueError):
            MixedParameters(**bad)
    assert MixedParameters().R == 8 and MixedParameters().c1 == 1e-4

    class Prog:  # MixedODEProblem reads only the shape of a program
        ny, nx, nparams = 2, 2, 3

    from mioc.ode_device import DeviceODEProblem, MixedODEProblem
    ok = dict(program=Prog(), nu=1, lo=0.0, hi=1.0, V=mixed.V, iterator=None, T0=0.0, T1=1.0, nt=8,
              state0=mixed.STATE0, params=mixed.PARAMS)
    mp = MixedODEProblem(**ok)
    assert mp.lo.shape == (8, 1) and mp.hi.shape == (8, 1)
    lo, hi = mixed.bounds(8)
    assert np.array_equal(MixedODEProblem(**{**ok, "lo": lo, "hi": hi}).hi, hi)
    assert MixedODEProblem(**{**ok, "hi": [0.5]}).hi.shape == (8, 1)
    for bad in (dict(nu=0), dict(nu=2), dict(V=[[0, 1]] * 2), dict(lo=2.0), dict(hi=np.ones((7, 1))),
                dict(lo=math.nan), dict(state0=[1.0]), dict(params=[]), dict(T1=0.0), dict(hi=np.ones(3))):
        with pytest.raises(ValueError):
            MixedODEProblem(**{**ok, **bad})
    with pytest.raises(ValueError, match="TRM_batch"):      # nu == 0 is TRM_batch's
        TRM_mixed_batch(DeviceODEProblem(Prog(), [[0, 1]] * 2, None, 0.0, 1.0, 8, mixed.STATE0, mixed.PARAMS), K=1)
    # the host objective: nu = 0 stays the default; bounds are needed and ordered
    from mioc.ode import AbstractODEObjective, LVMObj
    assert LVMObj(nt=8).nu == 0 and LVMObj(nt=8).nx == 3
    obj = mixed.MixedLVObj(nt=8)
    assert (obj.nu, obj.nv, obj.nx) == (1, 1, 2) and obj.umax.shape == (1, 8) and obj.x.shape == (2, 8)
    with pytest.raises(ValueError):
        AbstractODEObjective(0.0, 1.0, 8, mixed.V, None, mixed.STATE0, nu=1)
    with pytest.raises(ValueError):
        AbstractODEObjective(0.0, 1.0, 8, mixed.V, None, mixed.STATE0, nu=1, umin=1.0, umax=0.0)
    with pytest.raises(ValueError, match="nu >= 1"):
        TRM_mixed(LVMObj(nt=8), x0=np.zeros((3, 8)))
    with pytest.raises(ValueError):                         # a start outside the bounds
        TRM_mixed(obj, x0=np.full((2, 8), 2.0), solver=object())


def test_mixed_programs_compile():
    from mioc.ode_device import ODEProgram
    with ODEProgram(mixed.SOURCE, mixed.NY, mixed.NX, len(mixed.PARAMS), derive="all") as p:
        assert p.h and p.derive == ("Fy", "Fu", "Gy", "Gu")
    with ODEProgram(mixed.KA_SOURCE, mixed.KA_NY, mixed.KA_NX, 0, integrator="rk4", substeps=2, derive="all") as p:
        assert p.h
