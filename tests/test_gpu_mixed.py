"""GPU tier of mixed controls (include/mioc.h, "Mixed controls"; mioc.trm_mixed): the row copy around the DP, the
mixed eval entry, the fan and select kernels bit for bit against their plain-Python restatements (fan_host,
select_host), mioc_mixed_poll, a known-answer line search, and TRM_mixed_batch against the host loop TRM_mixed restart
by restart, bit for bit."""
import math

import numpy as np
import pytest

import mioc
from mioc import native
from mioc.iterators import LevelTable
from mioc.ode_device import MixedODEProblem, ODEProgram
from mioc.trm_mixed import MixedParameters, MixedState, TRM_mixed, TRM_mixed_batch, fan_host, select_host

import ode_mixed_problem as mixed
from ode_gpu_support import program_objective
from test_mixed_host import E2E, assert_not_vacuous

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def programs():
    progs = {"lv": ODEProgram(mixed.SOURCE, mixed.NY, mixed.NX, len(mixed.PARAMS), derive="all"),
             "ka": ODEProgram(mixed.KA_SOURCE, mixed.KA_NY, mixed.KA_NX, 0, integrator="rk4", substeps=2,
                              derive="all")}
    yield progs
    for p in progs.values():
        p.close()


def _dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def _sync():
    import torch
    torch.cuda.synchronize()


def _mstate(K, s, flags, jsel=None, csteps=None):
    """A mixed state block from host arrays (the layout of mioc_mixed_state_bytes)."""
    import torch
    b = np.zeros(16 + 20 * K, dtype=np.uint8)
    b[16:16 + 8 * K].view(np.float64)[:] = s
    iv = b[16 + 8 * K:].view(np.int32)
    iv[:K] = flags
    iv[K:2 * K] = 0 if jsel is None else jsel
    iv[2 * K:] = 0 if csteps is None else csteps
    return torch.from_numpy(b).cuda()


def _trm_state(K, flags, gate=0):
    """A TRM state block from host arrays (the layout of mioc_trm_state_bytes): the gate word and the flags."""
    import torch
    b = np.zeros(16 + 28 * K, dtype=np.uint8)
    b[:4].view(np.int32)[0] = gate
    b[16 + 20 * K:16 + 24 * K].view(np.int32)[:] = flags
    return torch.from_numpy(b).cuda()


def _trm_flags(t, K):
    return t.cpu().numpy()[16 + 20 * K:16 + 24 * K].view(np.int32).copy()


# ---- mioc_rows_copy_device -------------------------------------------------------------------------------------------
def test_rows_copy_split_join_inplace_gate():
    import torch
    K, nt, nx, nu = 3, 5, 3, 1
    rng = np.random.default_rng(0)
    x = _dev(rng.standard_normal((K, nt, nx)))
    with native.Context(0) as ctx:
        c = torch.full((K, nt, nu), math.nan, dtype=torch.float64, device="cuda")
        v = torch.full((K, nt, nx - nu), math.nan, dtype=torch.float64, device="cuda")
        y = torch.full_like(x, math.nan)
        _sync()
        ctx.rows_copy_tensors(c, 0, x, 0, nu)               # split
        ctx.rows_copy_tensors(v, 0, x, nu, nx - nu)
        ctx.rows_copy_tensors(y, 0, c, 0, nu)               # join
        ctx.rows_copy_tensors(y, nu, v, 0, nx - nu)
        ctx.synchronize()
        assert torch.equal(c, x[:, :, :nu]) and torch.equal(v, x[:, :, nu:]) and torch.equal(y, x)
        z = x.clone()
        _sync()
        ctx.rows_copy_tensors(z, 2, z, 0, 1)                # in place, disjoint rows
        ctx.synchronize()
        assert torch.equal(z[:, :, 2], x[:, :, 0]) and torch.equal(z[:, :, :2], x[:, :, :2])
        state = ctx.trm_state_tensor(K)                     # zero-initialised: the gate word is 0
        w = torch.full_like(x, math.nan)
        _sync()
        ctx.trm_attach(state)
        ctx.rows_copy_tensors(w, 0, x, 0, nx)
        ctx.synchronize()
        assert bool(torch.isnan(w).all())                   # a closed gate leaves dst untouched
        ctx.trm_attach(None)
        ctx.rows_copy_tensors(w, 0, x, 0, nx)
        ctx.synchronize()
        assert torch.equal(w, x)
        for args in ((y, 0, x, 2, 2), (y, 3, x, 0, 1), (c, 0, x, 0, 2), (y, -1, x, 0, 1), (y, 0, x, 0, 0),
                     (z, 1, z, 0, 2)):                      # ranges outside nx; overlapping rows in place
            with pytest.raises(native.MiocNativeError) as e:
                ctx.rows_copy_tensors(*args)
            assert e.value.code == native.MIOC_EINVAL


# ---- mioc_ode_program_eval_mixed_device ------------------------------------------------------------------------------
def test_eval_mixed_entry(programs):
    import torch
    K, nt = 70, 24
    x = _dev(mixed.start(K, nt, 1))
    prog = programs["lv"]

    def run(ctx, mixed_entry, nu=1):
        J = torch.full((K,), math.nan, dtype=torch.float64, device="cuda")
        df = torch.full_like(x, math.nan)
        _sync()
        if mixed_entry:
            ctx.ode_program_eval_mixed_tensors(prog, nu, x, 0.0, 3.0, mixed.STATE0, mixed.PARAMS, J, df)
        else:
            ctx.ode_program_eval_tensors(prog, x, 0.0, 3.0, mixed.STATE0, mixed.PARAMS, J, df)
        ctx.synchronize()
        return J, df

    with native.Context(0) as ctx:                          # no levels: both entries accept the program
        J0, df0 = run(ctx, False)
        J1, df1 = run(ctx, True)
        assert bool(torch.isfinite(J0).all()) and bool(torch.isfinite(df0).all())
        assert torch.equal(J0, J1) and torch.equal(df0, df1)
        ctx.set_levels(LevelTable(mixed.V))                 # M = 1 = nx - nu
        J2, df2 = run(ctx, True)
        assert torch.equal(J0, J2) and torch.equal(df0, df2)
        with pytest.raises(native.MiocNativeError):         # the integer-only entry still wants nx == M
            run(ctx, False)
        with pytest.raises(ValueError):                     # nu outside 1..nx-1
            run(ctx, True, nu=2)
        with pytest.raises(ValueError):
            run(ctx, True, nu=0)
        for nu in (0, 2):                                   # ... and the library's own check
            rc = ctx.lib.mioc_ode_program_eval_mixed_device(
                ctx.h, prog.h, nu, K, x.data_ptr(), nt, 0.0, 3.0, native._p(np.array(mixed.STATE0)),
                native._p(np.array(mixed.PARAMS)), None, None)
            assert rc == native.MIOC_EINVAL
        ctx.set_levels(LevelTable([[0, 1]] * 2))            # M = 2: nx != nu + M
        with pytest.raises(native.MiocNativeError) as e:
            run(ctx, True)
        assert e.value.code == native.MIOC_EINVAL


# ---- mioc_mixed_fan_device -------------------------------------------------------------------------------------------
def _fan_case(K, R, nt, nu, nx, seed, s):
    """Controls, gradients and bounds such that candidates are clamped at lo, at hi and stay interior."""
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-1.0, 0.0, size=(nt, nu))
    hi = lo + rng.uniform(0.5, 1.5, size=(nt, nu))
    x = np.empty((K, nt, nx))
    x[:, :, :nu] = lo + (hi - lo) * rng.random((K, nt, nu))
    x[:, :, nu:] = rng.integers(0, 3, size=(K, nt, nx - nu))
    g = rng.standard_normal((K, nt, nx)) * rng.choice([0.05, 1.0, 8.0], size=(K, nt, nx))
    return x, g, lo, hi, np.asarray(s, dtype=np.float64)


@pytest.mark.parametrize("K,R,nt,nu,nx", [(3, 4, 7, 2, 3), (2, 2, native.mixed_fan_chunk(1) + 3, 1, 2)])
def test_fan_bit_for_bit(K, R, nt, nu, nx):
    """The second case has nt nu three past the kernel's LDS chunk, so the sequential sum crosses a chunk boundary; its
    nt nx is even (the 16-byte path), the first case's is odd."""
    import torch
    tau = 0.37
    x, g, lo, hi, s = _fan_case(K, R, nt, nu, nx, 7, [1.0, 0.75, 3.0][:K])
    with native.Context(0) as ctx:
        ms = _mstate(K, s, 0)
        xfan = torch.full((R, K, nt, nx), math.nan, dtype=torch.float64, device="cuda")
        slope = torch.full((R, K), math.nan, dtype=torch.float64, device="cuda")
        dx, dg, dlo, dhi = _dev(x), _dev(g), _dev(lo), _dev(hi)
        _sync()
        ctx.mixed_fan_tensors(R, nu, tau, dx, dg, dlo, dhi, ms, xfan, slope)
        ctx.synchronize()
        xf, sl = xfan.cpu().numpy(), slope.cpu().numpy()
    at_lo = at_hi = inside = 0
    for k in range(K):
        hx, hs = fan_host(x[k], g[k], lo, hi, float(s[k]), R, nu, tau)
        assert np.array_equal(xf[:, k], hx), (k, np.argwhere(xf[:, k] != hx)[:4])
        assert np.array_equal(sl[:, k], hs), (k, sl[:, k], hs)
        c = hx[:, :, :nu]
        at_lo += int(np.sum((c == lo) & (x[k, :, :nu] != lo)))
        at_hi += int(np.sum((c == hi) & (x[k, :, :nu] != hi)))
        inside += int(np.sum((c > lo) & (c < hi)))
    assert at_lo and at_hi and inside and np.all(np.isfinite(sl))


# ---- mioc_mixed_select_device, mioc_mixed_poll -----------------------------------------------------------------------
STOP, FINAL, MOVED = 4, 1, 2
SELECT_CASES = [  # (s, mixed flags, DP stop flag, slope, Jfan, c1): J_old = 10, R = 3, smax = 6, ctol = 1e-3
    (2.0, 0, 0, [1.0, 0.5, 0.25], [9.6, 9.0, 8.0]),           # the first j that passes is 1
    (2.0, 0, 0, [1.0, 0.5, 0.25], [9.9, 9.9, 9.9]),           # none: s 2^-R
    (2.0, 0, 0, [1.0, math.nan, 0.25], [math.nan, 0.0, 9.0]),  # NaN never passes
    (2.0, 0, 0, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]),            # slope == 0 never passes
    (4.0, 0, 0, [1.0, 1.0, 1.0], [9.0, 0.0, 0.0]),            # 2 s_j capped by smax
    (2.0, 0, 0, [1e-3, 1.0, 1.0], [9.495, 0.0, 0.0]),         # accepted ... and moved
    (2.0, FINAL, STOP, [1.0] * 3, [0.0] * 3),                 # 1. final: left alone
    (2.0, FINAL | MOVED, 0, [1.0] * 3, [0.0] * 3),            # 1. final whatever the other flags
    (2.0, 0, STOP, [1.0] * 3, [0.0] * 3),                     # 2. STOP and not moved: final
    (2.0, MOVED, STOP, [1.0] * 3, [0.0] * 3),                 # 4. moves again: STOP cleared
    (2.0, MOVED, STOP, [1.0] * 3, [9.9] * 3),                 # 4. no candidate: final
    (2.0, MOVED, STOP, [1.0, 1.0, 1.0], [9.499, 9.499, 0.0]),  # 4. accepted j = 0 ... and moved
    (2.0, MOVED, 0, [1.0] * 3, [9.9] * 3),                    # not STOP, nothing accepted: moved cleared, not final
]


@pytest.mark.parametrize("ctol", [1e-3, 0.2])
def test_select_every_branch(ctol):
    """ctol = 0.2: the accepted steps that reduce J by 0.5 have not moved (0.5 <= 0.2 * 10)."""
    import torch
    K, R, nt, nu, nx = len(SELECT_CASES), 3, 5, 2, 3
    c1, smax, J0 = 0.5, 6.0, 10.0
    rng = np.random.default_rng(3)
    x, xfan = rng.standard_normal((K, nt, nx)), rng.standard_normal((R, K, nt, nx))
    s = np.array([c[0] for c in SELECT_CASES])
    mf = np.array([c[1] for c in SELECT_CASES], dtype=np.int32)
    tf = np.array([c[2] | 8 for c in SELECT_CASES], dtype=np.int32)    # another TRM flag bit, which must survive
    slope = np.array([c[3] for c in SELECT_CASES]).T.copy()
    Jfan = np.array([c[4] for c in SELECT_CASES]).T.copy()
    with native.Context(0) as ctx:
        ms, ts = _mstate(K, s, mf, jsel=7, csteps=5), _trm_state(K, tf, gate=1)
        dx, dJ = _dev(x), _dev(np.full(K, J0))
        dxfan, dslope, dJfan = _dev(xfan), _dev(slope), _dev(Jfan)
        _sync()
        ctx.mixed_select_tensors(R, nu, c1, smax, ctol, ms, ts, dxfan, dslope, dJfan, dJ, dx)
        gate, live = ctx.mixed_poll(ms, ts)
        got = ctx.mixed_state_arrays(ms, K)
        gx, gJ, gtf = dx.cpu().numpy(), dJ.cpu().numpy(), _trm_flags(ts, K)
    seen = set()
    any_live = False
    for k in range(K):
        st = MixedState(s[k])
        st.final, st.moved, st.jsel, st.csteps = bool(mf[k] & FINAL), bool(mf[k] & MOVED), 7, 5
        j, stop, J = select_host(st, bool(tf[k] & STOP), slope[:, k], Jfan[:, k], J0, R, c1, smax, ctol)
        want = x[k].copy()
        if j >= 0:
            want[:, :nu] = xfan[j, k, :, :nu]
        assert np.array_equal(gx[k], want), k
        assert gJ[k] == J and got["s"][k] == st.s and got["jsel"][k] == st.jsel and got["csteps"][k] == st.csteps, k
        assert got["flags"][k] == (FINAL if st.final else 0) | (MOVED if st.moved else 0), (k, got["flags"][k])
        assert gtf[k] == (STOP if stop else 0) | 8, (k, gtf[k])
        any_live |= not st.final and (not stop or st.moved)
        seen.add((bool(mf[k] & FINAL), bool(tf[k] & STOP), bool(mf[k] & MOVED), j >= 0, st.moved, st.final, stop))
    assert gate is True and live is any_live and live
    assert len(seen) >= 8                                    # the cases reach distinct branches
    # the any-live word is 0 when every restart is final or has stopped without a move
    with native.Context(0) as ctx:
        ms, ts = _mstate(2, [1.0, 1.0], [FINAL, 0]), _trm_state(2, [0, STOP], gate=0)
        z = _dev(np.zeros((3, 2)))
        dx, dxfan, dJ = _dev(np.zeros((2, nt, nx))), _dev(np.zeros((3, 2, nt, nx))), _dev(np.zeros(2))
        with pytest.raises(native.MiocNativeError) as e:    # no select has run on this block yet
            ctx.mixed_poll(ms, ts)
        assert e.value.code == native.MIOC_ESTATE
        _sync()
        ctx.mixed_select_tensors(3, nu, c1, smax, ctol, ms, ts, dxfan, z, z, dJ, dx)
        assert ctx.mixed_poll(ms, ts) == (False, False)
        assert ctx.mixed_state_arrays(ms, 2)["flags"].tolist() == [FINAL, FINAL]


# ---- known answer ----------------------------------------------------------------------------------------------------
def test_known_answer_step(programs):
    """G = (c - ct(i))^2 integrated by RK4: J = tau sum (c - ct)^2 and dJ/dc = 2 (c - ct) up to rounding.  With
    s0 = 1 candidate 0 reflects c about ct (J unchanged: the Armijo test fails), candidate 1 lands on ct up to a few
    ulps of O(1) values, clamped where ct is outside [0, 1]."""
    import torch
    K, nt, R = 4, 32, 4
    T1 = 0.05 * nt
    x0 = mixed.ka_start(K, nt, 2)
    ct = mixed.ka_ct(nt)
    prob = MixedODEProblem(programs["ka"], 1, 0.0, 1.0, mixed.KA_V, None, 0.0, T1, nt, mixed.KA_STATE0)
    with native.Context(0) as ctx:                          # the candidates themselves
        dx = _dev(x0)
        g, J = torch.empty_like(dx), torch.empty(K, dtype=torch.float64, device="cuda")
        xfan = torch.empty(R, K, nt, 2, dtype=torch.float64, device="cuda")
        slope, Jfan = (torch.empty(R, K, dtype=torch.float64, device="cuda") for _ in range(2))
        ms = ctx.mixed_state_tensor(K, 1.0)
        _sync()
        prob.eval_tensors(ctx, dx, J, g)
        ctx.mixed_fan_tensors(R, 1, T1 / nt, dx, g, _dev(prob.lo), _dev(prob.hi), ms, xfan, slope)
        prob.eval_tensors(ctx, xfan.view(R * K, nt, 2), Jfan, None)
        ctx.synchronize()
        Jh, Jf, sl, xf = J.cpu().numpy(), Jfan.cpu().numpy(), slope.cpu().numpy(), xfan.cpu().numpy()
    inside = (ct >= 0.0) & (ct <= 1.0)
    assert np.max(np.abs(xf[0][:, inside, 0] - (2 * ct[inside] - x0[:, inside, 0]))) <= 1e-12       # the reflection
    assert np.all(np.abs(Jf[0] - Jh) <= 1e-12 * Jh) and np.all(sl[0] > 0) and np.all(Jf[0] > Jh - 1e-4 * sl[0])
    assert np.max(np.abs(xf[1][:, :, 0] - np.clip(ct, 0.0, 1.0))) <= 1e-12
    assert np.all(Jf[1] <= Jh - 1e-4 * sl[1])
    par = mioc.TRM_parameters(beta=1e-3, Delta0=0.2, p=1, maxiter=1, kmax=1)
    stats = {}
    vals, x, iters = TRM_mixed_batch(prob, par, MixedParameters(s0=1.0, R=R), x0=_dev(x0), stats=stats)
    assert np.max(np.abs(x.cpu().numpy()[:, :, 0] - np.clip(ct, 0.0, 1.0))) <= 1e-12
    assert stats["jsel"].tolist() == [1] * K and stats["csteps"].tolist() == [1] * K
    assert stats["s"].tolist() == [1.0] * K                 # min(2 * s0 / 2, smax)
    assert iters.tolist() == [1] * K
    xv = x.cpu().numpy()[:, :, 1]                           # J does not depend on v: the value is J(c_1) + beta TV(v)
    assert [float(v) for v in vals] == [Jf[1][k] + par.beta * mioc.TV_p(xv[k][None], 1) for k in range(K)]


def test_random_starts_are_admissible_and_reproducible(programs):
    """x0 = None: rand_start_cont for c joined with the device's rand_func_int for v, from one seed."""
    K, nt = 5, 24
    lo, hi = mixed.bounds(nt)
    prob = MixedODEProblem(programs["lv"], mixed.NU, lo, hi, mixed.V, None, mixed.T0, 3.0, nt, mixed.STATE0, mixed.PARAMS)
    par = mioc.TRM_parameters(beta=1e-2, Delta0=0.5, p=1, maxiter=2, kmax=2)
    runs = [TRM_mixed_batch(prob, par, MixedParameters(R=3), K=K, seed=8) for _ in range(2)]
    other = TRM_mixed_batch(prob, par, MixedParameters(R=3), K=K, seed=9)
    for vals, x, iters in runs + [other]:
        xb = x.cpu().numpy()
        assert xb.shape == (K, nt, mixed.NX) and np.all(np.isfinite(vals)) and iters.shape == (K,)
        assert np.all(xb[:, :, 0] >= lo[:, 0]) and np.all(xb[:, :, 0] <= hi[:, 0])
        assert np.all(np.isin(xb[:, :, 1], mixed.V[0]))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1].cpu().numpy(), runs[1][1].cpu().numpy())
    assert not np.array_equal(runs[0][0], other[0])
    with pytest.raises(ValueError):
        TRM_mixed_batch(prob, par)                          # neither K nor x0


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_trm_mixed_batch_equals_host_loop(programs):
    K, nt = E2E["K"], E2E["nt"]
    par, cpar = mioc.TRM_parameters(**E2E["par"]), MixedParameters(**E2E["cpar"])
    x0 = mixed.start(K, nt, E2E["seed"])
    lo, hi = mixed.bounds(nt)
    prob = MixedODEProblem(programs["lv"], mixed.NU, lo, hi, mixed.V, None, mixed.T0, mixed.T1, nt, mixed.STATE0,
                           mixed.PARAMS)
    stats = {}
    vals, x, iters = TRM_mixed_batch(prob, par, cpar, x0=_dev(x0), stats=stats)
    xb = x.cpu().numpy()
    assert np.all(xb[:, :, 0] >= lo[:, 0]) and np.all(xb[:, :, 0] <= hi[:, 0]) and np.all(np.isin(xb[:, :, 1], mixed.V[0]))
    rows = []
    with native.Context(0) as ctx:
        for k in range(K):
            obj = program_objective(mixed.MixedLVObj(nt=nt), programs["lv"], ctx, mixed.STATE0, mixed.PARAMS,
                                    nu=mixed.NU, sync_torch=True)
            st = {}
            J = TRM_mixed(obj, par, cpar, x0=x0[k].T, stats=st)
            assert J == vals[k], (k, J, vals[k])
            assert np.array_equal(obj.x, xb[k].T), k
            assert st["iters"] == iters[k] and st["csteps"] == stats["csteps"][k], (k, st["iters"], iters[k])
            rows.append((st["csteps"], st["jsel"], not np.array_equal(xb[k, :, 1], x0[k, :, 1]), st["stop_cleared"]))
    assert_not_vacuous(rows, K)
    print(f"mixed: iterations per restart {iters.tolist()}, continuous steps {stats['csteps'].tolist()}, "
          f"polls {stats['polls']}")
