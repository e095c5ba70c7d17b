"""GPU parity of the one-target item of the persistent separable transform (k_sdt_run: a direct row with exactly one
target inside the trust region -- row B of every step, row B - 1 where u_old(i) is off the grid) against the CPU oracle;
the per-step driver (k_sdt_step, row B in block 0) beside it.  C4's β and Δt, p = 1; 8^4 levels unless noted:

  * exact ties across lanes and waves: zero gradients (every candidate of row B's target is a multiple of β) and
    integer gradients.  Before the GPU runs, the candidates (t1 + β·d(l0, j)) + Φ_1[B, j] of step 0 are formed in numpy in
    the reference's operation order from the oracle's two retained Φ buffers: their minimum is Φ_0[B, l0], at least two
    sources attain it, and U holds the lowest such rank.  B = 3 also puts geometric +Inf and seam placeholders among row
    B's sources;
  * row B over several consecutive items (B = 64, nt = 8, the u_old cycle of tests/test_gpu_c4_rows.py: the slot-reuse
    flag both 0 and 1): a one-row workgroup hands the head value from item to item;
  * u_old off the grid inside the dependency window, at step i, at step i + 1 and at both: row B is empty and row
    B - 1 has the one target; row B has no distance-0 source to take from its own previous output;
  * row B inside a two-row chunk (K = 2, B = 200, nt = 6, zero gradients): the next item is not row B;
  * the 8^3 grid (k_sdt_run<3>, one wave per workgroup): u_old at a corner makes row B - 1 a direct row with four
    targets (the whole-workgroup scan), u_old in the interior exercises the one-target item;
  * diagnostics [0], [1], [4], [5] of the steady Gaussian case equal the parent build's.

Every case: U equal wherever the oracle wrote it, u and Φ* equal at B' in {B, B // 2, 1}, kernel_stats(0)[2] the
expected kernel, diagnostics [6] == 0.
"""
import functools

import numpy as np
import pytest

from mioc import native
from mioc.iterators import LevelTable
from mioc.synth import CONFIGS, make_inputs
from oracle.oracle import P_ONE, Levels, OracleC, OracleError

pytestmark = pytest.mark.gpu

CFG = CONFIGS["C4"]
THREADS = 8  # the oracle's result does not depend on it
KERNEL = {"persistent": "k_sdt_run", "steps": "k_sdt_step"}
DRIVERS = ["persistent", "steps"]


@functools.lru_cache(maxsize=None)
def _levels(M=4):
    if M == 4:
        lt = CFG.levels()
        return lt, Levels(lt.nu, [tuple(int(x) for x in t) for t in lt.tuples])
    nu = [list(range(8))] * M
    return LevelTable(nu), Levels.product(nu)


def _cols(cols):
    return np.asfortranarray(np.array(cols, dtype=np.float64).T)


def _oracle(M, df, uo, B):
    return OracleC().bellman(_levels(M)[1], df, uo, B, P_ONE, CFG.beta, CFG.dt, threads=THREADS)


def _ctx(persist, M=4):
    ctx = native.Context(0)
    ctx.set_levels(_levels(M)[0])
    ctx.set_cost(1, CFG.beta)
    ctx.set_option(native.MIOC_OPT_TIMING, 1)
    ctx.set_option(native.MIOC_OPT_ALGO, native.MIOC_ALGO_SEPARABLE)
    ctx.set_option(native.MIOC_OPT_PERSIST, persist)
    return ctx


def _compare_tables(ctx, U, label, k=0):
    for i in range(U.shape[2]):
        d, o = ctx.argmin_table(i, k=k), U[:, :, i]
        m = o >= 0
        assert np.array_equal(d[m], o[m]), f"{label}: U at step {i}"


def _compare(ctx, oracle_c, lv, uo, phi, U, B, label):
    _compare_tables(ctx, U, label)
    for Bp in (B, B // 2, 1):
        try:
            ou, ops = oracle_c.backtrack(lv, uo, phi, U, B, Bp)
        except OracleError as e:  # no finite Φ_0 within B': the device says the same
            assert e.args == (native.MIOC_EINFEASIBLE,), e
            with pytest.raises(native.MiocNativeError) as err:
                ctx.backtrack(Bp)
            assert err.value.code == native.MIOC_EINFEASIBLE, f"{label}: B'={Bp}"
            continue
        u, ps, _ = ctx.backtrack(Bp)
        assert np.array_equal(u, ou) and ps == ops, f"{label}: B'={Bp}: {ps!r} vs {ops!r}"


def _run_case(oracle_c, df, uo, phi, U, B, driver, label, M=4):
    ctx = _ctx(int(driver == "persistent"), M)
    ctx.bellman(df, uo, B, CFG.dt)
    ctx.synchronize()
    assert ctx.kernel_stats(0)[2] == KERNEL[driver]
    diag = ctx.diagnostics()
    assert diag[6] == 0, diag
    _compare(ctx, oracle_c, _levels(M)[1], uo, phi, U, B, label)
    ctx.close()
    return diag


# ---- 1. ties across lanes and waves ----------------------------------------------------------------------------------
# (name, B, nt): zero gradients, and one integer draw (multiples of 4096, as test_gpu_c4_item.py's redo case)
TIES = [("zero", 60, 5), ("zero", 29, 4), ("zero", 3, 4), ("integer", 29, 4)]
INTEGER_SEED = 14  # eleven exact minimisers in row B of step 0 (ranks 176, 232, 240, ...: several lanes and waves)


@functools.lru_cache(maxsize=None)
def _tie_case(kind, B, nt):
    lt, lv = _levels()
    _, df, uo = make_inputs(CFG, nt=nt, levels=lt)
    if kind == "zero":
        df = np.zeros_like(df)
    else:
        df = np.asfortranarray(np.random.default_rng(INTEGER_SEED).integers(-3, 4, size=df.shape).astype(float) * 4096.0)
    phi, U = _oracle(4, df, uo, B)
    return df, uo, phi, U


def _row_b_minimisers(df, uo, phi, U, B):
    """Row B of step 0 by hand: the ranks whose candidate (t1 + β·d(l0, j)) + Φ_1[B, j] (the reference's operation order,
    HelpFunctions.jl:52-71) equals the minimum; asserts the minimum is Φ_0[B, l0] and U holds the lowest such rank."""
    _, lv = _levels()
    nuv = np.asarray(lv.nuval, dtype=np.int64)
    l0 = int(np.nonzero((nuv == uo[:, 0].astype(np.int64)).all(axis=1))[0][0])  # u_old(0) is a level: b̃ = 0
    t1 = 0.0
    for m in range(lv.M):
        t1 = t1 + (CFG.dt * float(df[m, 0])) * float(nuv[l0, m])
    d = np.abs(nuv - nuv[l0]).sum(axis=1).astype(np.float64)
    val = (t1 + CFG.beta * d) + phi[B, lv.gidx, 1]  # Φ_1 is the oracle's buffer 1, Φ_0 its buffer 0
    best = val.min()
    assert np.isfinite(best) and best == phi[B, lv.gidx[l0], 0], (best, phi[B, lv.gidx[l0], 0])
    ranks = np.nonzero(val == best)[0]
    assert U[B, lv.gidx[l0], 0] == ranks[0], (U[B, lv.gidx[l0], 0], ranks[:4])
    return ranks


@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("kind,B,nt", TIES, ids=[f"{k}-B{B}-nt{n}" for k, B, n in TIES])
def test_one_target_ties(oracle_c, kind, B, nt, driver):
    df, uo, phi, U = _tie_case(kind, B, nt)
    ranks = _row_b_minimisers(df, uo, phi, U, B)
    assert len(ranks) >= 2, "row B's target has a unique minimiser: the tie rule is not exercised"
    _run_case(oracle_c, df, uo, phi, U, B, driver, f"ties {kind} B={B} {driver}")


# ---- 2. row B over several consecutive items, 6. diagnostics ---------------------------------------------------------
STEADY_B, STEADY_NT = 64, 8
# diagnostics [0], [1], [4], [5] of the Gaussian case under the persistent driver, recorded from the parent build
# (commit f69f320) in the same GPU session as this build's
STEADY_DIAG_PARENT = (0, 5, 0, 0)


@functools.lru_cache(maxsize=None)
def _steady_case(kind):
    lt, lv = _levels()
    _, df, _ = make_inputs(CFG, nt=STEADY_NT, levels=lt)
    if kind == "zero":
        df = np.zeros_like(df)
    rng = np.random.default_rng(8)
    a, b = (tuple(int(x) for x in rng.integers(0, 8, size=4)) for _ in range(2))
    assert a != b
    uo = _cols([(0, 0, 0, 0), (3, 4, 3, 4), (0, 0, 0, 0), a, b, a, (7, 7, 7, 7), (4, 3, 4, 4)])
    same2 = [bool(np.array_equal(uo[:, s - 1], uo[:, s + 1])) for s in range(1, STEADY_NT - 1)]
    assert any(same2) and not all(same2), same2
    phi, U = _oracle(4, df, uo, STEADY_B)
    return df, uo, phi, U


@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("kind", ["gauss", "zero"])
def test_one_target_consecutive_items(oracle_c, kind, driver):
    df, uo, phi, U = _steady_case(kind)
    diag = _run_case(oracle_c, df, uo, phi, U, STEADY_B, driver, f"steady {kind} {driver}")
    if kind == "gauss" and driver == "persistent":
        assert (diag[0], diag[1], diag[4], diag[5]) == STEADY_DIAG_PARENT, diag


# ---- 3. u_old off the grid inside the dependency window --------------------------------------------------------------
OFF_B, OFF_NT = 29, 4
OFF = (8, 3, 4, 2)  # one step outside in dimension 0: b̃ in 1..21 <= 7·M
ON = [(3, 3, 3, 3), (4, 4, 4, 4), (3, 4, 3, 4), (4, 3, 4, 4)]
OFFGRID = {"step-i": (1,), "step-i+1": (2,), "both": (1, 2)}


@functools.lru_cache(maxsize=None)
def _offgrid_case(name):
    lt, lv = _levels()
    _, df, _ = make_inputs(CFG, nt=OFF_NT, levels=lt)
    uo = _cols([OFF if i in OFFGRID[name] else ON[i] for i in range(OFF_NT)])
    phi, U = _oracle(4, df, uo, OFF_B)
    return df, uo, phi, U


@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("name", list(OFFGRID))
def test_one_target_offgrid(oracle_c, name, driver):
    df, uo, phi, U = _offgrid_case(name)
    _run_case(oracle_c, df, uo, phi, U, OFF_B, driver, f"offgrid {name} {driver}")


# ---- 4. row B inside a two-row chunk ---------------------------------------------------------------------------------
def test_one_target_two_row_chunk(oracle_c):
    import torch
    lt, lv = _levels()
    K, B, nt = 2, 200, 6
    subs = [make_inputs(CFG, k=k, nt=nt, levels=lt)[1:] for k in (3, 4)]
    subs = [(np.zeros_like(df), uo) for df, uo in subs]  # zero gradients: the tie rule where the next item is not row B
    ctx = _ctx(1)
    ddf = torch.tensor(np.ascontiguousarray(np.stack([d.T for d, _ in subs])), dtype=torch.float64, device="cuda")
    duo = torch.tensor(np.ascontiguousarray(np.stack([u.T for _, u in subs])), dtype=torch.float64, device="cuda")
    du = torch.empty_like(ddf)
    dphi = torch.empty(K, dtype=torch.float64, device="cuda")
    dst = torch.empty(K, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.bellman_batch_tensors(ddf, duo, B, CFG.dt)
    ctx.synchronize()
    assert ctx.kernel_stats(0)[2] == "k_sdt_run"
    assert ctx.diagnostics()[6] == 0, ctx.diagnostics()
    cases = [_oracle(4, df, uo, B) for df, uo in subs]
    for k, (phi, U) in enumerate(cases):
        _compare_tables(ctx, U, f"chunk k={k}", k=k)
    for Bp in (B, B // 2, 1):
        ctx.backtrack_batch_tensors(Bp, du, dphi, dst)
        ctx.synchronize()
        for k, ((df, uo), (phi, U)) in enumerate(zip(subs, cases)):
            ou, ops = oracle_c.backtrack(lv, uo, phi, U, B, Bp)
            assert dst[k].item() == 0, f"chunk k={k} B'={Bp}: status {dst[k].item()}"
            assert np.array_equal(du[k].cpu().numpy().T, ou) and dphi[k].item() == ops, f"chunk k={k} B'={Bp}"
    ctx.close()


# ---- 5. the 8^3 grid -------------------------------------------------------------------------------------------------
G3_NT = 5
G3_UOLD = {"corner": [(0, 0, 0), (7, 7, 7), (0, 7, 0), (7, 0, 0), (0, 0, 7)],
           "interior": [(3, 3, 3), (4, 4, 4), (3, 4, 3), (4, 3, 4), (2, 5, 3)]}


@functools.lru_cache(maxsize=None)
def _g3_case(B, place, kind):
    rng = np.random.default_rng([B, int(place == "corner"), 0x83])
    df = np.asfortranarray(np.zeros((3, G3_NT)) if kind == "zero" else rng.standard_normal((3, G3_NT)))
    uo = _cols(G3_UOLD[place])
    phi, U = _oracle(3, df, uo, B)
    return df, uo, phi, U


@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("kind", ["gauss", "zero"])
@pytest.mark.parametrize("place", ["corner", "interior"])
@pytest.mark.parametrize("B", [8, 40])
def test_one_target_8x8x8(oracle_c, B, place, kind, driver):
    df, uo, phi, U = _g3_case(B, place, kind)
    _run_case(oracle_c, df, uo, phi, U, B, driver, f"8^3 B={B} {place} {kind} {driver}", M=3)
