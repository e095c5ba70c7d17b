"""GPU parity of the row classes of the persistent separable transform (k_sdt_run<4>; k_sdt_step<4> beside it) against
the CPU oracle -- C4's 8^4 = 4096 levels, β and Δt, p = 1:

  * three row classes in steady state (B = 64, nt = 8, both drivers): rows c' <= 28 hold sources whose staging row lies
    below 0 (geometric +Inf), rows c' > B - 28 have targets outside the trust region, rows 29..36 neither.  u_old cycles
    over grid corners, the centre and seeded on-grid columns, so that consecutive sphere orders differ and the reuse flag
    of the sphere-order slot (u_old(i-1) == u_old(i+1)) is both 0 and 1; from step nt - 4 down every row has finite
    inputs, so each class runs several such items;
  * geometric next to loaded +Inf, and the sparse threshold (B = 64, nt = 3 and 4): rows 1..3 of some step hold exactly
    4, 5 or 6 finite sources (SD_SPARSE = 4: the direct minimum over the sources up to 4, the transform above), asserted
    from the oracle's Φ.  At step nt - 2 the finite sources of row c' are the L1 sphere of radius c' around u_old(nt - 1):
    every other source is +Inf, loaded from the terminal step's staging rows >= 1 or geometric (its staging row lies
    below 0).  Later the finite sources of row c' are a ball around u_old(i + 1).  Exactly 3 finite sources, which the
    issue behind this file also names, cannot occur here: a sphere or ball of the 8^4 grid that has more than one member
    has at least 4 (from the nearest level, one unit move per dimension stays on the grid and adds one to the distance),
    and at C4's Δt = 2^-16 no linear term overflows to +Inf within four steps.  One case has an off-grid column with
    every b̃ inside the persistent kernel's dependency window;
  * several rows per workgroup (K = 2, B = 200, nt = 6, persistent driver): 128 workgroups per subproblem, chunks of one
    and two rows, so a row's successor is a row of the same step or the chunk's first row of the next step.

Every case: U equal wherever the oracle wrote it, u and Φ* equal at B' in {B, B // 2, 1}, kernel_stats(0)[2] the
expected kernel, diagnostics [6] == 0 (the persistent launch ran to the end).
"""
import functools

import numpy as np
import pytest

from mioc import native
from mioc.synth import CONFIGS, make_inputs
from oracle.oracle import P_ONE, Levels, OracleC, OracleError

pytestmark = pytest.mark.gpu

CFG = CONFIGS["C4"]
THREADS = 8  # the oracle's result does not depend on it (oracle/mioc_oracle.c: targets write disjoint columns)
KERNEL = {"persistent": "k_sdt_run", "steps": "k_sdt_step"}


@functools.lru_cache(maxsize=None)
def _levels():
    lt = CFG.levels()
    return lt, Levels(lt.nu, [tuple(int(x) for x in t) for t in lt.tuples])


def _cols(cols):
    return np.asfortranarray(np.array(cols, dtype=np.float64).T)


def _ctx(persist):
    lt, _ = _levels()
    ctx = native.Context(0)
    ctx.set_levels(lt)
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


def _compare(ctx, oracle_c, uo, phi, U, B, label):
    _, lv = _levels()
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


def _run_case(oracle_c, df, uo, phi, U, B, driver, label):
    ctx = _ctx(int(driver == "persistent"))
    ctx.bellman(df, uo, B, CFG.dt)
    ctx.synchronize()
    assert ctx.kernel_stats(0)[2] == KERNEL[driver]
    assert ctx.diagnostics()[6] == 0, ctx.diagnostics()
    _compare(ctx, oracle_c, uo, phi, U, B, label)
    ctx.close()


# ---- three row classes in steady state ------------------------------------------------------------------------------
STEADY_B, STEADY_NT = 64, 8


@functools.lru_cache(maxsize=None)
def _steady_case():
    lt, lv = _levels()
    _, df, _ = make_inputs(CFG, nt=STEADY_NT, levels=lt)
    rng = np.random.default_rng(8)
    a, b = (tuple(int(x) for x in rng.integers(0, 8, size=4)) for _ in range(2))
    assert a != b
    # columns 0 / 2 and 3 / 5 are equal (the slot's order is reused), every other pair two apart differs
    uo = _cols([(0, 0, 0, 0), (3, 4, 3, 4), (0, 0, 0, 0), a, b, a, (7, 7, 7, 7), (4, 3, 4, 4)])
    same2 = [bool(np.array_equal(uo[:, s - 1], uo[:, s + 1])) for s in range(1, STEADY_NT - 1)]
    assert any(same2) and not all(same2), same2
    phi, U = OracleC().bellman(lv, df, uo, STEADY_B, P_ONE, CFG.beta, CFG.dt, threads=THREADS)
    # every row class has items with finite inputs: the sources of steps 0 and 1 (Φ_1, Φ_2) are finite in every row
    for buf in (0, 1):
        assert np.all(np.isfinite(phi[:, :, buf]).any(axis=1)), "a budget row without a finite Φ"
    return df, uo, phi, U


@pytest.mark.parametrize("driver", ["persistent", "steps"])
def test_c4_row_classes_steady_state(oracle_c, driver):
    df, uo, phi, U = _steady_case()
    _run_case(oracle_c, df, uo, phi, U, STEADY_B, driver, f"steady {driver}")


# ---- geometric next to loaded +Inf, and the sparse threshold --------------------------------------------------------
SPARSE_B = 64
# name: (u_old columns, which Φ holds the counted sources, the finite sources of its rows 1, 2, 3)
#  * sphere (nt = 3): the sources of step 1 are the terminal Φ_2: the L1 spheres of radius 1, 2, 3 around (7,7,7,7);
#  * corner / edge (nt = 3): the sources of step 0 are Φ_1: the L1 balls of radius 1, 2, 3 around (0,0,0,0) / (0,0,0,3);
#  * offgrid (nt = 4): u_old(2) = (8,3,4,2) is one step outside the grid (b̃ in 1..22), so Φ_1[j, c'] is finite iff
#    b̃_j(1) <= c' - 1: rows 1, 2, 3 of step 0 hold the balls of radius 0, 1, 2 around (0,0,0,3).
SPARSE = {
    "sphere": ([(3, 3, 3, 3), (0, 0, 0, 0), (7, 7, 7, 7)], "terminal", (4, 10, 20)),
    "corner": ([(3, 3, 3, 3), (0, 0, 0, 0), (0, 0, 0, 0)], "phi1", (5, 15, 35)),
    "edge": ([(3, 3, 3, 3), (0, 0, 0, 3), (0, 0, 0, 0)], "phi1", (6, 20, 50)),
    "offgrid": ([(3, 3, 3, 3), (0, 0, 0, 3), (8, 3, 4, 2), (0, 0, 0, 0)], "phi1", (1, 6, 20)),
}


@functools.lru_cache(maxsize=None)
def _sparse_case(name):
    lt, lv = _levels()
    cols, which, want = SPARSE[name]
    nt = len(cols)
    _, df, _ = make_inputs(CFG, nt=nt, levels=lt)
    uo = _cols(cols)
    oc = OracleC()
    phi, U = oc.bellman(lv, df, uo, SPARSE_B, P_ONE, CFG.beta, CFG.dt, threads=THREADS)
    if which == "terminal":  # the terminal Φ: the oracle on the last column alone (one step: buffer (1 + 1) % 2 = 0)
        src = oc.bellman(lv, np.asfortranarray(df[:, -1:]), np.asfortranarray(uo[:, -1:]), SPARSE_B, P_ONE, CFG.beta,
                         CFG.dt)[0][:, :, 0]
    else:  # Φ_1, the sources of step 0: step i (1-based) is written to buffer (i + 1) % 2
        src = phi[:, :, 1]
    nf = tuple(int(np.isfinite(src[c]).sum()) for c in (1, 2, 3))
    assert nf == want, f"{name}: rows 1-3 hold {nf} finite sources, not {want}"
    return df, uo, phi, U, nf


def test_sparse_cases_cover_the_threshold():
    """Rows 1-3 of the cases hold exactly 4, 5 and 6 finite sources somewhere (by the oracle's Φ), on both sides of
    SD_SPARSE = 4."""
    seen = set()
    for name in SPARSE:
        seen |= set(_sparse_case(name)[4])
    assert {4, 5, 6} <= seen, seen


@pytest.mark.parametrize("driver", ["persistent", "steps"])
@pytest.mark.parametrize("name", list(SPARSE))
def test_c4_sparse_threshold_and_loaded_inf(oracle_c, name, driver):
    df, uo, phi, U, _ = _sparse_case(name)
    assert df.shape[1] in (3, 4)
    _run_case(oracle_c, df, uo, phi, U, SPARSE_B, driver, f"{name} {driver}")


# ---- several rows per workgroup -------------------------------------------------------------------------------------
def test_c4_two_rows_per_workgroup(oracle_c):
    import torch
    lt, lv = _levels()
    K, B, nt = 2, 200, 6
    subs = [make_inputs(CFG, k=k, nt=nt, levels=lt)[1:] for k in (3, 4)]
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
    cases = [oracle_c.bellman(lv, df, uo, B, P_ONE, CFG.beta, CFG.dt, threads=THREADS) for df, uo in subs]
    for k, (phi, U) in enumerate(cases):
        _compare_tables(ctx, U, f"batch k={k}", k=k)
    for Bp in (B, B // 2, 1):
        ctx.backtrack_batch_tensors(Bp, du, dphi, dst)
        ctx.synchronize()
        for k, ((df, uo), (phi, U)) in enumerate(zip(subs, cases)):
            ou, ops = oracle_c.backtrack(lv, uo, phi, U, B, Bp)
            assert dst[k].item() == 0, f"batch k={k} B'={Bp}: status {dst[k].item()}"
            assert np.array_equal(du[k].cpu().numpy().T, ou) and dphi[k].item() == ops, f"batch k={k} B'={Bp}"
    ctx.close()
