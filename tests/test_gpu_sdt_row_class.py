"""GPU parity of the one-row persistent driver's row classes (k_sdt_run1: every workgroup decides once whether its
budget row c' can have a source row below 0, `lowc` = c' <= 7·M, and whether a target of it can lie outside the trust
region, `highc` = B - c' < 7·M, and branches on the two at the class-dependent sites of the item) against the CPU
oracle, and device against device with MIOC_OPT_SDT_ROW_OWNER = 0 (the general driver, which does not know the class):
Φ and u at three budgets, the argmin table of every step and diagnostics [0], [1], [4], [5], [6] are equal, and
mioc_last_sdt_driver says which driver ran.

Shapes: every combination of the two class bits and both sides of each boundary, in steady state (nt = 8, u_old on the
grid, the sphere-order slot's reuse flag both 0 and 1):

  * 8^4 levels, 7·M = 28: B = 27 and 28 (every row low and high), B = 55 (rows 1-27 low, 28 low and high, 29-55 high: no
    interior row), B = 56 (rows 1-28 low only, 29-56 high only), B = 57 (exactly one interior row, 29), B = 64;
  * 8^3 levels, 7·M = 21: B = 41, 42 and 43 (the same three boundary shapes);
  * a loaded +Inf in a row that is not low: nt = 3 and 4 at B = 64 -- right after the terminal step the interior and
    high rows load +Inf from real rows, and their non-finite statistics must still be exact;
  * the ring wrap: B = 64, nt = 40 at 29 staging buffers, so the class branches run with the write-after-read polls
    armed (diagnostics [4] = (nt - NB)·(B - 1)).
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
GENERAL, ONE_ROW = 1, 2  # last_sdt_driver()
DIAG = (0, 1, 4, 5, 6)


@functools.lru_cache(maxsize=None)
def _levels(M):
    if M == 4:
        lt = CFG.levels()
        return lt, Levels(lt.nu, [tuple(int(x) for x in t) for t in lt.tuples])
    nu = [list(range(8))] * M
    return LevelTable(nu), Levels.product(nu)


def _cols(cols):
    return np.asfortranarray(np.array(cols, dtype=np.float64).T)


def _run(oracle_c, M, df, uo, phi, U, B, owner, label, nb=None):
    """One driver on the case, against the oracle; returns its tables, backtracks and diagnostics."""
    nt = df.shape[1]
    ctx = native.Context(0)
    ctx.set_levels(_levels(M)[0])
    ctx.set_cost(1, CFG.beta)
    ctx.set_option(native.MIOC_OPT_TIMING, 1)
    ctx.set_option(native.MIOC_OPT_ALGO, native.MIOC_ALGO_SEPARABLE)
    ctx.set_option(native.MIOC_OPT_PERSIST, 1)
    ctx.set_option(native.MIOC_OPT_SDT_ROW_OWNER, owner)
    if nb is not None:
        ctx.set_option(native.MIOC_OPT_SDT_BUFFERS, nb)
    ctx.bellman(df, uo, B, CFG.dt)
    ctx.synchronize()
    assert ctx.kernel_stats(0)[2] == "k_sdt_run"
    assert ctx.last_sdt_driver() == (ONE_ROW if owner else GENERAL), f"{label}: driver {ctx.last_sdt_driver()}"
    diag = ctx.diagnostics()
    assert diag[6] == 0, diag
    tabs = [ctx.argmin_table(i) for i in range(nt - 1)]
    for i, d in enumerate(tabs):
        o = U[:, :, i]
        m = o >= 0
        assert np.array_equal(d[m], o[m]), f"{label}: U at step {i}"
    res = []
    for Bp in (B, B // 2, 1):
        try:
            ou, ops = oracle_c.backtrack(_levels(M)[1], uo, phi, U, B, Bp)
        except OracleError as e:  # no finite Φ_0 within B': the device says the same
            assert e.args == (native.MIOC_EINFEASIBLE,), e
            with pytest.raises(native.MiocNativeError) as err:
                ctx.backtrack(Bp)
            assert err.value.code == native.MIOC_EINFEASIBLE, f"{label}: B'={Bp}"
            res.append(None)
            continue
        u, ps, _ = ctx.backtrack(Bp)
        assert np.array_equal(u, ou) and ps == ops, f"{label}: B'={Bp}: {ps!r} vs {ops!r}"
        res.append((u, ps))
    ctx.close()
    return tabs, res, diag


def _both(oracle_c, M, case, B, label, nb=None):
    """The one-row driver and the general driver: each against the oracle, then one against the other (the whole
    tables, also where the oracle left a cell unwritten).  Returns the one-row driver's diagnostics."""
    df, uo, phi, U = case
    t1, r1, d1 = _run(oracle_c, M, df, uo, phi, U, B, 1, f"{label} one-row", nb)
    t0, r0, d0 = _run(oracle_c, M, df, uo, phi, U, B, 0, f"{label} general", nb)
    for i, (a, b) in enumerate(zip(t1, t0)):
        assert np.array_equal(a, b), f"{label}: the drivers' U differ at step {i}"
    for a, b in zip(r1, r0):
        assert (a is None) == (b is None) and (a is None or (np.array_equal(a[0], b[0]) and a[1] == b[1])), label
    assert [d1[q] for q in DIAG] == [d0[q] for q in DIAG], (label, d1, d0)
    return d1


def _classes(M, B):
    """The (lowc, highc) combinations among rows 1..B."""
    S = 7 * M
    return {(c <= S, B - c < S) for c in range(1, B + 1)}


# u_old on the grid at every step; u_old(s - 1) == u_old(s + 1) at some steps and not at others (the slot's reuse flag)
UOLD = {
    4: [(0, 0, 0, 0), (3, 4, 3, 4), (0, 0, 0, 0), (1, 6, 2, 5), (6, 2, 5, 0), (1, 6, 2, 5), (7, 7, 7, 7), (4, 3, 4, 4)],
    3: [(0, 0, 0), (3, 4, 3), (0, 0, 0), (2, 5, 3), (7, 0, 1), (2, 5, 3), (7, 7, 7), (4, 3, 4)],
}


@functools.lru_cache(maxsize=None)
def _case(M, B, nt):
    lt, lv = _levels(M)
    if M == 4:
        _, df, _ = make_inputs(CFG, nt=nt, levels=lt)
    else:
        df = np.asfortranarray(np.random.default_rng(0x83).standard_normal((M, nt)))
    cyc = UOLD[M]
    uo = _cols([cyc[i % len(cyc)] for i in range(nt)])
    if nt >= 4:
        same2 = [bool(np.array_equal(uo[:, s - 1], uo[:, s + 1])) for s in range(1, nt - 1)]
        assert any(same2) and not all(same2), same2
    phi, U = OracleC().bellman(lv, df, uo, B, P_ONE, CFG.beta, CFG.dt, threads=THREADS)
    return df, uo, phi, U


STEADY_NT = 8
LOW_HIGH, LOW, HIGH, INTERIOR = (True, True), (True, False), (False, True), (False, False)
# (M, B, the classes its rows fall into)
BOUNDARIES = [
    (4, 27, {LOW_HIGH}),
    (4, 28, {LOW_HIGH}),
    (4, 55, {LOW, LOW_HIGH, HIGH}),
    (4, 56, {LOW, HIGH}),
    (4, 57, {LOW, INTERIOR, HIGH}),
    (4, 64, {LOW, INTERIOR, HIGH}),
    (3, 41, {LOW, LOW_HIGH, HIGH}),
    (3, 42, {LOW, HIGH}),
    (3, 43, {LOW, INTERIOR, HIGH}),
]


@pytest.mark.parametrize("M,B,want", BOUNDARIES, ids=[f"8^{M}-B{B}" for M, B, _ in BOUNDARIES])
def test_row_class_boundaries(oracle_c, M, B, want):
    assert _classes(M, B) == want
    S = 7 * M
    if B == 2 * S + 1:  # exactly one interior row
        assert [c for c in range(1, B + 1) if c > S and B - c >= S] == [S + 1]
    _both(oracle_c, M, _case(M, B, STEADY_NT), B, f"8^{M} B={B}")


@functools.lru_cache(maxsize=None)
def _tail_phi(nt):
    df, uo, _, _ = _case(4, 64, nt)
    lv = _levels(4)[1]
    sub = OracleC().bellman(lv, np.asfortranarray(df[:, -3:]), np.asfortranarray(uo[:, -3:]), 64, P_ONE, CFG.beta,
                            CFG.dt, threads=THREADS)[0]
    return sub[:, :, 1]


@pytest.mark.parametrize("nt", [3, 4])
def test_row_class_loaded_inf_in_upper_rows(oracle_c, nt):
    """The terminal Φ is finite only where the budget equals the distance from u_old(nt - 1), so in the first steps
    after it the rows above 7·M load +Inf from real rows, next to finite values."""
    B = 64
    df, uo, phi, U = _case(4, B, nt)
    # Φ_{nt-2}, the sources of step nt - 3, counted on the CPU first: the recursion runs backwards, so it is Φ_1 of the
    # last three columns alone
    src = _tail_phi(nt)
    mixed = [c for c in range(29, B + 1) if np.isinf(src[c]).any() and np.isfinite(src[c]).any()]
    assert any(B - c >= 28 for c in mixed) and any(B - c < 28 for c in mixed), mixed  # interior rows and high rows
    _both(oracle_c, 4, (df, uo, phi, U), B, f"loaded +Inf nt={nt}")


def test_row_class_ring_wrap(oracle_c):
    B, nt, nb = 64, 40, 29
    diag = _both(oracle_c, 4, _case(4, B, nt), B, "wrap nb=29", nb=nb)
    assert diag[4] == (nt - nb) * (B - 1) > 0, diag
