"""GPU parity of the certified winners' distance d(l, j*) in the separable transform (mioc_sdt.hip: sdt_body).  The
first, non-counting transform steps by 1.0 plus one ulp of the row's binade, so that payload bits 0..5 of every output
count the steps from its source, and its winners read d(l, j*) there; the counting redo keeps unit 1.0, its near-tie
count in those bits, and recomputes the winner's stamp.  Both run here, on all three drivers: one launch per step
(k_sdt_step, MIOC_OPT_PERSIST = 0), the general persistent driver (k_sdt_run) and the one-row driver (k_sdt_run1).

Shapes: 8^4 levels with B in {27, 57, 64} at nt = 6, 8^3 with B in {41, 43} at nt = 5: low, interior and high rows and
both sides of 7·M.  Per driver: the argmin table of every step equal to the oracle's wherever it wrote a cell, u and Φ*
equal at B' in {B, B // 2, 1}; device against device the whole tables, u, Φ* and diagnostics [0], [1], [5] between the
persistent drivers, [0] and [5] with the per-step driver (its row B counts a direct row in [1] wherever u_old is on the
grid, where the persistent drivers count the one-target items: tests/test_gpu_sdt_psi_copy.py).

Inputs:
  * Gaussian gradients (winners at small distances, no near tie);
  * zero gradients: every merge ties, so every transform row is redone counting and its targets are listed
    (diagnostics [5] > 0): the counting winners;
  * a dominant corner: β = 2^-30 against gradients of about -1 in every component, so that the top corner level
    (rank L - 1) is the cheapest source by far, and u_old at the bottom corner at two steps and at the top corner
    otherwise: there the bottom corner's cells (rank 0) take the top corner as their source at distance 7·M (28 at
    8^4, 21 at 8^3), the largest count the payload carries.  Shown on the CPU from the oracle's tables first;
  * the ring wrap: 8^3, B = 43, nt = 40 at 29 staging buffers (diagnostics [4] = (nt - NB)·(B - 1) on the persistent
    drivers).
"""
import functools

import numpy as np
import pytest

from mioc import native
from mioc.iterators import LevelTable
from mioc.synth import CONFIGS, make_inputs
from oracle.oracle import P_ONE, Levels, OracleC, OracleError

CFG = CONFIGS["C4"]
THREADS = 8  # the oracle's result does not depend on it
ONE_ROW, GENERAL, STEPS = "one-row", "general", "steps"
DRIVERS = (ONE_ROW, GENERAL, STEPS)
DIAG = (0, 1, 5)
TINY_BETA = 2.0 ** -30
SHAPES = [(4, 27, 6), (4, 57, 6), (4, 64, 6), (3, 41, 5), (3, 43, 5)]
IDS = [f"8^{M}-B{B}" for M, B, _ in SHAPES]
UOLD3 = [(0, 0, 0), (3, 4, 3), (0, 0, 0), (2, 5, 3), (7, 0, 1), (2, 5, 3), (7, 7, 7), (4, 3, 4)]


@functools.lru_cache(maxsize=None)
def _levels(M):
    if M == 4:
        lt = CFG.levels()
        return lt, Levels(lt.nu, [tuple(int(x) for x in t) for t in lt.tuples])
    nu = [list(range(8))] * M
    return LevelTable(nu), Levels.product(nu)


def _cols(cols):
    return np.asfortranarray(np.array(cols, dtype=np.float64).T)


def _uold(M, nt):
    if M == 4:
        return make_inputs(CFG, nt=nt, levels=_levels(4)[0])[2]
    return _cols([UOLD3[i % len(UOLD3)] for i in range(nt)])


def _corner_steps(nt):
    return (1, nt - 3)  # the steps whose u_old is the bottom corner


@functools.lru_cache(maxsize=None)
def _case(kind, M, B, nt):
    """(df, u_old, β, the oracle's Φ and U), computed once for the three drivers."""
    lv = _levels(M)[1]
    beta = CFG.beta
    if kind == "gauss":
        df = np.asfortranarray(np.random.default_rng(0xD15 + M).standard_normal((M, nt)))
        uo = _uold(M, nt)
    elif kind == "zero":
        df = np.zeros((M, nt), order="F")
        uo = _uold(M, nt)
    else:
        assert kind == "corner"
        beta = TINY_BETA
        df = np.asfortranarray(-np.ones((M, nt)) - 0.01 * np.random.default_rng(5).standard_normal((M, nt)))
        uo = _cols([(0,) * M if i in _corner_steps(nt) else (7,) * M for i in range(nt)])
    phi, U = OracleC().bellman(lv, df, uo, B, P_ONE, beta, CFG.dt, threads=THREADS)
    return df, uo, beta, phi, U


def _run(oracle_c, M, B, case, driver, label, nb=None):
    df, uo, beta, phi, U = case
    lv = _levels(M)[1]
    nt = df.shape[1]
    ctx = native.Context(0)
    ctx.set_levels(_levels(M)[0])
    ctx.set_cost(1, beta)
    ctx.set_option(native.MIOC_OPT_TIMING, 1)
    ctx.set_option(native.MIOC_OPT_ALGO, native.MIOC_ALGO_SEPARABLE)
    ctx.set_option(native.MIOC_OPT_PERSIST, int(driver != STEPS))
    ctx.set_option(native.MIOC_OPT_SDT_ROW_OWNER, int(driver == ONE_ROW))
    if nb is not None:
        ctx.set_option(native.MIOC_OPT_SDT_BUFFERS, nb)
    ctx.bellman(df, uo, B, CFG.dt)
    ctx.synchronize()
    assert ctx.kernel_stats(0)[2] == ("k_sdt_step" if driver == STEPS else "k_sdt_run"), label
    if driver != STEPS:
        assert ctx.last_sdt_driver() == (2 if driver == ONE_ROW else 1), label
    diag = ctx.diagnostics()
    print(label, "diagnostics", list(diag[:7]))
    assert diag[6] == 0, (label, diag)
    tabs = [ctx.argmin_table(i) for i in range(nt - 1)]
    for i, d in enumerate(tabs):
        o = U[:, :, i]
        m = o >= 0
        assert np.array_equal(d[m], o[m]), f"{label}: U at step {i}"
    res = []
    for Bp in (B, B // 2, 1):
        try:
            ou, ops = oracle_c.backtrack(lv, uo, phi, U, B, Bp)
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


def _drivers(oracle_c, M, B, case, label, nb=None, drivers=DRIVERS):
    """The case under the three drivers: each against the oracle, then one against the other."""
    runs = {d: _run(oracle_c, M, B, case, d, f"{label} {d}", nb) for d in drivers}
    t1, r1, d1 = runs[ONE_ROW]
    for other in drivers[1:]:
        t0, r0, d0 = runs[other]
        for i, (a, b) in enumerate(zip(t1, t0)):
            assert np.array_equal(a, b), f"{label}: U of {ONE_ROW} and {other} differ at step {i}"
        for a, b in zip(r1, r0):
            assert (a is None) == (b is None) and (a is None or (np.array_equal(a[0], b[0]) and a[1] == b[1])), label
        slots = DIAG if other == GENERAL else (0, 5)
        assert [d1[q] for q in slots] == [d0[q] for q in slots], (label, other, d1, d0)
    return runs


def _fast_winners_ran(runs, nt):
    """The results came from the first (non-counting) transform's winners: no row was redone counting ([5]), no target
    was listed for the exact scan ([0]), and the exact scans saw only the rows that are short by geometry ([1]): with
    u_old on the grid a step has one one-target row (row B) and, at an 8^3 corner, one direct row of 1 + M = SD_FEW
    targets (row B - 1); a row sent to the scans whole because its scale did not fit would add all its targets."""
    for d, (_, _, diag) in runs.items():
        assert diag[5] == 0 and diag[0] == 0, (d, diag)
        assert diag[1] <= (1 + 4) * (nt - 1), (d, diag)


@pytest.mark.gpu
@pytest.mark.parametrize("M,B,nt", SHAPES, ids=IDS)
def test_payload_dist_gaussian(oracle_c, M, B, nt):
    _fast_winners_ran(_drivers(oracle_c, M, B, _case("gauss", M, B, nt), f"gauss 8^{M} B={B}"), nt)


@pytest.mark.gpu
@pytest.mark.parametrize("M,B,nt", SHAPES, ids=IDS)
def test_payload_dist_zero_gradients(oracle_c, M, B, nt):
    runs = _drivers(oracle_c, M, B, _case("zero", M, B, nt), f"zero 8^{M} B={B}")
    for d in DRIVERS:  # the counting transform and its winners ran
        assert runs[d][2][5] > 0, (d, runs[d][2])


def _corner_cells(M, B, nt):
    """The oracle's cells of the bottom corner level (rank 0) at budgets c >= 1 that hold the top corner's rank, at the
    steps whose u_old is the bottom corner (b̃ = 0 there, so budget c is source row c' = c: a row with a workgroup)."""
    df, uo, beta, phi, U = _case("corner", M, B, nt)
    L = 8 ** M
    return {i: int((U[1:, 0, i] == L - 1).sum()) for i in _corner_steps(nt) if i < nt - 1}


@pytest.mark.parametrize("M,B,nt", SHAPES, ids=IDS)
def test_payload_dist_corner_case_reaches_the_far_corner(M, B, nt):
    """On the CPU: some cell of the bottom corner holds the top corner's rank, a winner at distance 7·M."""
    cells = _corner_cells(M, B, nt)
    print(M, B, cells)
    assert cells and any(n > 0 for n in cells.values()), (M, B, cells)


@pytest.mark.gpu
@pytest.mark.parametrize("M,B,nt", SHAPES, ids=IDS)
def test_payload_dist_dominant_corner(oracle_c, M, B, nt):
    cells = _corner_cells(M, B, nt)  # established before the device runs
    assert any(n > 0 for n in cells.values()), (M, B, cells)
    _fast_winners_ran(_drivers(oracle_c, M, B, _case("corner", M, B, nt), f"corner 8^{M} B={B}"), nt)


@pytest.mark.gpu
def test_payload_dist_ring_wrap(oracle_c):
    M, B, nt, nb = 3, 43, 40, 29
    # (the drivers that have a ring: the per-step driver keeps two staging buffers)
    runs = _drivers(oracle_c, M, B, _case("gauss", M, B, nt), "wrap nb=29", nb=nb, drivers=(ONE_ROW, GENERAL))
    for d in (ONE_ROW, GENERAL):
        assert runs[d][2][4] == (nt - nb) * (B - 1) > 0, (d, runs[d][2])
