"""The generic min-plus sweep (k_generic_step<uint8_t / uint16_t>, k_generic_argmin0, k_generic_walk) against the CPU
oracle, bit for bit, at the edges of its tiling: 32 target levels per workgroup, 64 source levels per LDS chunk, argmin
groups of 8, 64 budget rows per block, and the step from one to two bytes per argmin rank at L = 256 / 257.

Every case forces MIOC_ALGO_GENERIC and compares every U cell the oracle wrote, and u, Phi* and the switch flags at
four budgets (dp_cases.check_device).  The "zero" cases are all ties: tests/test_dp_cases.py shows on the CPU that
each holds cells whose minimum is attained in two argmin groups and (L > 64) in two source chunks, which is where a
grouped first-index argmin can go wrong.
"""
import pytest

import dp_cases as dc
from mioc import native

pytestmark = pytest.mark.gpu

GENERIC = native.MIOC_ALGO_GENERIC


@pytest.mark.parametrize("name,L", dc.GENERIC_EDGE_LEVELS, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", dc.KINDS)
def test_tile_and_table_edges(oracle_c, name, L, kind):
    """L at the last, full and first-of-the-next target tile (31/32/33), source chunk (63/64/65) and one-byte rank
    (255/256/257), and 257 levels on a line; B = 64, so RP = 128 and the second budget tile holds one real row."""
    for case in dc.generic_edge_cases():
        if (case.levels, case.L, case.kind) == (name, L, kind):
            dc.check_device(dc.Built(case, oracle_c), GENERIC)


@pytest.mark.parametrize("case", dc.generic_budget_cases(), ids=lambda c: c.id)
def test_budget_tiles(oracle_c, case):
    """B + 1 = 63, 64 (one full tile), 128 (two) and 131 (three, the last with three rows)."""
    dc.check_device(dc.Built(case, oracle_c), GENERIC)


@pytest.mark.parametrize("nt", [1, 2])
def test_degenerate_lengths(oracle_c, nt):
    """nt = 1: the terminal front alone (no U); nt = 2: one step."""
    for case in dc.generic_short_cases():
        if case.nt == nt:
            dc.check_device(dc.Built(case, oracle_c), GENERIC)


@pytest.mark.parametrize("case", dc.generic_walk_cases(), ids=lambda c: c.id)
def test_two_byte_walk_over_two_rounds(oracle_c, case):
    """k_generic_walk<uint16_t>: 69 steps are two 64-step rounds at least; u_old partly off the level grid (no level
    to follow) and piecewise constant (the walk's second guess holds for stretches)."""
    b = dc.Built(case, oracle_c)
    assert b.backtrack(b.B) is not None
    diag = dc.check_device(b, GENERIC)
    assert diag[2] >= 2 and diag[3] == 0, diag


@pytest.mark.parametrize("L", [65, 257])
def test_batch_of_three(oracle_c, L):
    """K = 3 restarts (all ties, integer gradients, u_old partly off the grid) in one batch, one cost and dt for all:
    per-restart strides of the fronts and of U, in both rank widths."""
    dc.check_batch([dc.Built(c, oracle_c) for c in dc.batch_cases((L,))[L]], GENERIC)
