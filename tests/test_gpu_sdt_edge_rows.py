"""GPU parity of the separable transform's rows next to the budget, B - c' in {0, 1, 2}, where the number of targets inside
the trust region decides the row's path (mioc_sdt.hip, sdt_body): none, one (the one-target item), two to SD_FEW (a direct
row), more (the transform) -- on all three drivers, through the rig and the oracle census of
tests/test_gpu_sdt_psi_copy.py.

With u_old(i) on an 8^M grid a row with B - c' >= 1 holds at least 1 + M targets (the level at distance 0 and at least M at
distance 1): five at 8^4, more than SD_FEW, so only row B is short there; four at an 8^3 corner, exactly SD_FEW, so row
B - 1 is a direct row.  With u_old(i) off the grid inside the persistent drivers' window (b̃ <= 7·M everywhere) the rows
shift: at u_old = (8, 3, 4, 2) the smallest b̃ is 1, row B has no target and row B - 1 is the one-target row -- a row's
path cannot be told from B - c' alone.

Every case first counts, on the CPU, the targets and the class of rows B, B - 1 and B - 2 of step 0; the device's
diagnostics [1] (the direct rows' targets + the one-target rows) must equal the census on both persistent drivers.
"""
import numpy as np
import pytest

import sdt_census as sc
import test_gpu_sdt_psi_copy as rig

B4, B3 = 28, 22


def _case(M, B, first, nt=3, seed=12):
    def build():
        rest = [(3,) * M, (4,) * M, (2,) * M]
        uo = rig._cols([first] + rest[:nt - 1])
        df = np.asfortranarray(np.random.default_rng(seed).standard_normal((M, nt)))
        return M, B, df, uo, ("winners",), ()
    return build


# name: (case, the (class, targets) of rows B, B - 1, B - 2 at step 0)
EDGE = {
    "g4-corner": (_case(4, B4, (0, 0, 0, 0)), [("one-target", 1), ("transform", 5), ("transform", 15)]),
    "g4-centre": (_case(4, B4, (3, 3, 3, 3)), [("one-target", 1), ("transform", 9), ("transform", 41)]),
    "g4-offgrid": (_case(4, B4, (8, 3, 4, 2)), [("empty", 0), ("one-target", 1), ("transform", 8)]),
    "g3-corner": (_case(3, B3, (7, 0, 7)), [("one-target", 1), ("direct", 4), ("transform", 10)]),
    "g3-centre": (_case(3, B3, (4, 3, 4)), [("one-target", 1), ("transform", 7), ("transform", 25)]),
}
rig.EXTRA.update({f"edge-{k}": v[0] for k, v in EDGE.items()})


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_rows_census(name):
    """On the CPU: the class and the number of targets of rows B, B - 1, B - 2 at step 0."""
    M, B, df, uo, phi, U, paths, cls, ties = rig._case(f"edge-{name}")
    got = [(cls[(0, B - t)][0], cls[(0, B - t)][2]) for t in range(3)]
    print(name, got)
    assert got == EDGE[name][1], (name, got)
    assert all(cls[(0, B - t)][1] > sc.SD_SPARSE for t in range(3)), "not a sparse row"


def test_edge_rows_cover_the_few_target_threshold():
    # 1 + M = SD_FEW at 8^3 (a direct row of exactly SD_FEW targets), 1 + M = SD_FEW + 1 at 8^4 (the smallest transform row)
    assert 1 + 3 == sc.SD_FEW and 1 + 4 == sc.SD_FEW + 1
    assert ("direct", sc.SD_FEW) in EDGE["g3-corner"][1] and ("transform", sc.SD_FEW + 1) in EDGE["g4-corner"][1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGE))
def test_edge_rows_on_every_driver(oracle_c, name):
    rig.run_drivers(oracle_c, f"edge-{name}")
