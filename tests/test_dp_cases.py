"""The cases of test_gpu_generic_shapes.py and test_gpu_fused_shapes.py on the CPU: the census of dp_cases restates
step 0 of the oracle exactly, and the all-tie cases do hold the ties that the device kernels' grouped argmin can get
wrong (so the GPU comparison is not vacuous)."""
import numpy as np
import pytest

import dp_cases as dc


@pytest.mark.parametrize("case", dc.all_cases_nt6(), ids=lambda c: c.id)
def test_census_reproduces_oracle_and_finds_ties(oracle_c, case):
    b = dc.Built(case, oracle_c)
    phi0, u0, ties, finite = b.census()
    assert np.array_equal(phi0, b.phi[:, :, 0])
    assert np.array_equal(u0, b.U[:, :, 0])
    assert finite == int((b.U[:, :, 0] >= 0).sum())
    L = case.L
    # a condition on the inputs, not a measurement: a case that misses it gets another seed (Case.salt)
    if case.mode == "zero" or (case.mode == "integer" and case.kind in ("one", "inf")):
        if L > 4:
            assert ties[4] > 0, (ties, finite)    # k_fused_run resolves groups of 4
        if L > 8:
            assert ties[8] > 0, (ties, finite)    # k_generic_step groups of 8
    if case.mode == "zero" and L > 64 and case.levels == "grid17":
        assert ties[64] > 0, (ties, finite)       # ... and LDS chunks of 64 sources


def test_case_builders():
    lv, lt = dc.grid17(65)
    assert lv.L == lt.L == 65 and lv.Lgrid == 289 and lv.M == 2
    assert lt.nuval[0].tolist() == [-3, 0] and lt.nuval[16].tolist() == [13, 0] and lt.nuval[17].tolist() == [-3, 1]
    assert np.array_equal(lv.nuval, lt.nuval) and np.array_equal(lv.gidx, np.arange(65))
    lv, lt = dc.line(257)
    assert lv.L == 257 and lv.M == 1 and lt.nuval[:, 0].tolist() == list(range(257))
    lv, lt = dc.grid17(33)
    for kind in dc.KINDS:
        pk, pint, tab, W = dc.cost(kind, lt)
        assert W.shape == (33, 33) and np.array_equal(W, W.T) and np.all(np.diag(W) == (1.0 if kind == "inf" else 0.0))
    assert dc.cost("lut2", lt)[3][0, 18] == 2.0 ** 0.5 and dc.cost("lut3", lt)[1] == 3
    df, uo, beta, dt = dc.inputs("outside", lv, 10, 3)
    off = ~((uo[0] >= -3) & (uo[0] <= 13) & (uo[1] >= 0) & (uo[1] <= 16))
    assert off.sum() == 2 and (beta, dt) == (1e-3, 2.0 ** -6)
    assert not dc.inputs("zero", lv, 5, 1)[0].any()
    # every instantiation of k_fused_run is the LP of some L in the list, full and padded
    lp = lambda L: next(x for x in dc.FU_LPS if L <= x)  # noqa: E731
    assert {lp(L) for L in dc.FUSED_LS} == set(dc.FU_LPS)
    assert {lp(L) for L in dc.FUSED_LS if L < lp(L)} == set(dc.FU_LPS) and set(dc.FU_LPS) <= set(dc.FUSED_LS) | {36}


def test_walk_cases_are_feasible(oracle_c):
    """The 16-bit walk cases must reach a backtrack (70 steps: two 64-step rounds), also where u_old leaves the grid."""
    for case in dc.generic_walk_cases():
        b = dc.Built(case, oracle_c)
        assert b.backtrack(b.B) is not None, case.id
