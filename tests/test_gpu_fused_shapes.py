"""The fused small-state DP (k_fused_run<LP>, LP = 4, 8, 16, 24, 32, 36, 48, 64) against the CPU oracle, bit for bit:
every instantiation with a full level list (L = LP) and a padded one (L < LP: the columns j >= L of K and of the front
stay +Inf), one and two 64-row blocks per level, all five cost kinds, and the two limits of its domain (a full task
list of 192 (row block, target) pairs; 160 KiB of LDS).

Every case forces MIOC_ALGO_FUSED and compares every U cell the oracle wrote, and u, Phi* and the switch flags at four
budgets (dp_cases.check_device).  The "zero" cases are all ties: tests/test_dp_cases.py shows on the CPU that each
with L > 4 holds cells whose minimum is attained in two of the kernel's argmin groups of 4.
"""
import pytest

import dp_cases as dc
from mioc import native

pytestmark = pytest.mark.gpu

FUSED = native.MIOC_ALGO_FUSED


@pytest.mark.parametrize("L", dc.FUSED_LS)
@pytest.mark.parametrize("B", [63, 64])
def test_every_instantiation_full_and_padded(oracle_c, L, B):
    """The first and the last L of each LP; B = 63 is one 64-row block per level, B = 64 two (the task list split over
    the waves)."""
    assert native.fused_eligible(L, B)
    for case in dc.fused_shape_cases():
        if (case.L, case.B) == (L, B):
            dc.check_device(dc.Built(case, oracle_c), FUSED)


@pytest.mark.parametrize("L", dc.FUSED_EDGE_LS)
def test_domain_edge(oracle_c, L):
    """The largest B the domain admits (searched, native.fused_eligible): at L = 23, 24, 36 and 49 the task list is
    full or nearly so, at L = 63 and 64 the LDS.  There the fused DP equals the oracle; one row further the forced
    algorithm is refused with MIOC_EINVAL and MIOC_ALGO_AUTO takes the generic sweep, which equals the oracle too.
    That the device accepts B and refuses B + 1 pins native.fused_eligible to the library's fused_supported."""
    B = dc.largest_fused_B(L)
    assert native.fused_eligible(L, B) and not native.fused_eligible(L, B + 1)
    for case in dc.fused_edge_cases():
        if case.L != L:
            continue
        b = dc.Built(case, oracle_c)
        if case.B == B:
            dc.check_device(b, FUSED)
            continue
        assert case.B == B + 1
        with dc.new_context(b, FUSED) as ctx:
            with pytest.raises(native.MiocNativeError) as e:
                ctx.bellman(b.df, b.uo, b.B, b.dt)
            assert e.value.code == native.MIOC_EINVAL, case.id
        dc.check_device(b, native.MIOC_ALGO_AUTO, expect_algo=native.MIOC_ALGO_GENERIC)


@pytest.mark.parametrize("L", [23, 47])
def test_batch_of_three(oracle_c, L):
    """K = 3 restarts (all ties, integer gradients, u_old partly off the grid) in one batch on LP = 24 and LP = 48: one
    workgroup per restart, per-restart strides of U and of the final front."""
    dc.check_batch([dc.Built(c, oracle_c) for c in dc.batch_cases((L,))[L]], FUSED)
