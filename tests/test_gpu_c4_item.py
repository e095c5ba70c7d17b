"""GPU parity of the row item of the separable transform (k_sdt_run<4>, k_sdt_step<4>) at the shapes where its
statistics phase changes path, against the CPU oracle -- 8^4 = 4096 levels, nt <= 4, p = 1:

  * trust-region edge: budgets B in {3, 27, 28, 29, 60} -- below, at and above 7·M = 28, where a row's mask of targets
    inside the trust region (`valid`), its count and the all-inside branch change over -- with u_old at grid corners, at
    the grid centre and one integer step outside the level grid in one dimension (b̃ >= 1 everywhere): once next to a
    corner, where the largest b̃ is 29 > 7·M and the host must take per-step launches, and once with every b̃ inside the
    persistent kernel's dependency window, which then runs without a level at distance 0.  nt = 3, 4: the first steps
    after the terminal one, where most rows are +Inf or hold a handful of finite sources (the sparse path, the
    non-finite statistics path, seam-straddling pairs);
  * the counting redo of a row that met a near tie (diagnostics [5]) under the oracle: integer gradients.

Every case: U equal wherever the oracle wrote it, u and Φ* equal at B' in {B, B // 2, 1}; the persistent driver ran to
the end (diagnostics [6] == 0).
"""
import functools

import numpy as np
import pytest

from mioc import native
from mioc.synth import CONFIGS, make_inputs
from oracle.oracle import P_ONE, Levels, OracleC, OracleError

pytestmark = pytest.mark.gpu

CFG = CONFIGS["C4"]
CORNER = [(0, 0, 0, 0), (7, 7, 7, 7), (0, 7, 0, 7), (7, 0, 0, 0)]
CENTRE = [(3, 3, 3, 3), (4, 4, 4, 4), (3, 4, 3, 4), (4, 3, 4, 4)]
# dimension 0 one step above its last level: the largest b̃ is 8 + 7 + 7 + 7 = 29 (per-step launches), or 21 (persistent)
OUTSIDE = [(8, 0, 0, 0)] * 4
OUTSIDE_NEAR = [(8, 3, 4, 2)] * 4

# (B, placement, nt)
EDGE = [(B, place, 4) for B in (3, 27, 28, 29, 60) for place in ("corner", "centre")]
EDGE += [(28, "corner", 3), (29, "outside", 4), (29, "outside-near", 4)]


@functools.lru_cache(maxsize=None)
def _levels():
    lt = CFG.levels()
    return lt, Levels(lt.nu, [tuple(int(x) for x in t) for t in lt.tuples])


def _u_old(place, nt):
    cols = {"corner": CORNER, "centre": CENTRE, "outside": OUTSIDE, "outside-near": OUTSIDE_NEAR}[place]
    return np.asfortranarray(np.array([cols[i % 4] for i in range(nt)], dtype=np.float64).T)


@functools.lru_cache(maxsize=None)
def _edge_case(B, place, nt):
    """(df, u_old, Φ, U) of one case: the oracle runs once for both drivers."""
    lt, lv = _levels()
    _, df, _ = make_inputs(CFG, nt=nt, levels=lt)
    uo = _u_old(place, nt)
    phi, U = OracleC().bellman(lv, df, uo, B, P_ONE, CFG.beta, CFG.dt)
    return df, uo, phi, U


def _run(df, uo, B, beta, persist):
    lt, _ = _levels()
    ctx = native.Context(0)
    ctx.set_levels(lt)
    ctx.set_cost(1, beta)
    ctx.set_option(native.MIOC_OPT_TIMING, 1)
    ctx.set_option(native.MIOC_OPT_ALGO, native.MIOC_ALGO_SEPARABLE)
    ctx.set_option(native.MIOC_OPT_PERSIST, persist)
    ctx.bellman(df, uo, B, CFG.dt)
    ctx.synchronize()
    return ctx


def _compare(ctx, oracle_c, df, uo, phi, U, B, label):
    _, lv = _levels()
    for i in range(df.shape[1] - 1):
        d, o = ctx.argmin_table(i), U[:, :, i]
        m = o >= 0
        assert np.array_equal(d[m], o[m]), f"{label}: U at step {i}"
    for Bp in (B, B // 2, 1):
        try:
            ou, ops = oracle_c.backtrack(lv, uo, phi, U, B, Bp)
        except OracleError as e:
            # no finite Φ_0 within B' (u_old off the grid costs at least one unit per step): the device says the same
            assert e.args == (native.MIOC_EINFEASIBLE,), e
            with pytest.raises(native.MiocNativeError) as err:
                ctx.backtrack(Bp)
            assert err.value.code == native.MIOC_EINFEASIBLE, f"{label}: B'={Bp}"
            continue
        u, ps, _ = ctx.backtrack(Bp)
        assert np.array_equal(u, ou) and ps == ops, f"{label}: B'={Bp}: {ps!r} vs {ops!r}"


@pytest.mark.parametrize("driver", ["persistent", "steps"])
@pytest.mark.parametrize("B,place,nt", EDGE, ids=[f"B{B}-{p}-nt{n}" for B, p, n in EDGE])
def test_c4_trust_region_edge(oracle_c, B, place, nt, driver):
    df, uo, phi, U = _edge_case(B, place, nt)
    ctx = _run(df, uo, B, CFG.beta, int(driver == "persistent"))
    # "outside": u_old reaches further back than the persistent kernel's dependency window (b̃ up to 29 > 7·M)
    want = "k_sdt_run" if driver == "persistent" and place != "outside" else "k_sdt_step"
    assert ctx.kernel_stats(0)[2] == want
    assert ctx.diagnostics()[6] == 0, ctx.diagnostics()
    _compare(ctx, oracle_c, df, uo, phi, U, B, f"B={B} {place} nt={nt} {driver}")
    ctx.close()


REDO_NT, REDO_B = 5, 60


@functools.lru_cache(maxsize=None)
def _redo_case():
    lt, lv = _levels()
    rng = np.random.default_rng(32)
    _, df, uo = make_inputs(CFG, nt=REDO_NT, levels=lt)
    df = rng.integers(-3, 4, size=df.shape).astype(float) * 4096.0
    phi, U = OracleC().bellman(lv, df, uo, REDO_B, P_ONE, CFG.beta, CFG.dt)
    return df, uo, phi, U


@pytest.mark.parametrize("driver", ["persistent", "steps"])
def test_c4_counting_redo_vs_oracle(oracle_c, driver):
    """Integer gradients (Δt·df a multiple of 1/16) with β = 1e-3: many candidates of a target tie exactly or within
    the certified tolerance, inside the transform's binade, so rows go through the counting transform again
    (diagnostics [5]) and their flagged targets through the exact scan."""
    df, uo, phi, U = _redo_case()
    ctx = _run(df, uo, REDO_B, CFG.beta, int(driver == "persistent"))
    assert ctx.kernel_stats(0)[2] == {"persistent": "k_sdt_run", "steps": "k_sdt_step"}[driver]
    diag = ctx.diagnostics()
    assert diag[6] == 0, diag
    _compare(ctx, oracle_c, df, uo, phi, U, REDO_B, f"redo {driver}")
    assert diag[5] > 0, diag  # rows redone with the counting transform
    ctx.close()
