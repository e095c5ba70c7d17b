"""The cases of test_gpu_pinf_shapes.py on the CPU (tests/pinf_cases.py): the restatement of the p=Inf tables is pinned
to the C oracle before any device is asked, every wrong version of it shows on some case (three of them on the cases
aimed at them), and no case compares mostly +Inf with +Inf.

Anchor: R_i[c] = min_l Φ_i[c, l], and Φ_i of the problem is the final front of the suffix problem df[:, i:],
u_old[:, i:], so every row of R equals the row minima of an oracle front, bit for bit (min is exact and both sides
form the same sums).

Conditions.  The plain ones -- at least half of the cells R_i[c], c <= B, finite, and R_0[B] finite -- cannot hold for
a shape with nt·(BW-1) < B: no path of nt steps that each spend at most BW-1 ends in row B.  That is arithmetic, not a
measurement, and it concerns the xr cases of two and three steps (2·31, 3·31 < 256), the one-level case (BW = 1) and
[[0,1]]³ at nt = 6, B = 20 (6·3 = 18).  For those (pinf_cases.reach_limited) the same two conditions are asked of the
rows a path can end in: c <= (nt-i)·(BW-1) at step i, and R_0 at the sum of the steps' largest non-empty classes.
"""
import numpy as np
import pytest

import pinf_cases as pc
from oracle.oracle import P_INF

_IDS = [c.id for c in pc.CASES]
SMALL = [c for c in pc.CASES if pc.levels_of(c)[0].L <= 256]


def _row_minima(oracle_c, lv, df, uo, B, beta, dt):
    phi, _ = oracle_c.bellman(lv, df, uo, B, P_INF, beta, dt)
    return phi[:, :, 0].min(axis=1)


def test_case_table():
    """Every case is on its side of the dispatch rules at 256 CUs, ids are unique, and each kernel name of the rules
    is pinned by some case."""
    assert len(set(_IDS)) == len(_IDS)
    recur, prep = set(), set()
    for c in pc.CASES:
        lv, _, dfs, uos, B, _, _, K = pc.build(c)
        r = pc.reference_k(c, 0)
        assert K == c.K(256) == len(dfs) == len(uos) and r.BW == pc.batch_bw(lv, uos, B)
        rk, pk = pc.recur_kernel(256, K, r.BW, B, c.nt), pc.prep_kernel(lv.L, lv.M, r.BW)
        assert c.recur in (None, rk[0]) and c.prep in (None, pk[0]), (c.id, rk, pk)
        recur.add(rk[0] + rk[1])
        prep.add(pk[0] + pk[1])
        if len(c.nu) == 1 and c.B >= len(c.nu[0]) - 1:  # dense one-dimensional windows: BW = n exactly
            assert r.BW == len(c.nu[0]), c.id
    assert recur >= {"k_pinf_recur<8,4>", "k_pinf_recur<16,4>", "k_pinf_recur<32,4>", "k_pinf_recur<64,4>",
                     "k_pinf_recur<8,1>", "k_pinf_recur<16,1>", "k_pinf_recur<32,1>", "k_pinf_recur<64,1>",
                     "k_pinf_recur_mcw<16>", "k_pinf_recur_mcw<32>", "k_pinf_recur_xr<32,8>", "k_pinf_recur_ws<4>",
                     "k_pinf_recur_ws<2>"}, recur
    assert prep == {"k_pinf_prep", "k_pinf_prep_small<8>", "k_pinf_prep_small<16>", "k_pinf_prep_m<2>",
                    "k_pinf_prep_m<3>", "k_pinf_prep_m<4>"}, prep
    Ls = {pc.levels_of(c)[0].L for c in pc.CASES}
    assert {64, 65, 256, 257, 4095, 4096, 4097} <= Ls


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_restatement_equals_oracle_fronts(oracle_c, case):
    """R_0 equals the row minima of the oracle's final front, and R_i at i in {1, nt//2, nt-2, nt-1} those of the
    suffix problem, for the first and the last subproblem of the batch."""
    lv, _, dfs, uos, B, beta, dt, K = pc.build(case)
    for k in sorted({0, K - 1}):
        ref = pc.reference_k(case, k)
        assert np.all(ref.R[:, B + 1:] == np.inf)
        for i in sorted({0, 1, case.nt // 2, case.nt - 2, case.nt - 1} & set(range(case.nt))):
            want = _row_minima(oracle_c, lv, dfs[k][:, i:], uos[k][:, i:], B, beta, dt)
            assert np.array_equal(ref.R[i, :B + 1], want), (case.id, k, i)


BRUTE = ("M1_16_nt2_B16_K1_gauss", "P1_2x2x2_nt6_B20_K1_zero", "P1_8x8_nt6_B20_K1_int", "P2_9x8c65_nt6_B20_K1_gauss",
         "P3_3p5_nt6_B20_K1_int")


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.id in BRUTE], ids=lambda c: c.id)
def test_class_tables_by_brute_force(case):
    """kmin and kfirst (and k2, kabs) of five small cases by a loop over the levels in rank order."""
    lv, _, dfs, uos, B, beta, dt, _ = pc.build(case)
    ref = pc.reference_k(case, 0)
    df, uo = dfs[0], uos[0]
    for i in range(case.nt):
        best, second, first, big = {}, {}, {}, 0.0
        for r in range(lv.L):
            nu = [float(x) for x in lv.nuval[r]]
            t = 0.0
            for m in range(lv.M):
                t = t + (dt * float(df[m, i])) * nu[m]
            v = t if i == case.nt - 1 else t + beta
            b = sum(int(abs(nu[m] - float(uo[m, i]))) for m in range(lv.M))
            if b >= ref.BW:
                continue
            big = max(big, abs(v))
            if b not in best or v < best[b]:
                if b in best:
                    second[b] = best[b]
                best[b], first[b] = v, r
            elif v != best[b] and v < second.get(b, np.inf):
                second[b] = v
        for b in range(ref.BWP):
            assert ref.kmin[i, b] == best.get(b, np.inf) and ref.kfirst[i, b] == first.get(b, -1), (case.id, i, b)
            assert ref.k2[i, b] == second.get(b, np.inf), (case.id, i, b)
        assert ref.kabs[i] == big


def _exposes(name, case, every_k=False):
    """Does the wrong version differ from the restatement on subproblem 0 (every_k: on any subproblem) of the case?"""
    lv, _, dfs, uos, B, beta, dt, K = pc.build(case)
    for k in range(K if every_k else 1):
        ref = pc.reference_k(case, k)
        if not pc.tables_equal(pc.MUTATIONS[name](lv, dfs[k], uos[k], B, beta, dt, ref.BW), ref):
            return True
    return False


# the cases that must expose a wrong version by name (each aimed at it)
AIMED = {
    "second_row_trip_missing": lambda c: c.id.startswith("R3_"),
    "extra_row_256_stale": lambda c: c.recur == "k_pinf_recur_xr" and c.nt >= 33,
    "stale_class_row_at_chunk": lambda c: c.id.startswith("R4_32_nt66"),       # 32-step chunks, 65 steps
    "stale_class_row_at_chunk64": lambda c: c.id.startswith("R1_8_nt130"),     # 64-step chunks, 129 steps
    "stale_rows_below_at_chunk": lambda c: c.id.startswith("M1_16_nt130_B39_K1"),
}


@pytest.mark.parametrize("name", list(pc.MUTATIONS))
def test_every_wrong_version_is_exposed(name):
    """Each wrong version differs from the restatement on subproblem 0 of at least one case, and the aimed cases
    expose theirs, every one of them (on some subproblem of its batch: the GPU test compares them all)."""
    if name in AIMED:
        aimed = [c for c in pc.CASES if AIMED[name](c)]
        missed = [c.id for c in aimed if not _exposes(name, c, every_k=True)]
        assert aimed and not missed, missed
        print(f"{name}: exposed by {[c.id for c in aimed]}")
        return
    hits = [c.id for c in pc.CASES if pc.levels_of(c)[0].L <= 257 and c.K(256) <= 8 and _exposes(name, c)]
    print(f"{name}: exposed by {len(hits)} cases, first {hits[:3]}")
    assert hits


@pytest.mark.parametrize("case", pc.CASES, ids=_IDS)
def test_conditions(case):
    """No case compares mostly +Inf with +Inf, ties and second minima are there to be got wrong (module docstring
    for the reach-limited shapes)."""
    lv, _, dfs, uos, B, _, _, K = pc.build(case)
    for k in sorted({0, K - 1}):
        ref = pc.reference_k(case, k)
        nt, step = case.nt, np.arange(case.nt)[:, None]
        rows = np.arange(B + 1)[None, :]
        if pc.reach_limited(case):
            asked = rows <= (nt - step) * (ref.BW - 1)
            top = int(sum(np.flatnonzero(np.isfinite(ref.kmin[i]))[-1] for i in range(nt)))
            assert top < B
        else:
            asked = np.ones((nt, B + 1), dtype=bool)
            top = B
        share = np.isfinite(ref.R[:, :B + 1])[asked].mean()
        assert share >= 0.5, (case.id, k, share)
        assert np.isfinite(ref.R[0, top]), (case.id, k)
        if case.mode == "zero":
            assert np.all(ref.k2 == np.inf)
            assert lv.L == 1 or any(np.sum(np.abs(lv.nuval - uos[k][:, i]).sum(axis=1) == b) >= 2
                                    for i in range(nt) for b in range(ref.BW))
    if case.mode != "zero" and lv.L > 1:  # a second minimum somewhere in the case
        assert any(np.isfinite(pc.reference_k(case, k).k2).any() for k in range(min(K, 8))), case.id
