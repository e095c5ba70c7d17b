"""The cases of test_gpu_ode_shapes.py on the CPU (tests/ode_cases.py): the restatement of k_ode_eval is pinned to
oracle/ode_oracle.py bit for bit at the examples' values and measured against an extended-precision reference of the
same recurrences on every case; every named wrong version of it shows where it must (and the parameter swaps do not
show at the examples' values, which is why the generic cases exist); and the inputs keep the conditions under which a
comparison means something (finite states, no tank near empty).
"""
import numpy as np
import pytest

import ode_cases as oc
from oracle import ode_oracle
from oracle.ode_oracle import ODEOracle

_IDS = [c.id for c in oc.CASES]


def _bits_differ(a, b):
    return not np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _exposed(c, wrong, restarts=3):
    """Some bit of J or df of the case's first restarts differs under the wrong version."""
    par, X, T0, T1 = oc.inputs(c)
    J, DF, _ = oc.mirror(c)
    for k in range(min(restarts, c.K)):
        Jw, dfw, _ = oc.eval_mirror(c.problem, par, X[k], T0, T1, wrong=wrong)
        if _bits_differ(Jw, J[k]) or _bits_differ(dfw, DF[k]):
            return True
    return False


def test_case_table():
    """Unique ids; the shapes the kernel's guards and branches turn on; parameters all distinct, inside the factors'
    range, T0 != 0 and a horizon of 2; half the steps one-hot, the other half with three non-integral components."""
    assert len(set(_IDS)) == len(_IDS)
    for pr in oc.PROBLEMS:
        shapes = {(c.nt, c.K) for c in oc.GENERIC if c.problem == pr and c.out == "both" and c.params == "generic"}
        assert shapes == {(1, 3), (2, 3), (130, 3), (130, 1), (130, 63), (130, 64), (130, 65), (130, 130)}
        assert {c.out for c in oc.GENERIC if c.problem == pr} == {"both", "J", "df"}
        assert sum(c.problem == pr and c.params == "default" for c in oc.CASES) == 1
        p, d = np.array(oc.generic_params(pr)), np.array(oc.DEFAULTS[pr])
        assert len(set(p)) == len(p) and p[-1] != p[-2]
        nz = d != 0
        assert np.all(p[~nz] == 0) and np.all((p[nz] / d[nz] >= 0.7) & (p[nz] / d[nz] <= 1.3))
        assert len(set(p[nz] / d[nz])) == int(nz.sum())
    po, pg = oc.generic_params("vanderpol", offset=True), oc.generic_params("vanderpol")
    assert po[:4] == pg[:4] and 0.7 * 0.3 <= po[4] <= 1.3 * 0.3 and len(set(po)) == 5
    assert [c.id for c in oc.GENERIC if c.params == "offset"] == ["vanderpol_nt1_K3_y0", "vanderpol_nt2_K3_y0"]
    for c in oc.GENERIC:
        _, X, T0, T1 = oc.inputs(c)
        assert X.shape == (c.K, c.nt, 3) and T0 != 0 and T1 - T0 == 2.0
        hot = np.all((X == 0) | (X == 1), axis=2) & (X.sum(axis=2) == 1)
        frac = np.all((X > 0) & (X < 1), axis=2)
        assert np.all(hot ^ frac)
        if c.nt > 1:
            assert np.all(np.abs(hot.sum(axis=1) - c.nt / 2) <= 0.5)
        if c.K > 1:
            assert hot.any() and frac.any()
    assert {oc.case(i).problem for i in oc.CONTEXT_SEQUENCE} == set(oc.PROBLEMS)
    # the entry's defaults are the oracle's example constants
    f, t, v = ode_oracle.FISHING, ode_oracle.DOUBLETANK, ode_oracle.VANDERPOL
    assert oc.DEFAULTS["fishing"] == (f["alpha"], f["beta"], f["gamma"], f["delta"], f["c1"], f["c2"], *f["v1"],
                                      *f["v2"], *f["state0"])
    assert oc.DEFAULTS["doubletank"] == (t["k1"], t["k2"], *t["c"], *t["state0"])
    assert oc.DEFAULTS["vanderpol"] == (*v["c"], *v["state0"])
    assert all(oc.EXAMPLE_T[pr] == (o["T0"], o["T1"]) for pr, o in zip(oc.PROBLEMS, (f, t, v)))


@pytest.mark.parametrize("case", [c for c in oc.CASES if c.params == "default"], ids=lambda c: c.id)
def test_mirror_equals_oracle_at_defaults(case):
    """J, df and every state, bit for bit, for every restart of the default case."""
    par, X, T0, T1 = oc.inputs(case)
    assert par is None
    J, DF, ST = oc.mirror(case)
    o = ODEOracle(case.problem, case.nt)
    assert (o.T0, o.T1) == (T0, T1)
    for k in range(case.K):
        x = [tuple(float(v) for v in r) for r in X[k]]
        Jo, dfo = o.eval_df(x)
        _, sto = o.eval_f(x, keep_states=True)
        assert J[k] == Jo and np.array_equal(DF[k], np.array(dfo)) and np.array_equal(ST[k], np.array(sto)), k
        assert np.all(np.isfinite(DF[k])) and np.isfinite(Jo)


def test_reference_precision():
    """numpy.longdouble carries at least 64 bits here; the distances below mean nothing otherwise."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_input_conditions():
    """On the reference alone: every state of every case except the NaN restart is finite, and every doubletank
    state of the generic and default cases is above 0.1 (the neighbours of the NaN restart start at 0.01 by the
    case's definition; they stay positive)."""
    low = np.inf
    for c in oc.CASES:
        par, X, T0, T1 = oc.inputs(c)
        _, _, ST = oc.eval_reference(c.problem, par, X, T0, T1)
        keep = np.ones(c.K, dtype=bool)
        if c.params == "nan":
            keep[oc.NAN_RESTART] = False
            assert np.isnan(ST[oc.NAN_RESTART, -1]).all() and np.isfinite(ST[oc.NAN_RESTART, 0]).all()
            first = int(np.flatnonzero(np.isnan(ST[oc.NAN_RESTART]).any(axis=1))[0])
            assert 2 <= first <= 40, first  # dry within a few steps, not at once
            assert np.all(ST[keep] > 0)
        assert np.all(np.isfinite(ST[keep].astype(np.float64))), c.id
        if c.problem == "doubletank" and c.params != "nan":
            low = min(low, float(ST.min()))
    print(f"smallest doubletank state {low:.3f}")
    assert low > 0.1


def test_mirror_distance_to_reference():
    """The mirror's relative distance to the extended-precision reference on every case; the largest per problem is the
    figure of ode_cases.MIRROR_DISTANCE (not below the measurement, not more than twice it)."""
    worst = dict.fromkeys(oc.PROBLEMS, 0.0)
    for c in oc.CASES:
        par, X, T0, T1 = oc.inputs(c)
        J, DF, _ = oc.mirror(c)
        Jr, DFr, _ = oc.eval_reference(c.problem, par, X, T0, T1)
        keep = np.ones(c.K, dtype=bool)
        if c.params == "nan":
            keep[oc.NAN_RESTART] = False
            k = oc.NAN_RESTART
            assert np.isnan(Jr[k]) and np.isnan(DFr[k]).all() and np.isnan(J[k]) and np.isnan(DF[k]).all()
        d = oc.distance(J[keep], DF[keep], Jr[keep], DFr[keep])
        assert d < 1e-11, (c.id, d)  # float64 against longdouble over at most 400 steps: a wrong formula is O(1)
        worst[c.problem] = max(worst[c.problem], d)
    print("mirror distance to the reference:", {k: f"{v:.3e}" for k, v in worst.items()})
    for pr in oc.PROBLEMS:
        assert worst[pr] <= oc.MIRROR_DISTANCE[pr] <= 2 * worst[pr], (pr, worst[pr])


_PARAM = sorted(n for n, (_, kind) in oc.WRONG.items() if kind == "param")
_STRUCT = sorted(n for n, (_, kind) in oc.WRONG.items() if kind == "struct")


def test_wrong_version_list():
    assert len(_PARAM) == 10 and len(_STRUCT) == 8
    assert {oc.WRONG[n][0][0] for n in _PARAM} == set(oc.PROBLEMS)


@pytest.mark.parametrize("wrong", _PARAM)
def test_parameter_swaps_show_on_generic_cases_only(wrong):
    """Exposed by a generic case of its problem (here: by every one of them with nt >= 2; after a single step
    doubletank's J and df do not depend on c, nor Van der Pol's from y0[1] = 0), and not by the default case of that
    problem where the swapped entries are equal -- the swaps of unequal defaults show there as well."""
    pr = oc.WRONG[wrong][0][0]
    cases = [c for c in oc.GENERIC if c.problem == pr and c.out == "both" and c.nt >= 2]
    assert len(cases) >= 6 and all(_exposed(c, wrong) for c in cases)
    default = next(c for c in oc.CASES if c.problem == pr and c.params == "default")
    d = oc.DEFAULTS[pr]
    perm = oc._PARAM_WRONG[wrong][1]
    invisible = all(d[q] == d[perm[q]] for q in range(len(d)))
    assert _exposed(default, wrong, restarts=default.K) == (not invisible)
    if wrong in ("alpha_beta_swapped", "gamma_delta_swapped", "c1_c2_swapped", "tank_y0_swapped"):
        assert invisible, wrong


@pytest.mark.parametrize("wrong", _STRUCT)
def test_structural_mistakes_show_on_every_generic_case(wrong):
    """Every generic case with nt >= 2 exposes it, for every problem -- except the pairs of ode_cases.BLIND, where the
    problem's hook does not read the argument the mistake changes, and those of BLIND_NT2 at Van der Pol's nt = 2 from
    y0[1] = 0 (the same shape from another y0 exposes them), and the fused Euler step at nt = 2, where tau = 1.0 makes
    its product exact: there the wrong version computes the same, and that is asserted too."""
    for c in oc.GENERIC:
        if c.nt < 2 or c.out != "both":
            continue
        blind_nt2 = c.nt == 2 and ((c.problem, wrong) in oc.BLIND_NT2_ANY_Y0 or
                                   (c.problem, wrong) in oc.BLIND_NT2 and c.params == "generic")
        if (c.problem, wrong) in oc.BLIND or blind_nt2:
            assert not _exposed(c, wrong), c.id
        else:
            assert _exposed(c, wrong), c.id


def test_rand_start_restatement_properties():
    """The restatement itself: exactly `jumps` distinct candidate times in 1..nt-1 (all of them at jumps = nt - 1),
    columns that are level rows, changes only at candidates, and a table of cases that covers the issue's list."""
    from mioc.iterators import LevelTable, product_iterator
    lts = {n: LevelTable(nu, product_iterator(nu)) for n, nu in oc.RS_TABLES.items()}
    assert [lts[n].L for n in ("L1", "L3_M1", "L15_3x5", "L256_M8")] == [1, 3, 15, 256]
    assert lts["L256_M8"].M == 8 and oc.RS_MAX_NT == 516096
    assert ((oc.RS_MAX_NT + 31) // 32 + 256) * 4 == 65536
    for nt in oc.RS_NT:
        js = oc.rs_jumps(nt)
        assert -1 in js and {nt // 10 if j < 0 else j for j in js} == {j for j in (0, 1, nt // 10, nt - 1) if j < nt}
        for j in js:
            jv = nt // 10 if j < 0 else j
            for k in (0, 2):
                u, S = oc.rand_start_host(lts["L15_3x5"], nt, jv, oc.RS_SEEDS[1], k)
                assert u.shape == (2, nt) and len(S) == jv and all(1 <= t <= nt - 1 for t in S)
                if jv == nt - 1:
                    assert S == set(range(1, nt))
                rows = {tuple(r) for r in lts["L15_3x5"].nuval}
                assert all(tuple(col) in rows for col in u.T)
                changes = set((np.flatnonzero(np.any(u[:, 1:] != u[:, :-1], axis=0)) + 1).tolist())
                assert changes <= S
