"""GPU parity of every reader of Ψ in the separable transform's row body, with Ψ kept once in the LDS at the swizzled
position of its rank (mioc_sdt.hip: psi[sd_swz(j)]; the transform buffer holds only pass outputs), on all three drivers:
the one-row persistent driver k_sdt_run1 (MIOC_OPT_SDT_ROW_OWNER = 1), the general persistent driver k_sdt_run (= 0) and
one launch per step, k_sdt_step (MIOC_OPT_PERSIST = 0) -- 8^4 levels with B in {28, 57}, 8^3 with B in {22, 43}, nt <= 5.

The readers, and the inputs that reach them:

  * pass 0 and the certified winners' Ψ_j* (every transform row);
  * the counting redo's pass 0 (diagnostics [5] > 0), the cooperative scans (at most SD_COOP listed targets: thread t
    reads sources t + T·s), the per-wave scans (up to SD_LCAP listed: lane + 64·t) and the overflow sweep (more than
    SD_LCAP listed, 8^4 only: a row has at most L targets) -- exact ties: zero gradients, or two equal gradient components
    with u_old on that diagonal;
  * the sparse fill (at most SD_SPARSE finite sources: the first steps after the terminal one);
  * the one-target item (row B, u_old on the grid);
  * direct rows (two to SD_FEW targets: row B - 1 of an 8^3 grid with u_old at a corner, 1 + M = SD_FEW targets).

Every case first shows on the CPU, from a census of the oracle's fronts (tests/sdt_census.py), that it holds an item of
each path it names; for the tie paths the census gives the exact number of listed targets of the item.  Then, per
driver: U equal wherever the oracle wrote it, u and Φ* equal at B' in {B, B // 2, 1}; device against device the whole
tables, and diagnostics [0], [1], [4], [5], [6] between the persistent drivers, [0], [5], [6] with the per-step driver
(its row B counts a direct row wherever u_old is on the grid, [1]; it has no ring, [4]).  Lower bounds that the census
implies are asserted on the device: [0] >= the tied targets of the censused items, [5] >= the censused items with a tie,
and for the persistent drivers [1] == the direct rows' targets + the one-target rows.
"""
import functools

import numpy as np
import pytest

import sdt_census as sc
from mioc import native
from mioc.iterators import LevelTable
from mioc.synth import CONFIGS, make_inputs
from oracle.oracle import P_ONE, Levels, OracleC, OracleError

CFG = CONFIGS["C4"]
THREADS = 8
ONE_ROW, GENERAL, STEPS = "one-row", "general", "steps"
DRIVERS = (ONE_ROW, GENERAL, STEPS)


@functools.lru_cache(maxsize=None)
def _levels(M):
    if M == 4:
        lt = CFG.levels()
        return lt, Levels(lt.nu, [tuple(int(x) for x in t) for t in lt.tuples])
    nu = [list(range(8))] * M
    return LevelTable(nu), Levels.product(nu)


def _cols(cols):
    return np.asfortranarray(np.array(cols, dtype=np.float64).T)


def _sym_df(M, nt, seed):
    """Generic gradients with components 0 and 1 equal: Ψ is symmetric under swapping those coordinates."""
    df = np.asfortranarray(np.random.default_rng(seed).standard_normal((M, nt)))
    df[1] = df[0]
    return df


# name: (M, B, df, u_old, the paths the case must reach, the items whose ties are censused (None: every transform item))
def _g4_generic():
    _, df, uo = make_inputs(CFG, nt=4, levels=_levels(4)[0])
    return 4, 57, df, uo, ("winners", "sparse", "one-target"), ()


def _g4_zero():
    uo = _cols([(0, 0, 0, 0), (3, 3, 3, 3), (4, 4, 4, 4)])
    return 4, 28, np.zeros((4, 3), order="F"), uo, ("winners", "sparse", "one-target", "redo", "coop", "wave", "overflow"), \
        ((0, 26), (0, 25), (1, 5))


def _g3_generic():
    df = np.asfortranarray(np.random.default_rng(3).standard_normal((3, 5)))
    uo = _cols([(0, 0, 0), (3, 4, 3), (7, 7, 7), (2, 5, 3), (0, 7, 0)])
    return 3, 22, df, uo, ("winners", "sparse", "one-target", "direct"), ()


def _g3_sym():
    uo = _cols([(3, 3, 2), (4, 4, 3), (2, 2, 5), (5, 5, 1), (3, 3, 3)])
    return 3, 43, _sym_df(3, 5, 7), uo, ("winners", "sparse", "one-target", "redo", "coop", "wave"), None


def _g3_zero():
    uo = _cols([(0, 0, 0), (3, 4, 3), (7, 7, 7), (2, 5, 3), (0, 7, 0)])
    return 3, 22, np.zeros((3, 5), order="F"), uo, ("winners", "direct", "redo", "coop", "wave"), None


CASES = {"g4-generic-B57": _g4_generic, "g4-zero-B28": _g4_zero, "g3-generic-B22": _g3_generic, "g3-sym-B43": _g3_sym,
         "g3-zero-B22": _g3_zero}
EXTRA = {}  # cases of other test files that run through this file's rig (tests/test_gpu_sdt_edge_rows.py)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs, the oracle's result and the census of one case, computed once for its three drivers."""
    M, B, df, uo, paths, tie_items = (CASES.get(name) or EXTRA[name])()
    lv = _levels(M)[1]
    phi, U = OracleC().bellman(lv, df, uo, B, P_ONE, CFG.beta, CFG.dt, threads=THREADS)
    fronts = sc.source_fronts(lv, df, uo, B, CFG.beta, CFG.dt, threads=THREADS)
    cls = sc.classes(lv, uo, B, fronts)
    if tie_items is None:
        tie_items = [k for k, v in cls.items() if v[0] == "transform"]
    ties = {}
    for k in tie_items:
        assert cls[k][0] == "transform", (name, k, cls[k])
        t, near = sc.item_ties(lv, df, uo, B, CFG.beta, CFG.dt, fronts, *k)
        if t == near:  # the item's listed targets are exactly its tied ones
            ties[k] = t
    return M, B, df, uo, phi, U, paths, cls, ties


def _reached(cls, ties):
    kinds = {v[0] for v in cls.values()}
    got = set()
    if "transform" in kinds:
        got.add("winners")
    got |= kinds & {"sparse", "one-target", "direct"}
    if any(t > 0 for t in ties.values()):
        got.add("redo")
    if any(1 <= t <= sc.SD_COOP for t in ties.values()):
        got.add("coop")
    if any(sc.SD_COOP < t <= sc.SD_LCAP for t in ties.values()):
        got.add("wave")
    if any(t > sc.SD_LCAP for t in ties.values()):
        got.add("overflow")
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_psi_copy_census(name):
    """On the CPU: the case holds an item of every path it names."""
    M, B, df, uo, phi, U, paths, cls, ties = _case(name)
    assert df.shape[1] <= 6
    got = _reached(cls, ties)
    print(name, sorted(got), "censused items with a tie:", sum(t > 0 for t in ties.values()))
    assert set(paths) <= got, (name, sorted(set(paths) - got))


def test_psi_copy_cases_cover_every_reader():
    want = {"winners", "redo", "coop", "wave", "overflow", "sparse", "one-target", "direct"}
    for M in (3, 4):
        have = set().union(*(CASES[n]()[4] for n in CASES if CASES[n]()[0] == M))
        # a row of an 8^3 grid has at most 512 = SD_LCAP targets; an 8^4 row with a target inside has at least 1 + 4 > SD_FEW
        assert want - have == ({"overflow"} if M == 3 else {"direct"}), (M, want - have)
    assert {(CASES[n]()[0], CASES[n]()[1]) for n in CASES} == {(4, 28), (4, 57), (3, 22), (3, 43)}


def _ctx(M, driver):
    ctx = native.Context(0)
    ctx.set_levels(_levels(M)[0])
    ctx.set_cost(1, CFG.beta)
    ctx.set_option(native.MIOC_OPT_TIMING, 1)
    ctx.set_option(native.MIOC_OPT_ALGO, native.MIOC_ALGO_SEPARABLE)
    ctx.set_option(native.MIOC_OPT_PERSIST, int(driver != STEPS))
    ctx.set_option(native.MIOC_OPT_SDT_ROW_OWNER, int(driver == ONE_ROW))
    return ctx


def _run(oracle_c, name, driver):
    M, B, df, uo, phi, U, paths, cls, ties = _case(name)
    lv = _levels(M)[1]
    label = f"{name} {driver}"
    ctx = _ctx(M, driver)
    ctx.bellman(df, uo, B, CFG.dt)
    ctx.synchronize()
    assert ctx.kernel_stats(0)[2] == ("k_sdt_step" if driver == STEPS else "k_sdt_run"), label
    if driver != STEPS:
        assert ctx.last_sdt_driver() == (2 if driver == ONE_ROW else 1), label
    diag = ctx.diagnostics()
    assert diag[6] == 0, (label, diag)
    tabs = [ctx.argmin_table(i) for i in range(df.shape[1] - 1)]
    for i, d in enumerate(tabs):
        o = U[:, :, i]
        m = o >= 0
        assert np.array_equal(d[m], o[m]), f"{label}: U at step {i}"
    res = []
    for Bp in (B, B // 2, 1):
        try:
            ou, ops = oracle_c.backtrack(lv, uo, phi, U, B, Bp)
        except OracleError as e:
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
    # what the census implies for the device's counters
    print(label, "diagnostics", list(diag[:7]))
    assert diag[0] >= sum(ties.values()), (label, diag, sum(ties.values()))
    assert diag[5] >= sum(t > 0 for t in ties.values()), (label, diag)
    if driver != STEPS:
        want1 = sum(v[2] for v in cls.values() if v[0] == "direct") + sum(v[0] == "one-target" for v in cls.values())
        assert diag[1] == want1, (label, diag, want1)
    return tabs, res, diag


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_psi_copy_every_reader_on_every_driver(oracle_c, name):
    run_drivers(oracle_c, name)


def run_drivers(oracle_c, name):
    """The case under the three drivers: each against the oracle and the census, then one against the other."""
    runs = {d: _run(oracle_c, name, d) for d in DRIVERS}
    t1, r1, d1 = runs[ONE_ROW]
    for other, slots in ((GENERAL, (0, 1, 4, 5, 6)), (STEPS, (0, 5, 6))):
        t0, r0, d0 = runs[other]
        for i, (a, b) in enumerate(zip(t1, t0)):
            assert np.array_equal(a, b), f"{name}: U of {ONE_ROW} and {other} differ at step {i}"
        for a, b in zip(r1, r0):
            assert (a is None) == (b is None) and (a is None or (np.array_equal(a[0], b[0]) and a[1] == b[1])), name
        assert [d1[q] for q in slots] == [d0[q] for q in slots], (name, other, d1, d0)
