"""GPU parity of the p=Inf collapse (csrc/mioc_pinf.hip) per kernel instantiation, table cell by cell.

Every case of tests/pinf_cases.py runs one DP with MIOC_ALGO_PINF forced, asserts by name which recursion and which
class-table kernel took it (mioc_kernel_stats windows 0 and 2), reads every row of R, kmin, k2, kfirst and kabs of
every step of every subproblem back (mioc_get_pinf_tables) and compares it with the plain restatement
pinf_cases.pinf_tables_ref bit for bit, +Inf and -1 included: min is exact and every candidate fl(kmin_i[b] +
R_{i+1}[c-b]) is the same expression in every kernel, as their own comments state.  tests/test_pinf_cases.py pins the
restatement to the C oracle on the CPU.  Then u and Φ* equal the oracle at the budgets {B, B//2, a seeded one, 0}.

The dispatch conditions are written in the device's CU count (256 on an MI355X): K is computed from it, and a case
whose condition another count cannot meet is skipped, never asserted against another kernel.

The row-segment kernel is k_pinf_recur_mcw (8-row segments, 64-step hand-off chunks, a 128-slot LDS ring of step
arrays) at 16 and 32 classes; 8 classes take k_pinf_recur_ws or k_pinf_recur.  Its predecessor without helper waves,
k_pinf_recur_mc, which no input could reach, has been removed.

The walks: the segmented walk at its segment-count boundaries and at one step, the serial walk's exact scan (whole rows
staged, and inside a band), and the serial walk around its staged chunk.
"""
import numpy as np
import pytest

import pinf_cases as pc
from mioc import native
from mioc.iterators import LevelTable
from oracle.oracle import P_INF, Levels

pytestmark = pytest.mark.gpu


def _ncu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _ctx(lt, beta, walk=0):
    ctx = native.Context(0)
    ctx.set_levels(lt)
    ctx.set_cost(None, beta, p_kind=P_INF)
    ctx.set_option(native.MIOC_OPT_ALGO, native.MIOC_ALGO_PINF)
    ctx.set_option(native.MIOC_OPT_TIMING, 1)
    if walk:
        ctx.set_option(native.MIOC_OPT_PINF_WALK, walk)
    return ctx


def _assert_tables(ctx, case, k, ref):
    for i in range(case.nt):
        t = ctx.pinf_tables(i, k)
        where = f"{case.id} k={k} step {i}"
        assert (t.BW, t.BWP, t.RP) == (ref.BW, ref.BWP, ref.RP), where
        for name in ("kmin", "k2", "kfirst", "R"):
            got, want = getattr(t, name), getattr(ref, name)[i]
            if not np.array_equal(got, want):
                bad = np.flatnonzero(~((got == want) | ((got != got) & (want != want))))
                raise AssertionError(f"{where}: {name} differs at {bad[:8].tolist()} ({bad.size} cells): "
                                     f"{got[bad[:4]].tolist()} vs {want[bad[:4]].tolist()}")
        assert t.kabs == ref.kabs[i], f"{where}: kabs {t.kabs!r} vs {ref.kabs[i]!r}"


@pytest.mark.parametrize("case", pc.CASES, ids=[c.id for c in pc.CASES])
def test_tables_cell_by_cell(oracle_c, case):
    ncu = _ncu()
    lv, lt, dfs, uos, B, beta, dt, K = pc.build(case, ncu)
    nt, BW = case.nt, pc.batch_bw(lv, uos, B)
    recur, prep = pc.recur_kernel(ncu, K, BW, B, nt), pc.prep_kernel(lv.L, lv.M, BW)
    if case.recur is not None and recur[0] != case.recur:
        pytest.skip(f"{ncu} CUs cannot meet this case's condition ({case.recur}: {case.edge})")
    assert case.prep in (None, prep[0])
    rng = np.random.default_rng(len(case.id) + 131 * nt + B)
    budgets = sorted({B, B // 2, int(rng.integers(0, B + 1)), 0})
    with _ctx(lt, beta) as ctx:
        if K == 1:
            ctx.bellman(dfs[0], uos[0], B, dt)
        else:
            import torch
            dev = torch.device("cuda:0")
            df_t = torch.tensor(np.stack([d.T for d in dfs]), dtype=torch.float64, device=dev).contiguous()
            uo_t = torch.tensor(np.stack([u.T for u in uos]), dtype=torch.float64, device=dev).contiguous()
            ub = torch.empty_like(df_t)
            pb = torch.empty(K, dtype=torch.float64, device=dev)
            st = torch.empty(K, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()  # the library runs on its own stream
            ctx.bellman_batch_tensors(df_t, uo_t, B, dt)
        ctx.synchronize()
        names = ctx.kernel_stats(0)[2], ctx.kernel_stats(2)[2]
        print(f"{case.id}: {names[0]}{recur[1]} {names[1]}{prep[1]} K={K} BW={BW}")
        assert names[0] == (case.recur or recur[0]), names
        assert names[1] == (case.prep or prep[0]), names
        for k in range(K):
            _assert_tables(ctx, case, k, pc.reference_k(case, k, ncu))
        assert ctx.diagnostics()[6] == 0  # no segmented launch was abandoned and redone by another kernel
        got = {}
        for Bp in budgets:
            if K == 1:
                u, ps, _ = ctx.backtrack(Bp)
                got[Bp] = ([u], [ps])
            else:
                ctx.backtrack_batch_tensors(Bp, ub, pb, st)
                ctx.synchronize()
                assert not st.cpu().numpy().any()
                got[Bp] = ([x.T for x in ub.cpu().numpy()], pb.cpu().numpy().tolist())
        assert ctx.diagnostics()[3] == 0
    threads = 16 if lv.L > 1024 else 1
    for k in range(K):
        phi, U = oracle_c.bellman(lv, dfs[k], uos[k], B, P_INF, beta, dt, threads=threads)
        for Bp in budgets:
            ou, ops = oracle_c.backtrack(lv, uos[k], phi, U, B, Bp)
            assert np.array_equal(got[Bp][0][k], ou), f"{case.id} k={k} B'={Bp}"
            assert got[Bp][1][k] == ops, f"{case.id} k={k} B'={Bp}: {got[Bp][1][k]!r} vs {ops!r}"


def test_accessor_contract(oracle_c):
    """mioc_get_pinf_tables: MIOC_ESTATE without a DP, MIOC_EINVAL out of range and after another algorithm, sizes
    alone with every other pointer NULL, and a rejected call changes nothing."""
    lv = Levels.product([[0, 1, 2]])
    lt = LevelTable(lv.nu, [tuple(t) for t in lv.tuples])
    rng = np.random.default_rng(3)
    df, uo = rng.standard_normal((1, 5)), np.zeros((1, 5))
    with _ctx(lt, 0.1) as ctx:
        with pytest.raises(native.MiocNativeError) as e:
            ctx.pinf_tables(0)
        assert e.value.code == native.MIOC_ESTATE
        ctx.bellman(df, uo, 7, 0.5)
        ref = pc.pinf_tables_ref(lv, df, uo, 7, 0.1, 0.5)
        before = ctx.pinf_tables(4)
        assert (before.BW, before.BWP, before.RP) == (3, 8, 64) and np.array_equal(before.R, ref.R[4])
        for step, k in ((5, 0), (-1, 0), (0, 1), (0, -1)):
            with pytest.raises(native.MiocNativeError) as e:
                ctx.pinf_tables(step, k)
            assert e.value.code == native.MIOC_EINVAL
        after = ctx.pinf_tables(4)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        u, ps, _ = ctx.backtrack(7)
        phi, U = oracle_c.bellman(lv, df, uo, 7, P_INF, 0.1, 0.5)
        ou, ops = oracle_c.backtrack(lv, uo, phi, U, 7, 7)
        assert np.array_equal(u, ou) and ps == ops
    with native.Context(0) as ctx:
        ctx.set_levels(lt)
        ctx.set_cost(None, 0.1, p_kind=P_INF)
        ctx.set_option(native.MIOC_OPT_ALGO, native.MIOC_ALGO_GENERIC)
        ctx.bellman(df, uo, 7, 0.5)
        with pytest.raises(native.MiocNativeError) as e:
            ctx.pinf_tables(0)
        assert e.value.code == native.MIOC_EINVAL
        assert ctx.argmin_table(0).shape == (8, 3)


# ------------------------------------------------------------------ the walks --------------------------------------

def _walk_vs_oracle(oracle_c, lv, df, uo, B, beta, dt, walk, budgets):
    lt = LevelTable(lv.nu, [tuple(t) for t in lv.tuples])
    phi, U = oracle_c.bellman(lv, df, uo, B, P_INF, beta, dt)
    diags = []
    with _ctx(lt, beta, walk) as ctx:
        ctx.bellman(df, uo, B, dt)
        for Bp in budgets:
            ou, ops = oracle_c.backtrack(lv, uo, phi, U, B, Bp)
            u, ps, _ = ctx.backtrack(Bp)
            assert np.array_equal(u, ou), f"B'={Bp}"
            assert ps == ops, f"B'={Bp}: {ps!r} vs {ops!r}"
            diags.append(ctx.diagnostics())
    return diags


@pytest.mark.parametrize("mode", ["gauss", "zero"])
@pytest.mark.parametrize("nt", [1, 2, 65, 66, 130, 1026])
def test_segmented_walk_at_its_edges(oracle_c, nt, mode):
    """MIOC_OPT_PINF_WALK = 1 on [[0..7]], B = 40: one step (the nt == 1 branch of launch_pinf_fwalk), nt - 1 = 64 | 65
    (one and two segments of 64 steps), 129, and 1025 (segments of 128 steps, nine of them); the class table is built
    eight steps per workgroup and 65, 129 and 1025 are no multiples of 8."""
    lv = Levels.product([list(range(8))])
    rng = np.random.default_rng(900 + nt)
    df = np.zeros((1, nt)) if mode == "zero" else rng.standard_normal((1, nt))
    uo = rng.integers(0, 8, size=(1, nt)).astype(np.float64)
    for d in _walk_vs_oracle(oracle_c, lv, df, uo, 40, 0.25, 1 / 3, 1, (40, 20, 7, 0)):
        assert d[9] in (0, 1) and d[3] == 0, d


def _state_dependent(nt, seed=7, tiny=1e-10):
    """One step with costs near 1e6, then class values `tiny` apart: fl(K_l + V_b) collapses classes for the large K_l
    of the walker's level, so which classes match depends on the walker's state."""
    rng = np.random.default_rng(seed)
    df = rng.standard_normal((1, nt)) * tiny
    df[0, 0] = -1e6
    return Levels.product([[0, 1, 2, 3]]), df, np.zeros((1, nt))


def _first_step_needs_the_scan(lv, df, uo, B, beta, dt):
    """From the definition alone (the restatement's tables): the walk's start (c0, l0) = the first minimum of Φ_0 in
    the reference's column-major order, Φ_0[c, l] = fl(K_l(0) + R_1[c - b~_l]), and whether at step 1 a class b matches
    the walker's target with its minimum AND with its second value, fl(K_l0 + fl(k2_1[b] + R_2[c' - b])) == Φ_0[c0, l0]:
    the one situation the class tables cannot resolve (k_pinf_walk's `amb`).  Returns (Φ*, l0, needs)."""
    ref = pc.pinf_tables_ref(lv, df, uo, B, beta, dt)
    best = None
    for l in range(lv.L):
        Kl = (dt * df[0, 0]) * float(lv.nuval[l, 0]) + beta
        bl = int(abs(lv.nuval[l, 0] - uo[0, 0]))
        for c in range(bl, B + 1):
            v = Kl + ref.R[1][c - bl]
            if best is None or v < best[0]:
                best = (v, c - bl, l, Kl)
    target, cp, l0, Kr = best
    b = np.arange(min(ref.BW, cp + 1))
    V, V2 = ref.kmin[1][b] + ref.R[2][cp - b], ref.k2[1][b] + ref.R[2][cp - b]
    match = np.isfinite(V) & (Kr + V == target)
    return target, l0, bool(np.any(match & np.isfinite(V2) & (Kr + V2 == target)))


@pytest.mark.parametrize("B", [40, 255])
def test_serial_walk_exact_scan(oracle_c, B):
    """The serial walk (MIOC_OPT_PINF_WALK = -1) at nt = 100, one step with costs near 1e6 and then tiny ones: with
    B = 40 it stages whole rows, with B = 255 the band of pinf_plan (RP = 256 >= 2·W, W = 106); the exact scan runs in
    both (diagnostics [2]).

    The construction of test_segmented_walk_state_dependent_rows_vs_oracle itself (levels 0..3, u_old = 0) cannot
    reach the serial walk's scan: each of its classes holds one level, so k2 = +Inf everywhere and k_pinf_walk's
    `amb` is never true (measured: diagnostics [2] = 0 at both budgets, u and Φ* equal to the oracle).  With every
    value tied under the rounding of 3e6 the walk also starts in the lowest row and spends as little as it can, so it
    only ever stands in class 0, which on the level grid is one level.  Hence: levels {0, 2, 3} and u_old = 1 at the
    steps 1..5, where the cheapest class is class 1 = {0, 2}, and small gradients of 1e-12, so that its two values lie
    well inside one rounding unit of 3e6 (4.7e-10) (at 1e-10 whether they do depends on the seed).
    _first_step_needs_the_scan derives from the tables that the walker's first step is then ambiguous, before the
    device is asked."""
    assert pc.walk_chunk(4, B)[1] == (B == 255)
    _, df, uo = _state_dependent(100, tiny=1e-12)
    lv = Levels.product([[0, 2, 3]])
    uo[0, 1:6] = 1.0
    assert pc.batch_bw(lv, [uo], B) == 4
    target, l0, needs = _first_step_needs_the_scan(lv, df, uo, B, 1e-3, 1.0)
    phi, U = oracle_c.bellman(lv, df, uo, B, P_INF, 1e-3, 1.0)
    ou, ops = oracle_c.backtrack(lv, uo, phi, U, B, B)
    assert needs and target == ops and lv.nuval[l0, 0] == ou[0, 0]
    diags = _walk_vs_oracle(oracle_c, lv, df, uo, B, 1e-3, 1.0, -1, (B,))
    print(f"serial walk B={B}: exact scans {diags[0][2]}")
    assert diags[0][2] >= 1 and diags[0][3] == 0 and diags[0][9] == -1, diags


@pytest.mark.parametrize("mode", ["gauss", "state"])
@pytest.mark.parametrize("off", [-1, 0, 1])
@pytest.mark.parametrize("B", [40, 255])
def test_serial_walk_around_its_chunk(oracle_c, B, off, mode):
    """nt - 1 one below, at and one above the chunk the serial walk stages for these shapes (32 steps of whole rows at
    B = 40, 16 steps of the band at B = 255)."""
    ch, band = pc.walk_chunk(4, B)
    assert (ch, band) == ((16, True) if B == 255 else (32, False))
    nt = ch + off + 1
    lv, df, uo = _state_dependent(nt, seed=11 + off)
    if mode == "gauss":
        rng = np.random.default_rng(40 + B + off)
        df = rng.standard_normal((1, nt))
        uo = rng.integers(0, 4, size=(1, nt)).astype(np.float64)
        uo[0, 0] = 0.0  # four classes, as pinf_cases.walk_chunk(4, B) assumes
    for d in _walk_vs_oracle(oracle_c, lv, df, uo, B, 1e-3, 1.0, -1, (B, B // 2, 0)):
        assert d[3] == 0 and d[9] == -1, d
