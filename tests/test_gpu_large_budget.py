"""GPU parity at trust-region budgets of 1024 rows and more: libmioc against the C oracle, bit for bit.

B = floor(Δ/τ) is the second dimension of every DP front.  The other modules stop at B = 819; the code below only
runs above that.  Every case compares u and Φ* with the oracle at several budgets of one DP (a budget the oracle
finds infeasible must raise on the device too) and requires diagnostics()[3] == 0.  The p = Inf cases run with the
segmented walk (MIOC_OPT_PINF_WALK = 1) and with the serial walk (-1) and assert through kernel_stats(0)[2] which
recursion kernel took the DP.  ncu: the device's CU count (256 on an MI355X), read from torch.

  case  levels, nt, B                              kernel(s) the case pins                       oracle: budget -> spent
  ----  -----------------------------------------  --------------------------------------------  -----------------------
  P1    [[0,7]] (BWP 8), nt 2400, B 7935            k_pinf_recur_ws, 124 segments; k_pinf_fseg    7935->7931 7168->7168
        (RP = 7936, the admitted maximum)           slots e = 0..7; ftab_steps 1; 8-row walk      6000->5999 4096->4095
                                                    chunks; serial walk: band of 16-step chunks   2048->2044 1029->1029
                                                                                                  1022->1022 7->7 6->0 0->0
  P1r   P1, MIOC_OPT_SPIN_LIMIT = 1                 the gated one-workgroup redo                  as P1
                                                    k_pinf_recur<8,4>, 16 row trips per step
  P2a   [0..7]x[-1..2] (L 32, BWP 16), nt 520,      k_pinf_recur_mcw, one segment per CU          B, B-1, B/2 in full
        B 8 ncu - 1                                                                               (2047, 2046, 1023)
  P2b   the same, B 8 ncu                           one segment too many: k_pinf_recur<16,4>,     B, B-1, B/2 in full
                                                    5 row trips per step                          (2048, 2047, 1024)
  P3    SOS1 [[0,1]]x3, u_old + 20 in all three     k_pinf_recur<64,4> at its largest LDS         7935->7846 7600->7600
        controls on ~30 % of the steps (b~ = 60,    request (157 KB); serial walk: a band of      3967 infeasible
        BWP 64), nt 400, B 7935                     8-step chunks (16-step chunks would need
                                                    537 KB of LDS: found by this case)
  P3b   P3's construction, nt 200, B 3967           k_pinf_recur<64,4>, 8 row trips; serial walk  3967->3966 3800->3800
        (RP = 3968 < two 16-step bands)             staging whole rows, one step per chunk        1983 infeasible
  P4    [[0,7]], K = max(65, ncu/4 + 1) by the      k_pinf_recur<8,1> (4 K > ncu), a second,      1100->1099 1029->1029
        batch tensor API, nt 400, B 1100            partial row trip; serial walk with K > 64     1022->1022 550->546
                                                                                                  (every subproblem)
  P5    [[0,7]], nt 40, B 7936                      the gate RP <= 7936: forced MIOC_ALGO_PINF    (nt 40 can spend 280
                                                    is MIOC_EINVAL, AUTO takes another algorithm  at most: no condition)
  F1    [[-2..2]] (L 5), p 1, beta 1e-4, nt 1500,   k_fused_run at its task-count limit;          2024->2024 1012->1012
        B 2024 (largest fused_eligible) and 2025    B + 1: forced FUSED is MIOC_EINVAL, AUTO      2025->2025
                                                    takes another algorithm
  F2    [[-2,0,3]] (L 3), p 1, beta 0.1, nt 900,    k_fused_run at its LDS limit; B + 1 as F1     3387->2319 1693->1693
        B 3387 and 3388, dt 1                                                                     3388->2319
  G1    F2's inputs, B 3000, forced GENERIC         k_generic_step over 47 row tiles, uint8 U     3000->2319 1500->1500
  S1    [0..7]^3, p 1, beta 0.3, K 2, nt 64,        chunked persistent k_sdt_run: 128 workgroups  300->300 150->150
        B 300, MIOC_OPT_SDT_BUFFERS 29              per subproblem, 2-3 rows each, the staging    (both subproblems)
                                                    ring wraps twice

F1, F2, G1 and S1 also compare the argmin table on 32 sampled steps (step 0, step nt - 2, for S1 the steps on either
side of the ring wraps) with test_gpu_parity._assert_U.

Condition, not a measurement: each case first asserts, from the oracle's result alone, that its path starts where the
case is aimed: the full-budget backtrack spends sum |u - u_old|_1 >= 1025 rows (S1, whose B is 300, excepted) and
>= B - 7 rows for P1, P2 and S1, and P1's budgets start in at least four different 1024-row blocks, the first and the last among them.  The last column was
computed on the CPU with these seeds; after a change of seed or size, check it there before a GPU run.
"""
import numpy as np
import pytest

from mioc import native
from mioc.iterators import LevelTable
from oracle.oracle import P_INF, P_ONE, Levels
from test_gpu_parity import _assert_U

pytestmark = pytest.mark.gpu

_BETA_INF, _DT_INF = 1e-3, 2.0 ** -6


def _ncu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _draw(lv, nt, rng):
    """Gaussian df, u_old a random level per step."""
    df = rng.standard_normal((lv.M, nt))
    uo = np.ascontiguousarray(lv.nuval[rng.integers(lv.L, size=nt)].T, dtype=np.float64)
    return df, uo


def _fused_bmax(L):
    B = max(b for b in range(8192) if native.fused_eligible(L, b))
    assert native.fused_eligible(L, B) and not native.fused_eligible(L, B + 1)
    return B


def problem(case, ncu=256):
    """(levels, [(df, u_old)] per subproblem, p_kind, beta, dt) of a case: pure numpy, shared with the CPU check."""
    if case == "P1":
        lv = Levels.product([[0, 7]])
        return lv, [_draw(lv, 2400, np.random.default_rng(101))], P_INF, _BETA_INF, _DT_INF
    if case == "P2":
        lv = Levels.product([list(range(8)), list(range(-1, 3))])
        return lv, [_draw(lv, 520, np.random.default_rng(102))], P_INF, _BETA_INF, _DT_INF
    if case in ("P3", "P3b"):
        lv = Levels.bounded_sum([[0, 1]] * 3, 1, 1)
        nt, seed = (400, 113) if case == "P3" else (200, 120)
        rng = np.random.default_rng(seed)
        df, uo = _draw(lv, nt, rng)
        uo[:, rng.random(nt) < 0.3] += 20.0
        return lv, [(df, uo)], P_INF, _BETA_INF, _DT_INF
    if case == "P4":
        lv = Levels.product([[0, 7]])
        rng = np.random.default_rng(104)
        return lv, [_draw(lv, 400, rng) for _ in range(max(65, ncu // 4 + 1))], P_INF, _BETA_INF, _DT_INF
    if case == "P5":
        lv = Levels.product([[0, 7]])
        return lv, [_draw(lv, 40, np.random.default_rng(105))], P_INF, _BETA_INF, _DT_INF
    if case == "F1":
        lv = Levels.product([[-2, -1, 0, 1, 2]])
        return lv, [_draw(lv, 1500, np.random.default_rng(106))], P_ONE, 1e-4, 2.0 ** -6
    if case in ("F2", "G1"):
        lv = Levels.product([[-2, 0, 3]])
        return lv, [_draw(lv, 900, np.random.default_rng(107))], P_ONE, 0.1, 1.0
    if case == "S1":
        lv = Levels.product([list(range(8))] * 3)
        rng = np.random.default_rng(108)
        return lv, [_draw(lv, 64, rng) for _ in range(2)], P_ONE, 0.3, 1.0
    raise KeyError(case)


def budgets(case, B):
    if case == "P1":
        return (7935, 7168, 6000, 4096, 2048, 1029, 1022, 7, 6, 0)
    if case == "P3":
        return (7935, 7600, B // 2)
    if case == "P3b":
        return (3967, 3800, B // 2)
    if case == "P4":
        return (1100, 1029, 1022, 550)
    if case == "P2":
        return (B, B - 1, B // 2)
    return (B, B // 2, 0) if case == "P5" else (B, B // 2)


def table_steps(case, nt):
    """32 sampled steps of the argmin table: step 0, step nt - 2, for S1 both sides of the ring wraps (29, 58)."""
    must = {0, nt - 2} | ({28, 29, 30, 57, 58, 59} if case == "S1" else set())
    fill = [int(x) for x in np.linspace(0, nt - 2, 64)]
    steps = sorted(must)
    for s in fill[::2] + fill[1::2]:
        if len(steps) >= 32:
            break
        if s not in steps:
            steps.append(s)
    return sorted(steps)


def oracle_answers(oracle_c, case, B, ncu=256, with_tables=False, threads=1):
    """Per subproblem: {budget: (u, Φ*) or None where the oracle finds no finite value}, and the sampled U steps."""
    lv, subs, pk, beta, dt = problem(case, ncu)
    out = []
    for df, uo in subs:
        phi, U = oracle_c.bellman(lv, df, uo, B, pk, beta, dt, threads=threads)
        ans = {}
        for Bp in budgets(case, B):
            try:
                ans[Bp] = oracle_c.backtrack(lv, uo, phi, U, B, Bp)
            except Exception:
                ans[Bp] = None
        Us = None
        if with_tables:
            Us = np.ascontiguousarray(U[:, :, table_steps(case, df.shape[1])])
        out.append((ans, Us))
    return out


def aimed(case, B, subs, answers):
    """The condition of the module docstring, from the oracle's result alone."""
    for (df, uo), (ans, _) in zip(subs, answers):
        if case == "P5":
            continue
        full = ans[B]
        assert full is not None, f"{case}: the full budget is infeasible"
        spent = int(np.abs(full[0] - uo).sum())
        if case != "S1":  # (S1 is aimed at more rows than CUs per subproblem: B = 300, and all of it spent)
            assert spent >= 1025, f"{case}: the full-budget path starts at row {spent}"
        if case in ("P1", "P2", "S1"):
            assert spent >= B - 7, f"{case}: the full-budget path starts at row {spent} of {B}"
        if case == "P1":
            blocks = {int(np.abs(a[0] - uo).sum()) // 1024 for a in ans.values() if a is not None}
            assert len(blocks) >= 4 and 0 in blocks and B // 1024 in blocks, sorted(blocks)


_CACHE = {}


def _oracle(oracle_c, case, B, ncu, with_tables=False, threads=1):
    """One oracle DP per (case, B) for the whole module; its answers are read, never changed."""
    key = (case, B, ncu)
    if key not in _CACHE:
        _CACHE[key] = oracle_answers(oracle_c, case, B, ncu, with_tables, threads)
        aimed(case, B, problem(case, ncu)[1], _CACHE[key])
    return _CACHE[key]


def _lt(lv):
    return LevelTable(lv.nu, [tuple(int(x) for x in t) for t in lv.tuples])


def _ctx(lv, pk, beta, algo, **opts):
    ctx = native.Context(0)
    ctx.set_levels(_lt(lv))
    ctx.set_cost(None, beta, p_kind=pk)
    ctx.set_option(native.MIOC_OPT_ALGO, algo)
    ctx.set_option(native.MIOC_OPT_TIMING, 1)
    for o, v in opts.items():
        ctx.set_option(getattr(native, o), v)
    return ctx


def _compare_single(ctx, ans, tag, walk=None, strict_segmented=False):
    for Bp, o in ans.items():
        if o is None:
            with pytest.raises(native.MiocNativeError):
                ctx.backtrack(Bp)
            continue
        u, ps, _ = ctx.backtrack(Bp)
        d = ctx.diagnostics()
        assert np.array_equal(u, o[0]), f"{tag} B'={Bp}: u differs at steps {np.nonzero((u != o[0]).any(axis=0))[0][:8]}"
        assert ps == o[1], f"{tag} B'={Bp}: {ps!r} vs {o[1]!r}"
        assert d[3] == 0, d
        if walk is not None:  # [9]: subproblems the segmented walk left to the serial walk (-1: serial walk alone)
            assert d[9] in ((0,) if strict_segmented else (0, 1)) if walk == 1 else d[9] == -1, d


class _Sampled:
    """The steps of table_steps as steps 0, 1, ... for _assert_U."""

    def __init__(self, ctx, steps, k=0):
        self.ctx, self.steps, self.k = ctx, steps, k

    def argmin_table(self, i):
        return self.ctx.argmin_table(self.steps[i], k=self.k)


def _compare_tables(ctx, case, nt, Us, tag, k=0):
    steps = table_steps(case, nt)
    assert len(steps) == 32 and Us.shape[2] == 32
    _assert_U(_Sampled(ctx, steps, k), Us, len(steps) + 1, f"{tag} sampled steps {steps}")


WALKS = pytest.mark.parametrize("walk", [1, -1], ids=["segmented_walk", "serial_walk"])


@WALKS
@pytest.mark.parametrize("spin", [0, 1], ids=["P1", "P1r"])
def test_p1_ws_124_segments(oracle_c, walk, spin):
    lv, subs, pk, beta, dt = problem("P1")
    B = 7935
    (ans, _), = _oracle(oracle_c, "P1", B, 0)
    opts = {"MIOC_OPT_PINF_WALK": walk}
    if spin:
        opts["MIOC_OPT_SPIN_LIMIT"] = 1
    ctx = _ctx(lv, pk, beta, native.MIOC_ALGO_PINF, **opts)
    ctx.bellman(*subs[0], B, dt)
    # (after an abandoned launch the gated one-workgroup redo runs behind it, under the same window name)
    assert ctx.kernel_stats(0)[2] == "k_pinf_recur_ws"
    _compare_single(ctx, ans, f"P1 spin={spin}", walk, strict_segmented=True)
    d = ctx.diagnostics()
    assert d[6] >= 1 if spin else d[6] == 0, d
    ctx.close()


@WALKS
@pytest.mark.parametrize("extra", [0, 1], ids=["P2a", "P2b"])
def test_p2_mcw_one_segment_per_cu(oracle_c, walk, extra):
    ncu = _ncu()
    lv, subs, pk, beta, dt = problem("P2")
    B = 8 * ncu - 1 + extra
    (ans, _), = _oracle(oracle_c, "P2", B, 0)
    ctx = _ctx(lv, pk, beta, native.MIOC_ALGO_PINF, MIOC_OPT_PINF_WALK=walk)
    ctx.bellman(*subs[0], B, dt)
    assert ctx.kernel_stats(0)[2] == ("k_pinf_recur" if extra else "k_pinf_recur_mcw")
    _compare_single(ctx, ans, f"P2 B={B}", walk)
    assert ctx.diagnostics()[6] == 0
    ctx.close()


@WALKS
@pytest.mark.parametrize("case, B", [("P3", 7935), ("P3b", 3967)], ids=["P3", "P3b"])
def test_p3_recur_64_classes(oracle_c, walk, case, B):
    lv, subs, pk, beta, dt = problem(case)
    (ans, _), = _oracle(oracle_c, case, B, 0)
    assert ans[B // 2] is None  # infeasible on the oracle's side: the device must raise too
    ctx = _ctx(lv, pk, beta, native.MIOC_ALGO_PINF, MIOC_OPT_PINF_WALK=walk)
    ctx.bellman(*subs[0], B, dt)
    assert ctx.kernel_stats(0)[2] == "k_pinf_recur"
    _compare_single(ctx, ans, case, walk)
    assert ctx.diagnostics()[6] == 0
    ctx.close()


@WALKS
def test_p4_batch_two_row_trips(oracle_c, walk):
    import torch
    ncu = _ncu()
    lv, subs, pk, beta, dt = problem("P4", ncu)
    K, B = len(subs), 1100
    assert K > 64 and 4 * K > ncu
    answers = _oracle(oracle_c, "P4", B, ncu)
    ddf = torch.tensor(np.ascontiguousarray(np.stack([d.T for d, _ in subs])), dtype=torch.float64, device="cuda")
    duo = torch.tensor(np.ascontiguousarray(np.stack([u.T for _, u in subs])), dtype=torch.float64, device="cuda")
    du = torch.empty_like(ddf)
    dphi = torch.empty(K, dtype=torch.float64, device="cuda")
    dst = torch.empty(K, dtype=torch.int32, device="cuda")
    ctx = _ctx(lv, pk, beta, native.MIOC_ALGO_PINF, MIOC_OPT_PINF_WALK=walk)
    torch.cuda.synchronize()
    ctx.bellman_batch_tensors(ddf, duo, B, dt)
    ctx.synchronize()
    assert ctx.kernel_stats(0)[2] == "k_pinf_recur"
    for Bp in budgets("P4", B):
        ctx.backtrack_batch_tensors(Bp, du, dphi, dst)
        ctx.synchronize()
        ub, pb, st = du.cpu().numpy(), dphi.cpu().numpy(), dst.cpu().numpy()
        for k, (ans, _) in enumerate(answers):
            if ans[Bp] is None:
                assert st[k] != 0, (k, Bp)
                continue
            assert st[k] == 0 and np.array_equal(ub[k].T, ans[Bp][0]) and pb[k] == ans[Bp][1], (k, Bp)
        d = ctx.diagnostics()
        assert d[3] == 0 and (d[9] in (0, 1) if walk == 1 else d[9] == -1), d
    assert ctx.diagnostics()[6] == 0
    ctx.close()


def test_p5_pinf_gate(oracle_c):
    lv, subs, pk, beta, dt = problem("P5")
    B = 7936  # RP = 8000 after rounding to 64: one tile past the collapse's limit
    (ans, _), = _oracle(oracle_c, "P5", B, 0)
    ctx = _ctx(lv, pk, beta, native.MIOC_ALGO_PINF)
    with pytest.raises(native.MiocNativeError) as e:
        ctx.bellman(*subs[0], B, dt)
    assert e.value.code == native.MIOC_EINVAL
    ctx.bellman(*subs[0], B - 1, dt)  # the admitted maximum
    assert ctx.last_algo() == native.MIOC_ALGO_PINF
    ctx.set_option(native.MIOC_OPT_ALGO, native.MIOC_ALGO_AUTO)
    ctx.bellman(*subs[0], B, dt)
    assert ctx.last_algo() not in (native.MIOC_ALGO_AUTO, native.MIOC_ALGO_PINF)
    _compare_single(ctx, ans, "P5 auto")
    ctx.close()


@pytest.mark.parametrize("case", ["F1", "F2"])
def test_fused_at_its_limits(oracle_c, case):
    lv, subs, pk, beta, dt = problem(case)
    df, uo = subs[0]
    Bmax = _fused_bmax(lv.L)
    # at the limit: the fused DP
    (ans, Us), = _oracle(oracle_c, case, Bmax, 0, with_tables=True)
    ctx = _ctx(lv, pk, beta, native.MIOC_ALGO_FUSED)
    ctx.bellman(df, uo, Bmax, dt)
    assert ctx.last_algo() == native.MIOC_ALGO_FUSED and ctx.kernel_stats(0)[2] == "k_fused_run"
    _compare_single(ctx, ans, f"{case} B={Bmax}")
    _compare_tables(ctx, case, df.shape[1], Us, f"{case} B={Bmax}")
    # one past it: refused when forced, another algorithm under AUTO
    (ans, Us), = _oracle(oracle_c, case, Bmax + 1, 0, with_tables=True)
    with pytest.raises(native.MiocNativeError) as e:
        ctx.bellman(df, uo, Bmax + 1, dt)
    assert e.value.code == native.MIOC_EINVAL
    ctx.set_option(native.MIOC_OPT_ALGO, native.MIOC_ALGO_AUTO)
    ctx.bellman(df, uo, Bmax + 1, dt)
    assert ctx.last_algo() not in (native.MIOC_ALGO_AUTO, native.MIOC_ALGO_FUSED)
    _compare_single(ctx, ans, f"{case} B={Bmax + 1} auto")
    _compare_tables(ctx, case, df.shape[1], Us, f"{case} B={Bmax + 1} auto")
    ctx.close()


def test_g1_generic_many_row_tiles(oracle_c):
    lv, subs, pk, beta, dt = problem("G1")
    df, uo = subs[0]
    B = 3000
    (ans, Us), = _oracle(oracle_c, "G1", B, 0, with_tables=True)
    ctx = _ctx(lv, pk, beta, native.MIOC_ALGO_GENERIC)
    ctx.bellman(df, uo, B, dt)
    assert ctx.last_algo() == native.MIOC_ALGO_GENERIC and ctx.kernel_stats(0)[2] == "k_generic_step"
    _compare_single(ctx, ans, "G1")
    _compare_tables(ctx, "G1", df.shape[1], Us, "G1")
    ctx.close()


def test_s1_chunked_persistent_separable_wrapping_ring(oracle_c):
    import torch
    lv, subs, pk, beta, dt = problem("S1")
    K, B, nt = len(subs), 300, subs[0][0].shape[1]
    answers = _oracle(oracle_c, "S1", B, 0, with_tables=True, threads=16)
    ddf = torch.tensor(np.ascontiguousarray(np.stack([d.T for d, _ in subs])), dtype=torch.float64, device="cuda")
    duo = torch.tensor(np.ascontiguousarray(np.stack([u.T for _, u in subs])), dtype=torch.float64, device="cuda")
    du = torch.empty_like(ddf)
    dphi = torch.empty(K, dtype=torch.float64, device="cuda")
    dst = torch.empty(K, dtype=torch.int32, device="cuda")
    ctx = _ctx(lv, pk, beta, native.MIOC_ALGO_SEPARABLE, MIOC_OPT_SDT_BUFFERS=29)
    torch.cuda.synchronize()
    ctx.bellman_batch_tensors(ddf, duo, B, dt)
    for Bp in budgets("S1", B):
        ctx.backtrack_batch_tensors(Bp, du, dphi, dst)
        ctx.synchronize()
        ub, pb, st = du.cpu().numpy(), dphi.cpu().numpy(), dst.cpu().numpy()
        for k, (ans, _) in enumerate(answers):
            assert ans[Bp] is not None
            assert st[k] == 0 and np.array_equal(ub[k].T, ans[Bp][0]) and pb[k] == ans[Bp][1], (k, Bp)
    assert ctx.last_algo() == native.MIOC_ALGO_SEPARABLE and ctx.kernel_stats(0)[2] == "k_sdt_run"
    d = ctx.diagnostics()
    assert d[3] == 0 and d[6] == 0, d  # no spin-limit redo hid a stall of the wrapping ring
    for k, (_, Us) in enumerate(answers):
        _compare_tables(ctx, "S1", nt, Us, f"S1 k={k}", k=k)
    ctx.close()
