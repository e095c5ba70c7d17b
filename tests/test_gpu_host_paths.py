"""GPU: two host-side paths of mioc_api.cpp that no other test walks.

* The fused separable DP asked for more row segments than the device can keep resident: the host declines the
  segmented launch before it is issued (nothing is launched that cannot run) and runs the DP again with one
  workgroup per subproblem, counted in diagnostics [6].
* One context whose two DP slots (inputs and p = Inf tables, mioc_ctx::Slot) are allocated and reused at different
  sizes while the p = Inf backtracks overlap the next DP.
"""
import numpy as np
import pytest

from mioc import native
from mioc.synth import CONFIGS, make_inputs

pytestmark = pytest.mark.gpu


def _batch(cfg, K, nt, k0=0):
    import torch
    lt = cfg.levels()
    dfs, uos = [], []
    for k in range(k0, k0 + K):
        _, df, uo = make_inputs(cfg, k=k, nt=nt, levels=lt)
        dfs.append(df.T)
        uos.append(uo.T)
    ddf = torch.tensor(np.ascontiguousarray(np.stack(dfs)), dtype=torch.float64, device="cuda")
    duo = torch.tensor(np.ascontiguousarray(np.stack(uos)), dtype=torch.float64, device="cuda")
    return lt, ddf, duo


def _fsep(lt, cfg, ddf, duo, B, seg, steps=()):
    """One fused separable DP + backtrack on a fresh context: (diagnostics before, after, u, Φ*, status, U tables)."""
    import torch
    K = ddf.shape[0]
    with native.Context(0) as ctx:
        ctx.set_levels(lt)
        ctx.set_cost(cfg.p, cfg.beta)
        ctx.set_option(native.MIOC_OPT_ALGO, native.MIOC_ALGO_FUSED_SEPARABLE)
        ctx.set_option(native.MIOC_OPT_FSEP_SEGMENTS, seg)
        before = ctx.diagnostics()
        du = torch.empty_like(ddf)
        dphi = torch.empty(K, dtype=torch.float64, device="cuda")
        dst = torch.empty(K, dtype=torch.int32, device="cuda")
        ctx.bellman_batch_tensors(ddf, duo, B, cfg.dt)
        ctx.backtrack_batch_tensors(B, du, dphi, dst)
        ctx.synchronize()
        after = ctx.diagnostics()
        tabs = [ctx.argmin_table(i, k=k) for k in (0, K - 1) for i in steps]
    return before, after, du.cpu().numpy(), dphi.cpu().numpy(), dst.cpu().numpy(), tabs


def test_fsep_segments_not_all_resident_fall_back():
    """C5 levels (6x6), nt = 4, B = 200, 8 row segments forced.  K = 2 runs segmented ([8] == 8).  Its diagnostics
    [7] is not the device's capacity, though: with at most one segment per CU to go round (8 K <= ncu) the host
    reserves more than half a CU's LDS per workgroup, which makes [7] == 1 (measured on the MI355X: [7] == 1 at
    K = 2, and 8 at K = 33).  So K = ncu / 8 + 1, the smallest batch without that reservation, tells the resident
    workgroups per CU, and K = ncu · [7] / 8 + 1 subproblems are one more than the device can hold as 8 segments
    each: the DP runs with one workgroup per subproblem ([8] == 1), the fallback is counted once ([6]), and u, Φ*,
    the status and the U tables equal a run that asked for one segment."""
    import torch
    cfg = CONFIGS["C5"]
    nt, B = 4, 200
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    occ = 0
    for K in (2, ncu // 8 + 1):
        lt, ddf, duo = _batch(cfg, K, nt)
        _, d, *_ = _fsep(lt, cfg, ddf, duo, B, 8)
        print("K =", K, "diagnostics", d)
        assert d[8] == 8 and d[7] >= 1 and d[6] == 0, d
        occ = int(d[7])
    K = ncu * occ // 8 + 1
    lt, ddf, duo = _batch(cfg, K, nt)
    steps = (0, nt - 2)
    b8, a8, u8, phi8, st8, tabs8 = _fsep(lt, cfg, ddf, duo, B, 8, steps)
    b1, a1, u1, phi1, st1, tabs1 = _fsep(lt, cfg, ddf, duo, B, 1, steps)
    print("K =", K, "ncu =", ncu, "8 segments asked: diagnostics", a8, "one segment:", a1)
    assert a8[6] == b8[6] + 1, (b8, a8)
    assert a8[8] == 1, a8
    assert a1[6] == b1[6] and a1[8] == 1, a1
    assert np.array_equal(u8, u1) and np.array_equal(phi8, phi1) and np.array_equal(st8, st1)
    assert np.all(st1 == 0)
    for x, y in zip(tabs8, tabs1):
        assert np.array_equal(x, y)


def test_pinf_slots_keep_their_buffers_across_sizes():
    """p = Inf, C1 levels, K = 1, one context: bellman(nt = 64), backtrack, bellman(nt = 256), backtrack,
    bellman(nt = 64), backtrack, no host synchronisation in between -- each DP takes the other slot, the slots'
    buffers are allocated at different sizes and the first one is reused.  Every u and Φ* equals a fresh context's."""
    import torch
    cfg = CONFIGS["C1"]
    probs = [_batch(cfg, 1, nt, k0=10 * q) for q, nt in enumerate((64, 256, 64))]
    lt = probs[0][0]

    def solve(ctx, ddf, duo):
        du = torch.empty_like(ddf)
        dphi = torch.empty(1, dtype=torch.float64, device="cuda")
        dst = torch.empty(1, dtype=torch.int32, device="cuda")
        ctx.bellman_batch_tensors(ddf, duo, cfg.B, cfg.dt)
        ctx.backtrack_batch_tensors(cfg.B, du, dphi, dst)
        return du, dphi, dst

    ctx = native.Context(0)
    ctx.set_levels(lt)
    ctx.set_cost(cfg.p, cfg.beta)
    got = [solve(ctx, ddf, duo) for _, ddf, duo in probs]
    ctx.synchronize()
    assert ctx.last_algo() == native.MIOC_ALGO_PINF
    got = [tuple(t.cpu().numpy() for t in g) for g in got]
    ctx.close()
    for q, (_, ddf, duo) in enumerate(probs):
        with native.Context(0) as fresh:
            fresh.set_levels(lt)
            fresh.set_cost(cfg.p, cfg.beta)
            want = solve(fresh, ddf, duo)
            fresh.synchronize()
            want = tuple(t.cpu().numpy() for t in want)
        assert want[2][0] == 0 and np.all(np.isfinite(want[1])), f"DP {q}"
        for g, w in zip(got[q], want):
            assert np.array_equal(g, w), f"DP {q}"
