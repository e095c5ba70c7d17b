"""GPU parity of the one-row persistent driver of the separable transform (k_sdt_run1: every workgroup owns one budget
row for the whole launch) against the CPU oracle, and device against device with MIOC_OPT_SDT_ROW_OWNER = 0 (the general
driver k_sdt_run on the same inputs) -- C4's 8^4 = 4096 levels, β and Δt, p = 1 (and one 8^3 case):

  * steady state (B = 64, nt = 8: the case of test_gpu_c4_rows.py): rows <= 28, interior rows, rows > B - 28 and row B in
    one launch, the sphere-order slot's reuse flag both 0 and 1;
  * ring wrap (B = 64, nt = 40 at 29 and 37 staging buffers): the write-after-read polls are armed, diagnostics [4] equals
    the general driver's and the closed form (nt - NB)·(B - 1) > 0; at the default buffer count it is 0;
  * u_old off the grid inside the dependency window, at step i, at i + 1 and at both, with a smallest b̃ of 1 and of 3:
    the one-target row is then B - 1 or B - 3, not row B;
  * the smallest shapes: nt = 2 (one item, no next item), nt = 3, B = 1 (row B is also a row <= 28), B = 29 and B = 57
    (the row classes' boundaries meet);
  * the sparse threshold: rows 1-3 with 4, 5 and 6 finite sources (B = 64, nt = 3 and 4, as test_gpu_c4_rows.py);
  * a spin limit of one poll: the launch is abandoned, diagnostics [6] counts the redo, the results equal the oracle's and
    the context runs the next DP;
  * 8^3 levels (B = 64, nt = 8): the M = 3 instantiation;
  * K = 2, B = 200, nt = 6: 128 workgroups per subproblem, so the general driver runs, and stays correct.

Every case asserts through last_sdt_driver() which driver ran (the timing label is "k_sdt_run" for both).  Device
against device: the argmin table of every step, u and Φ* at B' in {B, B // 2, 1} and diagnostics [0], [1], [4], [5],
[6] are equal.
"""
import functools

import numpy as np
import pytest

from mioc import native
from mioc.iterators import LevelTable
from mioc.synth import CONFIGS, make_inputs
from oracle.oracle import P_ONE, Levels, OracleC, OracleError

pytestmark = pytest.mark.gpu

CFG = CONFIGS["C4"]
THREADS = 8  # the oracle's result does not depend on it
GENERAL, ONE_ROW = 1, 2  # last_sdt_driver()
DIAG = (0, 1, 4, 5, 6)


@functools.lru_cache(maxsize=None)
def _levels(M=4):
    if M == 4:
        lt = CFG.levels()
        return lt, Levels(lt.nu, [tuple(int(x) for x in t) for t in lt.tuples])
    nu = [list(range(8))] * M
    return LevelTable(nu), Levels.product(nu)


def _cols(cols):
    return np.asfortranarray(np.array(cols, dtype=np.float64).T)


def _oracle(M, df, uo, B):
    return OracleC().bellman(_levels(M)[1], df, uo, B, P_ONE, CFG.beta, CFG.dt, threads=THREADS)


def _ctx(owner, M=4, nb=None):
    ctx = native.Context(0)
    ctx.set_levels(_levels(M)[0])
    ctx.set_cost(1, CFG.beta)
    ctx.set_option(native.MIOC_OPT_TIMING, 1)
    ctx.set_option(native.MIOC_OPT_ALGO, native.MIOC_ALGO_SEPARABLE)
    ctx.set_option(native.MIOC_OPT_PERSIST, 1)
    ctx.set_option(native.MIOC_OPT_SDT_ROW_OWNER, owner)
    if nb is not None:
        ctx.set_option(native.MIOC_OPT_SDT_BUFFERS, nb)
    return ctx


def _tables(ctx, nt, k=0):
    return [ctx.argmin_table(i, k=k) for i in range(nt - 1)]


def _compare_oracle(ctx, oracle_c, lv, uo, phi, U, B, label):
    """As test_gpu_c4_rows.py's _compare; returns what the device-against-device comparison needs."""
    tabs = _tables(ctx, U.shape[2] + 1)
    for i, d in enumerate(tabs):
        o = U[:, :, i]
        m = o >= 0
        assert np.array_equal(d[m], o[m]), f"{label}: U at step {i}"
    res = []
    for Bp in (B, B // 2, 1):
        try:
            ou, ops = oracle_c.backtrack(lv, uo, phi, U, B, Bp)
        except OracleError as e:  # no finite Φ_0 within B': the device says the same
            assert e.args == (native.MIOC_EINFEASIBLE,), e
            with pytest.raises(native.MiocNativeError) as err:
                ctx.backtrack(Bp)
            assert err.value.code == native.MIOC_EINFEASIBLE, f"{label}: B'={Bp}"
            res.append(None)
            continue
        u, ps, _ = ctx.backtrack(Bp)
        assert np.array_equal(u, ou) and ps == ops, f"{label}: B'={Bp}: {ps!r} vs {ops!r}"
        res.append((u, ps))
    return tabs, res


def _run(oracle_c, df, uo, phi, U, B, owner, label, M=4, nb=None):
    ctx = _ctx(owner, M, nb)
    ctx.bellman(df, uo, B, CFG.dt)
    ctx.synchronize()
    assert ctx.kernel_stats(0)[2] == "k_sdt_run"
    assert ctx.last_sdt_driver() == (ONE_ROW if owner else GENERAL), f"{label}: driver {ctx.last_sdt_driver()}"
    diag = ctx.diagnostics()
    assert diag[6] == 0, diag
    tabs, res = _compare_oracle(ctx, oracle_c, _levels(M)[1], uo, phi, U, B, label)
    ctx.close()
    return tabs, res, diag


def _both(oracle_c, df, uo, phi, U, B, label, M=4, nb=None):
    """The case under the one-row driver and under the general driver: each against the oracle, then one against the
    other (the whole tables, also where the oracle left a cell unwritten).  Returns the one-row driver's diagnostics."""
    t1, r1, d1 = _run(oracle_c, df, uo, phi, U, B, 1, f"{label} one-row", M, nb)
    t0, r0, d0 = _run(oracle_c, df, uo, phi, U, B, 0, f"{label} general", M, nb)
    for i, (a, b) in enumerate(zip(t1, t0)):
        assert np.array_equal(a, b), f"{label}: the drivers' U differ at step {i}"
    for a, b in zip(r1, r0):
        assert (a is None) == (b is None) and (a is None or (np.array_equal(a[0], b[0]) and a[1] == b[1])), label
    assert [d1[q] for q in DIAG] == [d0[q] for q in DIAG], (label, d1, d0)
    return d1


@functools.lru_cache(maxsize=None)
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- steady state ---------------------------------------------------------------------------------------------------
STEADY_B, STEADY_NT = 64, 8


def _steady_uold(nt):
    rng = np.random.default_rng(8)
    a, b = (tuple(int(x) for x in rng.integers(0, 8, size=4)) for _ in range(2))
    assert a != b
    cyc = [(0, 0, 0, 0), (3, 4, 3, 4), (0, 0, 0, 0), a, b, a, (7, 7, 7, 7), (4, 3, 4, 4)]
    return _cols([cyc[i % len(cyc)] for i in range(nt)])


@functools.lru_cache(maxsize=None)
def _steady_case():
    lt, lv = _levels()
    _, df, _ = make_inputs(CFG, nt=STEADY_NT, levels=lt)
    uo = _steady_uold(STEADY_NT)
    same2 = [bool(np.array_equal(uo[:, s - 1], uo[:, s + 1])) for s in range(1, STEADY_NT - 1)]
    assert any(same2) and not all(same2), same2
    return (df, uo) + tuple(_oracle(4, df, uo, STEADY_B))


def test_row_owner_steady_state(oracle_c):
    assert STEADY_B > 2 * 28  # rows <= 28, rows in between, rows > B - 28, row B
    df, uo, phi, U = _steady_case()
    _both(oracle_c, df, uo, phi, U, STEADY_B, "steady")


# ---- ring wrap ------------------------------------------------------------------------------------------------------
WRAP_B, WRAP_NT = 64, 40


@functools.lru_cache(maxsize=None)
def _wrap_case():
    lt, lv = _levels()
    _, df, _ = make_inputs(CFG, nt=WRAP_NT, levels=lt)
    uo = _steady_uold(WRAP_NT)
    return (df, uo) + tuple(_oracle(4, df, uo, WRAP_B))


@pytest.mark.parametrize("nb", [29, 37, None], ids=["nb29", "nb37", "nb-default"])
def test_row_owner_ring_wrap(oracle_c, nb):
    df, uo, phi, U = _wrap_case()
    diag = _both(oracle_c, df, uo, phi, U, WRAP_B, f"wrap nb={nb}", nb=nb)
    if nb is None:
        assert diag[4] == 0, diag  # 256 buffers: the ring never wraps in 40 steps
    else:
        # items (c', i) with c' < B and token(i + NB - 1) = nt - i - NB > 0
        assert diag[4] == (WRAP_NT - nb) * (WRAP_B - 1) > 0, diag


# ---- u_old off the grid inside the dependency window ----------------------------------------------------------------
OFF_B, OFF_NT = 64, 4
OFF = {1: (8, 3, 4, 2), 3: (10, 3, 4, 2)}  # outside in dimension 0 by 1 / by 3: b̃ in 1..21 / 3..23, all <= 7·M
ON = [(3, 3, 3, 3), (4, 4, 4, 4), (3, 4, 3, 4), (4, 3, 4, 4)]
OFF_AT = {"step-i": (1,), "step-i+1": (2,), "both": (1, 2)}


@functools.lru_cache(maxsize=None)
def _offgrid_case(name, bmin):
    lt, lv = _levels()
    _, df, _ = make_inputs(CFG, nt=OFF_NT, levels=lt)
    uo = _cols([OFF[bmin] if i in OFF_AT[name] else ON[i] for i in range(OFF_NT)])
    nuv = np.asarray(lv.nuval, dtype=np.int64)
    for i in OFF_AT[name]:  # the smallest b̃ of the off-grid step: its one-target row is B - bmin
        bt = np.abs(nuv - uo[:, i].astype(np.int64)).sum(axis=1)
        assert bt.min() == bmin and bt.max() <= 28 and (bt == bmin).sum() == 1, (bt.min(), bt.max())
    return (df, uo) + tuple(_oracle(4, df, uo, OFF_B))


@pytest.mark.parametrize("bmin", [1, 3])
@pytest.mark.parametrize("name", list(OFF_AT))
def test_row_owner_offgrid(oracle_c, name, bmin):
    df, uo, phi, U = _offgrid_case(name, bmin)
    _both(oracle_c, df, uo, phi, U, OFF_B, f"offgrid {name} b̃>={bmin}")


# ---- the smallest shapes --------------------------------------------------------------------------------------------
EDGES = [(64, 2), (64, 3), (1, 4), (29, 4), (57, 4)]  # (B, nt)


@functools.lru_cache(maxsize=None)
def _edge_case(B, nt):
    lt, lv = _levels()
    _, df, uo = make_inputs(CFG, nt=nt, levels=lt)
    return (df, uo) + tuple(_oracle(4, df, uo, B))


@pytest.mark.parametrize("B,nt", EDGES, ids=[f"B{B}-nt{n}" for B, n in EDGES])
def test_row_owner_smallest_shapes(oracle_c, B, nt):
    df, uo, phi, U = _edge_case(B, nt)
    _both(oracle_c, df, uo, phi, U, B, f"edge B={B} nt={nt}")


# ---- the sparse threshold -------------------------------------------------------------------------------------------
SPARSE_B = 64
# as test_gpu_c4_rows.py: (u_old columns, which Φ holds the counted sources, the finite sources of its rows 1, 2, 3)
SPARSE = {
    "sphere": ([(3, 3, 3, 3), (0, 0, 0, 0), (7, 7, 7, 7)], "terminal", (4, 10, 20)),
    "corner": ([(3, 3, 3, 3), (0, 0, 0, 0), (0, 0, 0, 0)], "phi1", (5, 15, 35)),
    "edge": ([(3, 3, 3, 3), (0, 0, 0, 3), (0, 0, 0, 0)], "phi1", (6, 20, 50)),
    "offgrid": ([(3, 3, 3, 3), (0, 0, 0, 3), (8, 3, 4, 2), (0, 0, 0, 0)], "phi1", (1, 6, 20)),
}


@functools.lru_cache(maxsize=None)
def _sparse_case(name):
    lt, lv = _levels()
    cols, which, want = SPARSE[name]
    nt = len(cols)
    _, df, _ = make_inputs(CFG, nt=nt, levels=lt)
    uo = _cols(cols)
    phi, U = _oracle(4, df, uo, SPARSE_B)
    if which == "terminal":  # the terminal Φ: the oracle on the last column alone
        src = _oracle(4, np.asfortranarray(df[:, -1:]), np.asfortranarray(uo[:, -1:]), SPARSE_B)[0][:, :, 0]
    else:  # Φ_1, the sources of step 0
        src = phi[:, :, 1]
    nf = tuple(int(np.isfinite(src[c]).sum()) for c in (1, 2, 3))
    assert nf == want, f"{name}: rows 1-3 hold {nf} finite sources, not {want}"
    return df, uo, phi, U


def test_row_owner_sparse_cases_cover_the_threshold():
    assert {4, 5, 6} <= {n for _, _, want in SPARSE.values() for n in want}


@pytest.mark.parametrize("name", list(SPARSE))
def test_row_owner_sparse_threshold(oracle_c, name):
    df, uo, phi, U = _sparse_case(name)
    assert df.shape[1] in (3, 4)
    _both(oracle_c, df, uo, phi, U, SPARSE_B, f"sparse {name}")


# ---- a spin limit of one poll ---------------------------------------------------------------------------------------
def test_row_owner_wait_timeout_redoes_dp(oracle_c):
    df, uo, phi, U = _steady_case()
    ctx = _ctx(1)
    ctx.set_option(native.MIOC_OPT_SPIN_LIMIT, 1)
    ctx.bellman(df, uo, STEADY_B, CFG.dt)
    assert ctx.last_sdt_driver() == ONE_ROW
    _compare_oracle(ctx, oracle_c, _levels()[1], uo, phi, U, STEADY_B, "timeout redo")
    assert ctx.diagnostics()[6] >= 1, ctx.diagnostics()  # the launch was abandoned and redone per step
    # the context stays usable: the same DP to the end
    ctx.set_option(native.MIOC_OPT_SPIN_LIMIT, 1 << 24)
    ctx.bellman(df, uo, STEADY_B, CFG.dt)
    assert ctx.last_sdt_driver() == ONE_ROW
    _compare_oracle(ctx, oracle_c, _levels()[1], uo, phi, U, STEADY_B, "after the redo")
    ctx.close()


# ---- 8^3 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _g3_case():
    rng = np.random.default_rng(0x83)
    df = np.asfortranarray(rng.standard_normal((3, STEADY_NT)))
    cyc = [(0, 0, 0), (3, 4, 3), (0, 0, 0), (2, 5, 3), (7, 0, 1), (2, 5, 3), (7, 7, 7), (4, 3, 4)]
    uo = _cols(cyc)
    return (df, uo) + tuple(_oracle(3, df, uo, STEADY_B))


def test_row_owner_8x8x8(oracle_c):
    df, uo, phi, U = _g3_case()
    _both(oracle_c, df, uo, phi, U, STEADY_B, "8^3", M=3)


# ---- several rows per workgroup: the general driver -----------------------------------------------------------------
def test_row_owner_fallback_two_rows_per_workgroup(oracle_c):
    import torch
    lt, lv = _levels()
    K, B, nt = 2, 200, 6
    assert K * B > _cus(), "every workgroup would own one row"
    subs = [make_inputs(CFG, k=k, nt=nt, levels=lt)[1:] for k in (3, 4)]
    ctx = _ctx(1)
    ddf = torch.tensor(np.ascontiguousarray(np.stack([d.T for d, _ in subs])), dtype=torch.float64, device="cuda")
    duo = torch.tensor(np.ascontiguousarray(np.stack([u.T for _, u in subs])), dtype=torch.float64, device="cuda")
    du = torch.empty_like(ddf)
    dphi = torch.empty(K, dtype=torch.float64, device="cuda")
    dst = torch.empty(K, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.bellman_batch_tensors(ddf, duo, B, CFG.dt)
    ctx.synchronize()
    assert ctx.kernel_stats(0)[2] == "k_sdt_run"
    assert ctx.last_sdt_driver() == GENERAL
    assert ctx.diagnostics()[6] == 0, ctx.diagnostics()
    cases = [_oracle(4, df, uo, B) for df, uo in subs]
    for k, (phi, U) in enumerate(cases):
        for i in range(U.shape[2]):
            d, o = ctx.argmin_table(i, k=k), U[:, :, i]
            m = o >= 0
            assert np.array_equal(d[m], o[m]), f"fallback k={k}: U at step {i}"
    for Bp in (B, B // 2, 1):
        ctx.backtrack_batch_tensors(Bp, du, dphi, dst)
        ctx.synchronize()
        for k, ((df, uo), (phi, U)) in enumerate(zip(subs, cases)):
            ou, ops = oracle_c.backtrack(lv, uo, phi, U, B, Bp)
            assert dst[k].item() == 0, f"fallback k={k} B'={Bp}: status {dst[k].item()}"
            assert np.array_equal(du[k].cpu().numpy().T, ou) and dphi[k].item() == ops, f"fallback k={k} B'={Bp}"
    ctx.close()
