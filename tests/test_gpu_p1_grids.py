"""GPU parity of the staged p = 1 DPs on product grids -- the separable transform (mioc_sdt.hip), the L1-ball pyramid
(mioc_pyramid.hip) and the two fused separable DPs (mioc_fsep.hip, mioc_fused.hip) -- against the CPU oracle, on the
inputs the rest of the suite does not feed them:

  A. level offsets (PyrGeom::base != 0) on the separable transform, 8^3 and 8^4, both drivers;
  B. the pyramid's ten instantiations k_pyr_step<M, N0> (M = 2..6, N0 = 4, 8), level counts other than 2, 4, 8,
     the mixed-radix sphere order, ncol = 512 (the 10-bit packed coordinate at its maximum);
  C. the fused separable DP: every shape (6x6, 4x4, 8x8, 8x4) with offsets on every driver (the one-lane-per-row
     kernel, two lanes per row unsegmented and 2 / 4 row segments), at each shape's largest B (the LDS limit) and at the
     workgroup-size edges;
  D. one DP whose gradient scale falls by 11 decades over its steps, so that the rows of one sweep lie on both sides
     of the transform's binade threshold (scaled range 2^31).

Bar, every case, no tolerance: every U cell the oracle wrote equals the device's argmin table, step by step; u and Φ*
bit-identical at B' in {B, B // 2, 1}; where the oracle finds no finite value for a B' (MIOC_EINFEASIBLE), the device
reports the same; last_algo() is the forced algorithm and diagnostics()[3] == 0.  Eligibility is asserted, never used
to skip.
"""
import functools

import numpy as np
import pytest

from mioc import native
from mioc.iterators import LevelTable
from mioc.synth import CONFIGS, synthetic_df, synthetic_u_old
from oracle.oracle import P_ONE, Levels, OracleC, OracleError

pytestmark = pytest.mark.gpu

GAUSS = (1e-3, 2.0 ** -10)   # (β, Δt) of the gauss / outside modes
INTEGER = (0.125, 0.25)      # ... of the integer mode: df in -3..3, so Δt·df·ν and β·S are dyadic and ties are exact
C4, C5 = CONFIGS["C4"], CONFIGS["C5"]


def R(a, k):
    return list(range(a, a + k))


@functools.lru_cache(maxsize=None)
def _grid(nu):
    """(device level table, oracle levels) of the product grid nu (a tuple of tuples)."""
    nu = [list(v) for v in nu]
    return LevelTable(nu), Levels.product(nu)


def _key(nu):
    return tuple(tuple(v) for v in nu)


def _random_uold(lt, n, rng):
    return np.asfortranarray(np.array([lt.nuval[rng.integers(lt.L)] for _ in range(n)], dtype=np.float64).T)


def _step_outside(uo, nu, cols, rng):
    """In the given columns, one coordinate one step below its first level or one step above its last."""
    uo = uo.copy(order="F")
    for i in cols:
        m = int(rng.integers(len(nu)))
        uo[m, i] = float(nu[m][0] - 1 if rng.integers(2) else nu[m][-1] + 1)
    return uo


def _ctx(lt, beta, algo, **opts):
    ctx = native.Context(0)
    ctx.set_levels(lt)
    ctx.set_cost(1, beta)
    ctx.set_option(native.MIOC_OPT_TIMING, 1)
    ctx.set_option(native.MIOC_OPT_ALGO, algo)
    for k, v in opts.items():
        ctx.set_option(getattr(native, "MIOC_OPT_" + k), v)
    return ctx


def _assert_U(ctx, U, label, k=0):
    for i in range(U.shape[2]):
        d, o = ctx.argmin_table(i, k=k), U[:, :, i]
        m = o >= 0
        bad = np.argwhere(m & (d != o))
        assert bad.size == 0, f"{label}: U at step {i}, (c, g) {bad[:5].tolist()}"


def _compare(ctx, oracle_c, lv, uo, phi, U, B, algo, label):
    """One single-subproblem DP on `ctx` against the oracle's (Φ, U)."""
    assert ctx.last_algo() == algo, f"{label}: ran algorithm {ctx.last_algo()}"
    _assert_U(ctx, U, label)
    for Bp in (B, B // 2, 1):
        try:
            ou, ops = oracle_c.backtrack(lv, uo, phi, U, B, Bp)
        except OracleError as e:
            assert e.args == (native.MIOC_EINFEASIBLE,), e
            with pytest.raises(native.MiocNativeError) as err:
                ctx.backtrack(Bp)
            assert err.value.code == native.MIOC_EINFEASIBLE, f"{label}: B'={Bp}"
            continue
        u, ps, _ = ctx.backtrack(Bp)
        assert np.array_equal(u, ou) and ps == ops, f"{label}: B'={Bp}: {ps!r} vs {ops!r}"
    diag = ctx.diagnostics()
    assert diag[3] == 0, diag
    return diag


# ---- A. offset grids on the separable transform ------------------------------------------------------------------
BASES3 = [(-3, -3, -3), (-7, 1, 100), (2 ** 20, -2 ** 20, 0)]
A_NT, A_B = 12, 20


@functools.lru_cache(maxsize=None)
def _a3_case(bases, mode, place):
    nu = [R(b, 8) for b in bases]
    lt, lv = _grid(_key(nu))
    rng = np.random.default_rng([BASES3.index(bases), int(mode == "integer"), int(place == "outside"), 0xA3])
    beta, dt = INTEGER if mode == "integer" else GAUSS
    if mode == "integer":
        df = rng.integers(-3, 4, size=(3, A_NT)).astype(float)
    else:
        df = rng.standard_normal((3, A_NT))
    uo = _random_uold(lt, A_NT, rng)
    if place == "outside":
        uo = _step_outside(uo, nu, rng.choice(A_NT, size=5, replace=False), rng)
    phi, U = OracleC().bellman(lv, df, uo, A_B, P_ONE, beta, dt)
    return lt, lv, df, uo, beta, dt, phi, U


@pytest.mark.parametrize("persist", [1, 0], ids=["persistent", "steps"])
@pytest.mark.parametrize("place", ["admissible", "outside"])
@pytest.mark.parametrize("mode", ["gauss", "integer"])
@pytest.mark.parametrize("bases", BASES3, ids=lambda b: "base" + "_".join(str(x) for x in b))
def test_sdt_offset_grid_8x8x8(oracle_c, bases, mode, place, persist):
    """8^3 levels whose first level is not 0: base[m] enters T1, b̃, the tolerance bound of the transform, the row-0
    chain and the sphere order.  Straddling zero, ending at zero, far from zero (|ν| = 2^20 must survive int -> double
    and enter the bound); tie-free and tie-heavy gradients; u_old on the grid and one step off it."""
    lt, lv, df, uo, beta, dt, phi, U = _a3_case(bases, mode, place)
    assert native.separable_eligible(lt)
    ctx = _ctx(lt, beta, native.MIOC_ALGO_SEPARABLE, PERSIST=persist)
    ctx.bellman(df, uo, A_B, dt)
    ctx.synchronize()
    name = ctx.kernel_stats(0)[2]
    if place == "outside":  # b̃ may leave the persistent kernel's 7·M window: then the host takes per-step launches
        assert name in ("k_sdt_run", "k_sdt_step"), name
    else:
        assert name == ("k_sdt_run" if persist else "k_sdt_step"), name
    diag = _compare(ctx, oracle_c, lv, uo, phi, U, A_B, native.MIOC_ALGO_SEPARABLE, f"{bases} {mode} {place}")
    if mode == "integer":
        assert diag[0] > 0, diag  # exact ties went through the exact scan
    ctx.close()


BASES4 = (-3, 0, 5, -7)
A4_NT = 4
CORNER = [(0, 0, 0, 0), (7, 7, 7, 7), (0, 7, 0, 7), (7, 0, 0, 0)]   # relative to the bases (tests/test_gpu_c4_item.py)
CENTRE = [(3, 3, 3, 3), (4, 4, 4, 4), (3, 4, 3, 4), (4, 3, 4, 4)]


@functools.lru_cache(maxsize=None)
def _a4_case(B, place):
    nu = [R(b, 8) for b in BASES4]
    lt, lv = _grid(_key(nu))
    df = synthetic_df(4, A4_NT, C4.seed_df)
    cols = CORNER if place == "corner" else CENTRE
    uo = np.asfortranarray(np.array([[BASES4[m] + cols[i % 4][m] for m in range(4)] for i in range(A4_NT)],
                                    dtype=np.float64).T)
    phi, U = OracleC().bellman(lv, df, uo, B, P_ONE, C4.beta, C4.dt, threads=4)  # (bit-identical to one thread)
    return lt, lv, df, uo, phi, U


@pytest.mark.parametrize("persist", [1, 0], ids=["persistent", "steps"])
@pytest.mark.parametrize("place", ["corner", "centre"])
@pytest.mark.parametrize("B", [27, 29])
def test_sdt_offset_grid_8x8x8x8(oracle_c, B, place, persist):
    """8^4 levels with bases (-3, 0, 5, -7), B on the two sides of 7·M = 28, u_old at the corners and the centre."""
    lt, lv, df, uo, phi, U = _a4_case(B, place)
    assert native.separable_eligible(lt)
    ctx = _ctx(lt, C4.beta, native.MIOC_ALGO_SEPARABLE, PERSIST=persist)
    ctx.bellman(df, uo, B, C4.dt)
    ctx.synchronize()
    assert ctx.kernel_stats(0)[2] == ("k_sdt_run" if persist else "k_sdt_step")
    _compare(ctx, oracle_c, lv, uo, phi, U, B, native.MIOC_ALGO_SEPARABLE, f"8^4 B={B} {place}")
    ctx.close()


# ---- B. the pyramid's other instantiations and shapes ------------------------------------------------------------
# (id, grid, nt, B)
PYR = [
    ("m4n4_offsets", [R(-1, 4), R(0, 4), R(2, 4), R(0, 4)], 10, 16),           # 256 levels, <4, 4>
    ("m5n8", [R(0, 8), R(0, 4), R(0, 4), R(0, 2), R(0, 2)], 10, 16),           # 512, <5, 8>
    ("m6n8", [R(0, 8), R(0, 4)] + [R(0, 2)] * 4, 10, 16),                      # 512, <6, 8>
    ("m5n4", [R(0, 4)] * 3 + [R(0, 2)] * 2, 10, 16),                           # 256, <5, 4>
    ("m6n4", [R(0, 4)] * 2 + [R(0, 2)] * 4, 10, 16),                           # 256, <6, 4>
    ("8x6x6_offsets", [R(0, 8), R(-2, 6), R(1, 6)], 10, 16),                   # 288: three 6-level heaters, one 8-level
    ("8x5x3x7", [R(0, 8), R(0, 5), R(0, 3), R(0, 7)], 10, 16),                 # 840: odd mixed radix
    ("8x512", [R(0, 8), R(0, 512)], 3, 12),                                    # 4096: ncol = 512
    ("4x512", [R(0, 4), R(0, 512)], 3, 12),                                    # 2048: the same, N0 = 4
]
PYR_BY_ID = {p[0]: p for p in PYR}
PYR_513 = ("8x513", [R(0, 8), R(0, 513)], 3, 12)                               # 4104: one grid column too many


@functools.lru_cache(maxsize=None)
def _pyr_case(gid, mode):
    _, nu, nt, B = PYR_BY_ID.get(gid, PYR_513)
    lt, lv = _grid(_key(nu))
    seed = sorted(PYR_BY_ID).index(gid) if gid in PYR_BY_ID else 99
    rng = np.random.default_rng([seed, int(mode == "integer"), 0xB])
    beta, dt = INTEGER if mode == "integer" else GAUSS
    M = len(nu)
    df = rng.integers(-3, 4, size=(M, nt)).astype(float) if mode == "integer" else rng.standard_normal((M, nt))
    uo = _random_uold(lt, nt, rng)
    phi, U = OracleC().bellman(lv, df, uo, B, P_ONE, beta, dt)
    return lt, lv, df, uo, B, beta, dt, phi, U


@pytest.mark.parametrize("mode", ["gauss", "integer"])
@pytest.mark.parametrize("gid", [p[0] for p in PYR])
def test_pyramid_instantiations_vs_oracle(oracle_c, gid, mode):
    lt, lv, df, uo, B, beta, dt, phi, U = _pyr_case(gid, mode)
    assert native.pyramid_eligible(lt) and lt.L >= 256
    ctx = _ctx(lt, beta, native.MIOC_ALGO_PYRAMID)
    ctx.bellman(df, uo, B, dt)
    assert ctx.kernel_stats(0)[2] == "k_pyr_step"
    _compare(ctx, oracle_c, lv, uo, phi, U, B, native.MIOC_ALGO_PYRAMID, f"{gid} {mode}")
    ctx.close()


@pytest.mark.parametrize("gid", [p[0] for p in PYR])
def test_pyramid_shapes_auto_vs_oracle(oracle_c, gid):
    """The automatic choice sends each of these shapes to the pyramid: none is in the domain of the separable
    transform or of a fused DP, and all have at least 256 levels."""
    lt, lv, df, uo, B, beta, dt, phi, U = _pyr_case(gid, "gauss")
    assert native.pyramid_eligible(lt) and lt.L >= 256
    assert not native.separable_eligible(lt) and not native.fused_separable_eligible(lt, B)
    assert not native.fused_eligible(lt.L, B)
    ctx = _ctx(lt, beta, native.MIOC_ALGO_AUTO)
    ctx.bellman(df, uo, B, dt)
    _compare(ctx, oracle_c, lv, uo, phi, U, B, native.MIOC_ALGO_PYRAMID, f"{gid} auto")
    ctx.close()


def test_pyramid_rejects_513_columns(oracle_c):
    """8 x 513 levels: one grid column more than a workgroup's thread pairs.  The forced pyramid refuses it, the
    automatic choice solves it with another algorithm."""
    lt, lv, df, uo, B, beta, dt, phi, U = _pyr_case("8x513", "gauss")
    assert not native.pyramid_eligible(lt)
    ctx = _ctx(lt, beta, native.MIOC_ALGO_PYRAMID)
    with pytest.raises(native.MiocNativeError) as err:
        ctx.bellman(df, uo, B, dt)
    assert err.value.code == native.MIOC_EINVAL
    ctx.close()
    ctx = _ctx(lt, beta, native.MIOC_ALGO_AUTO)
    ctx.bellman(df, uo, B, dt)
    assert ctx.last_algo() != native.MIOC_ALGO_PYRAMID
    _compare(ctx, oracle_c, lv, uo, phi, U, B, ctx.last_algo(), "8x513 auto")
    ctx.close()


# ---- C. fused separable: every shape on every driver, and the LDS limit -------------------------------------------
# shape id -> (counts, bases, B of the driver cases, largest eligible B)
FSEP = {"6x6": ((6, 6), (-2, 3), 200, 265), "4x4": ((4, 4), (-1, 0), 200, 511),
        "8x8": ((8, 8), (0, -7), 140, 141), "8x4": ((8, 4), (5, -1), 200, 298)}
SEGMENTS = [-1, 1, 2, 4]


def _fsep_nu(shape):
    (n0, n1), (b0, b1) = FSEP[shape][:2]
    return [R(b0, n0), R(b1, n1)]


@functools.lru_cache(maxsize=None)
def _fsep_case(shape, mode, K, nt, B):
    """K restarts with C5-style inputs (df ~ N(0, 1), u_old piecewise constant over the admissible tuples) and C5's β
    and Δt on the shape's offset grid; the oracle's (Φ, U) of each."""
    nu = _fsep_nu(shape)
    lt, lv = _grid(_key(nu))
    seed = 1000 * sorted(FSEP).index(shape) + 100 * ["gauss", "integer", "outside"].index(mode) + nt
    rng = np.random.default_rng(seed)
    subs = []
    for k in range(K):
        df = synthetic_df(2, nt, C5.seed_df + seed + k)
        uo = synthetic_u_old(lt, nt, C5.seed_u + seed + k)
        if mode == "integer":
            df = np.asfortranarray(rng.integers(-3, 4, size=df.shape).astype(float))
        elif mode == "outside":
            uo = _step_outside(uo, nu, rng.choice(nt, size=6, replace=False), rng)
        phi, U = OracleC().bellman(lv, df, uo, B, P_ONE, C5.beta, C5.dt)
        subs.append((df, uo, phi, U))
    return lt, lv, subs


def _fsep_check(oracle_c, shape, mode, K, nt, B, seg, want_seg=None, algo=native.MIOC_ALGO_FUSED_SEPARABLE):
    """The K restarts as one batch on driver `seg`: U, u, Φ* and the per-restart status at three budgets; a restart
    without a finite value in the budget is also run alone, where the host entry raises."""
    import torch
    lt, lv, subs = _fsep_case(shape, mode, K, nt, B)
    label = f"{shape} {mode} B={B} segments {seg}"
    ddf = torch.tensor(np.ascontiguousarray(np.stack([s[0].T for s in subs])), dtype=torch.float64, device="cuda")
    duo = torch.tensor(np.ascontiguousarray(np.stack([s[1].T for s in subs])), dtype=torch.float64, device="cuda")
    ctx = _ctx(lt, C5.beta, algo, FSEP_SEGMENTS=seg)
    ctx.bellman_batch_tensors(ddf, duo, B, C5.dt)
    if algo == native.MIOC_ALGO_FUSED_SEPARABLE:
        assert ctx.last_algo() == algo
    else:
        assert ctx.last_algo() != native.MIOC_ALGO_FUSED_SEPARABLE
    du = torch.empty_like(ddf)
    dphi = torch.empty(K, dtype=torch.float64, device="cuda")
    dst = torch.empty(K, dtype=torch.int32, device="cuda")
    for Bp in (B, B // 2, 1):
        ctx.backtrack_batch_tensors(Bp, du, dphi, dst)
        ctx.synchronize()
        u, ph, st = du.cpu().numpy(), dphi.cpu().numpy(), dst.cpu().numpy()
        for k, (df, uo, phi, U) in enumerate(subs):
            try:
                ou, ops = oracle_c.backtrack(lv, uo, phi, U, B, Bp)
            except OracleError as e:
                assert e.args == (native.MIOC_EINFEASIBLE,), e
                assert st[k] == native.MIOC_EINFEASIBLE, f"{label}: restart {k} B'={Bp}: status {st[k]}"
                one = _ctx(lt, C5.beta, algo, FSEP_SEGMENTS=seg)
                one.bellman(df, uo, B, C5.dt)
                with pytest.raises(native.MiocNativeError) as err:
                    one.backtrack(Bp)
                assert err.value.code == native.MIOC_EINFEASIBLE, f"{label}: restart {k} B'={Bp}"
                one.close()
                continue
            assert st[k] == 0 and np.array_equal(u[k].T, ou) and ph[k] == ops, \
                f"{label}: restart {k} B'={Bp}: status {st[k]}, {ph[k]!r} vs {ops!r}"
    for k, (_, _, _, U) in enumerate(subs):
        _assert_U(ctx, U, f"{label}: restart {k}", k=k)
    diag = ctx.diagnostics()
    assert diag[3] == 0, diag
    if want_seg is not None:
        assert diag[8] == want_seg, f"{label}: diagnostics {diag}"
    ctx.close()
    return diag


@pytest.mark.parametrize("seg", SEGMENTS)
@pytest.mark.parametrize("mode", ["gauss", "integer", "outside"])
@pytest.mark.parametrize("shape", list(FSEP))
def test_fsep_every_shape_every_driver(oracle_c, shape, mode, seg):
    """Offset grids of all four shapes, B = 200 (140 at 8x8, whose largest B is 141), K = 3, nt = 24.  diagnostics [8]:
    0 for the one-lane-per-row kernel, else the forced segment count -- an off-grid u_old reaches further than a
    segment's outbox rows, so such a DP runs unsegmented (tests/test_gpu_fsep.py, test_fsep_segments_vs_oracle)."""
    B = FSEP[shape][2]
    lt, _ = _grid(_key(_fsep_nu(shape)))
    assert native.fused_separable_eligible(lt, B)
    want = 0 if seg < 0 else (1 if mode == "outside" else seg)
    _fsep_check(oracle_c, shape, mode, 3, 24, B, seg, want_seg=want)


def _largest_B(lt):
    return max(B for B in range(512) if native.fused_separable_eligible(lt, B))


@pytest.mark.parametrize("seg", [-1, 1])
@pytest.mark.parametrize("shape", list(FSEP))
def test_fsep_at_lds_limit(oracle_c, shape, seg):
    """The largest B whose two fronts and K tables fit one CU's LDS, from the host mirror (a layout change shows up as
    another value)."""
    lt, _ = _grid(_key(_fsep_nu(shape)))
    B = _largest_B(lt)
    assert B == FSEP[shape][3]
    _fsep_check(oracle_c, shape, "gauss", 2, 6, B, seg)


@pytest.mark.parametrize("shape", list(FSEP))
def test_fsep_past_lds_limit(oracle_c, shape):
    """One row more: the forced fused separable DP refuses (MIOC_EINVAL), the automatic choice takes another
    algorithm and equals the oracle.  4x4: B = 512 is outside the API's own B < 512, so only the refusal is covered."""
    lt, _ = _grid(_key(_fsep_nu(shape)))
    B = _largest_B(lt) + 1
    assert not native.fused_separable_eligible(lt, B)
    df, uo = synthetic_df(2, 6, 11), synthetic_u_old(lt, 6, 12)
    ctx = _ctx(lt, C5.beta, native.MIOC_ALGO_FUSED_SEPARABLE)
    with pytest.raises(native.MiocNativeError) as err:
        ctx.bellman(df, uo, B, C5.dt)
    assert err.value.code == native.MIOC_EINVAL
    ctx.close()
    if shape != "4x4":
        _fsep_check(oracle_c, shape, "gauss", 2, 6, B, 0, algo=native.MIOC_ALGO_AUTO)


@pytest.mark.parametrize("seg", [-1, 1])
@pytest.mark.parametrize("B", [63, 64, 65])
def test_fsep_workgroup_size_edges(oracle_c, B, seg):
    """8x4 at the budgets where the workgroup grows by a wave (threads = 64·ceil((B + 1) / 64))."""
    lt, _ = _grid(_key(_fsep_nu("8x4")))
    assert native.fused_separable_eligible(lt, B)
    _fsep_check(oracle_c, "8x4", "gauss", 3, 24, B, seg, want_seg=max(seg, 0))


# ---- D. one DP that crosses the binade threshold ----------------------------------------------------------------
RAMP_N, RAMP_B, RAMP_SEED = 16, 20, 7
CUBE = _key([R(0, 8)] * 3)


@functools.lru_cache(maxsize=None)
def _ramp_inputs():
    """u_old and the N(0, 1) draws of the recipe (seed 7, numpy's default_rng: u_old column by column, then df), and
    the scale ramp 1e11 .. 1: the large steps come first in time, so the backward sweep meets them last."""
    lt, _ = _grid(CUBE)
    rng = np.random.default_rng(RAMP_SEED)
    uo = np.asfortranarray(np.array([lt.nuval[rng.integers(lt.L)] for _ in range(RAMP_N)], dtype=np.float64).T)
    z = rng.standard_normal((3, RAMP_N))
    return uo, z, 10.0 ** np.linspace(11, 0, RAMP_N)


@functools.lru_cache(maxsize=None)
def _ramp_case(scale):
    """scale: "ramp", or a constant for the two control DPs."""
    _, lv = _grid(CUBE)
    uo, z, ramp = _ramp_inputs()
    df = np.asfortranarray(z * (ramp if scale == "ramp" else float(scale)))
    phi, U = OracleC().bellman(lv, df, uo, RAMP_B, P_ONE, *GAUSS)
    return df, uo, phi, U


@functools.lru_cache(maxsize=None)
def _ramp_classes():
    """Per step i = 1..n-1, the scaled range rs = (max - min) / β + 21 of every budget row of the source front Φ_i that
    has a finite entry -- from the oracle alone (Φ_i is Φ_0 of the DP over the steps i..n-1)."""
    _, lv = _grid(CUBE)
    df, uo, _, _ = _ramp_case("ramp")
    out = {}
    for i in range(1, RAMP_N):
        phi, _ = OracleC().bellman(lv, df[:, i:], uo[:, i:], RAMP_B, P_ONE, *GAUSS)
        rs = []
        for row in phi[:, :, 0]:
            f = row[np.isfinite(row)]
            if f.size:
                rs.append((f.max() - f.min()) / GAUSS[0] + 21)
        out[i] = np.array(rs)
    return out


def _assert_ramp_crosses_threshold():
    """Conditions on the input, not measurements of the kernel: the DP has steps wholly inside the transform's binade,
    a step with rows on both sides, a step mostly outside, and rows near the threshold.  (With this numpy: steps 4-15
    inside, step 3 with 4 rows inside and 17 outside, steps 1-2 with 1 and 20, 63 rows in the near band.  Should
    another numpy change the draws, change RAMP_SEED until the conditions hold.)"""
    T = 2.0 ** 31
    cls = _ramp_classes()
    assert sum(1 for rs in cls.values() if rs.size and np.all(rs < T)) >= 3
    assert any(np.any(rs < T) and np.any(rs >= T) for rs in cls.values())
    assert any(np.sum(rs >= T) >= 15 for rs in cls.values())
    assert sum(int(np.sum((rs >= 2.0 ** 27) & (rs < 2.0 ** 35))) for rs in cls.values()) >= 20


def _ramp_sdt(oracle_c, scale, persist):
    lt, lv = _grid(CUBE)
    df, uo, phi, U = _ramp_case(scale)
    ctx = _ctx(lt, GAUSS[0], native.MIOC_ALGO_SEPARABLE, PERSIST=persist)
    ctx.bellman(df, uo, RAMP_B, GAUSS[1])
    ctx.synchronize()
    assert ctx.kernel_stats(0)[2] == ("k_sdt_run" if persist else "k_sdt_step")
    diag = _compare(ctx, oracle_c, lv, uo, phi, U, RAMP_B, native.MIOC_ALGO_SEPARABLE, f"scale {scale}")
    ctx.close()
    return diag


@pytest.mark.parametrize("persist", [1, 0], ids=["persistent", "steps"])
def test_sdt_mixed_scale_dp(oracle_c, persist):
    """The per-row branch of the transform (inside the binade: certified transform; outside: exact scan) changes
    within one DP.  The two control DPs (the same draws at scale 1 and at scale 1e11 throughout) bracket the count of
    rows sent straight to the exact scan (diagnostics [1]): the ramp sent some rows there, not all -- coverage
    evidence; correctness is the comparison with the oracle."""
    _assert_ramp_crosses_threshold()
    ramp = _ramp_sdt(oracle_c, "ramp", persist)
    ones = _ramp_sdt(oracle_c, 1.0, persist)
    steep = _ramp_sdt(oracle_c, 1e11, persist)
    print(f"mixed-scale separable persist={persist}: diag[0], [1], [5] = ramp {ramp[0], ramp[1], ramp[5]}, "
          f"ones {ones[0], ones[1], ones[5]}, 1e11 {steep[0], steep[1], steep[5]}")
    assert ones[1] < ramp[1] < steep[1], (ones, ramp, steep)


@pytest.mark.parametrize("algo", ["pyramid", "generic"])
def test_mixed_scale_dp_other_algorithms(oracle_c, algo):
    algo_id = {"pyramid": native.MIOC_ALGO_PYRAMID, "generic": native.MIOC_ALGO_GENERIC}[algo]
    lt, lv = _grid(CUBE)
    df, uo, phi, U = _ramp_case("ramp")
    ctx = _ctx(lt, GAUSS[0], algo_id)
    ctx.bellman(df, uo, RAMP_B, GAUSS[1])
    diag = _compare(ctx, oracle_c, lv, uo, phi, U, RAMP_B, algo_id, f"ramp {algo}")
    print(f"mixed-scale {algo}: diag[0], [1], [5] = {diag[0], diag[1], diag[5]}")
    ctx.close()


FSEP_RAMP_B = 40


@functools.lru_cache(maxsize=None)
def _fsep_ramp_case():
    nu = [R(0, 6)] * 2
    lt, lv = _grid(_key(nu))
    df = np.asfortranarray(synthetic_df(2, RAMP_N, C5.seed_df) * 10.0 ** np.linspace(11, 0, RAMP_N))
    uo = synthetic_u_old(lt, RAMP_N, C5.seed_u)
    phi, U = OracleC().bellman(lv, df, uo, FSEP_RAMP_B, P_ONE, C5.beta, C5.dt)
    return lt, lv, df, uo, phi, U


@pytest.mark.parametrize("seg", [-1, 1, 2])
def test_fsep_mixed_scale_dp(oracle_c, seg):
    """6x6 at base 0, n = 16, B = 40: C5's inputs under the same scale ramp, on the three drivers."""
    lt, lv, df, uo, phi, U = _fsep_ramp_case()
    assert native.fused_separable_eligible(lt, FSEP_RAMP_B)
    ctx = _ctx(lt, C5.beta, native.MIOC_ALGO_FUSED_SEPARABLE, FSEP_SEGMENTS=seg)
    ctx.bellman(df, uo, FSEP_RAMP_B, C5.dt)
    diag = _compare(ctx, oracle_c, lv, uo, phi, U, FSEP_RAMP_B, native.MIOC_ALGO_FUSED_SEPARABLE, f"ramp fsep {seg}")
    print(f"mixed-scale fsep segments {seg}: diag[0], [1], [5], [8] = {diag[0], diag[1], diag[5], diag[8]}")
    assert diag[8] == max(seg, 0), diag
    ctx.close()
