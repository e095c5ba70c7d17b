"""Case builders for the generic sweep (k_generic_step, k_generic_walk) and the fused DP (k_fused_run), a census of
exact ties, and the comparison of a device context with the CPU oracle.  Plain numpy; nothing here needs a GPU until
check_device is handed a context.

The level lists are truncated product grids: the first L tuples of a 17 x 17 grid are no product grid, so the pyramid,
the separable transform and the fused separable DP are ineligible and only the generic sweep and the fused DP can run
them.  L is free, which is what the tests need: every tile of k_generic_step (32 target levels per workgroup, 64 source
levels per LDS chunk, argmin groups of 8, 64 budget rows per block, one or two bytes per argmin rank) and every
instantiation of k_fused_run (LP = 4 ... 64, argmin groups of 4) has its own first and last L.
"""
from __future__ import annotations

import functools
import itertools
import zlib
from dataclasses import dataclass

import numpy as np

from mioc import native
from mioc.iterators import LevelTable, product_iterator
from oracle.oracle import P_INF, P_ONE, Levels, OracleError

NU17 = [list(range(-3, 14)), list(range(0, 17))]
KINDS = ("inf", "one", "lut2", "lut3", "tab1.5")
FU_LPS = (4, 8, 16, 24, 32, 36, 48, 64)  # the instantiations of k_fused_run


def _pair(nu, tuples):
    return Levels(nu, tuples), LevelTable(nu, tuples)


@functools.lru_cache(maxsize=None)
def grid17(L):
    """The first L tuples (first index fastest) of the 17 x 17 grid {-3..13} x {0..16}: (oracle Levels, LevelTable)."""
    assert 1 <= L <= 289
    return _pair(NU17, list(itertools.islice(iter(product_iterator(NU17)), L)))


@functools.lru_cache(maxsize=None)
def line(L):
    """One control with the levels 0 .. L-1."""
    nu = [list(range(L))]
    return _pair(nu, list(product_iterator(nu)))


def levels_of(name, L):
    return {"grid17": grid17, "line": line}[name](L)


@functools.lru_cache(maxsize=None)  # (per LevelTable object: grid17 / line return the same one for the same L)
def cost(kind, lt):
    """(p_kind, p_int, table, W): the arguments of set_cost / of the oracle, and the L x L weight matrix w(l, j) that
    the census uses (HelpFunctions.jl:63-67; unscaled, the switching cost is beta * W).  Shared: do not write to them."""
    nv = lt.nuval
    d = np.abs(nv[:, None, :] - nv[None, :, :])
    if kind == "inf":
        return P_INF, 1, None, np.ones((lt.L, lt.L))
    if kind == "one":
        W = np.zeros((lt.L, lt.L))
        for m in range(lt.M):  # a sum of small integers: exact in any order
            W = W + d[:, :, m]
        return P_ONE, 1, None, W
    if kind in ("lut2", "lut3"):
        p = int(kind[3:])
        pk, pint, tab = native.cost_spec(p, levels=lt)
        assert pk == native.MIOC_P_INTLUT and pint == p
        key = (d.astype(np.int64) ** p).sum(axis=2)
        return pk, pint, tab, tab[key]
    if kind == "tab1.5":
        pk, pint, tab = native.cost_spec(1.5, levels=lt)
        assert pk == native.MIOC_P_TABLE
        return pk, pint, tab, tab.reshape(lt.L, lt.L).copy()
    raise ValueError(kind)


def inputs(mode, lv, nt, seed, uo_kind="random"):
    """(df, u_old, beta, dt).  mode "zero": df = 0 (every candidate of a cell that differs only in exactly representable
    terms ties); "integer": df in {-3..3}; "gauss"; "outside": Gaussian df and about a fifth of the steps (at least one)
    with one u_old component off the level range, at min - 2 or max + 3.  u_old is otherwise a random level per step
    (uo_kind "piecewise": one random level per 10 steps)."""
    rng = np.random.default_rng(seed)
    M = lv.M
    if mode == "zero":
        df = np.zeros((M, nt))
    elif mode == "integer":
        df = rng.integers(-3, 4, size=(M, nt)).astype(np.float64)
    elif mode in ("gauss", "outside"):
        df = rng.standard_normal((M, nt))
    else:
        raise ValueError(mode)
    if uo_kind == "piecewise":
        idx = np.repeat(rng.integers(lv.L, size=nt // 10 + 1), 10)[:nt]
    else:
        idx = rng.integers(lv.L, size=nt)
    uo = np.ascontiguousarray(lv.nuval[idx].T.astype(np.float64))
    if mode == "outside":
        for i in rng.choice(nt, size=max(1, round(nt / 5)), replace=False):
            m = int(rng.integers(M))
            uo[m, i] = float(min(lv.nu[m]) - 2 if rng.integers(2) else max(lv.nu[m]) + 3)
    beta, dt = (1e-3, 2.0 ** -6) if mode in ("gauss", "outside") else (0.25, 0.5)
    return df, uo, beta, dt


def step0_census(lv, df, uo, B, W, beta, dt, phi, U):
    """Step 0 of bellman_TRM! (HelpFunctions.jl:45-81) restated from the oracle's last two fronts, in the reference's
    rounding order: K[l, j] = T1(l) + beta * W[l, j], candidates K[l, j] + Phi_1[c', j] for c' <= B - b(l), the first
    minimum wins.  Returns (Phi_0, U_0, ties, finite): the recomputed front (B+1, Lgrid) and first-index argmin (-1
    where Phi_0 = +Inf), and over the `finite` cells with a finite minimum the number whose minimum is attained by
    sources in two different groups of 4, of 8 and chunks of 64 (ties[4], ties[8], ties[64])."""
    M, nt = df.shape
    assert nt >= 2 and U.shape[2] == nt - 1
    L, R = lv.L, B + 1
    phi1 = phi[:, :, 1][:, lv.gidx]  # (R, L): Phi_1[c', j]
    phi0 = np.full((R, lv.Lgrid), np.inf)
    u0 = np.full((R, lv.Lgrid), -1, dtype=np.int32)
    ties = {4: 0, 8: 0, 64: 0}
    finite = 0
    nuv = lv.nuval.astype(np.float64)
    T1 = np.zeros(L)
    for m in range(M):
        T1 = T1 + (dt * df[m, 0]) * nuv[:, m]
    K = T1[:, None] + beta * W
    bt = np.abs(nuv - uo[:, 0][None, :]).sum(axis=1).astype(np.int64)
    for l in range(L):
        n = B - int(bt[l]) + 1
        if n <= 0:
            continue
        cand = K[l][None, :] + phi1[:n]  # (n, L)
        mn = cand.min(axis=1)
        fin = mn < np.inf
        att = (cand == mn[:, None]) & fin[:, None]
        first = np.where(fin, att.argmax(axis=1), -1)
        last = np.where(fin, L - 1 - att[:, ::-1].argmax(axis=1), -1)
        g = int(lv.gidx[l])
        phi0[bt[l]:bt[l] + n, g] = mn
        u0[bt[l]:bt[l] + n, g] = first
        finite += int(fin.sum())
        for q in ties:
            ties[q] += int((fin & (first // q != last // q)).sum())
    return phi0, u0, ties, finite


# ----------------------------------------------------------------------------------------------------------------------
# the cases of the GPU files (tests/test_dp_cases.py runs the oracle and the census over every one of them at nt = 6)
# ----------------------------------------------------------------------------------------------------------------------
# cases whose first seed misses the tie condition of tests/test_dp_cases.py (step 0 holds no tie between argmin groups)
SALTS = {"grid1733-B64-inf-integer": 2, "grid1723-B64-inf-integer": 3, "line257-B64-one-zero": 7,
         "line257-B64-tab1.5-zero": 3}


@dataclass(frozen=True)
class Case:
    levels: str          # "grid17" | "line"
    L: int
    B: int
    kind: str            # one of KINDS
    mode: str            # see inputs()
    nt: int = 6
    uo_kind: str = "random"
    shared_cost: bool = False  # a batch restart: beta = 0.25, dt = 0.5 whatever the mode (a batch shares cost and dt)
    salt: int = 0        # changes the seed of a case that misses a condition on its inputs

    @property
    def id(self):
        s = f"{self.levels}{self.L}-B{self.B}-{self.kind}-{self.mode}"
        if self.nt != 6:
            s += f"-nt{self.nt}"
        if self.uo_kind != "random":
            s += f"-{self.uo_kind}"
        if self.shared_cost:
            s += "-batch"
        return s

    @property
    def seed(self):
        salt = self.salt + SALTS.get(f"{self.levels}{self.L}-B{self.B}-{self.kind}-{self.mode}", 0)
        return zlib.crc32(f"{self.levels}/{self.L}/{self.B}/{self.kind}/{self.mode}/{self.uo_kind}/{salt}".encode())

    def at(self, **kw):
        return Case(**{**self.__dict__, **kw})


class Built:
    """A case's inputs and the oracle's answer to it."""

    def __init__(self, case, oracle_c):
        self.case = case
        self.lv, self.lt = levels_of(case.levels, case.L)
        self.p_kind, self.p_int, self.table, self.W = cost(case.kind, self.lt)
        self.df, self.uo, self.beta, self.dt = inputs(case.mode, self.lv, case.nt, case.seed, case.uo_kind)
        if case.shared_cost:
            self.beta, self.dt = 0.25, 0.5
        self.B = case.B
        self.phi, self.U = oracle_c.bellman(self.lv, self.df, self.uo, self.B, self.p_kind, self.beta, self.dt,
                                            p_int=self.p_int, wtab=self.table)
        self._oc = oracle_c

    def budgets(self):
        rng = np.random.default_rng(self.case.seed ^ 0x5EED)
        return sorted({self.B, self.B // 2, 0, int(rng.integers(0, self.B + 1))})

    def backtrack(self, Bp):
        """The oracle's (u, Phi*), or None where its backtrack raises (no finite value within B')."""
        try:
            return self._oc.backtrack(self.lv, self.uo, self.phi, self.U, self.B, Bp)
        except OracleError:
            return None

    def census(self):
        return step0_census(self.lv, self.df, self.uo, self.B, self.W, self.beta, self.dt, self.phi, self.U)


def new_context(built, algo):
    ctx = native.Context(0)
    ctx.set_levels(built.lt)
    ctx.set_cost(None, built.beta, table=built.table, p_int=built.p_int, p_kind=built.p_kind)
    ctx.set_option(native.MIOC_OPT_ALGO, algo)
    return ctx


def assert_U(ctx, U, nt, tag, k=0):
    """Every cell of the reference's U table that the reference writes equals the device's argmin, step by step."""
    for i in range(nt - 1):
        d, o = ctx.argmin_table(i, k=k), U[:, :, i]
        bad = (o >= 0) & (d != o)
        assert not bad.any(), (f"{tag} step {i}: (c, g) {np.argwhere(bad)[:5].tolist()} device {d[bad][:5]} "
                               f"ref {o[bad][:5]}")


def check_device(built, algo, expect_algo=None):
    """One DP on the device against the oracle: the algorithm that ran, every U cell the oracle wrote, and u, Phi* and
    the switch flags at the budgets {B, B // 2, 0, one seeded random}; where the oracle's backtrack raises, so does the
    device's.  Returns the diagnostics after the backtrack at B."""
    c = built.case
    with new_context(built, algo) as ctx:
        ctx.bellman(built.df, built.uo, built.B, built.dt)
        assert ctx.last_algo() == (algo if expect_algo is None else expect_algo), c.id
        assert_U(ctx, built.U, c.nt, c.id)
        diag = None
        for Bp in reversed(built.budgets()):
            ref = built.backtrack(Bp)
            if ref is None:
                try:
                    ctx.backtrack(Bp)
                except native.MiocNativeError as e:
                    assert e.code == native.MIOC_EINFEASIBLE, (c.id, Bp, e.code)
                else:
                    raise AssertionError(f"{c.id} B'={Bp}: the oracle finds no finite value, the device returned a path")
                continue
            u, ps, sw = ctx.backtrack(Bp)
            if Bp == built.B:
                diag = ctx.diagnostics()
            assert np.array_equal(u, ref[0]), f"{c.id} B'={Bp}"
            assert ps == ref[1], f"{c.id} B'={Bp}: {ps!r} vs {ref[1]!r}"
            assert not sw[0] and np.array_equal(sw[1:], np.any(ref[0][:, 1:] != ref[0][:, :-1], axis=0)), (c.id, Bp)
        return diag


def check_batch(builts, algo):
    """The restarts of one batch (equal levels, cost, B, nt, dt) through bellman_batch_tensors / backtrack_batch_tensors:
    each restart's U, u, Phi* and status against its own oracle run."""
    import torch
    b0 = builts[0]
    K, nt, B = len(builts), b0.case.nt, b0.B
    assert all((b.beta, b.dt, b.B, b.case.nt, b.case.kind, b.case.L) == (b0.beta, b0.dt, B, nt, b0.case.kind, b0.case.L)
               for b in builts)
    ddf = torch.tensor(np.ascontiguousarray(np.stack([b.df.T for b in builts])), dtype=torch.float64, device="cuda")
    duo = torch.tensor(np.ascontiguousarray(np.stack([b.uo.T for b in builts])), dtype=torch.float64, device="cuda")
    du = torch.empty_like(ddf)
    dphi = torch.empty(K, dtype=torch.float64, device="cuda")
    dst = torch.empty(K, dtype=torch.int32, device="cuda")
    with new_context(b0, algo) as ctx:
        torch.cuda.synchronize()
        ctx.bellman_batch_tensors(ddf, duo, B, b0.dt)
        assert ctx.last_algo() == algo
        for Bp in (B, B // 2):
            ctx.backtrack_batch_tensors(Bp, du, dphi, dst)
            ctx.synchronize()
            ub, ph, st = du.cpu().numpy(), dphi.cpu().numpy(), dst.cpu().numpy()
            for k, b in enumerate(builts):
                ref = b.backtrack(Bp)
                if ref is None:
                    assert st[k] == native.MIOC_EINFEASIBLE and np.all(np.isnan(ub[k])), (b.case.id, Bp, st[k])
                    continue
                assert st[k] == native.MIOC_OK, (b.case.id, Bp, st[k])
                assert np.array_equal(ub[k].T, ref[0]) and ph[k] == ref[1], (b.case.id, Bp)
        for k, b in enumerate(builts):
            assert_U(ctx, b.U, nt, f"{b.case.id} k={k}", k=k)


def largest_fused_B(L):
    """The largest B that native.fused_eligible admits for L levels (the domain is an interval of B from 0)."""
    assert native.fused_eligible(L, 0)
    B = 0
    while native.fused_eligible(L, B + 1):
        B += 1
    return B


GENERIC_EDGE_LEVELS = [("grid17", L) for L in (31, 32, 33, 63, 64, 65, 255, 256, 257)] + [("line", 257)]


def generic_edge_cases():
    """Tile and table edges of k_generic_step at B = 64 (RP = 128: a second budget tile that holds one real row)."""
    out = []
    for name, L in GENERIC_EDGE_LEVELS:
        modes = ("zero", "gauss") + (("integer", "outside") if name == "grid17" and L in (33, 65, 257) else ())
        out += [Case(name, L, 64, kind, mode) for kind in KINDS for mode in modes]
    return out


def generic_budget_cases():
    return [Case("grid17", L, B, kind, "zero") for L in (65, 257) for B in (62, 63, 127, 130)
            for kind in ("one", "lut2", "tab1.5")]


def generic_short_cases():
    return [Case("grid17", 65, 64, kind, mode, nt=nt) for nt in (1, 2) for kind in KINDS for mode in ("zero", "gauss")]


def generic_walk_cases():
    """k_generic_walk<uint16_t> over two 64-step rounds."""
    return [Case("grid17", 257, 40, kind, mode, nt=70, uo_kind=uk) for kind in ("one", "lut2")
            for mode, uk in (("outside", "random"), ("gauss", "piecewise"))]


def batch_cases(Ls):
    """Per L the three restarts of one batch."""
    return {L: [Case("grid17", L, 64, "lut2", mode, shared_cost=True) for mode in ("zero", "integer", "outside")]
            for L in Ls}


FUSED_LS = (1, 3, 4, 5, 8, 9, 16, 17, 23, 24, 25, 32, 33, 36, 37, 47, 48, 49, 63, 64)  # first and last L of each LP
FUSED_EDGE_LS = (23, 24, 36, 49, 63, 64)


def fused_shape_cases():
    out = []
    for L in FUSED_LS:
        modes = ("zero", "gauss") + (("integer", "outside") if L in (23, 47) else ())
        out += [Case("grid17", L, B, kind, mode) for B in (63, 64) for kind in KINDS for mode in modes]
    return out


def fused_edge_cases():
    """At the largest B of the fused domain, and one beyond it."""
    return [Case("grid17", L, largest_fused_B(L) + over, kind, "zero") for L in FUSED_EDGE_LS for over in (0, 1)
            for kind in ("one", "lut2")]


def all_cases_nt6():
    """Every (levels, B, kind, mode) of the two GPU files, at nt = 6."""
    seen, out = set(), []
    cases = (generic_edge_cases() + generic_budget_cases() + generic_short_cases() + generic_walk_cases() +
             fused_shape_cases() + fused_edge_cases() +
             [c for cs in batch_cases((65, 257, 23, 47)).values() for c in cs])
    for c in cases:
        c = c.at(nt=6)
        if c.id not in seen:
            seen.add(c.id)
            out.append(c)
    return out
