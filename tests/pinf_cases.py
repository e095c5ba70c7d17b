"""TEST INFRASTRUCTURE -- the p=Inf collapse (csrc/mioc_pinf.hip) table cell by cell: a plain restatement of its
tables, named wrong versions of that restatement, and the cases of tests/test_gpu_pinf_shapes.py, one per kernel
instantiation and edge that launch_pinf_prep / launch_pinf_recur choose from (K, L, M, BW, B, ncu).

  pinf_tables_ref(lv, df, u_old, B, beta, dt, BW=None)
        For one subproblem, in numpy double arithmetic, from the definition (HelpFunctions.jl:20-83 at p = Inf, where
        the switching weight is 1.0 for every pair of levels):
          K_l(i)   = fl(sum_m (dt·df_m(i))·nu_lm  [accumulated from 0.0 in order of m]  + beta), no beta at i = nt-1
          b~_l(i)  = sum_m |nu_lm - u_old_m(i)|                                   the budget class of level l
          kmin_i[b], k2_i[b], kfirst_i[b]: the smallest K_l of class b, the smallest value distinct from it (+Inf:
          none), the first rank at the minimum (-1: empty class); kabs_i: the largest |K_l| of the classes < BW
          R_{nt-1}[c] = kmin_{nt-1}[c];  R_i[c] = min_b fl(kmin_i[b] + R_{i+1}[c - b]);  +Inf where nothing reaches
          and in the rows B+1 .. RP-1.
        BW is a property of the whole batch (batch_bw: k_validate's bounding-box rule); None takes it from this
        subproblem alone.  test_pinf_cases.py anchors R to the C oracle's fronts before any device is asked.
  MUTATIONS     name -> function with the same arguments returning wrong tables, one per mistake a kernel could make
  CASES         the table of the GPU module; build(case, ncu) -> (lv, lt, dfs, uos, B, beta, dt, K), seeded
  recur_kernel, prep_kernel, walk_chunk: the dispatch rules restated, so that a test can tell whether a device with
        another CU count can meet a case's condition (it skips then; it never asserts another kernel)
"""
from __future__ import annotations

import collections
import functools
import zlib

import numpy as np

from mioc.iterators import LevelTable
from oracle.oracle import Levels, product_tuples

PinfRef = collections.namedtuple("PinfRef", "R kmin k2 kfirst kabs BW BWP RP")
INF = np.inf


# ------------------------------------------------------------------ the restatement --------------------------------

def class_sizes(BW, B):
    """(BWP, RP): the class row padded to a power of two >= max(8, BW), the budget rows to a multiple of 64."""
    BWP = 8
    while BWP < BW:
        BWP *= 2
    return BWP, (B + 1 + 63) // 64 * 64


def batch_bw(lv, uos, B):
    """Classes tracked for a batch: the largest distance of any u_old(:, i) of any subproblem from the levels'
    bounding box (not from the admissible levels: a cut or SOS1 level set has empty classes), capped at B, plus 1."""
    lo = np.array([min(v) for v in lv.nu], dtype=np.float64)[:, None]
    hi = np.array([max(v) for v in lv.nu], dtype=np.float64)[:, None]
    far = max(int(np.maximum(np.abs(hi - uo), np.abs(lo - uo)).astype(np.int64).sum(axis=0).max()) for uo in uos)
    return min(int(B), far) + 1


def _level_costs(lv, df, u_old, beta, dt, i, with_beta):
    nuv = lv.nuval.astype(np.float64)
    K = np.zeros(lv.L)
    for m in range(lv.M):
        K = K + (dt * df[m, i]) * nuv[:, m]
    if with_beta:
        K = K + beta
    bt = np.zeros(lv.L, dtype=np.int64)
    for m in range(lv.M):
        bt += np.abs(nuv[:, m] - u_old[m, i]).astype(np.int64)
    return K, bt


def _tables(lv, df, u_old, B, beta, dt, BW=None, wrong=None):
    """The restatement (wrong=None) and its wrong versions: every `wrong` branch is one named mistake."""
    df = np.asarray(df, dtype=np.float64)
    u_old = np.asarray(u_old, dtype=np.float64)
    nt = df.shape[1]
    BW = batch_bw(lv, [u_old], B) if BW is None else int(BW)
    BWP, RP = class_sizes(BW, B)
    kmin = np.full((nt, BWP), INF)
    k2 = np.full((nt, BWP), INF)
    kfirst = np.full((nt, BWP), -1, dtype=np.int32)
    kabs = np.zeros(nt)
    for i in range(nt):
        K, bt = _level_costs(lv, df, u_old, beta, dt, i, i != nt - 1 or wrong == "terminal_beta")
        if np.any(bt < BW):
            kabs[i] = np.abs(K[bt < BW]).max()
        for b in range(BW):
            ranks = np.flatnonzero(bt == b)
            if ranks.size == 0:
                continue
            v = K[ranks]
            kmin[i, b] = v.min()
            at_min = ranks[v == kmin[i, b]]
            kfirst[i, b] = at_min[-1] if wrong == "kfirst_last" else at_min[0]
            others = np.sort(v)[1:] if wrong == "k2_with_duplicates" else v[v != kmin[i, b]]
            if others.size:
                k2[i, b] = others.min()

    def classes(i):  # (b, value of class b as the recursion sees it)
        row = kmin[i].copy()
        if wrong == "pad_classes_zero":
            row[BW:] = 0.0
        top = BWP if wrong == "pad_classes_zero" else BW
        if wrong == "classes_from_8_dropped":
            top = min(top, 8)
        if wrong == "top_class_dropped":
            top = BW - 1
        return [(b, row[b]) for b in range(top)]

    R = np.full((nt, RP), INF)
    R[nt - 1, :min(BW, B + 1)] = kmin[nt - 1, :min(BW, B + 1)]
    if wrong == "rows_above_B_kept":
        R[nt - 1, :BW] = kmin[nt - 1, :BW]
    if wrong == "second_row_trip_missing":
        R[nt - 1, 512:] = INF
    rows = RP if wrong == "rows_above_B_kept" else B + 1
    chunk = {"stale_class_row_at_chunk": 32, "stale_class_row_at_chunk64": 64, "stale_rows_below_at_chunk": 64}.get(wrong)
    for i in range(nt - 2, -1, -1):
        handoff = chunk is not None and i != nt - 2 and (nt - 2 - i) % chunk == 0  # first step of a later chunk
        src = i + 1 if handoff and wrong.startswith("stale_class_row") else i
        nxt = R[i + 1]
        out = np.full(rows, INF)
        for b, kb in classes(src):
            if b >= rows:
                break
            shift = b + 1 if wrong == "window_shifted" and b >= BWP // 2 else b
            if shift >= rows:
                continue
            prev = nxt[:rows - shift]
            if handoff and wrong == "stale_rows_below_at_chunk" and i + 2 < nt:
                # target row c reads row c - b: where that lies in a lower 8-row segment, one step late
                c = np.arange(shift, rows)
                prev = np.where((c - shift) // 8 < c // 8, R[i + 2][:rows - shift], prev)
            if wrong == "extra_row_256_stale" and b == 0 and rows > 256 and i + 2 < nt:
                prev = prev.copy()
                prev[256] = R[i + 2][256]
            out[shift:] = np.minimum(out[shift:], kb + prev)
        if wrong == "second_row_trip_missing":
            out[512:] = INF
        R[i, :rows] = out
    return PinfRef(R, kmin, k2, kfirst, kabs, BW, BWP, RP)


def pinf_tables_ref(lv, df, u_old, B, beta, dt, BW=None):
    return _tables(lv, df, u_old, B, beta, dt, BW)


MUTATIONS = {name: functools.partial(_tables, wrong=name) for name in (
    "terminal_beta",               # beta added on the last step
    "kfirst_last",                 # last rank at the minimum instead of the first
    "k2_with_duplicates",          # k2 equals kmin on a tie
    "classes_from_8_dropped",      # classes 8 and above ignored (a helper wave's share lost)
    "top_class_dropped",           # class BW-1 ignored
    "pad_classes_zero",            # classes BW..BWP-1 read as 0.0 instead of +Inf
    "window_shifted",              # R_{i+1}[c-b-1] read for the upper half of the classes
    "stale_class_row_at_chunk",    # the first step of each 32-step chunk uses the previous step's class row
    "stale_class_row_at_chunk64",  # ... of each 64-step chunk
    "stale_rows_below_at_chunk",   # first step of each 64-step chunk: rows of a lower 8-row segment one step late
    "second_row_trip_missing",     # rows >= 512 left +Inf
    "extra_row_256_stale",         # row 256 takes R_{i+1}[256] from two steps back
    "rows_above_B_kept",           # rows above B keep their finite values
)}


def tables_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5])) and tuple(a[5:]) == tuple(b[5:])


# ------------------------------------------------------------------ the dispatch rules, restated -------------------

def recur_kernel(ncu, K, BW, B, nt):
    """(name, detail) of the recursion kernel launch_pinf_recur takes in the default build."""
    BWP, RP = class_sizes(BW, B)
    nseg64 = (B + 1 + 63) // 64
    small = nt * RP * 8 < 2 ** 31
    if 1 <= BW <= 8 and BWP == 8 and nseg64 >= 2 and K * nseg64 <= ncu and small:
        return "k_pinf_recur_ws", f"<{max(BW, 2)}>"
    nseg8 = (B + 1 + 7) // 8
    if 16 <= BWP <= 32 and nseg8 >= 3 and K * nseg8 <= ncu and small:
        return "k_pinf_recur_mcw", f"<{BWP}>"
    G = 4 if 4 * K <= ncu else 1
    if G == 4 and BWP == 32 and B + 1 == 257:
        return "k_pinf_recur_xr", "<32,8>"
    return "k_pinf_recur", f"<{BWP},{G}>"


def prep_kernel(L, M, BW):
    BWP = class_sizes(BW, 0)[0]
    if L <= 64 and BWP <= 16:
        return "k_pinf_prep_small", f"<{BWP}>"
    if L <= 4096 and 2 <= M <= 4:
        return "k_pinf_prep_m", f"<{M}>"
    return "k_pinf_prep", ""


def walk_chunk(BW, B):
    """Steps per staged chunk of the serial walk (pinf_plan) and whether it stages a band instead of whole rows."""
    BWP, RP = class_sizes(BW, B)
    ch = 16
    while ch >= 1:
        w = (2 * ch * (BW - 1) + BWP + 2 + 1) & ~1
        if 2 * w > RP:
            break
        if 2 * ch * (w * 8 + BWP * 20) + 32 <= 160 * 1024:
            return ch, True
        ch //= 2
    return max(1, min(32, (96 * 1024) // (2 * (RP * 8 + BWP * 20)))), False


# ------------------------------------------------------------------ the cases --------------------------------------

MODES = ("zero", "int", "gauss")  # gradients: every class one tie; integers in -4..4 (many ties); Gaussian


class Case(collections.namedtuple("Case", "id nu cut kof nt B mode recur prep edge")):
    """nu: the level grid; cut: keep the first `cut` tuples of the product (None: all); kof: K from the CU count;
    recur / prep: the kernel pinned (None: not pinned, the test takes the name from recur_kernel / prep_kernel)."""

    def K(self, ncu=256):
        return KOF[self.kof](ncu)


KOF = {
    "1": lambda ncu: 1,
    "3": lambda ncu: 3,
    "ncu//65+1": lambda ncu: ncu // 65 + 1,
    "ncu//5+1": lambda ncu: ncu // 5 + 1,
    "ncu//4+1": lambda ncu: ncu // 4 + 1,
    "ncu//33+1": lambda ncu: ncu // 33 + 1,
    "ncu//4": lambda ncu: ncu // 4,
}


KTAG = {"1": "K1", "3": "K3", "ncu//65+1": "Kcu65p1", "ncu//5+1": "Kcu5p1", "ncu//4+1": "Kcu4p1", "ncu//33+1": "Kcu33p1",
        "ncu//4": "Kcu4"}  # in a case's id


def _r(n):
    return tuple(range(n))


def levels_of(case):
    nu = [list(v) for v in case.nu]
    tuples = list(product_tuples(nu))
    lv = Levels(nu, tuples if case.cut is None else tuples[:case.cut])
    return lv, LevelTable(lv.nu, [tuple(int(x) for x in t) for t in lv.tuples])


@functools.lru_cache(maxsize=None)
def _build(case, ncu):
    lv, lt = levels_of(case)
    seed = zlib.crc32(case.id.encode())
    rng = np.random.default_rng(seed)
    K, nt = case.K(ncu), case.nt
    beta = [1e-3, 0.25, 0.1][seed % 3]
    dt = [0.5, 1 / 3, 2.0 ** -6][(seed // 3) % 3]
    dfs, uos = [], []
    for _ in range(K):
        if case.mode == "zero":
            df = np.zeros((lv.M, nt))
        elif case.mode == "int":
            df = rng.integers(-4, 5, size=(lv.M, nt)).astype(np.float64)
        else:
            df = rng.standard_normal((lv.M, nt))
        # u_old on the level grid, step 0 on the first level (every lower bound: the widest class window there is)
        uo = np.array([lv.nuval[rng.integers(lv.L)] for _ in range(nt)], dtype=np.float64).T.reshape(lv.M, nt)
        uo[:, 0] = lv.nuval[0]
        df.setflags(write=False)
        uo.setflags(write=False)
        dfs.append(df)
        uos.append(uo)
    return lv, lt, tuple(dfs), tuple(uos), case.B, beta, dt, K


def build(case, ncu=256):
    """(lv, lt, dfs, uos, B, beta, dt, K): built once per (case, ncu), shared read-only."""
    return _build(case, int(ncu))


@functools.lru_cache(maxsize=None)
def reference_k(case, k, ncu=256):
    """The restatement's tables of subproblem k of the case (with the batch's BW), computed once."""
    lv, _, dfs, uos, B, beta, dt, _ = build(case, ncu)
    ref = pinf_tables_ref(lv, dfs[k], uos[k], B, beta, dt, batch_bw(lv, uos, B))
    for a in ref[:5]:
        a.setflags(write=False)
    return ref


def reference(case, ncu=256):
    return tuple(reference_k(case, k, ncu) for k in range(case.K(ncu)))


def _cases():
    out = []

    def add(name, nu, kof, nt, B, recur, prep=None, edge="", cut=None, modes=("int", "gauss")):
        for mode in modes:
            out.append(Case(f"{name}_nt{nt}_B{B}_{KTAG[kof]}_{mode}", tuple(map(tuple, nu)), cut, kof, nt, B, mode, recur,
                            prep, edge))

    R = "k_pinf_recur"
    add("R1_8", [_r(8)], "1", 130, 63, R, edge="<8,4>, one 64-row segment (not _ws); nt-1 = 2*64+1")
    add("R2_16", [_r(16)], "1", 66, 15, R, edge="<16,4>, two 8-row segments (not _mcw); B+1 = BW")
    add("R3_16", [_r(16)], "ncu//65+1", 66, 519, R, edge="<16,4>, RP = 576: a second, 64-row trip")
    for nt in (34, 66):
        add("R4_32", [_r(32)], "ncu//5+1", nt, 39, R, edge="<32,4> (4K <= ncu); nt-1 = 32+1, 2*32+1")
    add("R5_64", [_r(64)], "1", 34, 100, R, edge="<64,4>")
    for n, ch, B in ((8, 64, 63), (16, 64, 40), (32, 32, 40), (64, 32, 70)):
        add(f"R6_{n}", [_r(n)], "ncu//4+1", 2 * ch + 2, B, R, edge=f"<{n},1>: one lane per row pair, 4K > ncu")
    for kof in ("1", "3"):
        for nt, B, edge in ((2, 16, "three segments, the top one of one row; one step"),
                            (65, 23, "three full segments; one full chunk"),
                            (66, 24, "four segments; a chunk hand-off"),
                            (130, 39, "five segments; the 128-slot ring wraps")):
            add("M1_16", [_r(16)], kof, nt, B, "k_pinf_recur_mcw", edge="<16>: " + edge)
        for n in (32, 17):
            for nt, B in ((66, 39), (130, 40)):
                add(f"M2_{n}", [_r(n)], kof, nt, B, "k_pinf_recur_mcw",
                    edge="<32>" + (": 15 padded classes" if n == 17 else ""))
    for n in (32, 17):
        for nt in (2, 33, 34, 66):
            add(f"X1_{n}", [_r(n)], "ncu//33+1", nt, 256, "k_pinf_recur_xr",
                edge="RP = 320: rows 257..319 +Inf, row 256 split across the waves")
    add("X1_32", [_r(32)], "ncu//4", 3, 256, "k_pinf_recur_xr", edge="the largest batch that still splits (4K = ncu)")
    add("W1_4", [_r(4)], "1", 65, 127, "k_pinf_recur_ws", edge="<4>: two full segments")
    add("W1_4", [_r(4)], "1", 130, 128, "k_pinf_recur_ws", edge="<4>: a third segment with one row")
    add("W1_one", [(5,)], "1", 3, 64, "k_pinf_recur_ws", edge="L = 1, BW = 1: ws<2>")
    P = "k_pinf_prep"
    add("P1_2x2x2", [(0, 1)] * 3, "1", 6, 20, None, P + "_small", "<8>", modes=MODES)
    add("P1_8x8", [_r(8)] * 2, "1", 6, 20, None, P + "_small", "<16>, L = 64", modes=MODES)
    add("P2_9x8c65", [_r(9), _r(8)], "1", 6, 20, None, P + "_m", "M = 2, L = 65", cut=65, modes=MODES)
    add("P2_8x8x8c256", [_r(8)] * 3, "1", 5, 24, None, P + "_m", "M = 3, L = 256: one slot", cut=256,
        modes=MODES)
    add("P2_8x8x8c257", [_r(8)] * 3, "1", 5, 24, None, P + "_m", "M = 3, L = 257: the second slot",
        cut=257, modes=MODES)
    add("P2_5x5x5", [_r(5)] * 3, "1", 6, 20, None, P + "_m", "M = 3, L = 125", modes=MODES)
    add("P2_8p4", [_r(8)] * 4, "1", 3, 29, None, P + "_m", "M = 4, L = 4096: all sixteen slots",
        modes=MODES)
    add("P2_8p4c4095", [_r(8)] * 4, "1", 3, 28, None, P + "_m", "M = 4, L = 4095", cut=4095, modes=MODES)
    add("P3_9x8x8x8c4097", [_r(9), _r(8), _r(8), _r(8)], "1", 3, 29, None, P,
        "L = 4097: past the register kernel", cut=4097, modes=MODES)
    add("P3_32", [_r(32)], "1", 4, 25, None, P, "M = 1, BWP = 32", modes=MODES)
    add("P3_3p5", [(0, 1, 2)] * 5, "1", 6, 20, None, P, "M = 5, L = 243", modes=MODES)
    return out


CASES = _cases()


def reach_limited(case, ncu=256):
    """nt·(BW-1) < B: no path of nt steps, each spending at most BW-1, ends in row B, so R_0[B] = +Inf by arithmetic
    (the xr cases of two and three steps, and the one-level case).  The conditions of test_pinf_cases.py are then
    asked of the rows a path can end in, c <= (nt-i)·(BW-1), instead of all rows up to B."""
    return case.nt * (reference_k(case, 0, ncu).BW - 1) < case.B
