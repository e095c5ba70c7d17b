"""CPU census of the separable transform's row items, from the oracle alone: which path of the row body (mioc_sdt.hip,
sdt_body) each item (step i, source row c') of a p = 1 DP on an 8^M grid takes, so that a GPU test can show on the CPU
that its inputs reach the path it is about before it runs them.

An item reads Ψ_j = Φ_{i+1}[j, c'] (the oracle's Φ_0 of the DP over the columns i+1 .. nt-1 alone) and writes the targets
l with c' + b̃_l(i) <= B.  With nf finite sources and nv targets, the row body's classes are, in its own order:

    empty       nv == 0 or nf == 0
    sparse      nf <= SD_SPARSE
    one-target  nv == 1                 (the persistent drivers' one-target item; a direct row of one for the per-step one)
    direct      nv <= SD_FEW            (every target goes to the exact scan)
    transform   otherwise               (the certified winners)

For a transform item, `ties` counts the targets whose minimum of R(l, j) = fl(fl(T1_l + fl(β·d)) + Ψ_j) is attained by two
or more sources exactly.  The certified transform's invariant (an unflagged winner beats every other source by more than
tol) makes each of them a listed target of the exact scan, and its row a redone (counting) row.  `near` counts the targets
whose runner-up lies within 2^-30 of the row's span (2·max|R| + 8·M·β) of the minimum: `near == ties` says every other
target is decided by a margin some thousand times the transform's tolerance (3g + the reference's rounding, about 2^-42 of
the row's range), so exactly the tied ones are listed.
"""
import numpy as np

from oracle.oracle import P_ONE, OracleC

SD_FEW, SD_SPARSE, SD_COOP, SD_LCAP = 4, 4, 8, 512  # mioc_sdt_common.h


def source_fronts(lv, df, uo, B, beta, dt, threads=8):
    """Φ_s for s = 1 .. nt-1 as (B+1, L) arrays (index s; entry 0 is None): the oracle on the columns s .. nt-1."""
    nt = df.shape[1]
    out = [None]
    for s in range(1, nt):
        phi, _ = OracleC().bellman(lv, np.asfortranarray(df[:, s:]), np.asfortranarray(uo[:, s:]), B, P_ONE, beta, dt,
                                   threads=threads)
        out.append(np.array(phi[:, :, 0]))  # the last front written is buffer 0 for every column count
    return out


def item_class(nf, nv):
    if nv == 0 or nf == 0:
        return "empty"
    if nf <= SD_SPARSE:
        return "sparse"
    if nv == 1:
        return "one-target"
    if nv <= SD_FEW:
        return "direct"
    return "transform"


def classes(lv, uo, B, fronts):
    """{(i, c'): (class, nf, nv)} for every item of rows 1 .. B."""
    nuv = np.asarray(lv.nuval, dtype=np.int64)
    out = {}
    for i in range(len(fronts) - 1):
        bt = np.abs(nuv - uo[:, i].astype(np.int64)).sum(axis=1)
        for c in range(1, B + 1):
            nf = int(np.isfinite(fronts[i + 1][c]).sum())
            nv = int((c + bt <= B).sum())
            out[(i, c)] = (item_class(nf, nv), nf, nv)
    return out


def item_ties(lv, df, uo, B, beta, dt, fronts, i, c, chunk=256):
    """(ties, near) of item (i, c): see the module's docstring."""
    nuv = np.asarray(lv.nuval, dtype=np.int64)
    M = nuv.shape[1]
    bt = np.abs(nuv - uo[:, i].astype(np.int64)).sum(axis=1)
    tg = np.nonzero(c + bt <= B)[0]
    psi = fronts[i + 1][c]
    t1 = np.zeros(len(nuv))
    for m in range(M):
        t1 = t1 + (dt * df[m, i]) * nuv[:, m].astype(np.float64)
    ties = near = 0
    for s in range(0, len(tg), chunk):
        l = tg[s:s + chunk]
        d = np.abs(nuv[l][:, None, :] - nuv[None, :, :]).sum(axis=2).astype(np.float64)
        val = (t1[l][:, None] + beta * d) + psi[None, :]
        mn = val.min(axis=1)
        ties += int(((val == mn[:, None]).sum(axis=1) >= 2).sum())
        fin = val[np.isfinite(val)]
        if fin.size == 0:
            continue
        span = 2.0 * np.abs(fin).max() + 8 * M * beta
        near += int(((val <= mn[:, None] + span * 2.0 ** -30).sum(axis=1) >= 2).sum())
    return ties, near
