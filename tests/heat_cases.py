"""TEST INFRASTRUCTURE -- generic caller data for the heat objective, and its restatement in extended precision.

mioc_heat_setup (include/mioc.h) takes a caller's M_invA, M_invF, mass, state0 and yd of any N from 1 to 2048; the
stand-in mioc.heat.HeatProblem only ever supplies a constant yd, a constant state0, a symmetric M, T0 = 0 and
N = n².  The builders here break each of those structures, so that a wrong step index of yd, Mᵀ for M, a permuted
row or a wrong tile of the operand layout moves J or df (tests/test_heat_cases.py measures by how much).

  generic_case(N, nx, nt, seed)  the arguments of Context.heat_setup / HeatOracle, every array from one seeded rng
  controls(nx, nt, K, seed)      K distinct controls (K, nx, nt): half integral in 0..5, half doubles in [-1, 6]
  heat_ref_ld(case, x)           julia_opt/PDEObjective.jl:129-199 with the hooks of example_heat.jl:135-161 in
                                 np.longdouble (eps 1.08e-19 on x86), its own Gaussian elimination with partial
                                 pivoting (scipy's LU has no extended type); shares only the formulas with
                                 oracle/heat_oracle.py
  MUTATIONS                      named wrong versions of that restatement, one per mistake the kernel could make
  CASES                          the shapes of tests/test_gpu_heat_shapes.py: one per edge of mioc_heat.hip's tiling
"""
from __future__ import annotations

import collections
import functools

import numpy as np

LD = np.longdouble

HeatCase = collections.namedtuple("HeatCase", "M_invA M_invF mass state0 yd T0 T1 gamma")
TAU = 0.25


def generic_case(N, nx, nt, seed, gamma=0.37, blocks=1):
    """Non-symmetric M_invA with its spectrum right of 0 (cond(I + τ·M_invA) < 1.9 for N = 1..528), non-symmetric
    mass (the hooks use M literally: Gy = M·v, G = ½(vᵀM)v, so M and Mᵀ differ), T0 ≠ 0, random M_invF and state0,
    yd random in space and time with a fifth of its entries exactly 0.0 (setup skips y == 0.0).  blocks > 1 makes
    M_invA block-diagonal, so S⁻¹ has exact zeros (setup skips b == 0.0)."""
    assert gamma not in (0.0, 1.0)
    rng = np.random.default_rng(seed)
    M_invA = np.diag(rng.uniform(0.5, 4.0, N)) + 0.3 * rng.standard_normal((N, N)) / np.sqrt(N)
    mass = np.diag(rng.uniform(0.5, 2.0, N)) + 0.2 * rng.standard_normal((N, N)) / np.sqrt(N)
    M_invF = rng.standard_normal((N, nx))
    state0 = rng.standard_normal(N)
    yd = rng.standard_normal((N, nt + 1))
    yd[rng.uniform(size=yd.shape) < 0.2] = 0.0
    if blocks > 1:
        blk = np.arange(N) * blocks // N
        M_invA[blk[:, None] != blk[None, :]] = 0.0
    T0 = 0.75
    return HeatCase(M_invA, M_invF, mass, state0, yd, T0, T0 + TAU * nt, gamma)


def controls(nx, nt, K, seed):
    """(K, nx, nt), all distinct: the even ones integral in 0..5 (the DP's levels), the odd ones arbitrary doubles
    in [-1, 6] (the ABI takes doubles, and TRM_mixed feeds non-integral ones)."""
    rng = np.random.default_rng(seed)
    assert 6 ** (nx * nt) >= (K + 1) // 2, "not enough distinct integral controls"
    xs, seen = [], set()
    for k in range(K):
        while True:
            x = (rng.integers(0, 6, (nx, nt)).astype(np.float64) if k % 2 == 0 else rng.uniform(-1.0, 6.0, (nx, nt)))
            if x.tobytes() not in seen:
                break
        seen.add(x.tobytes())
        xs.append(x)
    return np.stack(xs)


# ------------------------------------------------------------------ extended-precision restatement -----------------

def _lu_factor(S):
    """PS = LU by Gaussian elimination with partial pivoting (L unit lower, both in one array); rows of S in perm."""
    A = np.array(S, dtype=LD)
    N = A.shape[0]
    perm = np.arange(N)
    for k in range(N):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        assert A[p, k] != 0.0, "singular"
        if p != k:
            A[[k, p]] = A[[p, k]]
            perm[[k, p]] = perm[[p, k]]
        if k + 1 < N:
            A[k + 1:, k] /= A[k, k]
            A[k + 1:, k + 1:] -= A[k + 1:, k, None] * A[None, k, k + 1:]
    return A, perm


def _solve(lu, b):
    """S⁻¹ b."""
    A, perm = lu
    N = A.shape[0]
    y = np.array(b, dtype=LD)[perm]
    for k in range(1, N):                     # L y = P b
        y[k] -= A[k, :k] @ y[:k]
    for k in range(N - 1, -1, -1):            # U x = y
        y[k] = (y[k] - A[k, k + 1:] @ y[k + 1:]) / A[k, k]
    return y


def _solve_t(lu, b):
    """S⁻ᵀ b: Sᵀ = Uᵀ Lᵀ P."""
    A, perm = lu
    N = A.shape[0]
    w = np.array(b, dtype=LD)
    for k in range(N):                        # Uᵀ w = b
        w[k] /= A[k, k]
        w[k + 1:] -= A[k, k + 1:] * w[k]
    for k in range(N - 1, 0, -1):             # Lᵀ v = w
        w[:k] -= A[k, :k] * w[k]
    x = np.empty_like(w)
    x[perm] = w
    return x


class HeatRefLD:
    """The factored case; eval(x, mutation) restates eval_f_helper / eval_df_helper, or a named wrong version."""

    def __init__(self, case):
        # the x87 80-bit type; a platform whose long double is a plain double cannot judge a float64 oracle
        assert np.finfo(LD).eps < 1e-18, "np.longdouble is not an extended type here: restate this with mpmath"
        c = self.case = HeatCase(*(np.asarray(a, dtype=LD) for a in case))
        self.N, self.nx = c.M_invF.shape
        self.nt = c.yd.shape[1] - 1
        self.tau = (c.T1 - c.T0) / LD(self.nt)                                 # example_heat.jl:90
        self.lu = _lu_factor(np.eye(self.N, dtype=LD) + self.tau * c.M_invA)    # :113-115 (one factorisation
        # serves StateMat and StateMat': in exact arithmetic lu(S') solves what the transposed sweeps of lu(S) do)

    def eval(self, x, mutation=None):
        """x (nx, nt) -> (fval, df (nx, nt)) in longdouble."""
        c, nt, tau, m = self.case, self.nt, self.tau, mutation
        assert m is None or m in MUTATION_RULES, m
        x = np.asarray(x, dtype=LD)
        xe = np.hstack([x, x[:, -1:]])                                          # PDEObjective.jl:145
        yd = {None: lambda i: c.yd[:, i], "yd one step early": lambda i: c.yd[:, max(i - 1, 0)],
              "yd one step late": lambda i: c.yd[:, min(i + 1, nt)]}.get(m, lambda i: c.yd[:, i])
        state = np.empty((self.N, nt + 1), dtype=LD)
        state[:, 0] = c.state0[::-1] if m == "state0 rows reversed" else c.state0    # :130
        for i in range(1, nt + 1):                                              # :134-137
            xi = xe[:, i] if m == "M_invF applied with x of step j+1" else xe[:, i - 1]
            state[:, i] = _solve(self.lu, state[:, i - 1] + tau * (c.M_invF @ xi))
        v = [state[:, i] - yd(i) for i in range(nt + 1)]
        G = lambda i: LD(0.5) * ((v[i] @ c.mass) @ v[i])                        # noqa: E731  example_heat.jl:135-140
        Gt = lambda i: c.gamma * np.sum(xe[:, i])                               # noqa: E731  :143-145
        if m == "x not extended in G_t":
            Gt = lambda i: c.gamma * np.sum(x[:, i]) if i < nt else LD(0)       # noqa: E731
        w0 = LD(1) if m == "first trapezoid weight 1" else LD(0.5)
        wn = LD(1) if m == "last trapezoid weight 1" else LD(0.5)
        fval = w0 * (G(0) + Gt(0))                                              # PDEObjective.jl:148
        for i in range(1, nt):                                                  # :149-151
            fval += G(i) + Gt(i)
        fval += wn * (G(nt) + Gt(nt))                                           # :152
        fval *= tau                                                             # :153
        Mgy = c.mass.T if m == "M^T in Gy" else c.mass
        back = _solve if m == "S^-1 for S^-T in the adjoint" else _solve_t
        adj = np.zeros((self.N, nt + 1), dtype=LD)                              # :163
        for i in range(nt - 1, -1, -1):                                         # :167-170
            adj[:, i] = back(self.lu, adj[:, i + 1] + tau * (Mgy @ v[i]))       # Gy! (example_heat.jl:152-155)
        df = np.zeros((self.nx, nt), dtype=LD)                                  # :182
        for i in range(nt):                                                     # :185-187
            df[:, i] += c.M_invF.T @ adj[:, i]
        for i in range(1, nt):                                                  # :193-197 (Gu of i = 1 is dropped)
            if not (m == "Gu missing at step 1" and i == 1):
                df[:, i] += c.gamma                                             # Gu! (example_heat.jl:158-161)
        if m == "Gu added at step 0":
            df[:, 0] += c.gamma
        return fval, df


def heat_ref_ld(case, x, mutation=None):
    return HeatRefLD(case).eval(x, mutation)


# name -> the rule that says whether the mutation can change anything on an (N, nt) case at all: a 1 x 1 M equals its
# transpose, one row cannot be reversed, and with nt = 1 the extended x has two equal columns and no step 1 < nt
MUTATION_RULES = {
    "yd one step early": lambda N, nt: True,
    "yd one step late": lambda N, nt: True,
    "M^T in Gy": lambda N, nt: N >= 2,
    "S^-1 for S^-T in the adjoint": lambda N, nt: N >= 2,
    "last trapezoid weight 1": lambda N, nt: True,
    "first trapezoid weight 1": lambda N, nt: True,
    "Gu added at step 0": lambda N, nt: True,
    "Gu missing at step 1": lambda N, nt: nt >= 2,
    "x not extended in G_t": lambda N, nt: True,
    "state0 rows reversed": lambda N, nt: N >= 2,
    "M_invF applied with x of step j+1": lambda N, nt: nt >= 2,
}
MUTATIONS = list(MUTATION_RULES)
# what the constant yd, constant state0 and symmetric M of the stand-in cannot see
STANDIN_BLIND = ["yd one step early", "yd one step late", "M^T in Gy", "state0 rows reversed"]


# ------------------------------------------------------------------ the shapes -------------------------------------

class Shape(collections.namedtuple("Shape", "id N nx nt K seed gamma blocks edge")):
    """One shape of CASES; .case and .xs are built once and shared (read-only) by the tests that use them."""

    @property
    def case(self):
        return _built(self)[0]

    @property
    def xs(self):
        return _built(self)[1]


@functools.lru_cache(maxsize=None)
def _built(s):
    case = generic_case(s.N, s.nx, s.nt, s.seed, gamma=s.gamma, blocks=s.blocks)
    xs = controls(s.nx, s.nt, s.K, s.seed + 1)
    for a in (*case[:5], xs):
        a.setflags(write=False)
    return case, xs


def _shape(N, nx, nt, K, gamma, edge, blocks=1, tag="", salt=0):
    """salt: another seed for a case whose controls leave a mutation of test_heat_cases.py without effect."""
    return Shape(f"N{N}{tag}_nx{nx}_nt{nt}_K{K}", N, nx, nt, K, 7000 + 10 * N + nt + 100000 * salt, gamma, blocks, edge)


# Np = 16·ceil(N/16) rows in Np/16 tiles; 16 waves, wave w owns tiles w, w + 16 (two slots) and then steps by 32.
# nx in 1..4, nt in {1, 2, 3, 7} (1 and 2 once on each side of HMAXN_LDS = 496), K in {1, 15, 16, 17, 33}.
CASES = [
    _shape(1, 1, 1, 1, 0.37, "one real row, 15 padded; E = 256 < the 1024 threads; nt = 1 in LDS"),
    _shape(15, 2, 3, 15, 2.5, "last row of the only tile unused"),
    _shape(16, 3, 7, 16, 0.6, "one full tile"),
    _shape(17, 1, 2, 1, 1.7, "one row into the second tile; nt = 2 in LDS"),
    _shape(31, 4, 3, 17, 0.37, "two tiles, KB = 4"),
    _shape(33, 2, 7, 33, 3.1, "odd tile count (3), KB = 6; block-diagonal M_invA", blocks=3),
    _shape(255, 3, 3, 15, 0.6, "16 tiles, the last short: every wave's second slot off"),
    _shape(256, 1, 7, 17, 2.5, "16 full tiles: every wave's second slot off", salt=1),
    _shape(257, 4, 3, 16, 1.7, "17 tiles: wave 0 alone has both slots on"),
    _shape(496, 2, 3, 17, 0.37, "31 tiles: the largest LDS variant, 145 KB of dynamic LDS"),
    _shape(497, 2, 3, 17, 0.37, "32 tiles: the smallest global-scratch variant, all 32 slots on"),
    _shape(497, 3, 1, 16, 2.5, "nt = 1 in the global scratch; block-diagonal M_invA", blocks=2, tag="b"),
    _shape(513, 4, 7, 33, 0.6, "33 tiles: second trip of the t0 += 32 loop for wave 0 only"),
    _shape(1025, 3, 2, 15, 1.7, "65 tiles: third trip; nt = 2 in the global scratch"),
]
BY_ID = {s.id: s for s in CASES}


@functools.lru_cache(maxsize=None)
def ref_ld(shape):
    """The factored restatement of a shape, shared by the tests of one process."""
    return HeatRefLD(shape.case)
