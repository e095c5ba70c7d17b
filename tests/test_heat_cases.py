"""The cases of test_gpu_heat_shapes.py on the CPU (tests/heat_cases.py): the LU oracle is good enough to judge the
device on them, every case is sharp for every mistake of the mutation list, and the stand-in HeatProblem is not.

Measured (x86, np.longdouble eps 1.08e-19):
  oracle/heat_oracle.py against the extended-precision restatement, over every control of every case with N <= 257:
    at most 3.4e-16 relative in J and 1.1e-15 in df (bound 1e-12: three orders above, three below the device's 1e-9);
  smallest movement of any applicable mutation on the first or last control of any case: 2.7e-4 ("x not extended
    in G_t" at N = 513, nt = 7; bound 1e-6, 1000 times the device bar);
  on HeatProblem(n=5, nt=24) the four mutations of STANDIN_BLIND move J and df by at most 4.1e-18.
"""
import numpy as np
import pytest

import heat_cases as hc
from mioc.heat import HeatProblem
from oracle.heat_oracle import HeatOracle


def _rel(f, df, f0, df0):
    """(relative distance in J, max-norm relative distance in df) from the true (f0, df0)."""
    return float(abs(f - f0) / abs(f0)), float(np.max(np.abs(df - df0)) / np.max(np.abs(df0)))


def test_case_builders():
    Ns = [s.N for s in hc.CASES]
    assert sorted(set(Ns)) == [1, 15, 16, 17, 31, 33, 255, 256, 257, 496, 497, 513, 1025]
    assert len({s.id for s in hc.CASES}) == len(hc.CASES)
    assert {s.nx for s in hc.CASES} == {1, 2, 3, 4} and {s.nt for s in hc.CASES} == {1, 2, 3, 7}
    assert {s.K for s in hc.CASES} == {1, 15, 16, 17, 33}
    for nt in (1, 2):  # once on each side of the LDS / global-scratch split
        assert sorted(s.N > 496 for s in hc.CASES if s.nt == nt) == [False, True]
    assert any(s.blocks > 1 for s in hc.CASES)
    for s in hc.CASES[:9]:
        c, xs = s.case, s.xs
        N = s.N
        assert c.M_invA.shape == c.mass.shape == (N, N) and c.M_invF.shape == (N, s.nx)
        assert c.state0.shape == (N,) and c.yd.shape == (N, s.nt + 1) and xs.shape == (s.K, s.nx, s.nt)
        assert c.T0 == 0.75 and (c.T1 - c.T0) / s.nt == hc.TAU and c.gamma not in (0.0, 1.0)
        if N >= 15:
            assert not np.allclose(c.mass, c.mass.T) and not np.allclose(c.M_invA, c.M_invA.T)
            assert 0.1 < np.mean(c.yd == 0.0) < 0.3
            assert np.linalg.cond(np.eye(N) + hc.TAU * c.M_invA) < 1.9
            assert np.all(np.linalg.eigvals(c.M_invA).real > 0.0)
            Sinv = np.linalg.inv(np.eye(N) + hc.TAU * c.M_invA)
            assert (s.blocks > 1) == bool(np.any(Sinv == 0.0))
        assert len({x.tobytes() for x in xs}) == s.K                    # all distinct
        assert all(np.array_equal(x, np.round(x)) and x.min() >= 0 and x.max() <= 5 for x in xs[0::2])
        assert all(not np.array_equal(x, np.round(x)) and x.min() >= -1 and x.max() <= 6 for x in xs[1::2])


def test_ld_solves_invert_the_matrix():
    """The restatement's own elimination: S·(S⁻¹b) = b and Sᵀ·(S⁻ᵀb) = b to extended precision, with a matrix that
    needs its row exchanges."""
    rng = np.random.default_rng(5)
    S = rng.standard_normal((40, 40))
    b = rng.standard_normal(40)
    lu = hc._lu_factor(S)
    assert not np.array_equal(lu[1], np.arange(40))
    Sl = S.astype(hc.LD)
    assert np.max(np.abs(Sl @ hc._solve(lu, b) - b)) < 1e-15
    assert np.max(np.abs(Sl.T @ hc._solve_t(lu, b) - b)) < 1e-15
    s = hc.CASES[1]
    f, df = hc.heat_ref_ld(s.case, s.xs[1])                     # the one-call form is the cached one
    f2, df2 = hc.ref_ld(s).eval(s.xs[1])
    assert f.dtype == hc.LD and df.dtype == hc.LD and f == f2 and np.array_equal(df, df2)


@pytest.mark.parametrize("shape", [s for s in hc.CASES if s.N <= 257], ids=lambda s: s.id)
def test_lu_oracle_against_extended_precision(shape):
    """|J − J_ld| <= 1e-12·|J_ld| and max|df − df_ld| <= 1e-12·max|df_ld| for every control of the case (largest
    observed: 3.4e-16 and 1.1e-15, module docstring).  N = 496 and above are left to the GPU file: the elimination
    in extended precision takes seconds there, and the oracle's error grows no faster than √N."""
    o = HeatOracle(*shape.case)
    ref = hc.ref_ld(shape)
    worst = [0.0, 0.0]
    for x in shape.xs:
        f, df, _ = o.eval(x)
        eJ, ed = _rel(f, df, *ref.eval(x))
        worst = [max(worst[0], eJ), max(worst[1], ed)]
    print(f"oracle vs longdouble {shape.id}: J {worst[0]:.2e} df {worst[1]:.2e}")
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12, worst


@pytest.mark.parametrize("shape", hc.CASES, ids=lambda s: s.id)
def test_every_case_is_sharp_for_every_mutation(shape):
    """Each wrong version of the restatement that can differ at this (N, nt) does differ from the true one by at
    least 1e-6 in J (relative) or in df (max-norm relative), 1000 times the device bar, on the case's first
    integral and last control."""
    ref = hc.ref_ld(shape)
    for m in hc.MUTATIONS:
        if not hc.MUTATION_RULES[m](shape.N, shape.nt):
            continue
        for x in (shape.xs[0], shape.xs[-1]):
            moved = max(_rel(*ref.eval(x, m), *ref.eval(x)))
            print(f"mutation {shape.id} {m}: {moved:.2e}")
            assert moved >= 1e-6, (m, moved)


def test_every_mutation_applies_to_three_cases():
    applies = {m: sum(bool(rule(s.N, s.nt)) for s in hc.CASES) for m, rule in hc.MUTATION_RULES.items()}
    assert hc.MUTATIONS == list(hc.MUTATION_RULES) and len(hc.MUTATIONS) == 11
    assert min(applies.values()) >= 3, applies


def test_standin_is_blind_to_four_mutations():
    """Why the stand-in alone was not enough: with its constant yd, constant state0 and symmetric M, a yd taken a
    step early or late, Mᵀ in Gy and a reversed state0 move J and df by no more than 1e-13 relative, while the other
    mutations move them by 1e-6 or more.  (If HeatProblem is ever made generic this assertion can go.)"""
    hp = HeatProblem(n=5, nt=24)
    ref = hc.HeatRefLD(hc.HeatCase(hp.M_invA, hp.M_invF, hp.M, hp.state0, hp.yd, hp.T0, hp.T1, hp.gamma))
    x = hc.controls(2, 24, 2, seed=3)[1]
    true = ref.eval(x)
    for m in hc.MUTATIONS:
        moved = max(_rel(*ref.eval(x, m), *true))
        print(f"stand-in {m}: {moved:.2e}")
        if m in hc.STANDIN_BLIND:
            assert moved <= 1e-13, (m, moved)
        else:
            assert moved >= 1e-6, (m, moved)
