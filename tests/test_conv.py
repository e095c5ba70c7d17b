"""The signal-reconstruction (convolution) objective, CPU tier: the problem data against the dense restatement.

tests/conv_ref.py restates julia_opt/example_convolution.jl:73-141 with the reference's dense loops.  ConvProblem
(mioc/conv.py) computes only what the device needs -- κ, fvec, τ -- and must describe the same matrices bit for
bit; the restatement itself is pinned by a finite-difference check (the reference's own test_df, :156-185) and by a
committed fixture.
"""
import os

import numpy as np
import pytest

from conv_ref import ConvRef, controls, target

from mioc.conv import ConvProblem

CONV_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv", "conv_nt24.npz")


@pytest.mark.parametrize("nt", [7, 64])
def test_problem_dense_equals_restatement(nt):
    cp, ref = ConvProblem(nt=nt), ConvRef(nt)
    K, M = cp.dense()
    assert K.shape == (nt + 1, nt) and M.shape == (nt + 1, nt + 1)
    assert np.array_equal(K, ref.K) and np.array_equal(M, ref.M)
    assert np.array_equal(cp.kappa, ref.K[1:, 0])          # κ is column 1 of K below its first row
    assert np.array_equal(cp.fvec, ref.fvec)
    assert cp.tau == ref.tau and cp.levels == [[-2, -1, 0, 1, 2]]


def test_K_is_strictly_lower_triangular_toeplitz():
    ref = ConvRef(33)
    r, c = np.indices(ref.K.shape)
    assert np.all(ref.K[r - c < 1] == 0.0)                  # row 1 and the diagonal included
    assert np.all(ref.K[r - c >= 1] == ref.K[1:, 0][(r - c - 1)[r - c >= 1]])


def test_fvec_starts_one_step_after_T0():
    cp = ConvProblem(nt=16)
    assert cp.fvec[0] == target(cp.T0 + cp.tau)             # example_convolution.jl:77, i = 1
    assert cp.fvec[-1] == target(cp.T0 + cp.tau * 17)
    assert cp.fvec.shape == (17,)


def test_restatement_gradient_is_first_order_consistent():
    """|ΔJ/t − df·h| shrinks linearly in t (J is quadratic: the remainder is t·½·(Kh)ᵀM(Kh))."""
    ref = ConvRef(7)
    rng = np.random.default_rng(0)
    x = np.ones((1, 7))
    h = rng.standard_normal((1, 7))
    f0, dfh = ref.eval_f(x), float(np.sum(ref.eval_df(x) * h))
    q = 0.5 * float((ref.K @ h[0]) @ ref.M @ (ref.K @ h[0]))
    ts = (1e-4, 1e-5, 1e-6)
    errs = [abs((ref.eval_f(x + t * h) - f0) / t - dfh) for t in ts]
    for t, e in zip(ts, errs):  # the difference quotient's own rounding is a few ulp of f0 divided by t
        assert abs(e - t * q) <= 1e-3 * t * q + 1e-14 / t, (t, e, t * q)
    assert 9.0 < errs[0] / errs[1] < 11.0 and 9.0 < errs[1] / errs[2] < 11.0, errs


def test_float64_restatement_close_to_longdouble():
    """The restatement's own rounding is far below the 1e-9 bar the device is held to."""
    ref = ConvRef(64)
    for x in controls(64, 3, seed=1):
        f, fl = ref.eval_f(x), ref.eval_f(x, np.longdouble)
        d, dl = ref.eval_df(x), ref.eval_df(x, np.longdouble)
        assert abs(f - fl) <= 1e-13 * abs(fl)
        assert np.max(np.abs(d - dl)) <= 1e-13 * np.max(np.abs(dl))


def test_restatement_reproduces_conv_golden():
    """The committed fixture (tests/golden/conv/make_conv_golden.py): κ and fvec bit for bit (libm's exp / sin / cos
    may differ in the last place elsewhere: 1e-15), J and df to 1e-12 relative (BLAS summation order)."""
    g = np.load(CONV_GOLDEN, allow_pickle=False)
    nt = g["kappa"].size
    assert nt == 24 and g["x"].shape == (5, 1, 24) and set(np.unique(g["x"])) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    ref = ConvRef(nt, *g["scalars"])
    assert np.max(np.abs(ref.K[1:, 0] - g["kappa"])) <= 1e-15 * np.max(np.abs(g["kappa"]))
    assert np.max(np.abs(ref.fvec - g["fvec"])) <= 1e-15
    for k in range(5):
        assert abs(ref.eval_f(g["x"][k]) - g["J"][k]) <= 1e-12 * abs(g["J"][k]), k
        assert np.max(np.abs(ref.eval_df(g["x"][k]) - g["df"][k])) <= 1e-12 * np.max(np.abs(g["df"][k])), k
