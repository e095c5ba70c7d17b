"""A numpy restatement of julia_opt/example_convolution.jl:73-141, built from the reference's dense loops.

It does not go through κ: K is filled by the double loop of toeplitz (:110-122), M by Mmat's loops (:89-97), fvec by
f_to_vec's (:76-78), and the value and gradient are the dense products of eval_f_helper (:130-134) and
eval_df_helper (:140).  The device kernel's assumption -- K is strictly lower triangular Toeplitz, defined by its
first column -- is therefore tested against this file, not shared with it.  Julia's 1-based indices are kept in
the loops (arrays are shifted by one on access).
"""
import math

import numpy as np


def target(t):  # example_convolution.jl:45
    return .4 * math.cos(2 * math.pi * t)


def make_int_k(omega0=math.pi):  # :60-63
    def int_k(t):
        a = omega0 * (t - 1) / math.sqrt(2)
        return 1 / 10 * math.exp(-a) * (math.sin(a) + math.cos(a))
    return int_k


def f_to_vec(nt, T0, tau, target):  # :73-81
    fvec = np.zeros(nt + 1)
    for i in range(1, nt + 2):
        fvec[i - 1] = target(T0 + tau * i)
    return fvec


def Mmat(nt, tau):  # :85-100
    M = np.zeros((nt + 1, nt + 1))
    M[0, 0] = tau / 3
    M[nt, nt] = tau / 3
    for i in range(2, nt + 1):
        M[i - 1, i - 1] = 2 / 3 * tau
    for i in range(1, nt + 1):
        M[i - 1, i] = tau / 6
        M[i, i - 1] = tau / 6
    return M


def toeplitz(T0, nt, tau, int_k):  # :104-125
    K = np.zeros((nt + 1, nt))
    tj = T0
    for i in range(2, nt + 2):
        ti = T0 + (i - 1) * tau
        val = int_k(ti - tj) - int_k(ti - tj - tau)
        # for j = i:nt+1: K[j, j-i+1] = val -- the (i-1)-th subdiagonal
        j = np.arange(i, nt + 2)
        K[j - 1, j - i] = val
    return K


class ConvRef:
    """ConvObj(nt) of the reference with its defaults (T0 = -1, T1 = 1, ω₀ = π)."""

    def __init__(self, nt, T0=-1.0, T1=1.0, omega0=math.pi):
        self.nt, self.T0, self.T1 = nt, T0, T1
        self.tau = (T1 - T0) / nt
        self.fvec = f_to_vec(nt, T0, self.tau, target)
        self.K = toeplitz(T0, nt, self.tau, make_int_k(omega0))
        self.M = Mmat(nt, self.tau)

    def eval_f(self, u, dtype=np.float64):
        """u: (1, nt).  :128-135."""
        K, M, f = (a.astype(dtype, copy=False) for a in (self.K, self.M, self.fvec))
        v = K @ np.asarray(u, dtype=dtype).reshape(-1) - f
        return (.5 * v) @ M @ v

    def eval_df(self, x, dtype=np.float64):
        """x: (1, nt) -> df (1, nt).  :138-141."""
        K, M, f = (a.astype(dtype, copy=False) for a in (self.K, self.M, self.fvec))
        return (K.T @ (M @ (K @ np.asarray(x, dtype=dtype).reshape(-1) - f))).reshape(1, -1)


def controls(nt, K, seed, lo=-2, hi=2):
    """K integer piecewise-constant controls (1, nt) with values in lo..hi, like rand_func_int."""
    rng = np.random.default_rng(seed)
    xs = []
    for _ in range(K):
        nj = min(nt - 1, max(1, nt // 10))
        jumps = np.sort(rng.choice(np.arange(1, nt), size=nj, replace=False)) if nt > 1 else np.array([], dtype=int)
        seg = np.searchsorted(jumps, np.arange(nt), side="right")
        lv = rng.integers(lo, hi + 1, size=(1, seg.max() + 1)).astype(np.float64)
        xs.append(lv[:, seg])
    return xs
