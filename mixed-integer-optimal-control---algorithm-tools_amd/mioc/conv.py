"""The signal-reconstruction (convolution) objective: host-side problem data + the device gradient producer.

Reference: julia_opt/example_convolution.jl (ConvObj; Marko / Wachsmuth, "Integer optimal control problems with total
variation regularization", §6.2): one control with the signed levels 𝓥 = [[-2,-1,0,1,2]] on [T0, T1] = [-1, 1],
v = K·xᵀ − fvec, J = ½·vᵀ·M·v (:128-135), df = (Kᵀ·(M·v))ᵀ (:138-141).  It is the fifth preset of the reference's
main() (multi-trust.jl:190-192: β = 1e-4, Δ⁰ = 0.125, p = 1).

``ConvProblem`` computes what the Julia struct computes when it is built, operation by operation:
  fvec   f_to_vec (:73-81): fvec[i] = target(T0 + τ·i), i = 1..nt+1 -- one step AFTER T0, as the reference has it;
  kappa  column 1 of toeplitz (:104-125) below its first row: κ[d] = int_k(ti − tj) − int_k(ti − tj − τ) with
         tj = T0 and ti = T0 + d·τ (the reference's expressions, so ti − tj carries their rounding);
  M      Mmat (:85-100).
K is strictly lower triangular Toeplitz (row 1 and the diagonal are zero), so the nt numbers κ define it; the device
never stores it (mioc_conv_setup takes κ and fvec).  κ and fvec hold exp / sin / cos of the host's libm, so parity
with Julia's own floats is unpinned (as for the heat example); the Julia binding passes obj.K / obj.fvec instead.
"""
from __future__ import annotations

import math

import numpy as np

from .iterators import LevelTable, product_iterator
from .objective import AbstractObjectiveLazy


class ConvProblem:
    """Data of example_convolution.jl:17-70 for nt steps: tau, kappa (nt,), fvec (nt+1,), levels."""

    def __init__(self, nt=2048, T0=-1.0, T1=1.0, omega0=math.pi, target=None, int_k=None):
        nt = int(nt)
        if nt < 1:
            raise ValueError("nt must be positive")
        self.nt, self.T0, self.T1, self.omega0 = nt, float(T0), float(T1), float(omega0)
        self.tau = (self.T1 - self.T0) / nt  # example_convolution.jl:31
        self.levels = [[-2, -1, 0, 1, 2]]    # 𝓥 (:24)
        w0 = self.omega0
        if target is None:
            def target(t):  # :45
                return .4 * math.cos(2 * math.pi * t)
        if int_k is None:
            def int_k(t):   # the kernel's antiderivative, :60-63
                a = w0 * (t - 1) / math.sqrt(2)
                return 1 / 10 * math.exp(-a) * (math.sin(a) + math.cos(a))
        self.target, self.int_k = target, int_k
        T0, tau = self.T0, self.tau
        self.fvec = np.array([target(T0 + tau * i) for i in range(1, nt + 2)], dtype=np.float64)
        tj = T0
        kap = np.empty(nt)
        for i in range(2, nt + 2):  # :110-118, val of row i
            ti = T0 + (i - 1) * tau
            kap[i - 2] = int_k(ti - tj) - int_k(ti - tj - tau)
        self.kappa = kap

    def dense(self):
        """(K, M) as numpy arrays: K (nt+1, nt) from kappa, M (nt+1, nt+1) of Mmat -- for tests and yardsticks."""
        nt, tau = self.nt, self.tau
        r, c = np.arange(nt + 1)[:, None], np.arange(nt)[None, :]
        d = r - c
        K = np.where(d >= 1, self.kappa[np.clip(d - 1, 0, nt - 1)], 0.0)
        i = np.arange(nt + 1)
        M = np.zeros((nt + 1, nt + 1))
        M[i, i] = 2 / 3 * tau
        M[0, 0] = M[nt, nt] = tau / 3
        M[i[:-1], i[:-1] + 1] = M[i[:-1] + 1, i[:-1]] = tau / 6
        return K, M

    def setup(self, ctx):
        """Hand kappa and fvec to a native.Context (mioc_conv_setup)."""
        ctx.conv_setup(self.kappa, self.fvec, self.T0, self.T1)

    # the rest of what mioc.trm_batch.TRM_batch asks of a problem
    fixes_nt = "the convolution problem fixes nt"  # kappa and fvec are sampled for it

    def level_table(self):
        return LevelTable(self.levels)

    def eval_tensors(self, ctx, x, J=None, df=None):
        ctx.conv_eval_tensors(x, J, df)

    def check_restarts(self, K):
        """Any number of restarts."""


class ConvObj(AbstractObjectiveLazy):
    """The reference's ConvObj (example_convolution.jl:17-70) as a lazy objective for TRM: eval_f_helper and
    eval_df_helper (:128-141) run on the device through mioc_conv_eval (no CPU path).  One device call computes
    both; the gradient of the last eval_f at obj.x is kept and handed out by eval_df."""

    def __init__(self, problem=None, ctx=None, device=0, **kw):
        from .native import Context
        self.problem = ConvProblem(**kw) if problem is None else problem
        cp = self.problem
        self.T0, self.T1, self.nt, self.tau = cp.T0, cp.T1, cp.nt, cp.tau
        self.V = [list(v) for v in cp.levels]
        self.iterator = product_iterator(self.V)  # :25
        self.nu, self.nv = 0, len(self.V)
        self.nx = self.nu + self.nv
        self._init_fields(self.nx, self.nt)
        self.ctx = Context(device) if ctx is None else ctx
        cp.setup(self.ctx)
        self._df_at = None

    def eval_f_helper(self, x, cache):
        J, df = self.ctx.conv_eval(np.asarray(x, dtype=np.float64)[None])
        if cache:
            self._df_at = (np.array(x, copy=True), df[0])
        return float(J[0])

    def eval_df_helper(self):
        if self._df_at is None or not np.array_equal(self._df_at[0], self.x):
            _, df = self.ctx.conv_eval(np.asarray(self.x, dtype=np.float64)[None])
            self._df_at = (np.array(self.x, copy=True), df[0])
        self.df[:, :] = self._df_at[1]
