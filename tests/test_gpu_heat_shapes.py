"""mioc_heat.hip on generic caller data at every edge of its tiling: mioc_heat_eval_device against the LU oracle
(oracle/heat_oracle.py) on the same matrices.

The data (tests/heat_cases.py) has none of the stand-in's structure -- yd and state0 random in every entry, M and
M_invA non-symmetric, T0 ≠ 0, N no perfect square, half of the controls non-integral -- so a wrong step index of yd or
M·yd, Mᵀ for M, a permuted or dropped row of the operand layout and a column that reads its neighbour's control each
move J or df by 2.7e-4 or more (tests/test_heat_cases.py), against a bar of 1e-9.  The shapes are the smallest that
reach each edge: N = 1, 15 / 16 / 17, 31 / 33 (row padding to Np = 16·ceil(N/16), odd tile counts), 255 / 256 / 257
(16 waves with one tile each; the second slot of heat_gemm first used), 496 / 497 (k_heat_run<false>, state columns
in LDS, against k_heat_run<true>, in the global scratch), 513 and 1025 (second and third trip of the t0 += 32 loop);
nt = 1 and 2 on both sides of the split (the adjoint's prefetch never or once refilled).  N = 2048, the largest the
ABI takes, stays out: its host-side Gauss-Jordan alone is about 1.7e10 operations, not a test of seconds; the
rejection of N > 2048 is tested in test_heat.py.

Bar: the project's own for a floating-point producer (tests/test_heat.py, tests/test_gpu_conv.py):
|J − J_ref| <= 1e-9·|J_ref| and max|df − df_ref| <= 1e-9·max|df_ref|.  The oracle is within 3.4e-16 / 1.1e-15 of an
extended-precision restatement on these inputs (N <= 257, tests/test_heat_cases.py).  Largest device error observed
against the oracle: 7.2e-16 in J (N = 513) and 2.9e-15 in df (N = 497), six orders under the bar.
"""
import functools

import numpy as np
import pytest

import heat_cases as hc
from oracle.heat_oracle import HeatOracle

pytestmark = pytest.mark.gpu

LDS_CASE, GM_CASE = hc.BY_ID["N496_nx2_nt3_K17"], hc.BY_ID["N497_nx2_nt3_K17"]
SEQUENCE = [hc.BY_ID[i] for i in ("N513_nx4_nt7_K33", "N17_nx1_nt2_K1", "N496_nx2_nt3_K17", "N497_nx2_nt3_K17")]


@functools.lru_cache(maxsize=None)
def _ref(shape):
    """The oracle's (J (K,), df (K, nx, nt)) of a shape, computed once."""
    o = HeatOracle(*shape.case)
    out = [o.eval(x)[:2] for x in shape.xs]
    return np.array([f for f, _ in out]), np.stack([df for _, df in out])


def _eval(ctx, shape, want_J=True, want_df=True):
    """One mioc_heat_eval_device call into NaN-filled outputs -> (J (K,) or None, df (K, nx, nt) or None)."""
    import torch
    dx = torch.tensor(np.ascontiguousarray(shape.xs.transpose(0, 2, 1)), dtype=torch.float64, device="cuda")
    J = torch.full((shape.K,), float("nan"), dtype=torch.float64, device="cuda") if want_J else None
    df = torch.full_like(dx, float("nan")) if want_df else None
    ctx.heat_eval_tensors(dx, J, df)
    ctx.synchronize()
    return (J.cpu().numpy() if want_J else None), (df.cpu().numpy().transpose(0, 2, 1) if want_df else None)


@functools.lru_cache(maxsize=None)
def _fresh(shape):
    """J and df of a shape from a context that has seen nothing else."""
    from mioc import native
    ctx = native.Context(0)
    ctx.heat_setup(*shape.case)
    out = _eval(ctx, shape)
    ctx.close()
    return out


@pytest.mark.parametrize("shape", hc.CASES, ids=lambda s: s.id)
def test_heat_generic_data_vs_oracle(shape):
    J, df = _fresh(shape)
    Jo, dfo = _ref(shape)
    eJ = np.abs(J - Jo) / np.abs(Jo)
    ed = np.max(np.abs(df - dfo), axis=(1, 2)) / np.max(np.abs(dfo), axis=(1, 2))
    print(f"device vs oracle {shape.id}: J {eJ.max():.2e} df {ed.max():.2e}")
    assert np.all(eJ <= 1e-9), (int(np.argmax(~(eJ <= 1e-9))), eJ.max())
    assert np.all(ed <= 1e-9), (int(np.argmax(~(ed <= 1e-9))), ed.max())


@pytest.mark.parametrize("shape", [LDS_CASE, GM_CASE], ids=lambda s: s.id)
def test_heat_single_outputs_equal_both(shape):
    """J alone (d_df null: no Gy scratch, no adjoint) and df alone (d_J null) are the bits of the call with both."""
    from mioc import native
    J, df = _fresh(shape)
    assert not np.isnan(J).any() and not np.isnan(df).any()
    ctx = native.Context(0)
    ctx.heat_setup(*shape.case)
    J1, none = _eval(ctx, shape, want_df=False)
    assert none is None and np.array_equal(J1, J)
    none, df1 = _eval(ctx, shape, want_J=False)
    assert none is None and np.array_equal(df1, df)
    ctx.close()


def test_heat_host_entry_equals_device_entry_global_scratch():
    """mioc_heat_eval (host arrays) on the global-scratch variant gives the device entry's bits."""
    from mioc import native
    J, df = _fresh(GM_CASE)
    ctx = native.Context(0)
    ctx.heat_setup(*GM_CASE.case)
    Jh, dfh = ctx.heat_eval(GM_CASE.xs)
    ctx.close()
    assert np.array_equal(Jh, J) and np.array_equal(dfh, df)


def test_heat_one_context_several_problems():
    """A larger problem, then smaller ones, then the switch between the two kernel variants on one context: the
    tables shrink under the Gy and state scratch of the first call, which stay allocated with stale contents.
    Every result is the fresh context's, bit for bit.  A setup that fails validation (documented in mioc.h) leaves
    the last good problem in place: the next evaluation repeats its bits."""
    from mioc import native
    ctx = native.Context(0)
    for shape in SEQUENCE:
        ctx.heat_setup(*shape.case)
        J, df = _eval(ctx, shape)
        Jf, dff = _fresh(shape)
        assert np.array_equal(J, Jf) and np.array_equal(df, dff), shape.id
    last = SEQUENCE[-1]
    c, N = last.case, last.N
    tau = (c.T1 - c.T0) / last.nt
    nan_A = c.M_invA.copy()
    nan_A[N // 2, N - 1] = np.nan
    rng = np.random.default_rng(1)
    bad = [c._replace(M_invA=nan_A),                                    # a NaN in M_invA
           c._replace(M_invA=-np.eye(N) / tau),                         # I + τ·M_invA = 0: singular
           c._replace(M_invF=rng.standard_normal((N, 5)))]              # nx = 5 > 4
    assert np.all(np.eye(N) + tau * bad[1].M_invA == 0.0)
    for b in bad:
        with pytest.raises(native.MiocNativeError) as e:
            ctx.heat_setup(*b)
        assert e.value.code == native.MIOC_EINVAL
        J, df = _eval(ctx, last)
        Jf, dff = _fresh(last)
        assert np.array_equal(J, Jf) and np.array_equal(df, dff)
    ctx.close()
