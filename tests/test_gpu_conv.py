"""The signal-reconstruction (convolution) objective on the device: mioc_conv_eval_device against the dense
restatement (tests/conv_ref.py, julia_opt/example_convolution.jl:73-141 loop by loop).

Bar: the project's own for a floating-point producer (tests/test_heat.py): |J − J_ref| <= 1e-9·|J_ref| and
max|df − df_ref| <= 1e-9·max|df_ref|.  The device builds K's entries from κ on the fly and sums on the FP64 matrix
cores in its own order; float64 numpy differs from np.longdouble by ~3e-15 relative at nt = 2048, six orders below
the bar, while the easiest mistake (fvec shifted by one sample) moves df by 1e-1 relative at nt <= 64 -- the small
shapes are the sharp ones.  nt around 16 and K around 16 / 32 straddle the 16 x 16 MFMA tile in both dimensions.
"""
import functools
import math
import os

import numpy as np
import pytest

from conv_ref import ConvRef, controls

from mioc.conv import ConvProblem

pytestmark = pytest.mark.gpu

CONV_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv", "conv_nt24.npz")


@functools.lru_cache(maxsize=None)
def _ref(nt):
    return ConvRef(nt)


def _device_eval(cp, xs, want_df=True):
    import torch
    from mioc import native
    ctx = native.Context(0)
    cp.setup(ctx)
    dx = torch.tensor(np.ascontiguousarray(np.stack([x.T for x in xs])), dtype=torch.float64, device="cuda")
    J = torch.empty(len(xs), dtype=torch.float64, device="cuda")
    df = torch.empty_like(dx) if want_df else None
    ctx.conv_eval_tensors(dx, J, df)
    ctx.synchronize()
    out = J.cpu().numpy(), (df.cpu().numpy() if want_df else None)
    ctx.close()
    return out


def _check(ref, xs, J, df):
    for k, x in enumerate(xs):
        fo, dfo = ref.eval_f(x), ref.eval_df(x)
        assert abs(J[k] - fo) <= 1e-9 * abs(fo), (k, J[k], fo)
        if df is not None:
            err, scale = np.max(np.abs(df[k].T - dfo)), np.max(np.abs(dfo))
            assert err <= 1e-9 * scale, (k, err, scale)


@pytest.mark.parametrize("K", [1, 16, 17, 33])
@pytest.mark.parametrize("nt", [1, 2, 15, 16, 17, 64, 100])
def test_conv_eval_device_vs_restatement(nt, K):
    xs = controls(nt, K, seed=nt * 1000 + K)
    J, df = _device_eval(ConvProblem(nt=nt), xs)
    _check(_ref(nt), xs, J, df)


def test_conv_eval_device_vs_restatement_nt2048():
    """The reference's default size (128 / 129 column tiles, 32 / 33 workgroups per restart tile, two restart tiles)."""
    xs = controls(2048, 20, seed=2048)
    J, df = _device_eval(ConvProblem(nt=2048), xs)
    _check(_ref(2048), xs, J, df)


def test_conv_device_vs_golden():
    """The device on the committed fixture's κ, fvec and controls against its stored J / df (1e-9 relative)."""
    import torch
    from mioc import native
    g = np.load(CONV_GOLDEN, allow_pickle=False)
    ctx = native.Context(0)
    ctx.conv_setup(g["kappa"], g["fvec"], *g["scalars"])
    dx = torch.tensor(np.ascontiguousarray(g["x"].transpose(0, 2, 1)), dtype=torch.float64, device="cuda")
    J = torch.empty(len(g["x"]), dtype=torch.float64, device="cuda")
    df = torch.empty_like(dx)
    ctx.conv_eval_tensors(dx, J, df)
    ctx.synchronize()
    J, df = J.cpu().numpy(), df.cpu().numpy()
    ctx.close()
    for k in range(len(g["x"])):
        assert abs(J[k] - g["J"][k]) <= 1e-9 * abs(g["J"][k]), k
        assert np.max(np.abs(df[k].T - g["df"][k])) <= 1e-9 * np.max(np.abs(g["df"][k])), k


def test_conv_J_only_equals_J_with_gradient():
    cp = ConvProblem(nt=100)
    xs = controls(100, 19, seed=3)
    J1, _ = _device_eval(cp, xs, want_df=False)
    J2, _ = _device_eval(cp, xs, want_df=True)
    assert np.array_equal(J1, J2)


def test_conv_batch_restart_independence():
    """1024 restarts (64 restart tiles): copies of the same control in different tiles and lanes give bit-identical
    J / df, and the first 8 match the restatement."""
    base = controls(100, 8, seed=11)
    xs = [base[k % 8] for k in range(1024)]
    J, df = _device_eval(ConvProblem(nt=100), xs)
    for k in range(8, 1024):
        assert J[k] == J[k % 8] and np.array_equal(df[k], df[k % 8]), k
    _check(_ref(100), base, J[:8], df[:8])


def test_conv_single_restart_equals_its_row_in_a_batch():
    """K = 1 (one padded tile) against the same control at position 20 of a batch of 37, and against its copies in a
    batch of 4800: 300 restart tiles x 4 column pairs >= 1024 waves, where a wave takes two column tiles instead of
    one (launch_conv_mm) -- the results must not depend on that choice."""
    xs = controls(100, 37, seed=5)
    cp = ConvProblem(nt=100)
    J, df = _device_eval(cp, xs)
    J1, df1 = _device_eval(cp, [xs[20]])
    assert J1[0] == J[20] and np.array_equal(df1[0], df[20])
    Jb, dfb = _device_eval(cp, [xs[k % 37] for k in range(4800)])
    for k in range(4800):
        assert Jb[k] == J[k % 37] and np.array_equal(dfb[k], df[k % 37]), k


def test_conv_host_entry_equals_device_entry():
    """mioc_conv_eval (host arrays, what the Julia binding calls) gives the device entry's results bit for bit."""
    from mioc import native
    cp = ConvProblem(nt=60)
    xs = controls(60, 21, seed=8)
    J, df = _device_eval(cp, xs)
    ctx = native.Context(0)
    cp.setup(ctx)
    Jh, dfh = ctx.conv_eval(np.stack(xs))
    ctx.close()
    assert np.array_equal(Jh, J) and np.array_equal(dfh.transpose(0, 2, 1), df)


def test_conv_errors():
    import torch
    from mioc import native
    ctx = native.Context(0)

    def code(f):
        with pytest.raises(native.MiocNativeError) as e:
            f()
        return e.value.code

    assert code(lambda: ctx.conv_setup(np.zeros(0), np.zeros(1), -1.0, 1.0)) == native.MIOC_EINVAL          # nt = 0
    assert code(lambda: ctx.conv_setup(np.zeros(16385), np.zeros(16386), -1.0, 1.0)) == native.MIOC_EINVAL  # nt > 16384
    assert code(lambda: ctx.conv_setup(np.ones(4), np.ones(5), 1.0, 1.0)) == native.MIOC_EINVAL             # T1 <= T0
    kap = np.ones(4)
    kap[2] = math.nan
    assert code(lambda: ctx.conv_setup(kap, np.ones(5), -1.0, 1.0)) == native.MIOC_EINVAL                   # NaN in κ
    ctx.conv_shape = (1, 4)
    x = torch.zeros((1, 4, 1), dtype=torch.float64, device="cuda")
    assert code(lambda: ctx.conv_eval_tensors(x)) == native.MIOC_ESTATE                                     # no setup yet
    ctx.conv_setup(np.ones(4), np.ones(5), -1.0, 1.0)
    ctx.conv_eval_tensors(x, torch.empty(1, dtype=torch.float64, device="cuda"))
    ctx.synchronize()
    assert code(lambda: ctx.conv_setup(kap, np.ones(5), -1.0, 1.0)) == native.MIOC_EINVAL
    ctx.close()


def _trm_batch_vs_sequential(nt, K, par, seed):
    import torch

    import mioc
    from mioc import native
    from mioc.conv import ConvObj
    from mioc.iterators import LevelTable
    from mioc.trm_batch import TRM_batch
    cp = ConvProblem(nt=nt)
    ctx = native.Context(0)
    ctx.set_levels(LevelTable(cp.levels))
    x0 = torch.empty(K, nt, 1, dtype=torch.float64, device="cuda")
    ctx.rand_start_tensor(x0, seed=seed)
    ctx.synchronize()
    ctx.close()
    stats = {}
    vals, u, iters = TRM_batch(cp, par, x0=x0, stats=stats)
    ub = u.cpu().numpy()
    for k in range(K):
        obj = ConvObj(cp)
        J = mioc.TRM(obj, par, x0=x0[k].cpu().numpy().T.copy())
        assert J == vals[k], (k, J, vals[k])
        assert np.array_equal(obj.x, ub[k].T), k
        assert math.isfinite(J)
        obj.ctx.close()
    print(f"conv nt={nt}: iterations per restart {iters.tolist()}, values {vals.tolist()}")
    return ub, stats


def test_trm_batch_conv_equals_sequential_trm():
    """Multi-start TRM on the convolution example entirely on the device against the host TRM loop
    (multi-trust.jl:53-170 mirror) run restart by restart on ConvObj, whose eval_f! / eval_df! call the same kernels:
    identical values J + β·TV_p(u) and controls.  nt = 256: τ = 2/256, B = floor(0.125 / τ) = 16."""
    import mioc
    par = mioc.TRM_parameters(beta=1e-4, Delta0=0.125, p=1, maxiter=4, kmax=4)
    assert math.floor(par.Delta0 / ConvProblem(nt=256).tau) == 16
    _trm_batch_vs_sequential(256, 6, par, seed=5)


def test_trm_batch_conv_reference_config():
    """The reference's own run, main("convolution") (multi-trust.jl:190-192) at its default n = 1024: β = 1e-4,
    Δ⁰ = 0.125, p = 1, τ = 2/1024, B = 64, levels -2..2; maxiter capped.  Same equality; every control stays on the
    levels; the DP that served it is the fused small-state one."""
    import mioc
    from mioc import native
    par = mioc.TRM_parameters(beta=1e-4, Delta0=0.125, p=1, maxiter=3, kmax=4)
    assert math.floor(par.Delta0 / ConvProblem(nt=1024).tau) == 64
    ub, stats = _trm_batch_vs_sequential(1024, 4, par, seed=11)
    assert set(np.unique(ub)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert stats["algo"] == native.MIOC_ALGO_FUSED, stats
    assert stats["diagnostics"][3] == 0 and stats["diagnostics"][7] >= 1, stats   # no errors; resident fused workgroups
