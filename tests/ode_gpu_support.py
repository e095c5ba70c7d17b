"""What the GPU tests of ODE programs share (test_gpu_ode_program.py, _integrators.py, _implicit.py, _program_ad.py,
_bolza.py, test_gpu_mixed.py): random controls, one evaluation through prefilled device buffers, the host test double
whose eval_f! / eval_df! run a device program, and the comparison with a host mirror at the project's bar."""
import math

import numpy as np


def sos1(K, nt, seed):
    """Random admissible SOS1 controls (K, nt, 3): one control is 1 at every step."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.eye(3)[rng.integers(0, 3, size=(K, nt))])


def grid(K, nt, seed):
    """Random controls (K, nt, 2) on the product grid [[0,1,2],[0,1]] of the tests' problems."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([rng.integers(0, 3, size=(K, nt)), rng.integers(0, 2, size=(K, nt))],
                                         axis=2).astype(np.float64))


def run_eval(ctx, x, evalf, want_J=True, want_df=True, fill=math.nan):
    """evalf(dx, J, df) on the controls x (K, nt, nx): J (K,) and df (K, nt, nx) as numpy from device buffers prefilled
    with `fill` (None where not asked for)."""
    import torch
    dx = torch.tensor(x, dtype=torch.float64, device="cuda")
    J = torch.full((x.shape[0],), fill, dtype=torch.float64, device="cuda") if want_J else None
    df = torch.full_like(dx, fill) if want_df else None
    torch.cuda.synchronize()
    evalf(dx, J, df)
    ctx.synchronize()
    return (None if J is None else J.cpu().numpy()), (None if df is None else df.cpu().numpy())


def run_program(ctx, prog, x, T0, T1, state0, params, data=None, nu=None, want_J=True, want_df=True, want_Y=False,
                fill=math.nan):
    """One evaluation of the program: J (K,), df (K, nt, nx) and Y (K, nt + 1, ny) as numpy from device buffers
    prefilled with `fill` (None where not asked for).  data: the (nt, ndata) rows; nu: the mixed entry."""
    import torch
    K, nt, _ = x.shape
    dd = None if data is None else torch.tensor(data, dtype=torch.float64, device="cuda")
    Y = torch.full((K, nt + 1, prog.ny), fill, dtype=torch.float64, device="cuda") if want_Y else None

    def evalf(dx, J, df):
        if nu is None:
            ctx.ode_program_eval_tensors(prog, dx, T0, T1, state0, params, J, df, data=dd, Y=Y)
        else:
            ctx.ode_program_eval_mixed_tensors(prog, nu, dx, T0, T1, state0, params, J, df, data=dd, Y=Y)
    J, df = run_eval(ctx, x, evalf, want_J, want_df, fill)
    return J, df, (None if Y is None else Y.cpu().numpy())


def program_objective(host_obj, prog, ctx, state0, params, data=None, nu=None, sync_torch=False):
    """Test double: host_obj (the problem's host objective or shape) with eval_f! / eval_df! running the device program
    for one restart, so that the host TRM loops and the batch drivers see bit-identical objective values and
    gradients.  data: the device tensor of the data rows; nu None: the plain entry, nu >= 1: the mixed one;
    sync_torch: torch's streams are synchronised before each evaluation."""
    import torch
    obj = host_obj

    def ev(X, J, D):
        if sync_torch:
            torch.cuda.synchronize()
        if nu is None:
            ctx.ode_program_eval_tensors(prog, X, obj.T0, obj.T1, state0, params, J, D, data=data)
        else:
            ctx.ode_program_eval_mixed_tensors(prog, nu, X, obj.T0, obj.T1, state0, params, J, D, data=data)
        ctx.synchronize()

    def f_helper(x, cache):
        X = torch.tensor(np.ascontiguousarray(np.asarray(x).T[None]), dtype=torch.float64, device="cuda")
        J = torch.empty(1, dtype=torch.float64, device="cuda")
        ev(X, J, None)
        return J.item()

    def df_helper():
        X = torch.tensor(np.ascontiguousarray(obj.x.T[None]), dtype=torch.float64, device="cuda")
        D = torch.empty_like(X)
        ev(X, None, D)
        obj.df[:, :] = D[0].cpu().numpy().T

    obj.eval_f_helper = f_helper
    obj.eval_df_helper = df_helper
    return obj


def assert_at_bar(dev, ref, label=""):
    """The device's (J, df) or (J, df, Y) against the mirror's, per restart: 1e-12 relative for J, 1e-12 of the maximum
    for df and Y; every figure printed before it is held."""
    names = ("J", "df", "Y")[:len(ref)]
    (J, Jh), K = (dev[0], ref[0]), ref[0].shape[0]
    worst = [max(abs(J[k] - Jh[k]) / abs(Jh[k]) for k in range(K))]
    worst += [max(np.max(np.abs(a[k] - b[k])) / max(1e-300, np.max(np.abs(b[k]))) for k in range(K))
              for a, b in zip(dev[1:], ref[1:])]
    exact = sum(int(J[k] == Jh[k]) + sum(int(np.array_equal(a[k], b[k])) for a, b in zip(dev[1:], ref[1:]))
                for k in range(K))
    print(f"{label}: {exact} of {len(names) * K} {' / '.join(names)} arrays bit-identical to the mirror; worst relative "
          f"errors " + ", ".join(f"{n} {w:.3e}" for n, w in zip(names, worst)))
    assert all(np.all(np.isfinite(a)) for a in dev)
    for k in range(K):
        assert abs(J[k] - Jh[k]) <= 1e-12 * abs(Jh[k]), (label, k, J[k], Jh[k])
        for n, a, b in zip(names[1:], dev[1:], ref[1:]):
            assert np.max(np.abs(a[k] - b[k])) <= 1e-12 * max(1e-300, np.max(np.abs(b[k]))), (label, n, k)
    assert all(w <= 1e-12 for w in worst), (label, worst)
