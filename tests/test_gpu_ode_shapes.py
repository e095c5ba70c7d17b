"""GPU: k_ode_eval (mioc_ode_eval_device) on caller data -- generic parameter vectors, mixed one-hot and fractional
controls, the block's tail guard, nt = 1 and 2, single outputs, one context over several calls, and a restart whose
state leaves sqrt's domain -- against the plain restatement of tests/ode_cases.py, which test_ode_cases.py pins to
oracle/ode_oracle.py and measures against an extended-precision reference.

Bar: bit equality of J and of every df entry with the restatement, for all three problems.  Fishing and Van der Pol
use only +, - and * in a fixed order and the library is built with -ffp-contract=off, so that is derived.  doubletank
adds sqrt and 1.0 / x, both correctly rounded IEEE operations on the host and (no fast-math) on the device, so the same
is expected and asserted (and observed: on an MI355X every doubletank J and df row of every case is bit-identical);
every case also prints its distance to the reference beside the restatement's own.  NaNs are
compared by position.  Outputs are views between two sentinel rows that must stay untouched, as must an output that
was not asked for.
"""
import numpy as np
import pytest

import ode_cases as oc
from mioc import native

pytestmark = pytest.mark.gpu

PROB = {"fishing": native.MIOC_ODE_FISHING, "doubletank": native.MIOC_ODE_DOUBLETANK,
        "vanderpol": native.MIOC_ODE_VANDERPOL}
SENT = -1.2345678e300


def _run(ctx, c):
    """One call for a case: (J, df) as numpy arrays (None where not asked for), sentinels checked."""
    import torch
    par, X, T0, T1 = oc.inputs(c)
    K, nt = c.K, c.nt
    dx = torch.tensor(np.ascontiguousarray(X), dtype=torch.float64, device="cuda")
    jbuf = torch.full((K + 2,), SENT, dtype=torch.float64, device="cuda")
    dbuf = torch.full((K + 2, nt, 3), SENT, dtype=torch.float64, device="cuda")
    J = jbuf[1:K + 1] if c.out in ("both", "J") else None
    df = dbuf[1:K + 1] if c.out in ("both", "df") else None
    ctx.ode_eval_tensors(PROB[c.problem], dx, T0, T1, J, df, params=par)
    ctx.synchronize()
    assert np.array_equal(dx.cpu().numpy(), X), "the controls were written"
    jh, dh = jbuf.cpu().numpy(), dbuf.cpu().numpy()
    assert jh[0] == SENT and jh[-1] == SENT and np.all(dh[0] == SENT) and np.all(dh[-1] == SENT), c.id
    if J is None:
        assert np.all(jh == SENT), c.id
    if df is None:
        assert np.all(dh == SENT), c.id
    return (jh[1:K + 1] if J is not None else None), (dh[1:K + 1] if df is not None else None)


def _check(c, J, df):
    Jm, DFm, _ = oc.mirror(c)
    par, X, T0, T1 = oc.inputs(c)
    Jr, DFr, _ = oc.eval_reference(c.problem, par, X, T0, T1)
    keep = np.ones(c.K, dtype=bool)
    if c.params == "nan":
        keep[oc.NAN_RESTART] = False
    if J is not None and df is not None:
        same = sum(int(np.array_equal(J[k], Jm[k], equal_nan=True)) + int(np.array_equal(df[k], DFm[k], equal_nan=True))
                   for k in range(c.K))
        print(f"{c.id}: {same} of {2 * c.K} J / df rows bit-identical; distance to the reference: device "
              f"{oc.distance(J[keep], df[keep], Jr[keep], DFr[keep]):.3e}, restatement "
              f"{oc.distance(Jm[keep], DFm[keep], Jr[keep], DFr[keep]):.3e}")
    if J is not None:
        assert np.array_equal(J, Jm, equal_nan=True), (c.id, np.flatnonzero(~((J == Jm) | (np.isnan(J) & np.isnan(Jm)))))
    if df is not None:
        bad = ~((df == DFm) | (np.isnan(df) & np.isnan(DFm)))
        assert not bad.any(), (c.id, np.argwhere(bad)[:5])


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.id)
def test_ode_eval_case(case):
    ctx = native.Context(0)
    J, df = _run(ctx, case)
    _check(case, J, df)
    ctx.close()


def test_nan_restart_and_its_neighbours():
    """doubletank from y0 = (0.01, 2): the restart without inflow runs its first tank dry, sqrt sees a negative state,
    and its J and whole df row are NaN; the other restarts of the wave are finite and as the restatement has them."""
    c = oc.case("doubletank_nan_nt130_K5")
    ctx = native.Context(0)
    J, df = _run(ctx, c)
    ctx.close()
    k = oc.NAN_RESTART
    assert np.isnan(J[k]) and np.isnan(df[k]).all()
    others = [q for q in range(c.K) if q != k]
    assert np.isfinite(J[others]).all() and np.isfinite(df[others]).all()
    Jm, DFm, _ = oc.mirror(c)
    assert np.array_equal(J[others], Jm[others]) and np.array_equal(df[others], DFm[others])


def test_one_context_serves_growing_and_shrinking_calls():
    """One context: a call, a larger one (the state scratch grows), a smaller one (the scratch is reused, with the
    larger call's states still in it), then the other two problems."""
    ctx = native.Context(0)
    for cid in oc.CONTEXT_SEQUENCE:
        c = oc.case(cid)
        J, df = _run(ctx, c)
        _check(c, J, df)
    ctx.close()
