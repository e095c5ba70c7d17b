"""GPU: k_rand_start (mioc_rand_start_device) at the sizes its bitmap, its per-thread word ranges and Floyd's sampling
turn on, against the host restatement of the stream (tests/ode_cases.py: rand_start_host; test_ode_cases.py checks the
restatement's own properties).  Every restart of every case must equal the restatement bit for bit, and a sentinel row
behind the output must be intact.

  nt      1, 2 (no or one candidate), 31 / 32 / 33 and 63 / 64 / 65 (a bitmap word partly beyond nt), 8191 / 8192 / 8193
          (from one to two words per thread) and 8225 (257 words and one step)
  jumps   the default floor(nt / 10), 0, 1 and nt - 1 (every candidate: Floyd's collision branch on nearly every draw, a
          new segment at every step)
  levels  L = 1; L = 3 with M = 1; a 3 x 5 product (L = 15, no power of two); M = 8 (the kernels' limit), L = 256
  seeds   0, 2^64 - 1 and one in between
  LDS     the entry rejects, before any launch, an nt whose bitmap a launch cannot be given (nt > 516096: more than
          64 KB); the largest admitted nt runs and equals the restatement.
"""
import numpy as np
import pytest

import ode_cases as oc
from mioc import native
from mioc.iterators import LevelTable, product_iterator

pytestmark = pytest.mark.gpu

SENT = -1.2345678e300


def _table(name):
    nu = oc.RS_TABLES[name]
    return LevelTable(nu, product_iterator(nu))


def _compare(ctx, lt, K, nt, jumps, seed):
    import torch
    buf = torch.full((K + 1, nt, lt.M), SENT, dtype=torch.float64, device="cuda")
    ctx.rand_start_tensor(buf[:K], seed=seed, jumps=jumps)
    ctx.synchronize()
    u = buf.cpu().numpy()
    assert np.all(u[K] == SENT), (nt, jumps, "sentinel row")
    jv = nt // 10 if jumps < 0 else jumps
    for k in range(K):
        hu, S = oc.rand_start_host(lt, nt, jv, seed, k)
        assert len(S) == jv
        assert np.array_equal(u[k].T, hu), (nt, jumps, seed, k)


@pytest.mark.parametrize("nt", oc.RS_NT)
def test_rand_start_nt_and_jumps(nt):
    lt = _table("L15_3x5")
    ctx = native.Context(0)
    ctx.set_levels(lt)
    for jumps in oc.rs_jumps(nt):
        _compare(ctx, lt, 3, nt, jumps, oc.RS_SEEDS[2])
    with pytest.raises(native.MiocNativeError):
        _compare(ctx, lt, 3, nt, nt, oc.RS_SEEDS[2])
    ctx.close()


@pytest.mark.parametrize("seed", oc.RS_SEEDS, ids=["seed0", "seedmax", "seedmid"])
@pytest.mark.parametrize("table", list(oc.RS_TABLES))
def test_rand_start_tables_and_seeds(table, seed):
    lt = _table(table)
    ctx = native.Context(0)
    ctx.set_levels(lt)
    for nt in (2, 33, 8225):
        for jumps in (-1, nt - 1):
            _compare(ctx, lt, 3, nt, jumps, seed)
    ctx.close()


def test_rand_start_lds_bound():
    """nt = 516097 needs 65540 bytes of LDS: MIOC_EINVAL from the entry, nothing launched, the output untouched.
    nt = 516096 (exactly 64 KB) runs: K = 1, M = 1, two levels."""
    import torch
    lt = LevelTable([[0, 1]], product_iterator([[0, 1]]))
    ctx = native.Context(0)
    ctx.set_levels(lt)
    big = torch.full((1, oc.RS_MAX_NT + 1, 1), SENT, dtype=torch.float64, device="cuda")
    with pytest.raises(native.MiocNativeError) as e:
        ctx.rand_start_tensor(big, seed=5)
    assert e.value.code == native.MIOC_EINVAL
    ctx.synchronize()
    assert bool((big == SENT).all())
    del big
    _compare(ctx, lt, 1, oc.RS_MAX_NT, -1, 5)
    ctx.close()
