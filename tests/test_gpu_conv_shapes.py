"""mioc_conv.hip on generic caller data, with one and with two column tiles per wave and with more than 64 KB of
dynamic LDS: mioc_conv_eval_device against the restatements of tests/conv_cases.py.

The data has none of the stand-in's structure -- T1 − T0 = 0.75, κ random with exact zeros, fvec random, half of every
control off the levels -- so τ = 2/nt, a shifted diagonal, a dropped row or column of K, a wrong end of M and a permuted
operand each move J or df by 1.3e-4 or more (tests/test_conv_cases.py), against a bar of 1e-9.  Which variant of
k_conv_mm a case runs is asked of the library (mioc_conv_tiles_per_wave), not restated.  SHAPES_TWO_TILES reaches
the two-tile variant at the smallest batch that selects it, at nt on both sides of the 16-, 32- and 128-column edges
(column groups grp > 0 from nt = 128 on); SHAPES_BIG_LDS launches κ in 65536 and 65544 bytes of LDS with either
variant and in the 131200 / 131328 bytes of the documented maximum nt = 16384.

Outputs are slices of a larger buffer with a sentinel on both sides and NaN inside: a store past either end, or an
element never written, fails.

Bar: the project's own for a floating-point producer (tests/test_gpu_conv.py): |J − J_ref| <= 1e-9·|J_ref| and
max|df − df_ref| <= 1e-9·max|df_ref| per restart.  The float64 references are within 1.2e-15 (dense) and 2.2e-15
(convolution form, large shapes) of np.longdouble (tests/test_conv_cases.py).  Largest device error observed against
them (J, df): SHAPES_ONE_TILE 5.1e-16, 1.4e-15; SHAPES_TWO_TILES 7.2e-16, 1.8e-15; SHAPES_BIG_LDS 2.6e-16, 4.6e-15 --
five orders under the bar (each test prints its own with -s).
"""
import ctypes
import functools

import numpy as np
import pytest

import conv_cases as cc

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 37, -7.25
WORST = {}


def _ids(shapes):
    return [s.id for s in shapes]


@functools.lru_cache(maxsize=None)
def _ref(shape):
    """(J (K,), df (K, nt)) of a shape in float64, computed once: the dense restatement up to nt = 1100, the
    convolution form above."""
    f = cc.dense_ref if shape.nt <= cc.DENSE_MAX_NT else cc.conv_form
    J, df = f(shape.case, shape.X, np.float64)
    J.setflags(write=False)
    df.setflags(write=False)
    return J, df


class _Out:
    """n doubles inside a buffer of GUARD + n + GUARD: SENTINEL on both sides, NaN inside."""

    def __init__(self, n):
        import torch
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(float("nan"))

    def get(self):
        """The inside as numpy, after the checks: both guards intact, every element written with a finite number."""
        b = self.buf.cpu().numpy()
        assert np.all(b[:GUARD] == SENTINEL) and np.all(b[GUARD + self.n:] == SENTINEL), "a store outside the output"
        inside = b[GUARD:GUARD + self.n]
        assert np.all(np.isfinite(inside)), f"{int(np.sum(~np.isfinite(inside)))} elements not written"
        return inside

    def untouched(self):
        b = self.buf.cpu().numpy()
        return np.all(b[:GUARD] == SENTINEL) and np.all(b[GUARD + self.n:] == SENTINEL) and \
            np.all(np.isnan(b[GUARD:GUARD + self.n]))


def _eval(ctx, X, want_J=True, want_df=True):
    """One mioc_conv_eval_device call on controls X (K, nt) -> (J (K,) or None, df (K, nt) or None)."""
    import torch
    K, nt = X.shape
    dx = torch.tensor(np.ascontiguousarray(X), dtype=torch.float64, device="cuda").view(K, nt, 1)
    J, df = (_Out(K) if want_J else None), (_Out(K * nt) if want_df else None)
    ctx.conv_eval_tensors(dx, J.t if want_J else None, df.t.view(K, nt, 1) if want_df else None)
    ctx.synchronize()
    return (J.get() if want_J else None), (df.get().reshape(K, nt) if want_df else None)


def _setup(ctx, case):
    ctx.conv_setup(case.kappa, case.fvec, case.T0, case.T1)


def _fresh_eval(case, X, **kw):
    from mioc import native
    ctx = native.Context(0)
    _setup(ctx, case)
    out = _eval(ctx, X, **kw)
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def _fresh(shape):
    """J and df of a shape from a context that has seen nothing else."""
    return _fresh_eval(shape.case, shape.X)


@functools.lru_cache(maxsize=None)
def _variant(nt, K):
    """What the library says it runs for K restarts at nt: 1 or 2 column tiles per wave."""
    from mioc import native
    with native.Context(0) as ctx:
        return ctx.conv_tiles_per_wave(nt, K)


def _against_ref(shape, key):
    J, df = _fresh(shape)
    Jo, dfo = _ref(shape)
    eJ, ed = cc.rel(J, df, Jo, dfo)
    w = WORST.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], eJ.max()), max(w[1], ed.max())
    print(f"device vs reference {shape.id} ({_variant(*shape)} tiles per wave): J {eJ.max():.2e} df {ed.max():.2e}; "
          f"largest of {key} so far: J {w[0]:.2e} df {w[1]:.2e}")
    assert np.all(eJ <= 1e-9), (int(np.argmax(~(eJ <= 1e-9))), eJ.max())
    assert np.all(ed <= 1e-9), (int(np.argmax(~(ed <= 1e-9))), ed.max())


@pytest.mark.parametrize("shape", cc.SHAPES_ONE_TILE, ids=_ids(cc.SHAPES_ONE_TILE))
def test_conv_one_tile_per_wave_vs_restatement(shape):
    """Every nt at an edge of the 16-column tile, the 64-column workgroup and k_conv_J's 256-thread stride, with one
    exact and one padded restart tile."""
    assert _variant(*shape) == 1
    _against_ref(shape, "SHAPES_ONE_TILE")


@pytest.mark.parametrize("shape", cc.SHAPES_TWO_TILES, ids=_ids(cc.SHAPES_TWO_TILES))
def test_conv_two_tiles_per_wave_vs_restatement(shape):
    assert _variant(*shape) == 2 and _variant(shape.nt, shape.K - 1) == 1
    _against_ref(shape, "SHAPES_TWO_TILES")


@pytest.mark.parametrize("shape", cc.SHAPES_TWO_TILES, ids=_ids(cc.SHAPES_TWO_TILES))
def test_conv_variants_agree_bit_for_bit(shape):
    """The first 33 controls of the large batch, evaluated as a batch of 33 with one tile per wave, have the J and df
    bits of their rows in the large batch with two: a restart's result depends neither on K nor on its position."""
    assert _variant(shape.nt, 33) == 1 and _variant(*shape) == 2
    J, df = _fresh(shape)
    J33, df33 = _fresh_eval(shape.case, shape.X[:33])
    assert np.array_equal(J33, J[:33]) and np.array_equal(df33, df[:33])


@pytest.mark.parametrize("shape", cc.SHAPES_BIG_LDS, ids=_ids(cc.SHAPES_BIG_LDS))
def test_conv_big_lds_vs_convolution_form(shape):
    """κ in 64 KB of dynamic LDS and one double more, with either variant, and at the documented maximum."""
    assert _variant(*shape) == cc.tiles_per_wave(*shape)
    _against_ref(shape, "SHAPES_BIG_LDS")


def test_conv_big_lds_has_both_variants_at_the_maximum():
    got = {s.id: (_variant(*s), cc.lds_bytes(*s) > 65536) for s in cc.SHAPES_BIG_LDS}
    assert got == {"nt8176_K1": (1, False), "nt8177_K1": (1, True), "nt8161_K513": (2, True),
                   "nt16384_K1": (1, True), "nt16384_K17": (2, True)}, got


ONE = next(s for s in cc.SHAPES_ONE_TILE if s.nt == 65 and s.K % 16)   # two column workgroups, a padded restart tile
TWO = next(s for s in cc.SHAPES_TWO_TILES if s.nt == 129)               # two column groups of two-tile waves


@pytest.mark.parametrize("shape", [ONE, TWO], ids=_ids([ONE, TWO]))
def test_conv_single_outputs_equal_both(shape):
    """J alone (d_df null: the call stops after k_conv_J, no w rows) and df alone (d_J null) are the bits of the call
    with both, and the output that is not asked for -- the one the same context wrote in the joint call before,
    NaN-filled again -- stays NaN."""
    import torch
    from mioc import native
    assert shape in cc.DENSE_SHAPES and _variant(*shape) == (1 if shape is ONE else 2)
    J, df = _fresh(shape)
    K, nt = shape.K, shape.nt
    ctx = native.Context(0)
    _setup(ctx, shape.case)
    dx = torch.tensor(np.ascontiguousarray(shape.X), dtype=torch.float64, device="cuda").view(K, nt, 1)
    oJ, odf = _Out(K), _Out(K * nt)
    for want_J, want_df in ((True, True), (True, False), (False, True)):
        oJ.t.fill_(float("nan"))
        odf.t.fill_(float("nan"))
        ctx.conv_eval_tensors(dx, oJ.t if want_J else None, odf.t.view(K, nt, 1) if want_df else None)
        ctx.synchronize()
        assert np.array_equal(oJ.get(), J) if want_J else oJ.untouched(), (want_J, want_df)
        assert np.array_equal(odf.get().reshape(K, nt), df) if want_df else odf.untouched(), (want_J, want_df)
    ctx.close()


def test_conv_host_entry_with_one_output():
    """mioc_conv_eval with J = NULL and with df = NULL equals the device entry; with both NULL it is MIOC_EINVAL."""
    from mioc import native
    shape = ONE
    J, df = _fresh(shape)
    K, nt = shape.K, shape.nt
    ctx = native.Context(0)
    _setup(ctx, shape.case)
    x = np.ascontiguousarray(shape.X)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    Jh, dfh = np.full(K, np.nan), np.full((K, nt), np.nan)
    assert ctx.lib.mioc_conv_eval(ctx.h, K, p(x), None, p(dfh)) == native.MIOC_OK
    assert np.array_equal(dfh, df)
    assert ctx.lib.mioc_conv_eval(ctx.h, K, p(x), p(Jh), None) == native.MIOC_OK
    assert np.array_equal(Jh, J)
    assert ctx.lib.mioc_conv_eval(ctx.h, K, p(x), None, None) == native.MIOC_EINVAL
    Jh2, dfh2 = ctx.conv_eval(shape.X[:, None, :])
    assert np.array_equal(Jh2, J) and np.array_equal(dfh2[:, 0, :], df)
    ctx.close()


def test_conv_one_context_several_problems():
    """Problems and batch sizes in a row on one context, each the fresh context's bits: the v / w scratch is kept
    and its split point V + K·(nt+1) moves with K and nt, the w rows (stride nt + 16) rely on zeros behind r = nt
    that every gradient call must write itself, and κ / fvec shrink and grow."""
    from mioc import native
    big = cc.Shape(257, 1809)
    assert _variant(*big) == 2
    steps = [(cc.Shape(100, 40), None, "both"), (cc.Shape(17, 3), None, "J"), (cc.Shape(17, 3), None, "df"),
             (cc.Shape(257, 1), None, "both"), (cc.Shape(100, 40), None, "both"),
             (big, None, "both"), (big, slice(5, 6), "both"), (cc.Shape(257, 1), None, "both")]
    ctx = native.Context(0)
    for shape, rows, what in steps:
        X = shape.X if rows is None else shape.X[rows]
        kw = dict(want_J=what != "df", want_df=what != "J")
        _setup(ctx, shape.case)
        J, df = _eval(ctx, X, **kw)
        Jf, dff = _fresh_eval(shape.case, X, **kw)
        for a, b in ((J, Jf), (df, dff)):
            assert (a is None and b is None) or np.array_equal(a, b), (shape.id, rows, what)
    ctx.close()


def test_conv_failed_setup_keeps_the_last_problem():
    """A setup that fails validation returns MIOC_EINVAL and leaves the last good problem in force (mioc.h): the
    next evaluation repeats its bits."""
    from mioc import native
    shape = ONE
    J, df = _fresh(shape)
    c, nt = shape.case, shape.nt
    nan_k, nan_f = c.kappa.copy(), c.fvec.copy()
    nan_k[nt // 2] = np.nan
    nan_f[nt] = np.nan
    bad = [c._replace(kappa=nan_k), c._replace(fvec=nan_f), c._replace(T1=c.T0), c._replace(T1=c.T0 - 1.0),
           cc.ConvCase(np.ones(16385), np.ones(16386), c.T0, c.T1)]
    ctx = native.Context(0)
    _setup(ctx, c)
    for b in bad:
        with pytest.raises(native.MiocNativeError) as e:
            _setup(ctx, b)
        assert e.value.code == native.MIOC_EINVAL
        J2, df2 = _eval(ctx, shape.X)
        assert np.array_equal(J2, J) and np.array_equal(df2, df)
    ctx.close()
