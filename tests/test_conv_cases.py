"""The cases of test_gpu_conv_shapes.py on the CPU (tests/conv_cases.py): the float64 references are good enough to
judge the device on them, every case is sharp for every wrong version of the list, and the stand-in ConvProblem
with conv_ref.controls is not.

Measured (x86, np.longdouble eps 1.08e-19; CENSUS below is filled in by these tests and printed with -s):
  the dense float64 restatement against np.longdouble over the probed restarts of every shape with nt <= 1100:
    at most 4.7e-16 relative in J and 1.2e-15 in df (bound 1e-12: three orders above, three below the device's 1e-9);
  the convolution form against the dense restatement, both float64, same shapes: 3.9e-16 in J, 1.1e-15 in df;
  the convolution form in float64 against itself in np.longdouble on two restarts of every SHAPES_BIG_LDS case:
    7.6e-17 in J, 2.2e-15 in df;
  smallest move of any applicable wrong version on any probed restart of any dense shape: 1.4e-4 ("M last diagonal
    2/3 tau" at nt = 31; then "w[nt] dropped from the adjoint" 3.7e-4 at nt = 145, "K last column dropped" 5.4e-4 at
    nt = 240, "M first diagonal 2/3 tau", which only J sees, 7.5e-4 at nt = 1025; bound 1e-6, 1000 times the device
    bar);
  on ConvProblem data with conv_ref.controls, nt in {1, 2, 15, 16, 17, 31, 33, 63, 65}: "tau = 2/nt" moves nothing
    (0.0) at every shape; "K diagonal included" and "fvec shifted by one" move nothing at nt = 1, "x permuted in
    fours" nothing at nt = 15; generic data of the same shapes moves every version by 2.5e-4 or more.
"""
import math

import numpy as np
import pytest

import conv_cases as cc
from conv_ref import controls

from mioc.conv import ConvProblem

CENSUS = {}


def _ids(shapes):
    return [s.id for s in shapes]


def test_generic_data_has_no_structure_of_the_standin():
    for s in (cc.Shape(1, 3), cc.Shape(17, 33), cc.Shape(257, 40)):
        c, X = s.case, s.X
        nt = s.nt
        assert c.kappa.shape == (nt,) and c.fvec.shape == (nt + 1,) and X.shape == (s.K, nt)
        assert (c.T0, c.T1) == (0.25, 1.0) and c.T1 - c.T0 != 2.0 and c.T0 != -c.T1
        assert 0.5 / math.sqrt(nt) <= abs(c.kappa[0]) <= 1.5 / math.sqrt(nt) and 1.0 <= abs(c.fvec[0]) <= 2.0
        on = X == np.round(X)
        assert not on[:, 0].any() and np.all(X[:, -1] != 0.0) and np.all(np.abs(X) <= 2.45)
        if nt >= 17:
            assert 0.3 < on.mean() < 0.7 and np.all(on.any(axis=1)) and np.all((~on).any(axis=1))
        if nt >= 257:
            assert 0.1 < np.mean(c.kappa == 0.0) < 0.3
            assert 0.3 < np.mean((X == 0.0)[on]) / 0.2 < 1.7     # the level 0 itself is among the integral entries
        assert len({x.tobytes() for x in X}) == s.K
        c2, X2 = cc.generic(nt, s.K, s.seed)                      # one seed, one case
        assert np.array_equal(c2.kappa, c.kappa) and np.array_equal(c2.fvec, c.fvec) and np.array_equal(X2, X)
        with pytest.raises(ValueError):
            X[0, 0] = 0.0                                         # shared read-only


def test_toeplitz_loop_against_the_standins_matrix():
    """The double loop fed with ConvProblem's κ is conv_ref's K, and the two shifted variants are shifts of it."""
    from conv_ref import ConvRef
    for nt in (1, 2, 7, 33):
        ref, cp = ConvRef(nt), ConvProblem(nt=nt)
        K = cc.toeplitz(cp.kappa, np.float64)
        assert np.array_equal(K, ref.K)
        assert np.array_equal(cc.Mmat(nt, cp.tau, np.float64), ref.M)
        K0, K2 = cc.toeplitz(cp.kappa, np.float64, 0), cc.toeplitz(cp.kappa, np.float64, 2)
        assert np.array_equal(K0[:-1], K[1:]) and np.array_equal(K0[-1, 1:], K[-1, :-1]) and K0[-1, 0] == 0.0
        assert np.array_equal(K2[1:], K[:-1]) and np.all(K2[0] == 0.0)


def test_shape_lists():
    nts = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 239, 240, 241, 255, 256, 257, 1025]
    assert sorted({s.nt for s in cc.SHAPES_ONE_TILE}) == nts
    assert {s.K for s in cc.SHAPES_ONE_TILE} == {1, 2, 15, 16, 17, 31, 33}
    for nt in nts:  # every nt meets an exact and a padded restart tile
        Ks = [s.K for s in cc.SHAPES_ONE_TILE if s.nt == nt]
        assert any(K % 16 == 0 for K in Ks) and any(K % 16 != 0 for K in Ks), nt
    assert {nt + 16 for nt in nts} >= {255, 256, 257} and {63, 65} <= set(nts)
    assert [s.nt for s in cc.SHAPES_TWO_TILES] == [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 127, 128, 129, 145, 255, 257]
    assert cc.Shape(1, 16369) in cc.SHAPES_TWO_TILES and cc.Shape(257, 1809) in cc.SHAPES_TWO_TILES
    assert max(s.nt * s.K for s in cc.SHAPES_TWO_TILES) < 2 ** 19 + 2 ** 12
    assert cc.SHAPES_BIG_LDS == [(8176, 1), (8177, 1), (8161, 513), (16384, 1), (16384, 17)]
    ids = _ids(cc.DENSE_SHAPES + cc.SHAPES_BIG_LDS)
    assert len(set(ids)) == len(ids)
    assert all(s.nt <= cc.DENSE_MAX_NT for s in cc.DENSE_SHAPES)


def test_every_shape_is_on_its_side_of_the_selection_rule():
    """The rule restated in Python (the GPU tests ask the library): one tile per wave on SHAPES_ONE_TILE and on the 33
    restarts test_gpu_conv_shapes.py cuts out of a large batch, two on SHAPES_TWO_TILES, which one restart tile
    less would not select, with a last restart tile of one restart; SHAPES_BIG_LDS has both, the first shapes on
    either side of 64 KB of dynamic LDS for each, and the largest nt."""
    for s in cc.SHAPES_ONE_TILE:
        assert cc.tiles_per_wave(*s) == 1, s
    for s in cc.SHAPES_TWO_TILES:
        assert cc.tiles_per_wave(*s) == 2 and cc.tiles_per_wave(s.nt, s.K - 1) == 1 and s.K % 16 == 1, s
        assert cc.tiles_per_wave(s.nt, 33) == 1, s
    # with CNS tiles per wave a workgroup spans 64·CNS columns: grp > 0 needs nt + 1 (forward) or nt (adjoint) beyond
    assert sum(s.nt > 128 for s in cc.SHAPES_TWO_TILES) >= 4 and any(s.nt == 128 for s in cc.SHAPES_TWO_TILES)
    got = {s.id: (cc.tiles_per_wave(*s), cc.lds_bytes(*s)) for s in cc.SHAPES_BIG_LDS}
    assert got == {"nt8176_K1": (1, 65536), "nt8177_K1": (1, 65544), "nt8161_K513": (2, 65544),
                   "nt16384_K1": (1, 131200), "nt16384_K17": (2, 131328)}, got
    assert cc.tiles_per_wave(16384, 16) == 1 and cc.lds_bytes(8160, 513) == 65536


def _note(key, eJ, ed):
    w = CENSUS.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], float(np.max(eJ))), max(w[1], float(np.max(ed)))


@pytest.mark.parametrize("shape", cc.DENSE_SHAPES, ids=_ids(cc.DENSE_SHAPES))
def test_float64_references_against_extended_precision(shape):
    """On the probed restarts of the shape: the dense float64 restatement within 1e-12 of np.longdouble in J
    (relative) and df (max-norm relative), and the convolution form within 1e-12 of the dense one."""
    X = shape.X[shape.rows()]
    Jl, dl = cc.dense_ref(shape.case, X, cc.LD)
    assert Jl.dtype == cc.LD and dl.dtype == cc.LD and np.finfo(cc.LD).eps < 1e-18
    J, d = cc.dense_ref(shape.case, X, np.float64)
    Jc, dc = cc.conv_form(shape.case, X, np.float64, block=48)   # several blocks at these sizes, as at the large ones
    a, b = cc.rel(J, d, Jl, dl), cc.rel(Jc, dc, J, d)
    print(f"{shape.id}: dense f64 vs longdouble J {a[0].max():.2e} df {a[1].max():.2e}; "
          f"convolution form vs dense J {b[0].max():.2e} df {b[1].max():.2e}")
    _note("dense f64 vs longdouble", *a)
    _note("convolution form vs dense", *b)
    assert a[0].max() <= 1e-12 and a[1].max() <= 1e-12, a
    assert b[0].max() <= 1e-12 and b[1].max() <= 1e-12, b


@pytest.mark.parametrize("shape", cc.SHAPES_BIG_LDS, ids=_ids(cc.SHAPES_BIG_LDS))
def test_convolution_form_against_extended_precision_large(shape):
    """The reference of the large shapes, float64, within 1e-12 of the same sums in np.longdouble on the first and
    the last restart (K = 1: on the case's own control and on one more of the same kind)."""
    X = shape.X[[0, -1]] if shape.K > 1 else np.concatenate([shape.X, cc.generic(shape.nt, 1, shape.seed + 1)[1]])
    assert X.shape == (2, shape.nt) and not np.array_equal(X[0], X[1])
    J, d = cc.conv_form(shape.case, X, np.float64)
    Jl, dl = cc.conv_form(shape.case, X, cc.LD)
    eJ, ed = cc.rel(J, d, Jl, dl)
    print(f"{shape.id}: convolution form f64 vs longdouble J {eJ.max():.2e} df {ed.max():.2e}")
    _note("convolution form f64 vs longdouble, large", eJ, ed)
    assert Jl.dtype == cc.LD and eJ.max() <= 1e-12 and ed.max() <= 1e-12, (eJ, ed)


def _moved(case, X, wrong, true):
    """Per restart: max(|ΔJ| / |J|, max|Δdf| / max|df|) of a wrong version."""
    return np.maximum(*cc.rel(*cc.dense_ref(case, X, cc.LD, wrong), *true))


@pytest.mark.parametrize("shape", cc.DENSE_SHAPES, ids=_ids(cc.DENSE_SHAPES))
def test_every_case_is_sharp_for_every_wrong_version(shape):
    """Each wrong version that can differ at this nt does differ from the true one by at least 1e-6 in J (relative) or
    in df (max-norm relative), 1000 times the device bar, on every probed restart of the case."""
    X = shape.X[shape.rows(6)]
    true = cc.dense_ref(shape.case, X, cc.LD)
    for name, (applies, _) in cc.WRONG.items():
        if not applies(shape.nt):
            continue
        m = _moved(shape.case, X, name, true)
        print(f"{shape.id} {name}: {m.min():.2e}")
        CENSUS.setdefault("smallest move", {})
        CENSUS["smallest move"][name] = min(CENSUS["smallest move"].get(name, (math.inf, "")), (float(m.min()), shape.id))
        assert m.min() >= 1e-6, (name, m)


def test_every_wrong_version_applies_somewhere():
    assert len(cc.WRONG_NAMES) == 13
    for name, (applies, what) in cc.WRONG.items():
        assert sum(bool(applies(s.nt)) for s in cc.DENSE_SHAPES) >= len(cc.DENSE_SHAPES) - 3 and what, name


def test_standin_is_blind():
    """Why ConvProblem with conv_ref.controls was not enough: with T1 − T0 = 2, τ = 2/nt is τ, at every shape (it
    moves J and df by no more than 1e-13 relative); and at some of the shapes of the census other versions move
    nothing either (a piecewise-constant integral control that ends in 0, or is constant over its first groups of
    four).  On generic data the same shapes see every applicable version (1e-6 or more)."""
    nts = (1, 2, 15, 16, 17, 31, 33, 63, 65)
    lo = {n: (math.inf, None) for n in cc.WRONG_NAMES}
    hi = {n: 0.0 for n in cc.WRONG_NAMES}
    lo_gen = {n: math.inf for n in cc.WRONG_NAMES}
    for nt in nts:
        cp = ConvProblem(nt=nt)
        case = cc.ConvCase(cp.kappa, cp.fvec, cp.T0, cp.T1)
        X = np.concatenate(controls(nt, 4, seed=nt))
        gen = cc.Shape(nt, 4)
        for case_, X_, generic in ((case, X, False), (gen.case, gen.X, True)):
            true = cc.dense_ref(case_, X_, cc.LD)
            for name, (applies, _) in cc.WRONG.items():
                if not applies(nt):
                    continue
                m = _moved(case_, X_, name, true)
                if generic:
                    lo_gen[name] = min(lo_gen[name], float(m.min()))
                else:
                    lo[name] = min(lo[name], (float(m.min()), nt))
                    hi[name] = max(hi[name], float(m.max()))
    for name in cc.WRONG_NAMES:
        print(f"stand-in {name}: smallest move {lo[name][0]:.2e} (nt = {lo[name][1]}), largest {hi[name]:.2e}; "
              f"generic data, smallest {lo_gen[name]:.2e}")
    CENSUS["stand-in"] = {n: (lo[n], hi[n]) for n in cc.WRONG_NAMES}
    for name in cc.STANDIN_BLIND:
        assert hi[name] <= 1e-13, (name, hi[name])
    blind_somewhere = sorted(n for n in cc.WRONG_NAMES if lo[n][0] <= 1e-13)
    assert blind_somewhere == sorted(cc.STANDIN_BLIND + cc.STANDIN_BLIND_SOMEWHERE), blind_somewhere
    assert all(v >= 1e-6 for v in lo_gen.values()), lo_gen


def test_zz_census():
    """Prints what the tests above measured (run the module with -s)."""
    for key, val in CENSUS.items():
        print(f"conv census: {key}: {val}")
