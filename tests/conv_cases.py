"""TEST INFRASTRUCTURE -- generic caller data for the convolution objective, its restatement in extended precision,
named wrong versions of it, and the shapes of tests/test_gpu_conv_shapes.py.

mioc_conv_setup (include/mioc.h) takes a caller's κ, fvec, T0 and T1 for any nt from 1 to 16384; the stand-in
mioc.conv.ConvProblem only ever supplies T1 − T0 = 2, a smooth κ without zeros and a cosine fvec, and
conv_ref.controls are integral and piecewise constant.  The builders here break each of those structures, so that
τ = 2/nt, a shifted diagonal, a dropped row or column of K, a wrong end of M or a permuted operand moves J or df
(tests/test_conv_cases.py measures by how much).

  generic(nt, K, seed)          κ, fvec, T0, T1 and K controls (K, nt), every array from one seeded rng
  dense_ref(case, X, dtype, wrong)   julia_opt/example_convolution.jl:73-141 with its dense loops, K from the
                                caller's κ by toeplitz's double loop (:110-122), vectorised over the batch: one
                                X @ Kᵀ per call; np.longdouble (eps 1.08e-19 on x86) or float64; for nt <= 1100
  conv_form(case, X, dtype)     the same function without the matrix, for the large shapes: v = [0, (κ * x)[:nt]] − fvec,
                                the tridiagonal product elementwise, df by correlation with κ
  WRONG                         named wrong versions of dense_ref, one per mistake the kernel could make
  SHAPES_ONE_TILE / SHAPES_TWO_TILES / SHAPES_BIG_LDS   (nt, K) per variant of the product kernel
"""
from __future__ import annotations

import collections
import functools

import numpy as np

LD = np.longdouble
DENSE_MAX_NT = 1100

ConvCase = collections.namedtuple("ConvCase", "kappa fvec T0 T1")
T0, T1 = 0.25, 1.0  # not symmetric, T1 − T0 = 0.75: τ = 2/nt is wrong by a factor 8/3


def generic(nt, K, seed):
    """(ConvCase, X (K, nt)).

    κ: normal / √nt (v = K·x − fvec stays of order one at every nt, so that single entries of M and fvec remain
    visible in J) with a fifth of its entries exactly 0.0; κ[0], the first subdiagonal and the only entry of K's
    last column, is ±[0.5, 1.5] / √nt.  fvec: normal, fvec[0] = ±[1, 2] (v[0] = −fvec[0] is all that M's first
    diagonal entry and row 0 of the adjoint see).  Controls: levels −2..2, then about half of each control's
    entries moved off them by ±[0.05, 0.45]; entry 0 always is (never 0.0, and different from every other entry of
    its group of four), the last entry is never 0.0 (K's last column multiplies it alone)."""
    rng = np.random.default_rng(seed)
    s = 1.0 / np.sqrt(nt)
    kappa = rng.standard_normal(nt) * s
    kappa[rng.uniform(size=nt) < 0.2] = 0.0
    kappa[0] = rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 1.5) * s
    fvec = rng.standard_normal(nt + 1)
    fvec[0] = rng.choice([-1.0, 1.0]) * rng.uniform(1.0, 2.0)
    X = rng.integers(-2, 3, size=(K, nt)).astype(np.float64)
    off = rng.uniform(size=(K, nt)) < 0.5
    off[:, 0] = True
    off[:, -1] |= X[:, -1] == 0.0
    X += off * rng.choice([-1.0, 1.0], size=(K, nt)) * rng.uniform(0.05, 0.45, size=(K, nt))
    for a in (kappa, fvec, X):
        a.setflags(write=False)
    return ConvCase(kappa, fvec, T0, T1), X


# ------------------------------------------------------------------ the dense restatement --------------------------

# name -> (the rule that says whether the wrong version can differ at this nt at all, what it is)
WRONG = {
    "tau = 2/nt": (lambda nt: True, "τ from the stand-in's interval instead of (T1 − T0)/nt"),
    "K diagonal included": (lambda nt: True, "r − c >= 0: subdiagonal d holds κ[d + 1] (1-based), the diagonal κ[1]"),
    "K from the second subdiagonal": (lambda nt: True, "r − c >= 2: subdiagonal d holds κ[d − 1]"),
    "K last row dropped": (lambda nt: True, "the forward product stops at r < nt: v[nt] = −fvec[nt]"),
    "K last column dropped": (lambda nt: True, "x[nt − 1] ignored, df[nt − 1] = 0"),
    "M first diagonal 2/3 tau": (lambda nt: True, "M[1,1] like the inner entries; only J sees it (K's row 1 is 0)"),
    "M last diagonal 2/3 tau": (lambda nt: True, "M[nt+1,nt+1] like the inner entries"),
    "M off-diagonal tau/3": (lambda nt: True, "τ/3 beside the diagonal instead of τ/6"),
    "fvec shifted by one": (lambda nt: True, "fvec[i + 1] for fvec[i] (rotated)"),
    "v[0] forced to 0": (lambda nt: True, "row 1 of K is zero, but v[1] = −fvec[1] is not"),
    "w[nt] dropped from the adjoint": (lambda nt: True, "the adjoint product stops at r < nt; J does not see it"),
    "df index off by one": (lambda nt: True, "Kᵀ replaced by K shifted one column: df[c] = true df[c + 1], 0 at the end"),
    "x permuted in fours": (lambda nt: nt >= 2, "each group of four of the first 16 entries of x reversed"),
}
WRONG_NAMES = list(WRONG)
# what ConvProblem's T1 − T0 = 2 cannot see at any shape (test_conv_cases.py finds what else it misses at some shape)
STANDIN_BLIND = ["tau = 2/nt"]
# what it misses at one shape or another of nt in {1, 2, 15, 16, 17, 31, 33, 63, 65}: at nt = 1 the 2 x 1 K and the
# symmetric two-entry fvec, at nt = 15 a control that is constant over its first groups of four
STANDIN_BLIND_SOMEWHERE = ["K diagonal included", "fvec shifted by one", "x permuted in fours"]


def toeplitz(kappa, dtype, first=1):
    """K (nt+1, nt) by the loops of toeplitz (:110-122) from the caller's κ = K[2:nt+1, 1]: for i = 2..nt+1 the value
    val = κ[i − 1] goes to K[j, j − i + 1], j = i..nt+1 (Julia's 1-based indices, shifted on access).  first = 1 is
    the reference; first = 0 starts the same values on the diagonal, first = 2 on the second subdiagonal."""
    nt = kappa.size
    K = np.zeros((nt + 1, nt), dtype=dtype)
    for i in range(2, nt + 2):
        val = kappa[i - 2]
        ii = i + first - 1                      # the reference: ii = i
        j = np.arange(max(ii, 1), nt + 2)       # rows j, columns j − ii + 1 <= nt
        j = j[j - ii + 1 <= nt]
        K[j - 1, j - ii] = val
    return K


def Mmat(nt, tau, dtype, first=None, last=None, off=None):
    """Mmat (:85-100); first / last / off replace M[1,1], M[nt+1,nt+1] and the off-diagonal entries."""
    M = np.zeros((nt + 1, nt + 1), dtype=dtype)
    third, six = dtype(3), dtype(6)
    M[0, 0] = tau / third
    M[nt, nt] = tau / third
    for i in range(2, nt + 1):
        M[i - 1, i - 1] = dtype(2) / third * tau
    for i in range(1, nt + 1):
        M[i - 1, i] = tau / six
        M[i, i - 1] = tau / six
    if first is not None:
        M[0, 0] = first
    if last is not None:
        M[nt, nt] = last
    if off is not None:
        i = np.arange(nt)
        M[i, i + 1] = M[i + 1, i] = off
    return M


def dense_ref(case, X, dtype=LD, wrong=None):
    """X (K, nt) -> (J (K,), df (K, nt)) in dtype: v = K·xᵀ − fvec, J = ½·vᵀ·M·v (:128-135), df = (Kᵀ·(M·v))ᵀ
    (:138-141), or the named wrong version of it."""
    assert wrong is None or wrong in WRONG, wrong
    kappa, fvec = np.asarray(case.kappa, dtype=dtype), np.asarray(case.fvec, dtype=dtype)
    nt = kappa.size
    assert nt <= DENSE_MAX_NT and X.shape[1:] == (nt,)
    X = np.array(X, dtype=dtype)
    tau = (dtype(case.T1) - dtype(case.T0)) / dtype(nt)        # example_convolution.jl:31
    if wrong == "tau = 2/nt":
        tau = dtype(2) / dtype(nt)
    Km = toeplitz(kappa, dtype, {"K diagonal included": 0, "K from the second subdiagonal": 2}.get(wrong, 1))
    if wrong == "K last row dropped":
        Km[nt, :] = 0
    if wrong == "K last column dropped":
        Km[:, nt - 1] = 0
    two3 = dtype(2) / dtype(3) * tau
    M = Mmat(nt, tau, dtype, first=two3 if wrong == "M first diagonal 2/3 tau" else None,
             last=two3 if wrong == "M last diagonal 2/3 tau" else None,
             off=tau / dtype(3) if wrong == "M off-diagonal tau/3" else None)
    if wrong == "fvec shifted by one":
        fvec = np.roll(fvec, -1)
    if wrong == "x permuted in fours":
        for g in range(0, min(nt, 16), 4):
            e = min(g + 4, nt)
            X[:, g:e] = X[:, g:e][:, ::-1].copy()
    V = X @ Km.T - fvec                                         # (K, nt+1)
    if wrong == "v[0] forced to 0":
        V[:, 0] = 0
    W = V @ M.T                                                 # rows M·v
    J = dtype(0.5) * np.sum(V * W, axis=1)
    Ka = Km
    if wrong == "w[nt] dropped from the adjoint":
        Ka = Km.copy()
        Ka[nt, :] = 0
    if wrong == "df index off by one":
        Ka = np.zeros_like(Km)
        Ka[:, :-1] = Km[:, 1:]
    return J, W @ Ka


def conv_form(case, X, dtype=np.float64, block=1024):
    """The same J and df without the matrix: v[0] = −fvec[0], v[r] = Σ_{c<r} κ[r − c] x[c] − fvec[r] (1-based κ; the
    first nt terms of the convolution κ * x), w = M·v entry by entry, df[c] = Σ_{r>c} κ[r − c] w[r] (the correlation
    of w with κ).  Both sums are taken for the whole batch at once, `block` outputs r at a time, through a
    window view of κ (row r holds κ[r − c] for c < r; nothing is stored but one block)."""
    kappa, fvec = np.asarray(case.kappa, dtype=dtype), np.asarray(case.fvec, dtype=dtype)
    nt = kappa.size
    X = np.asarray(X, dtype=dtype)
    Kn = X.shape[0]
    assert X.shape == (Kn, nt)
    tau = (dtype(case.T1) - dtype(case.T0)) / dtype(nt)
    z = np.concatenate([kappa[::-1], np.zeros(nt, dtype=dtype)])
    # win[nt − r, c] = z[nt − r + c] = κ[r − c] (1-based) for c < r and 0 from c = r on;  rows r = 1..nt
    rows = np.lib.stride_tricks.sliding_window_view(z, nt)[:nt][::-1]
    V = np.empty((Kn, nt + 1), dtype=dtype)
    V[:, 0] = 0
    for r0 in range(0, nt, block):
        e = min(r0 + block, nt)
        V[:, r0 + 1:e + 1] = X[:, :e] @ np.ascontiguousarray(rows[r0:e, :e]).T
    V -= fvec
    md_end, md_in, m_off = tau / dtype(3), dtype(2) / dtype(3) * tau, tau / dtype(6)
    W = md_in * V
    W[:, 0] = md_end * V[:, 0]
    W[:, nt] = md_end * V[:, nt]
    W[:, :-1] += m_off * V[:, 1:]
    W[:, 1:] += m_off * V[:, :-1]
    J = dtype(0.5) * np.sum(V * W, axis=1)
    DF = np.zeros((Kn, nt), dtype=dtype)
    for r0 in range(0, nt, block):
        e = min(r0 + block, nt)
        DF[:, :e] += np.ascontiguousarray(W[:, r0 + 1:e + 1]) @ np.ascontiguousarray(rows[r0:e, :e])
    return J, DF


def rel(J, df, J0, df0):
    """Per restart: (|J − J0| / |J0|, max|df − df0| / max|df0|) as float64 arrays (K,)."""
    eJ = np.abs(J - J0) / np.abs(J0)
    ed = np.max(np.abs(df - df0), axis=1) / np.max(np.abs(df0), axis=1)
    return eJ.astype(np.float64), ed.astype(np.float64)


# ------------------------------------------------------------------ the shapes -------------------------------------

def tiles_per_wave(nt, K):
    """The selection rule of launch_conv_mm restated (the GPU tests ask mioc_conv_tiles_per_wave instead): a wave
    takes two column tiles of 16 once the ceil(K/16) restart tiles x ceil(nt/32) such waves reach 1024, one wave
    for each SIMD of 256 CUs."""
    return 2 if -(-K // 16) * -(-nt // 32) >= 1024 else 1


def lds_bytes(nt, K):
    """Dynamic LDS of k_conv_mm: κ and one wave's width of zeros."""
    return (nt + 16 * tiles_per_wave(nt, K)) * 8


class Shape(collections.namedtuple("Shape", "nt K")):
    """One (nt, K); .case and .X are built once and shared (read-only) by the tests that use them."""

    @property
    def id(self):
        return f"nt{self.nt}_K{self.K}"

    @property
    def seed(self):
        return 9000 + 100 * self.nt + self.K % 97

    @property
    def case(self):
        return _built(self)[0]

    @property
    def X(self):
        return _built(self)[1]

    def rows(self, all_up_to=33):
        """The restarts the extended-precision checks look at: all of a small batch, else the first three, the
        middle one and the last two."""
        K = self.K
        return np.arange(K) if K <= all_up_to else np.array([0, 1, 2, K // 2, K - 2, K - 1])


@functools.lru_cache(maxsize=None)
def _built(s):
    return generic(s.nt, s.K, s.seed)


# One column tile per wave.  nt: 1..3, the MFMA tile (15..17), one and two column tiles and the 32-column pair
# (31..33), the 64-column workgroup (63..65, 127..129), k_conv_J's 256-thread stride over nt + 16 (239..241) and over
# nt (255..257), and 1025 (17 workgroups per restart tile, past the prefetch loops' first trips).  Every nt meets
# K = 16 (one exact restart tile) and one of the padded K in turn.
_NT_ONE = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 239, 240, 241, 255, 256, 257, 1025]
_K_PAD = [1, 2, 15, 17, 31, 33]
SHAPES_ONE_TILE = [Shape(nt, K) for i, nt in enumerate(_NT_ONE) for K in (16, _K_PAD[i % len(_K_PAD)])]


def _k_two(nt):
    """The smallest K that selects two tiles per wave, with the last restart tile padded to one restart."""
    wc = -(-nt // 32)
    return 16 * (-(-1024 // wc) - 1) + 1


# Two column tiles per wave at the smallest batch that selects them.  nt: one pair (1..32, where the second tile of
# the pair is empty up to nt = 15 / 16), 33 (a second wave), 47..49 (the d = 1 diagonal chunk kc = n0 + 16 on its edge
# nt in both directions), 127..129 (one 128-column workgroup and one column more: grp > 0), 145, 255 / 257.
_NT_TWO = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 127, 128, 129, 145, 255, 257]
SHAPES_TWO_TILES = [Shape(nt, _k_two(nt)) for nt in _NT_TWO]

# Dynamic LDS on both sides of 64 KB for either variant, and the documented maximum with both.
SHAPES_BIG_LDS = [Shape(8176, 1), Shape(8177, 1), Shape(8161, 33 * 16 - 15), Shape(16384, 1), Shape(16384, 17)]

DENSE_SHAPES = SHAPES_ONE_TILE + SHAPES_TWO_TILES
