"""TEST INFRASTRUCTURE -- the ODE examples' kernel k_ode_eval and the restart generator k_rand_start (csrc/mioc_ode.hip)
on caller data: a plain restatement of the kernel, an extended-precision reference of the same recurrences, named wrong
versions of the restatement, and the cases of tests/test_gpu_ode_shapes.py and tests/test_gpu_rand_start_shapes.py.
No torch, no device.

  eval_mirror(problem, params, x, T0, T1, wrong=None) -> (J, df, states)
        One restart in plain Python floats, one operation at a time, in the order include/mioc.h documents ("Rounding
        order") with the hooks restated term for term from mioc_ode.hip.  x: nt rows of 3 controls; params: the entry's
        parameter vector (None: the examples' values, DEFAULTS); df: nt rows of 3, states: nt rows of 2 (the state
        after each step).  sqrt of a negative number and a division by zero give what IEEE gives, not an exception.
  eval_reference(problem, params, x, T0, T1) -> (J, df, states)
        The same recurrences in numpy.longdouble, vectorised over the restarts of x (K x nt x 3, or nt x 3), summed in
        whatever order is convenient.  tau is the double the entry computes, (T1 - T0) / nt: it is data of the
        recurrence, like the parameters.
  WRONG         name -> (problems it applies to, kind); eval_mirror(..., wrong=name) is that mistake.  Kind "param": the
        hook reads another entry of the parameter vector (invisible at the examples' values, which is why the generic
        cases exist).  Kind "struct": a mistake in the sweeps.  BLIND, BLIND_NT2 and BLIND_NT2_ANY_Y0 list the pairs
        that compute the same as the restatement by arithmetic, with the reason beside them.
  CASES         the table of the GPU module; inputs(case) -> (params, X, T0, T1), seeded; mirror(case) -> (J, df, states)
        of every restart, computed once per process and shared.
  MIRROR_DISTANCE  per problem, the mirror's largest relative distance to eval_reference over all cases (measured by
        test_ode_cases.py, which holds the table to the measurement).
  rand_start_host, RS_NT, rs_jumps, RS_TABLES, RS_SEEDS, RS_MAX_NT  the host restatement of k_rand_start's stream and
        the generator's cases.
"""
from __future__ import annotations

import collections
import functools
import math
import zlib
from fractions import Fraction

import numpy as np

PROBLEMS = ("fishing", "doubletank", "vanderpol")
# the entry's defaults (mioc_ode_eval_device; example_fishing.jl, example_doubletank.jl, example_vanderpol.jl)
DEFAULTS = {
    "fishing": (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.4, 0.01, 0.1, 0.2, 0.1, 0.5, 0.7),  # a b g d c1 c2 v1[3] v2[3] y0[2]
    "doubletank": (2.0, 3.0, 1.0, 0.5, 2.0, 2.0, 2.0),                                   # k1 k2 c[3] y0[2]
    "vanderpol": (-1.0, 0.75, -2.0, 1.0, 0.0),                                           # c[3] y0[2]
}
EXAMPLE_T = {"fishing": (0.0, 12.0), "doubletank": (0.0, 10.0), "vanderpol": (0.0, 20.0)}
NAN = float("nan")


# ------------------------------------------------------------------ the restatement --------------------------------

def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else NAN  # NaN and negative arguments: NaN, as the device's sqrt


def _div(a, b):
    if b == 0.0:  # IEEE: x / +-0 is an infinity of the product's sign, 0 / 0 and NaN / 0 are NaN
        return NAN if a != a or a == 0.0 else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _fused(y, tau, f):
    """fl(y + tau*f) with one rounding: what an FMA-contracted build would compute."""
    return float(Fraction(y) + Fraction(tau) * Fraction(f))


# kind "param": the permutation of the parameter vector the hooks would see (new[q] = p[perm[q]])
def _swap(n, a, b):
    q = list(range(n))
    for i, j in zip(a, b):
        q[i], q[j] = j, i
    return tuple(q)


_PARAM_WRONG = {
    "alpha_beta_swapped": ("fishing", _swap(14, [0], [1])),
    "gamma_delta_swapped": ("fishing", _swap(14, [2], [3])),
    "c1_c2_swapped": ("fishing", _swap(14, [4], [5])),
    "v1_v2_swapped": ("fishing", _swap(14, [6, 7, 8], [9, 10, 11])),
    "fishing_y0_swapped": ("fishing", _swap(14, [12], [13])),
    "tank_k1_k2_swapped": ("doubletank", _swap(7, [0], [1])),
    "tank_c_rotated": ("doubletank", (0, 1, 3, 4, 2, 5, 6)),
    "tank_y0_swapped": ("doubletank", _swap(7, [5], [6])),
    "vdp_c_rotated": ("vanderpol", (1, 2, 0, 3, 4)),
    "vdp_y0_swapped": ("vanderpol", _swap(5, [3], [4])),
}
_STRUCT_WRONG = ("fy_not_transposed", "fy_gy_at_state_i", "fy_at_x_prev", "fu_at_state_i", "terminal_weight_one_J",
                 "terminal_weight_one_lambda", "euler_step_fused", "df_without_minus")
WRONG = {n: ((pr,), "param") for n, (pr, _) in _PARAM_WRONG.items()}
WRONG.update({n: (PROBLEMS, "struct") for n in _STRUCT_WRONG})
# Pairs that are no mistake, by arithmetic.  doubletank's Fy does not read x and its Fu reads neither y nor x: for it
# these two are the same program.  BLIND_NT2: Van der Pol from y0[1] = 0 has Fu(y0) = 0, so at nt = 2 the one adjoint
# step ends in df[:, 0] = 0 and what Fy or Gy it took cannot show (the "offset" cases start elsewhere and show it).
# And with the horizon of 2 the step tau is 1.0 at nt = 2: tau*f is exact, so y + tau*f has one rounding either way and
# the fused Euler step is the same program for every problem; it shows from nt = 130 (tau = 2/130) on.
BLIND = {("doubletank", "fy_at_x_prev"), ("doubletank", "fu_at_state_i")}
BLIND_NT2 = {("vanderpol", "fy_not_transposed"), ("vanderpol", "fy_gy_at_state_i"), ("vanderpol", "fy_at_x_prev")}
BLIND_NT2_ANY_Y0 = {(pr, "euler_step_fused") for pr in PROBLEMS}


def _hooks(problem, p):
    """(F, Fy, Fu, G, Gy, y0off) of Hooks<PROB> in mioc_ode.hip, term for term."""
    if problem == "fishing":
        def s1(x):
            return ((0.0 + x[0] * p[6]) + x[1] * p[7]) + x[2] * p[8]

        def s2(x):
            return ((0.0 + x[0] * p[9]) + x[1] * p[10]) + x[2] * p[11]

        def F(y, x):
            return (y[0] * ((p[0] - p[1] * y[1]) - p[4] * s1(x)), y[1] * ((-p[2] + p[3] * y[0]) - p[5] * s2(x)))

        def Fy(y, x):
            return (((p[0] - p[1] * y[1]) - p[4] * s1(x), y[0] * -p[1]),
                    (y[1] * p[3], (-p[2] + p[3] * y[0]) - p[5] * s2(x)))

        def Fu(y, x):
            return (tuple((y[0] * -p[4]) * p[6 + m] for m in range(3)),
                    tuple((y[1] * -p[5]) * p[9 + m] for m in range(3)))

        def G(y):
            a, b = y[0] - 1.0, y[1] - 1.0
            return 0.5 * (a * a) + 0.5 * (b * b)

        def Gy(y):
            return (y[0] - 1.0, y[1] - 1.0)
        return F, Fy, Fu, G, Gy, 12
    if problem == "doubletank":
        def cx(x):
            return ((0.0 + p[2] * x[0]) + p[3] * x[1]) + p[4] * x[2]

        def F(y, x):
            return (cx(x) - _sqrt(y[0]), _sqrt(y[0]) - _sqrt(y[1]))

        def Fy(y, x):
            return ((_div(-1.0, 2.0 * _sqrt(y[0])), 0.0),
                    (_div(1.0, 2.0 * _sqrt(y[0])), _div(-1.0, 2.0 * _sqrt(y[1]))))

        def Fu(y, x):
            return ((p[2], p[3], p[4]), (0.0, 0.0, 0.0))

        def G(y):
            d = y[1] - p[1]
            return p[0] * (d * d)

        def Gy(y):
            return (0.0, (2.0 * p[0]) * (y[1] - p[1]))
        return F, Fy, Fu, G, Gy, 5
    if problem == "vanderpol":
        def cx(x):
            return ((0.0 + p[0] * x[0]) + p[1] * x[1]) + p[2] * x[2]

        def F(y, x):
            return (y[1], ((1.0 - y[0] * y[0]) * y[1]) * cx(x) - y[0])

        def Fy(y, x):
            s = cx(x)
            return ((0.0, 1.0), (((-2.0 * y[0]) * y[1]) * s - 1.0, (1.0 - y[0] * y[0]) * s))

        def Fu(y, x):
            return ((0.0, 0.0, 0.0), tuple((p[m] * (1.0 - y[0] * y[0])) * y[1] for m in range(3)))

        def G(y):
            return y[0] * y[0] + y[1] * y[1]

        def Gy(y):
            return (2.0 * y[0], 2.0 * y[1])
        return F, Fy, Fu, G, Gy, 3
    raise ValueError(problem)


def eval_mirror(problem, params, x, T0, T1, wrong=None):
    """k_ode_eval for one restart (see the module docstring); `wrong` names one mistake of WRONG."""
    p = [float(v) for v in (DEFAULTS[problem] if params is None else params)]
    assert len(p) == len(DEFAULTS[problem])
    if wrong is not None:
        assert problem in WRONG[wrong][0], (problem, wrong)
    if wrong in _PARAM_WRONG:
        p = [p[q] for q in _PARAM_WRONG[wrong][1]]
    F, Fy, Fu, G, Gy, y0off = _hooks(problem, p)
    x = [(float(r[0]), float(r[1]), float(r[2])) for r in x]
    nt = len(x)
    tau = (float(T1) - float(T0)) / float(nt)
    y0 = (p[y0off], p[y0off + 1])
    # forward: explicit Euler, trapezoid cost
    y, st = y0, []
    fval = 0.5 * G(y0)
    for i in range(nt):
        f = F(y, x[i])
        if wrong == "euler_step_fused":
            y = (_fused(y[0], tau, f[0]), _fused(y[1], tau, f[1]))
        else:
            y = (y[0] + tau * f[0], y[1] + tau * f[1])
        st.append(y)
        fval = fval + (G(y) if i < nt - 1 or wrong == "terminal_weight_one_J" else 0.5 * G(y))
    J = fval * tau
    # backward: adjoint, df = Gu - Fu' lam with Gu = 0
    g = Gy(st[nt - 1])
    w = -tau if wrong == "terminal_weight_one_lambda" else -0.5 * tau
    lam = (w * g[0], w * g[1])
    df = [None] * nt
    for i in range(nt - 1, -1, -1):
        sprev = y0 if i == 0 else st[i - 1]
        fu = Fu(st[i] if wrong == "fu_at_state_i" else sprev, x[i])
        if wrong == "df_without_minus":
            df[i] = tuple((fu[0][m] * lam[0] + fu[1][m] * lam[1]) + 0.0 for m in range(3))
        else:
            df[i] = tuple((0.0 - (fu[0][m] * lam[0] + fu[1][m] * lam[1])) + 0.0 for m in range(3))
        if i == 0:
            break
        si = st[i] if wrong == "fy_gy_at_state_i" else st[i - 1]
        g = Gy(si)
        fy = Fy(si, x[i - 1] if wrong == "fy_at_x_prev" else x[i])
        if wrong == "fy_not_transposed":
            a0 = fy[0][0] * lam[0] + fy[0][1] * lam[1]
            a1 = fy[1][0] * lam[0] + fy[1][1] * lam[1]
        else:
            a0 = fy[0][0] * lam[0] + fy[1][0] * lam[1]
            a1 = fy[0][1] * lam[0] + fy[1][1] * lam[1]
        lam = (lam[0] + tau * (a0 - g[0]), lam[1] + tau * (a1 - g[1]))
    return J, df, st


# ------------------------------------------------------------------ the extended-precision reference ---------------
LD = np.longdouble


def eval_reference(problem, params, x, T0, T1):
    """The recurrences of ODEObjective.jl:125-184 with the example's hooks in numpy.longdouble, all restarts of x at
    once.  Written from the formulas (matrices and dot products), not from the kernel's order of operations."""
    p = [LD(float(v)) for v in (DEFAULTS[problem] if params is None else params)]
    X = np.asarray(x, dtype=np.float64)
    single = X.ndim == 2
    X = (X[None] if single else X).astype(LD)
    K, nt, _ = X.shape
    tau = LD((float(T1) - float(T0)) / float(nt))
    zero, one = np.zeros(K, dtype=LD), np.ones(K, dtype=LD)
    if problem == "fishing":
        al, be, ga, de, c1, c2 = p[:6]
        v1, v2, y0 = np.array(p[6:9]), np.array(p[9:12]), p[12:14]

        def F(y, u):
            return np.stack([y[0] * (al - be * y[1] - c1 * (u @ v1)), y[1] * (de * y[0] - ga - c2 * (u @ v2))])

        def Fy(y, u):
            return [[al - be * y[1] - c1 * (u @ v1), -be * y[0]], [de * y[1], de * y[0] - ga - c2 * (u @ v2)]]

        def Fu(y, u):
            return [[-c1 * v1[m] * y[0] for m in range(3)], [-c2 * v2[m] * y[1] for m in range(3)]]

        def G(y):
            return ((y[0] - 1) ** 2 + (y[1] - 1) ** 2) / 2

        def Gy(y):
            return np.stack([y[0] - 1, y[1] - 1])
    elif problem == "doubletank":
        k1, k2 = p[:2]
        c, y0 = np.array(p[2:5]), p[5:7]

        def F(y, u):
            r = np.sqrt(y)
            return np.stack([u @ c - r[0], r[0] - r[1]])

        def Fy(y, u):
            r = np.sqrt(y)
            return [[-1 / (2 * r[0]), zero], [1 / (2 * r[0]), -1 / (2 * r[1])]]

        def Fu(y, u):
            return [[c[m] * one for m in range(3)], [zero] * 3]

        def G(y):
            return k1 * (y[1] - k2) ** 2

        def Gy(y):
            return np.stack([zero, 2 * k1 * (y[1] - k2)])
    elif problem == "vanderpol":
        c, y0 = np.array(p[:3]), p[3:5]

        def F(y, u):
            return np.stack([y[1], (1 - y[0] ** 2) * y[1] * (u @ c) - y[0]])

        def Fy(y, u):
            s = u @ c
            return [[zero, one], [-2 * y[0] * y[1] * s - 1, (1 - y[0] ** 2) * s]]

        def Fu(y, u):
            return [[zero] * 3, [c[m] * (1 - y[0] ** 2) * y[1] for m in range(3)]]

        def G(y):
            return y[0] ** 2 + y[1] ** 2

        def Gy(y):
            return 2 * y
    else:
        raise ValueError(problem)
    with np.errstate(invalid="ignore", divide="ignore"):
        ystart = np.stack([y0[0] * one, y0[1] * one])
        y, st = ystart, []
        fval = G(ystart) / 2
        for i in range(nt):
            y = y + tau * F(y, X[:, i])
            st.append(y)
            fval = fval + (G(y) if i < nt - 1 else G(y) / 2)
        J = tau * fval
        lam = -tau / 2 * Gy(st[-1])
        df = np.zeros((K, nt, 3), dtype=LD)
        for i in range(nt - 1, -1, -1):
            yp = ystart if i == 0 else st[i - 1]
            fu = Fu(yp, X[:, i])
            for m in range(3):
                df[:, i, m] = -(fu[0][m] * lam[0] + fu[1][m] * lam[1])
            if i == 0:
                break
            fy = Fy(yp, X[:, i])
            lam = lam + tau * (np.stack([fy[0][0] * lam[0] + fy[1][0] * lam[1], fy[0][1] * lam[0] + fy[1][1] * lam[1]])
                               - Gy(yp))
    states = np.stack(st, axis=1).transpose(2, 1, 0)  # K x nt x 2
    return (J[0], df[0], states[0]) if single else (J, df, states)


# ------------------------------------------------------------------ the cases ---------------------------------------
# params: "generic" (the example's values times distinct seeded factors in [0.7, 1.3], T0 != 0, T1 - T0 = 2), "offset"
# (the same with a nonzero y0[1] for Van der Pol, see _cases),
# "default" (params=None, the example's horizon: ties the mirror to oracle/ode_oracle.py) or "nan" (doubletank with
# y0 = (0.01, 2): restart NAN_RESTART has zero inflow, its first tank runs dry and sqrt sees a negative state).
# out: which outputs the call asks for.
Case = collections.namedtuple("Case", "id problem nt K params out")
KPOOL = 130          # generic restarts per (problem, nt): a case with K restarts takes the first K
T0_GENERIC = 0.75
NAN_RESTART, NAN_K = 2, 5
# nt of the default cases: explicit Euler over the example's horizon stays finite at these step counts
_DEFAULT_NT = {"fishing": 200, "doubletank": 200, "vanderpol": 400}


def _cases():
    out = []
    for pr in PROBLEMS:
        for nt in (1, 2, 130):                      # i == 0 takes sprev = y0; a terminal that is also the first step
            out.append(Case(f"{pr}_nt{nt}_K3", pr, nt, 3, "generic", "both"))
        for K in (1, 63, 64, 65, 130):              # the 64-thread block's tail guard k >= K, a second and third block
            out.append(Case(f"{pr}_nt130_K{K}", pr, 130, K, "generic", "both"))
        out.append(Case(f"{pr}_nt130_K65_Jonly", pr, 130, 65, "generic", "J"))
        out.append(Case(f"{pr}_nt130_K65_dfonly", pr, 130, 65, "generic", "df"))
        out.append(Case(f"{pr}_default_nt{_DEFAULT_NT[pr]}_K4", pr, _DEFAULT_NT[pr], 4, "default", "both"))
    # Van der Pol starts at y0[1] = 0, and a factor leaves that 0: Fu(y0) = 0, so df[:, 0] is zero whatever the adjoint
    # at step 0 is, and at nt = 1, 2 nothing else would show it.  The same shapes from y0[1] = 0.3 times its factor.
    for nt in (1, 2):
        out.append(Case(f"vanderpol_nt{nt}_K3_y0", "vanderpol", nt, 3, "offset", "both"))
    out.append(Case("doubletank_nan_nt130_K5", "doubletank", 130, NAN_K, "nan", "both"))
    return out


CASES = _cases()
GENERIC = [c for c in CASES if c.params in ("generic", "offset")]
# one context, in this order: a call, a larger one (the state scratch grows), a smaller one (reused), another problem
CONTEXT_SEQUENCE = ("fishing_nt130_K64", "fishing_nt130_K130", "fishing_nt2_K3", "doubletank_nt130_K65",
                    "vanderpol_nt1_K3")


def case(cid):
    return next(c for c in CASES if c.id == cid)


# Every draw below is keyed by this salt and the names of what is drawn.  It is the first value (from 0) at which the
# conditions test_ode_cases.py asserts on the inputs hold: the states' bounds (at 0 and 2 a tank runs below 0.1), and the
# fused Euler step showing in the one restart of doubletank's K = 1 case (at 1, 3 and 4 its roundings are absorbed).
# Nothing a device computes enters the choice.
SALT = 5


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr((SALT,) + key).encode()))


def generic_params(problem, offset=False):
    """The example's values times distinct factors in [0.7, 1.3]; offset: a zero entry (Van der Pol's y0[1]) becomes
    0.3 times its factor."""
    f = _rng("ode-params", problem).uniform(0.7, 1.3, size=len(DEFAULTS[problem]))
    return tuple(float((a if a != 0.0 or not offset else 0.3) * b) for a, b in zip(DEFAULTS[problem], f))


@functools.lru_cache(maxsize=None)
def _controls(problem, nt, K, tag):
    """K x nt x 3: step i of restart k is a one-hot SOS1 level when i + k is even, else three non-integral components
    in (0, 1) -- so s1, s2 and cx see one term on half the steps and three on the other half."""
    rng = _rng("ode-controls", problem, nt, tag)
    X = rng.uniform(0.05, 0.95, size=(K, nt, 3))
    lev = rng.integers(0, 3, size=(K, nt))
    hot = (np.add.outer(np.arange(K), np.arange(nt)) % 2) == 0
    X[hot] = np.eye(3)[lev[hot]]
    X.setflags(write=False)
    return X


def inputs(c):
    """(params or None, X of K x nt x 3, T0, T1) of a case."""
    if c.params in ("generic", "offset"):
        par = generic_params(c.problem, offset=c.params == "offset")
        return par, _controls(c.problem, c.nt, KPOOL, "generic")[:c.K], T0_GENERIC, T0_GENERIC + 2.0
    if c.params == "default":
        return None, _controls(c.problem, c.nt, c.K, "default"), *EXAMPLE_T[c.problem]
    par = list(generic_params(c.problem))
    par[5:7] = [0.01, 2.0]
    X = np.array(_controls(c.problem, c.nt, c.K, "nan"))
    X[NAN_RESTART] = 0.0
    X.setflags(write=False)
    return tuple(par), X, T0_GENERIC, T0_GENERIC + 2.0


@functools.lru_cache(maxsize=None)
def _mirror_pool(problem, nt, kind, K):
    c = Case("", problem, nt, K, kind, "both")
    par, X, T0, T1 = inputs(c)
    J, DF, ST = np.empty(K), np.empty((K, nt, 3)), np.empty((K, nt, 2))
    for k in range(K):
        J[k], df, st = eval_mirror(problem, par, X[k], T0, T1)
        DF[k], ST[k] = df, st
    for a in (J, DF, ST):
        a.setflags(write=False)
    return J, DF, ST


def mirror(c):
    """(J of K, df of K x nt x 3, states of K x nt x 2) of the restatement for every restart of a case; the generic
    cases of one (problem, nt) share one evaluation of the pool."""
    J, DF, ST = _mirror_pool(c.problem, c.nt, c.params, KPOOL if c.params in ("generic", "offset") else c.K)
    return J[:c.K], DF[:c.K], ST[:c.K]


# The mirror's largest relative distance to eval_reference per problem, over every case but the NaN restart:
# max over restarts of |J - J_ref| / |J_ref| and of max|df - df_ref| / max|df_ref|.  Measured on the CPU by
# test_ode_cases.py::test_mirror_distance_to_reference, which fails if a figure here is below the measurement or more
# than twice it.  A device that is not bit-identical to the mirror would be held to 4x these (two float64 evaluations
# of one recurrence that differ in single roundings), never to its own output.
MIRROR_DISTANCE = {"fishing": 1.9e-15, "doubletank": 3.1e-15, "vanderpol": 3.5e-15}


def distance(J, DF, Jr, DFr):
    """The relative distance of MIRROR_DISTANCE between float64 results and a longdouble reference."""
    Jr, DFr = np.asarray(Jr, dtype=LD), np.asarray(DFr, dtype=LD)
    dj = np.max(np.abs(np.asarray(J, dtype=LD) - Jr) / np.abs(Jr))
    err, scale = np.max(np.abs(np.asarray(DF, dtype=LD) - DFr), axis=(1, 2)), np.max(np.abs(DFr), axis=(1, 2))
    # a gradient that is zero throughout (Van der Pol from y0[1] = 0 at nt = 1) must be met exactly
    dd = np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err > 0, np.inf, 0)))
    return float(max(dj, dd))


# ------------------------------------------------------------------ the restart generator ---------------------------
_M64 = (1 << 64) - 1


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _uniform(key, stream, idx, n):
    v = _mix(key ^ ((stream << 56) & _M64) ^ idx)
    return ((v >> 32) * n) >> 32


def rand_start_host(levels, nt, jumps, seed, k):
    """Host restatement of k_rand_start's stream (test-only): Floyd's sample of the jump times, a level per segment.
    Returns (u of M x nt, the set of candidate jump times)."""
    key = _mix((seed + 0x9E3779B97F4A7C15 * (k + 1)) & _M64)
    N, S = nt - 1, set()
    for q, j in enumerate(range(N - jumps + 1, N + 1)):
        t = 1 + _uniform(key, 1, q, j)
        S.add(j if t in S else t)
    jump = np.zeros(nt, dtype=np.int64)
    jump[sorted(S)] = 1
    seg = np.cumsum(jump)  # segment of step i = number of jump times <= i
    ranks = np.array([_uniform(key, 2, s, levels.L) for s in range(int(seg[-1]) + 1)])
    u = np.ascontiguousarray(np.asarray(levels.nuval, dtype=np.float64)[ranks[seg]].T)
    return u, S


# nt: one, two, below / at / above one bitmap word and two, and the step from one to two bitmap words per thread
# (256 threads x 32 steps = 8192), with a last word partly beyond nt (8193, 8225 = 257 words + 1 step)
RS_NT = (1, 2, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193, 8225)
RS_SEEDS = (0, (1 << 64) - 1, 0x9E3779B97F4A7C15 - 1)  # 0 and 2^64 - 1 (seed + phi*(k+1) wraps), one in between
RS_TABLES = {                                          # name -> nu (product iterator)
    "L1": [[4]],
    "L3_M1": [[-1, 0, 2]],
    "L15_3x5": [[0, 1, 2], [-2, -1, 0, 1, 2]],
    "L256_M8": [[0, 1]] * 8,
}
RS_MAX_NT = (65536 // 4 - 256) * 32  # the largest nt whose bitmap and counts fit the 64 KB of LDS: 516096


def rs_jumps(nt):
    """The jump counts of a case: the default floor(nt / 10) (as -1, the entry's spelling), 0, 1 and nt - 1, where
    admissible (jumps <= nt - 1), without duplicates of the value."""
    out, seen = [], set()
    for j in (-1, 0, 1, nt - 1):
        v = nt // 10 if j < 0 else j
        if v <= nt - 1 and v not in seen:
            seen.add(v)
            out.append(j)
    return out
