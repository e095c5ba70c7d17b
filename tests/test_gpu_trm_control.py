"""GPU tier of the device-resident TRM control (csrc/mioc_trm.hip: k_trm_outer_begin, k_trm_inner_end, k_trm_copy, the
gate word they drive, mioc_trm_poll) against its plain-Python restatement (tests/trm_control_mirror.py, anchored to the
host loop mioc.TRM in tests/test_trm_control.py), branch by branch and bit for bit: the file is built without
floating-point contraction, so there is no tolerance anywhere here.  Float arrays are compared by their bit patterns
(NaN equals NaN, 0.0 differs from -0.0).

Both control kernels are one 1024-thread workgroup that strides over the restarts and folds three block-wide ORs, so
the shapes are K around 64 and around 1024, 2049 and the ABI's limit 4096, and flags set by one restart only.
k_trm_copy strides over at most 64 chunks of 256 elements: n_per_restart around 256 and 16384.  Then every entry point
gated by mioc_trm_attach with the gate word 0 and 1, the argument checks, and TRM_batch with more restarts than one
pass of the workgroup.
"""
import copy
import math

import numpy as np
import pytest

import mioc
from mioc import native
from mioc.iterators import LevelTable

import trm_control_mirror as tm
from trm_control_mirror import COPY_U, COPY_UOLD, HALVED, INNER, STOP

pytestmark = pytest.mark.gpu

BETA, SIGMA, KMAX, TAU, B, D0 = 0.25, 0.5, 4, 0.1, 10, 1.0
NAN = math.nan
F64 = ("int_val", "tv_new", "J_new", "J_old", "J", "tv_u", "trial", "u", "u_old")
I32 = ("budgets", "decision")

# (flags, k, Δᵏ, TV_old, int_val, TV_new, J_old, J_new): β = 0.25, σ = 0.5, kmax = 4, Δt = 0.1, B = 10
_JUNK = (2.0, NAN, NAN, 5.0, NAN)                       # a restart outside its loop: the inputs must not be read
CASES = [
    (INNER, 1, 1.0, 2.0, -1.0, 2.0, 5.0, 4.0),          # pred = -1: stop
    (INNER, 2, 1.0, 2.0, 0.0, 2.0, 5.0, 4.0),           # pred = 0.0: stop
    (INNER, 1, 1.0, -0.0, -0.0, 0.0, 5.0, 4.0),         # pred = -0.0 + 0.25 (-0.0 - 0.0) = -0.0: stop
    (INNER, 1, 1.0, 3.0, 0.5, 1.0, 5.0, 4.0),           # pred = 1, ared = 1.5: accept
    (INNER, 1, 1.0, 2.0, 1.0, 2.0, 5.0, 5.0),           # pred = 1, ared = 0: halve; 0.5 / 0.1 = 5 exactly
    (INNER, 1, 1.0, 2.0, NAN, 2.0, 5.0, 4.0),           # NaN int_val: NaN pred, accept
    (INNER, 1, 1.0, 2.0, 1.0, NAN, 5.0, 4.0),           # NaN TV_new: NaN pred and ared, accept; TV_old becomes NaN
    (INNER, 1, 1.0, 2.0, 1.0, 2.0, 5.0, NAN),           # NaN J_new: NaN ared, accept; J_old becomes NaN
    (INNER, 1, 1.0, 2.0, 2.0, 2.0, 5.0, 4.0),           # ared = 1 = σ pred exactly: accept
    (INNER, 1, 1.0, 3.0, 1.0, 1.0, 5.0, 4.75),          # pred = 1.5, ared = 0.25 + 0.5 = σ pred exactly: accept
    (INNER, 1, 1.0, 2.0, 2.0, 2.0, 5.0, 4.000000000000001),  # ared one ulp of 4 below σ pred: halve
    (INNER, KMAX, 1.0, 2.0, 1.0, 2.0, 5.0, 5.0),        # halve at k = kmax: leaves the loop with HALVED set
    (INNER, KMAX, 1.0, 2.0, 1.0, 2.0, 5.0, 4.0),        # accept at k = kmax
    (INNER, KMAX, 1.0, 2.0, -1.0, 2.0, 5.0, 4.0),       # stop at k = kmax
    (INNER | HALVED, 2, 0.5, 2.0, 1.0, 2.0, 5.0, 5.0),  # halve, halved before: 0.25 / 0.1 -> 2
    (INNER | HALVED, 2, 0.5, 2.0, 1.0, 2.0, 5.0, 4.0),  # accept, halved before: the budget is floor(0.5 / 0.1)
    (INNER | HALVED, 3, 0.25, 2.0, -1.0, 2.0, 5.0, 4.0),  # stop, halved before
    (INNER, 1, 0.6, 2.0, 1.0, 2.0, 5.0, 5.0),           # halve to 0.3: 0.3 / 0.1 = 2.9999999999999996 -> 2
    (INNER | HALVED, 3, 0.125, 2.0, 1.0, 2.0, 5.0, 5.0),  # halve to 0.0625: budget 0
    (INNER | COPY_UOLD, 1, 1.0, 2.0, 1.0, 2.0, 5.0, 5.0),  # halve with a stale u_old bit: u_old must stay
    (INNER | COPY_U | COPY_UOLD, 1, 1.0, 2.0, -1.0, 2.0, 5.0, 4.0),  # stop with stale bits
    (0, 3, 0.5) + _JUNK,                                # outside the loop, never entered
    (STOP, 2, 1.0) + _JUNK,                             # stopped
    (HALVED, KMAX + 1, 0.5) + _JUNK,                    # left at kmax after a halving
    (STOP | COPY_U | COPY_UOLD, 2, 1.0) + _JUNK,        # stopped, the copy bits of its last trial still set
    (COPY_U | COPY_UOLD, 2, 1.0) + _JUNK,               # accepted in the last call
]
STOPPED_ROW = (STOP, 2, 1.0) + _JUNK
REQUIRED = {
    "stop pred<0", "stop pred==0.0", "stop pred==-0.0", "accept", "halve budget 5", "accept NaN pred",
    "accept NaN J_new", "accept ared==sigma*pred", "halve k==kmax budget 5", "accept k==kmax", "stop k==kmax pred<0",
    "halve halved budget 2", "accept halved", "halve budget 2", "halve halved budget 0", "halve stale budget 5",
    "out 0", "out %d" % STOP, "out %d" % HALVED, "out %d" % (STOP | COPY_U | COPY_UOLD),
}


def _label(row):
    """The branch a table row reaches, from the reference's expressions."""
    f, k, Dk, tvo, iv, tvn, Jo, Jn = row
    if not f & INNER:
        return "out %d" % f
    pred = iv + BETA * (tvo - tvn)
    ared = (Jo - Jn) + BETA * (tvo - tvn)
    d = 2 if pred <= 0 else 1 if ared < SIGMA * pred else 0
    parts = [("accept", "halve", "stop")[d]]
    parts += ["k==kmax"] if k == KMAX else []
    parts += ["halved"] if f & HALVED else []
    parts += ["stale"] if f & (COPY_U | COPY_UOLD) and d == 1 else []
    if d == 2:
        parts.append("pred<0" if pred < 0 else "pred==-0.0" if math.copysign(1.0, pred) < 0 else "pred==0.0")
    elif d == 1:
        parts.append("budget %d" % math.floor(Dk / 2 / TAU))
    elif math.isnan(pred):
        parts.append("NaN pred")
    elif math.isnan(Jn):
        parts.append("NaN J_new")
    elif ared == SIGMA * pred:
        parts.append("ared==sigma*pred")
    return " ".join(parts)


def _dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def _sync():
    import torch
    torch.cuda.synchronize()


def _ctx():
    ctx = native.Context(0)
    ctx.set_levels(LevelTable([[0, 1]]))
    ctx.set_cost(1, BETA)
    return ctx


def _case(rows, n=3):
    """Host arrays of one call from table rows: the state, the three words (7: a word the kernel does not write
    shows), the per-restart inputs, and sentinels in everything a kernel may write."""
    K = len(rows)
    col = lambda j: np.array([r[j] for r in rows], dtype=np.float64)  # noqa: E731
    st = tm.new_state(K)
    st["flags"][:] = [r[0] for r in rows]
    st["k"][:] = [r[1] for r in rows]
    st["Dk"][:], st["tv_old"][:] = col(2), col(3)
    st["iters"][:] = np.arange(K) % 3
    e = np.arange(K * n, dtype=np.float64).reshape(K, n)
    return dict(state=st, words=(7, 7, 7), int_val=col(4), tv_new=col(5), J_old=col(6), J_new=col(7),
                J=100.0 + np.arange(K), tv_u=50.0 + np.arange(K), budgets=np.full(K, 77, dtype=np.int32),
                decision=np.full(K, -9, dtype=np.int32), trial=e + 0.5, u=1e6 + e, u_old=2e6 + e)


def _cycle(K):
    return [CASES[r % len(CASES)] for r in range(K)]


def _upload(c):
    import torch
    d = {"block": torch.from_numpy(tm.pack_state(c["state"], c["words"])).cuda()}
    d.update({n: _dev(c[n]) for n in F64})
    d.update({n: _dev(c[n], torch.int32) for n in I32})
    return d


def _download(ctx, d, K):
    ctx.synchronize()
    st, words = tm.unpack_state(d["block"].cpu().numpy(), K)
    out = dict(state=st, words=words)
    out.update({n: d[n].cpu().numpy() for n in F64 + I32})
    return out


def _host_outer(c):
    budgets, _, c["words"] = tm.outer_begin_host(c["state"], c["tv_u"], D0, B)
    c["budgets"][:] = budgets


def _host_inner(c, decision=True, kmax=KMAX):
    _, dec, c["words"] = tm.inner_end_host(c["state"], BETA, SIGMA, kmax, TAU, B, c["int_val"], c["tv_new"],
                                           c["J_new"], c["J_old"], c["J"], c["tv_u"], c["budgets"])
    if decision:
        c["decision"][:] = dec
    tm.copy_host(c["state"]["flags"], c["trial"], c["u"], c["u_old"])
    return dec


def _dev_outer(ctx, d):
    ctx.trm_outer_begin(d["block"], d["tv_u"], D0, B, d["budgets"])


def _dev_inner(ctx, d, decision=True, kmax=KMAX):
    ctx.trm_inner_end(d["block"], SIGMA, kmax, TAU, B, d["int_val"], d["tv_new"], d["J_new"], d["J_old"], d["J"],
                      d["tv_u"], d["budgets"], d["trial"], d["u"], d["u_old"],
                      decision=d["decision"] if decision else None)


def _assert_same(got, want, tag=""):
    assert got["words"] == want["words"], (tag, got["words"], want["words"])
    for n in ("Dk", "tv_old"):
        assert np.array_equal(tm.bits(got["state"][n]), tm.bits(want["state"][n])), \
            (tag, n, np.flatnonzero(tm.bits(got["state"][n]) != tm.bits(want["state"][n]))[:8])
    for n in ("k", "flags", "iters"):
        assert np.array_equal(got["state"][n], want["state"][n]), \
            (tag, n, np.flatnonzero(got["state"][n] != want["state"][n])[:8])
    for n in F64:
        assert np.array_equal(tm.bits(got[n]), tm.bits(want[n])), \
            (tag, n, np.argwhere(tm.bits(got[n]) != tm.bits(want[n]))[:8])
    for n in I32:
        assert np.array_equal(got[n], want[n]), (tag, n, np.flatnonzero(got[n] != want[n])[:8])


def _check_call(ctx, c, which, tag, **kw):
    """One device call on a fresh upload of c against the restatement on a copy of c; the poll must return the
    first two words.  Returns the expected arrays."""
    K = len(c["J"])
    want = copy.deepcopy(c)
    d = _upload(c)
    _sync()
    if which == "outer":
        _host_outer(want)
        _dev_outer(ctx, d)
    else:
        _host_inner(want, **kw)
        _dev_inner(ctx, d, **kw)
    poll = ctx.trm_poll(d["block"])
    _assert_same(_download(ctx, d, K), want, tag)
    assert poll == (bool(want["words"][0]), bool(want["words"][1])), (tag, poll, want["words"])
    return want


# ---- k_trm_inner_end, k_trm_copy: every branch -----------------------------------------------------------------------
@pytest.mark.parametrize("decision", [True, False])
def test_inner_end_every_branch(decision):
    seen = {_label(r) for r in CASES}
    assert REQUIRED <= seen, REQUIRED - seen
    c = _case(CASES)
    with _ctx() as ctx:
        want = _check_call(ctx, c, "inner", "table", decision=decision)
    # what the restatement says about the restarts outside their loop, spelled out
    out = np.array([not r[0] & INNER for r in CASES])
    assert out.sum() >= 5 and want["words"] == (1, 1, 1)
    for n in F64 + ("budgets",):
        assert np.array_equal(tm.bits(want[n][out]) if n in F64 else want[n][out],
                              tm.bits(c[n][out]) if n in F64 else c[n][out]), n
    for n in ("Dk", "tv_old", "k", "iters"):
        assert np.array_equal(want["state"][n][out], c["state"][n][out]), n
    assert np.array_equal(want["state"]["flags"][out], c["state"]["flags"][out] & ~(COPY_U | COPY_UOLD))
    assert np.all(want["decision"][out] == (-1 if decision else -9))
    if not decision:
        assert np.all(want["decision"] == -9)
    # and about those inside: the trial is obj.x; u_old follows an accept only; NaN J_new becomes J_old
    labels = [_label(r) for r in CASES]
    for r, lab in enumerate(labels):
        if out[r]:
            continue
        assert np.array_equal(want["u"][r], c["trial"][r]), lab
        assert np.array_equal(want["u_old"][r], c["trial"][r] if lab.startswith("accept") else c["u_old"][r]), lab
    r = labels.index("accept NaN J_new")
    assert math.isnan(want["J_old"][r]) and math.isnan(want["J"][r])
    r = labels.index("halve k==kmax budget 5")
    assert want["state"]["flags"][r] == HALVED | COPY_U and want["budgets"][r] == 5
    assert [want["budgets"][labels.index(s)] for s in ("halve budget 5", "halve budget 2", "halve halved budget 0")] \
        == [5, 2, 0]


# ---- the one workgroup's stride over the restarts, the three block-wide ORs ----------------------------------------
def _sparse(K, idx, row):
    rows = [STOPPED_ROW] * K
    rows[idx] = row
    return rows


@pytest.mark.parametrize("K", [1, 63, 64, 1023, 1024, 1025, 2049, 4096])
def test_control_strides_over_restarts(K):
    assert tm.state_bytes(K) == native.load_library().mioc_trm_state_bytes(K)
    halve, idle = CASES[4], (HALVED, KMAX + 1, 0.5) + _JUNK
    with _ctx() as ctx:
        c = _case(_cycle(K), n=1)
        _check_call(ctx, c, "outer", "outer table")
        _check_call(ctx, c, "inner", "inner table")
        if K <= 1024:
            return
        want = _check_call(ctx, _case([STOPPED_ROW] * K, n=1), "outer", "outer all stopped")
        assert want["words"] == (0, 0, 0)
        want = _check_call(ctx, _case([STOPPED_ROW] * K, n=1), "inner", "inner all stopped")
        assert want["words"] == (0, 0, 0)
        # one restart alone sets a word: the last one, the first of the second pass, lane 0 of wave 15 of the first
        for idx in dict.fromkeys((K - 1, 1024, 960)):
            want = _check_call(ctx, _case(_sparse(K, idx, idle), n=1), "outer", f"outer one live at {idx}")
            assert want["words"] == (1, 1, 0) and want["state"]["flags"][idx] == INNER
            want = _check_call(ctx, _case(_sparse(K, idx, halve), n=1), "inner", f"inner one in its loop at {idx}")
            assert want["words"] == (1, 1, 1)
            want = _check_call(ctx, _case(_sparse(K, idx, idle), n=1), "inner", f"inner one not stopped at {idx}")
            assert want["words"] == (0, 1, 0)


# ---- several outer iterations in sequence ----------------------------------------------------------------------------
def _synthetic(rng, c, n):
    """Seeded inputs of one trial: stops (pred <= 0), halvings (J unchanged or TV worse) and accepts all occur."""
    K = len(c["J"])
    c["int_val"] = rng.choice([-1.0, 0.0, 0.5, 1.0, 2.0], size=K, p=[0.04, 0.01, 0.3, 0.35, 0.3])
    c["tv_new"] = rng.integers(0, 4, size=K).astype(np.float64)
    c["J_new"] = c["J_old"] - rng.choice([0.0, 0.25, 1.0, 3.0], size=K)
    c["trial"] = rng.integers(0, 3, size=(K, n)).astype(np.float64)


def test_multi_round_sequence():
    K, kmax, n = 1500, 3, 2
    rng = np.random.default_rng(42)
    c = _case([(0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)] * K, n=n)   # the zero-initialised block of trm_state_tensor
    c["state"]["iters"][:] = 0
    c["words"] = (0, 0, 0)
    c["J_old"] = rng.normal(size=K) * 3
    c["tv_u"] = rng.integers(0, 4, size=K).astype(np.float64)
    c["J"][:] = math.inf
    with _ctx() as ctx:
        d = _upload(c)
        _sync()

        def new_inputs():
            import torch
            _synthetic(rng, c, n)
            ins = {m: _dev(c[m]) for m in ("int_val", "tv_new", "J_new", "trial")}
            torch.cuda.synchronize()
            return ins

        for it in range(1, 5):
            stopped_before = int(np.sum(c["state"]["flags"] & STOP != 0))
            _host_outer(c)
            _dev_outer(ctx, d)
            _assert_same(_download(ctx, d, K), c, f"outer {it}")
            assert np.all(c["budgets"] == B) and np.array_equal(tm.bits(c["state"]["tv_old"]), tm.bits(c["tv_u"]))
            assert c["words"] == (1, 1, 0)
            for j in range(1, kmax + 1):
                d.update(new_inputs())
                dec = _host_inner(c, kmax=kmax)
                _dev_inner(ctx, d, kmax=kmax)
                assert ctx.trm_poll(d["block"]) == (bool(c["words"][0]), bool(c["words"][1]))
                _assert_same(_download(ctx, d, K), c, f"outer {it} inner {j}")
                assert {0, 1, 2} <= set(dec.tolist()), (it, j, np.bincount(dec + 1))   # all three decisions
            assert c["words"][0] == 0 and c["words"][1] == 1                           # k > kmax closed the gate
            stopped = int(np.sum(c["state"]["flags"] & STOP != 0))
            assert stopped > stopped_before, it                                        # a stop in this outer iteration
            live = c["state"]["flags"] & STOP == 0
            assert np.all(c["state"]["iters"][live] == it) and np.all(c["state"]["iters"][~live] <= it)
        assert len(set(c["state"]["iters"].tolist())) >= 3       # restarts stopped in different outer iterations
        # one whole outer iteration enqueued without a synchronisation in between
        _host_outer(c)
        ins = []
        for j in range(kmax):
            ins.append(new_inputs())
            _host_inner(c, kmax=kmax)
        _dev_outer(ctx, d)
        for j in range(kmax):
            d.update(ins[j])
            _dev_inner(ctx, d, kmax=kmax)
        _assert_same(_download(ctx, d, K), c, "outer 5, enqueued as a whole")


# ---- k_trm_copy: its grid-stride, its early exit, stale copy bits ----------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 16384, 16385, 40000])
def test_copy_shapes_and_stale_bits(n):
    """Restart 0 accepts, restart 1 halves, restart 2 is outside its loop.  In the second call restart 0 is outside
    its loop with the copy bits of its accept still in the block: its u and u_old must keep the first trial."""
    import torch
    K = 3
    accept, halve, idle = CASES[3], CASES[4], (0, 3, 0.5) + _JUNK
    c = _case([accept, halve, idle], n=n)
    with _ctx() as ctx:
        d = _upload(c)
        _sync()
        first = c["trial"].copy()
        u0, uold0 = c["u"].copy(), c["u_old"].copy()
        _host_inner(c)
        _dev_inner(ctx, d)
        _assert_same(_download(ctx, d, K), c, "first")
        assert np.array_equal(c["u"][:2], first[:2]) and np.array_equal(c["u"][2], u0[2])
        assert np.array_equal(c["u_old"][0], first[0]) and np.array_equal(c["u_old"][1:], uold0[1:])
        assert c["state"]["flags"].tolist() == [COPY_U | COPY_UOLD, INNER | HALVED | COPY_U, 0]
        # a later, unrelated trial: restart 1 accepts it, restart 0 must not see it
        c["trial"] = first + 0.25
        c["int_val"], c["tv_new"], c["J_new"] = np.array([NAN, 1.0, NAN]), np.array([NAN, 2.0, NAN]), \
            np.array([NAN, 4.0, NAN])
        d.update({m: _dev(c[m]) for m in ("trial", "int_val", "tv_new", "J_new")})
        torch.cuda.synchronize()
        _host_inner(c)
        _dev_inner(ctx, d)
        _assert_same(_download(ctx, d, K), c, "second")
        assert np.array_equal(c["u"][0], first[0]) and np.array_equal(c["u_old"][0], first[0])
        assert np.array_equal(c["u"][1], first[1] + 0.25) and np.array_equal(c["u_old"][1], first[1] + 0.25)
        assert c["words"] == (0, 1, 1) and c["state"]["flags"].tolist() == [0, HALVED | COPY_U | COPY_UOLD, 0]
        # no restart in its loop: the copy word is 0 and nothing moves
        before = copy.deepcopy(c)
        c["trial"] = first + 0.75
        d["trial"] = _dev(c["trial"])
        torch.cuda.synchronize()
        _host_inner(c)
        _dev_inner(ctx, d)
        _assert_same(_download(ctx, d, K), c, "third")
        assert c["words"] == (0, 1, 0) and np.all(c["state"]["flags"] & (COPY_U | COPY_UOLD) == 0)
        assert np.array_equal(c["u"], before["u"]) and np.array_equal(c["u_old"], before["u_old"])


# ---- the gate --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs():
    """The runtime-compiled ODE programs of the gate test, each compiled once, on first use."""
    from mioc.ode_device import ODEProgram, example_program

    import ode_bolza_problem as bp
    import ode_mixed_problem as mixed
    progs = {}
    make = {"euler": lambda: example_program("fishing", "euler"),
            "rk4": lambda: example_program("doubletank", "rk4"),
            "midpoint": lambda: example_program("vanderpol", "midpoint"),
            "mixed": lambda: ODEProgram(mixed.SOURCE, mixed.NY, mixed.NX, len(mixed.PARAMS), derive="all"),
            "bolza": lambda: ODEProgram(bp.SOURCE, bp.NY, bp.NX, bp.NP, integrator="heun", ndata=bp.ND, terminal=True,
                                        states=True)}

    def get(key):
        if key not in progs:
            progs[key] = make[key]()
        return progs[key]
    yield get
    for p in progs.values():
        p.close()


def _nan(*shape):
    import torch
    return torch.full(shape, NAN, dtype=torch.float64, device="cuda")


def _sos1(K, nt, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.eye(3)[rng.integers(0, 3, size=(K, nt))])


def _entry_dp(algo, key):
    def setup(ctx, programs):
        import torch
        from mioc.synth import CONFIGS, make_inputs
        cfg = CONFIGS[key]                                  # C5: 6 x 6 product levels, p = 1; C2: SOS1, p = Inf
        K, nt, Bdp = 3, 40, 8
        lt = cfg.levels()
        ins = [make_inputs(cfg, k=k, nt=nt, levels=lt) for k in range(K)]
        ddf, duo = (_dev(np.stack([i[j].T for i in ins])) for j in (1, 2))
        budgets = _dev([8, 3, 0], torch.int32)
        ctx.set_levels(lt)
        ctx.set_cost(cfg.p, cfg.beta)
        ctx.set_option(native.MIOC_OPT_ALGO, algo)
        _sync()
        ctx.bellman_batch_tensors(ddf, duo, Bdp, cfg.dt)
        assert ctx.last_algo() == algo

        def outputs():
            return [_nan(K, nt, lt.M), _nan(K), torch.full((K,), -7, dtype=torch.int32, device="cuda")] + \
                [_nan(K) for _ in range(4)]

        def call(o):
            ctx.backtrack_batch_budgets_tensors(budgets, o[0], o[1], o[2])
            ctx.pred_batch_tensors(*o[3:])
        return outputs, call, (ddf, duo, budgets)
    return setup


def _entry_ode_eval(ctx, programs):
    K, nt = 5, 24
    x = _dev(_sos1(K, nt, 3))
    return (lambda: [_nan(K), _nan(K, nt, 3)],
            lambda o: ctx.ode_eval_tensors(native.MIOC_ODE_FISHING, x, 0.0, 0.24, o[0], o[1]), x)


def _entry_program(name, key):
    def setup(ctx, programs):
        from mioc.ode_device import EXAMPLE_PARAMS, EXAMPLE_STATE0
        K, nt = 5, 24
        x = _dev(_sos1(K, nt, 4))
        prog = programs(key)
        return (lambda: [_nan(K), _nan(K, nt, 3)],
                lambda o: ctx.ode_program_eval_tensors(prog, x, 0.0, 0.24, EXAMPLE_STATE0[name], EXAMPLE_PARAMS[name],
                                                       o[0], o[1]), x)
    return setup


def _entry_mixed(ctx, programs):
    import ode_mixed_problem as mixed
    K, nt = 5, 24
    x = _dev(mixed.start(K, nt, 1))
    prog = programs("mixed")
    return (lambda: [_nan(K), _nan(K, nt, mixed.NX)],
            lambda o: ctx.ode_program_eval_mixed_tensors(prog, 1, x, 0.0, 3.0, mixed.STATE0, mixed.PARAMS, o[0], o[1]),
            x)


def _entry_bolza(ctx, programs):
    import ode_bolza_problem as bp
    K, nt = 5, 24
    rng = np.random.default_rng(5)
    x = _dev(np.stack([rng.integers(0, 3, size=(K, nt)), rng.integers(0, 2, size=(K, nt))], axis=2))
    data = _dev(bp.make_data(nt))
    prog = programs("bolza")
    return (lambda: [_nan(K), _nan(K, nt, bp.NX), _nan(K, nt + 1, bp.NY)],
            lambda o: ctx.ode_program_eval_tensors(prog, x, 0.0, 0.96, bp.STATE0, bp.PARAMS, o[0], o[1], data=data,
                                                   Y=o[2]), (x, data))


def _entry_heat(ctx, programs):
    from mioc.heat import HeatProblem
    hp = HeatProblem(n=5, nt=8)
    hp.setup(ctx)
    K = 3
    x = _dev(np.random.default_rng(6).integers(0, 6, size=(K, hp.nt, 2)))
    return lambda: [_nan(K), _nan(K, hp.nt, 2)], lambda o: ctx.heat_eval_tensors(x, o[0], o[1]), x


def _entry_conv(ctx, programs):
    from conv_ref import controls

    from mioc.conv import ConvProblem
    K, nt = 3, 17
    ConvProblem(nt=nt).setup(ctx)
    x = _dev(np.stack([c.T for c in controls(nt, K, seed=7)]))
    return lambda: [_nan(K), _nan(K, nt, 1)], lambda o: ctx.conv_eval_tensors(x, o[0], o[1]), x


def _entry_tv(ctx, programs):
    K, nt = 4, 9
    rng = np.random.default_rng(8)
    ctx.set_levels(LevelTable([[0, 1, 2], [0, 1]]))
    ctx.set_cost(1, BETA)
    u = _dev(np.stack([rng.integers(0, 3, size=(K, nt)), rng.integers(0, 2, size=(K, nt))], axis=2))
    return lambda: [_nan(K)], lambda o: ctx.tv_tensors(u, o[0]), u


GATED = {
    "dp_generic": _entry_dp(native.MIOC_ALGO_GENERIC, "C5"), "dp_fused": _entry_dp(native.MIOC_ALGO_FUSED, "C5"),
    "dp_fused_separable": _entry_dp(native.MIOC_ALGO_FUSED_SEPARABLE, "C5"),
    "dp_pinf": _entry_dp(native.MIOC_ALGO_PINF, "C2"),
    "ode_eval": _entry_ode_eval, "program_euler": _entry_program("fishing", "euler"),
    "program_rk4": _entry_program("doubletank", "rk4"), "program_midpoint": _entry_program("vanderpol", "midpoint"),
    "program_mixed": _entry_mixed, "program_bolza_states": _entry_bolza, "heat_eval": _entry_heat,
    "conv_eval": _entry_conv, "tv": _entry_tv,
}


def _raw(t):
    """A tensor's bytes: untouched means every byte, whatever the dtype."""
    return t.cpu().numpy().view(np.uint8).copy()


def _block(flags, words):
    import torch
    st = tm.new_state(len(flags))
    st["flags"][:] = flags
    return torch.from_numpy(tm.pack_state(st, words)).cuda()


@pytest.mark.parametrize("entry", list(GATED))
def test_closed_gate_skips_every_gated_entry(entry, programs):
    with native.Context(0) as ctx:
        outputs, call, _keep = GATED[entry](ctx, programs)
        ref, fresh = outputs(), [_raw(t) for t in outputs()]
        _sync()
        call(ref)                                           # detached: the result
        ctx.synchronize()
        ref = [_raw(t) for t in ref]
        assert all(not np.array_equal(r, f) for r, f in zip(ref, fresh)), "the detached call wrote nothing"
        state = _block([0, 0, 0], (0, 1, 1))                # the gate word is 0, the other two words are not
        out = outputs()
        _sync()
        ctx.trm_attach(state)
        try:
            call(out)                                       # MIOC_OK: anything else raises
            ctx.synchronize()
            for q, (t, f) in enumerate(zip(out, fresh)):
                assert np.array_equal(_raw(t), f), (entry, "output", q, "written behind a closed gate")
            state[0] = 1                                    # the gate word, in the same block
            _sync()
            call(out)
            ctx.synchronize()
            for q, (t, r) in enumerate(zip(out, ref)):
                assert np.array_equal(_raw(t), r), (entry, "output", q, "differs behind an open gate")
        finally:
            ctx.trm_attach(None)


def test_gate_follows_outer_begin_without_synchronisation(programs):
    """One stream, nothing in between: outer_begin on a block whose restarts have all stopped closes an open gate, and
    the eval behind it leaves its outputs alone; with one restart live it runs."""
    import torch
    K = 3
    with native.Context(0) as ctx:
        outputs, call, _keep = _entry_conv(ctx, programs)
        ref, fresh = outputs(), [_raw(t) for t in outputs()]
        tv_u, budgets = _dev(np.zeros(K)), _dev(np.zeros(K), torch.int32)
        _sync()
        call(ref)
        ctx.synchronize()
        ref = [_raw(t) for t in ref]
        for flags, runs in (([STOP] * K, False), ([STOP, STOP, HALVED], True)):
            state, out = _block(flags, (0 if runs else 1, 7, 7)), outputs()
            _sync()
            ctx.trm_attach(state)
            try:
                ctx.trm_outer_begin(state, tv_u, D0, B, budgets)
                call(out)
                assert ctx.trm_poll(state) == (runs, runs)
            finally:
                ctx.trm_attach(None)
            for t, r, f in zip(out, ref, fresh):
                assert np.array_equal(_raw(t), r if runs else f), (flags, runs)


# ---- argument checks -------------------------------------------------------------------------------------------------
def test_control_argument_errors():
    lib = native.load_library()
    assert lib.mioc_trm_state_bytes(0) == -1 and lib.mioc_trm_state_bytes(4097) == -1
    assert lib.mioc_trm_state_bytes(1) == 44 and lib.mioc_trm_state_bytes(4096) == 16 + 28 * 4096
    K = 5
    c = _case(_cycle(K))
    with native.Context(0) as ctx:
        d = _upload(c)
        _sync()
        p = {n: t.data_ptr() for n, t in d.items()}
        inner_ptrs = ("int_val", "tv_new", "J_new", "J_old", "J", "tv_u", "budgets", "decision")

        def outer(h=ctx.h, K=K, D0=D0, B=B, **null):
            a = {n: (None if n in null else p[n]) for n in ("block", "tv_u", "budgets")}
            return lib.mioc_trm_outer_begin_device(h, K, a["block"], a["tv_u"], D0, B, a["budgets"])

        def inner(h=ctx.h, K=K, sigma=SIGMA, kmax=KMAX, tau=TAU, B=B, n=3, **null):
            a = {m: (None if m in null else p[m]) for m in ("block", "trial", "u", "u_old") + inner_ptrs}
            return lib.mioc_trm_inner_end_device(h, K, a["block"], sigma, kmax, tau, B, *[a[m] for m in inner_ptrs], n,
                                                 a["trial"], a["u"], a["u_old"])

        def unchanged(tag):
            _assert_same(_download(ctx, d, K), c, tag)

        assert inner() == native.MIOC_ESTATE                # before mioc_set_cost
        unchanged("inner before set_cost")
        ctx.set_levels(LevelTable([[0, 1]]))
        ctx.set_cost(1, BETA)
        bad = [dict(K=0), dict(K=4097), dict(h=None), dict(B=-1), dict(B=2 ** 20 + 1)]
        for kw in bad + [dict(block=1), dict(tv_u=1), dict(budgets=1), dict(D0=math.inf), dict(D0=-math.inf),
                         dict(D0=NAN)]:
            assert outer(**kw) == native.MIOC_EINVAL, ("outer", kw)
            unchanged(("outer", kw))
        for kw in bad + [{m: 1} for m in ("block", "trial", "u", "u_old") + inner_ptrs[:-1]] + \
                [dict(tau=0.0), dict(tau=-0.1), dict(tau=NAN), dict(kmax=-1), dict(n=0)]:
            assert inner(**kw) == native.MIOC_EINVAL, ("inner", kw)
            unchanged(("inner", kw))
        # the same arguments, none of them bad: accepted (d_decision may be NULL)
        assert outer() == native.MIOC_OK and inner(decision=1) == native.MIOC_OK
        ctx.synchronize()


# ---- end to end across the stride ------------------------------------------------------------------------------------
def test_trm_batch_beyond_one_block():
    """TRM_batch on 1030 restarts of the convolution problem: 6 of them belong to the workgroup's second pass.  Rows
    1024..1029 and 0..5 equal TRM_batch on those starts alone; restarts 0, 1023, 1024, 1029 equal the host loop."""
    import torch
    from mioc.conv import ConvObj, ConvProblem
    from mioc.trm_batch import TRM_batch
    K, nt = 1030, 64
    cp = ConvProblem(nt=nt)
    par = mioc.TRM_parameters(beta=1e-4, Delta0=0.125, p=1, maxiter=3, kmax=3)
    assert math.floor(par.Delta0 / cp.tau) == 4
    with native.Context(0) as ctx:
        ctx.set_levels(LevelTable(cp.levels))
        x0 = torch.empty(K, nt, 1, dtype=torch.float64, device="cuda")
        ctx.rand_start_tensor(x0, seed=9)
        ctx.synchronize()
    log = []
    vals, u, iters = TRM_batch(cp, par, x0=x0, log=log)
    ub = u.cpu().numpy()
    decisions = np.concatenate([e[4] for e in log])
    counts = {name: int(np.sum(decisions == v)) for name, v in (("accept", 0), ("halve", 1), ("stop", 2))}
    print(f"K = {K}: decisions {counts}, outer iterations {np.bincount(iters).tolist()}")
    assert counts["halve"] >= 1 and counts["accept"] >= 1      # else the run did not exercise the control
    for lo in (1024, 0):
        v2, u2, i2 = TRM_batch(cp, par, x0=x0[lo:lo + 6].contiguous())
        assert np.array_equal(tm.bits(vals[lo:lo + 6]), tm.bits(v2)), (lo, vals[lo:lo + 6], v2)
        assert np.array_equal(ub[lo:lo + 6], u2.cpu().numpy()) and np.array_equal(iters[lo:lo + 6], i2), lo
    for k in (0, 1023, 1024, 1029):
        obj = ConvObj(cp)
        Jk = mioc.TRM(obj, par, x0=x0[k].cpu().numpy().T.copy())
        assert Jk == vals[k] and math.isfinite(Jk), (k, Jk, vals[k])
        assert np.array_equal(obj.x, ub[k].T), k
        obj.ctx.close()
