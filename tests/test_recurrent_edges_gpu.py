"""GPU: recurrent Q-networks at the edges of their kernels' schedules and in stacks, through the C ABI, against the fp64 reference for any recurrent
chain (tests/recurrent_reference.py).  Every case runs several recurrent batch_train! steps on drawn sequences (episodes shorter than T, so the masks
bite) and compares, at every step, the loss, each parameter block's gradient, grad_norm and the parameters after Adam (an fp64 Adam carried across
the steps on the engine's own gradients).  The schedule each case takes (whole-sequence kernels or per-step launches) is asserted from the launch
names against the fit rules restated below; GRU and RNN layers on the whole-sequence kernels are also bit-identical to their per-step schedule
(DQN_GRU_STEPWISE / DQN_RNN_STEPWISE), LSTM networks to the C twin.  Stacks of recurrent layers also run graph / eager / a second engine bit for bit,
and carry the policy's per-layer state (hiddenstates / sethiddenstates! / resetstate!)."""
import importlib
import types

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import recurrent_reference as R
import ref
from drqn_common import draws, feed, make_episodes
from gru_reference import param_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    p = ge.load_package(); p.lib()
    return p, importlib.import_module(p.__name__ + ".nn")


# ------------------------------------------------------------------ the fit rules of drqn.hip / gru.hip / rnn.hip, restated
def _cb(H, B):
    cb = max(1, 256 // H); cb = min(cb, B)
    while B % cb:
        cb -= 1
    return cb


def lstm_seq_fits(H, B, T):
    cb = _cb(H, B)
    fwd, bwd = H * 4 * H + 4 * H + 7 * H * cb, H * (4 * H + 1) + 6 * H * cb
    return fwd <= 16384 and bwd <= 16384 and (H * cb) % 64 == 0 and H * cb <= 256 and T <= 64


def gru_seq_fits(H, B, T):
    cb = _cb(H, B)
    fwd, bwd = H * 3 * H + 3 * H + 4 * H * cb, H * (3 * H + 1) + 4 * H * cb
    return fwd <= 16384 and bwd <= 16384 and (H * cb) % 64 == 0 and H * cb <= 256 and T <= 64


def rnn_seq_fits(H, B, T):
    cb = _cb(H, B)
    fwd, bwd = H * H + H + 2 * H * cb, H * (H + 1) + 2 * H * cb
    return 4 * fwd <= 80 * 1024 and 4 * bwd <= 80 * 1024 and H * cb <= 1024 and T <= 64


FITS = {"lstm": lstm_seq_fits, "gru": gru_seq_fits, "rnn": rnn_seq_fits}
KERNELS = {"seq": ("{}_seq", "{}_bwd_seq"), "step": ("{}_step", "{}_bwd")}


def schedules(net, nn, B, T):
    """layer index -> "seq" | "step" for every recurrent layer, by the fit rules"""
    return {i: "seq" if FITS[l.kind](l.n_out, B, T) else "step" for i, l in enumerate(nn.all_layers(net)) if l.kind in R.RECURRENT}


def assert_schedule(h, net, nn, want):
    launched = {tuple(n.rsplit("_dense", 1)) for n, _ in h.profile_step(max_entries=4096)}      # (op, layer index); T = 65 per-step: ~140 launches
    for i, s in want.items():
        kind = nn.all_layers(net)[i].kind
        other = "step" if s == "seq" else "seq"
        for op in KERNELS[s]:
            assert (op.format(kind), str(i)) in launched, (i, kind, s, sorted(launched))
        for op in KERNELS[other]:
            assert (op.format(kind), str(i)) not in launched, (i, kind, s, sorted(launched))


# ------------------------------------------------------------------ one case: engine + ring + parameters, deterministic from the case
class Case(types.SimpleNamespace):
    """mk(nn) -> net; E obs features; nA actions; B, T; gamma, double_q; mfma, graph; want: expected schedule of the recurrent layers (or None)"""


def _params(nn, net, seed, scale=0.05):
    rng = np.random.default_rng(seed)
    n = nn.glorot_params(net, seed=3).size
    p_on = (nn.glorot_params(net, seed=3) + scale * rng.standard_normal(n)).astype(np.float32)      # non-zero biases and state0
    p_tg = (nn.glorot_params(net, seed=4) + scale * rng.standard_normal(n)).astype(np.float32)
    return p_on, p_tg


def _episodes(c, seed):
    cap = max(12, c.B + 4)
    eps = make_episodes(types.SimpleNamespace(obs_shape=(c.E,), n_actions=c.nA), cap + 3, c.T, np.random.default_rng(seed))     # the ring wraps
    ring = [None] * cap
    for i, ep in enumerate(eps):
        ring[i % cap] = ep
    return cap, eps, ring


def make_engine(mods, c, graph=None, plan=None, env=None, monkeypatch=None, twin=False):
    """the case's engine (twin: the C twin instead), its replay filled and its parameters set; env: a switch set while the engine is created"""
    pkg, nn = mods
    net = c.mk(nn)
    layers, dueling = nn.lower(net)
    cap, eps, ring = _episodes(c, c.seed)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=c.E, dueling=int(dueling), buffer_size=cap, recurrence=1, trace_length=c.T, learning_rate=1e-3,
                             prioritized_replay=0, use_mfma=c.mfma, use_graph=c.graph if graph is None else graph, seed=5, gamma=c.gamma, double_q=c.double_q)
    if twin:
        h = ref.Twin(layers, hp, plan=plan, threads=4)
    elif env:
        monkeypatch.setenv(env, "1")
        try:
            h = pkg.Engine(layers, hp, plan=plan, device=0)
        finally:
            monkeypatch.delenv(env, raising=False)
    else:
        h = pkg.Engine(layers, hp, plan=plan, device=0)
    feed(h, eps)
    p_on, p_tg = _params(nn, net, c.seed)
    h.set_params(p_on, 0); h.set_params(p_tg, 1)
    return net, h, ring, layers, hp, eps, (p_on, p_tg)


def multi_launch_plan(mods, c):
    """the default plan, but never the fused column-parallel LSTM step (drqn_cols.hip, covered by test_drqn_gpu.py): the LSTM's own schedules"""
    net, h, *_ = make_engine(mods, c)
    plan = [(p[0], p[1], max(p[2], 0)) for p in h.plan()]
    h.close()
    return plan


def run_checked(mods, c, steps=3, plan=None):
    """steps train steps against the fp64 reference; returns the engine (open) and what the steps produced"""
    pkg, nn = mods
    net, h, ring, layers, hp, eps, (p_on, p_tg) = make_engine(mods, c, plan=plan)
    gamma = float(np.float32(c.gamma))
    adam = R.Adam(p_on.size)
    rng = np.random.default_rng(c.seed + 100)
    out = []
    for k in range(steps):
        p_prev = h.get_params(0)
        idx, start = draws(ring, c.B, rng)
        batch = h.episode_get_batch(idx, start)
        o = R.train_grads(net, nn, p_prev, p_tg, batch, gamma, bool(c.double_q))
        loss, gn = h.train_step_drqn(idx, start)
        g = h.get_grads()
        np.testing.assert_allclose(loss, o["loss"], rtol=2e-5, atol=1e-7, err_msg=f"{c.name} step {k}: loss")
        R.check_grads(net, nn, g, o["grads"], live=k == 0)
        np.testing.assert_allclose(gn, o["grad_norm"], rtol=1e-4, err_msg=f"{c.name} step {k}: grad_norm")
        R.check_params(h.get_params(0), adam.step(p_prev, g))
        out.append(((loss, gn), idx, start))
    return net, h, ring, out


def replay(h, out):
    """the same draws on another engine: (loss, grad_norm) per step"""
    return [h.train_step_drqn(idx, start) for _, idx, start in out]


def same_state(a, b):
    np.testing.assert_array_equal(a.get_grads(), b.get_grads())
    np.testing.assert_array_equal(a.get_params(0), b.get_params(0))
    for x, y in zip(a.get_adam_state(), b.get_adam_state()):
        np.testing.assert_array_equal(x, y)


def check_case(mods, c, monkeypatch):
    pkg, nn = mods
    net = c.mk(nn)
    kinds = {l.kind for l in nn.all_layers(net)}
    plan = multi_launch_plan(mods, c) if "lstm" in kinds else None
    want = schedules(net, nn, c.B, c.T)
    if c.want is not None:
        assert [want[i] for i in sorted(want)] == c.want, (c.name, want)      # the table states the schedule the fit rules give
    net, h, ring, out = run_checked(mods, c, plan=plan)
    # the companion: per-step schedule (GRU / RNN on the whole-sequence kernels) or the C twin (LSTM), bit for bit
    envs = {l.kind: {"gru": "DQN_GRU_STEPWISE", "rnn": "DQN_RNN_STEPWISE"}[l.kind] for i, l in enumerate(nn.all_layers(net)) if want.get(i) == "seq" and l.kind != "lstm"}
    for env in envs.values():
        _, h2, *_ = make_engine(mods, c, plan=plan, env=env, monkeypatch=monkeypatch)
        assert replay(h2, out) == [o[0] for o in out], (c.name, env)
        same_state(h, h2)
        h2.close()
    if "lstm" in kinds and not kinds & {"gru", "rnn"}:      # the twin runs Dense, Conv and LSTM layers
        _, tw, *_ = make_engine(mods, c, plan=plan, twin=True)
        assert replay(tw, out) == [o[0] for o in out], c.name
        same_state(h, tw)
        tw.close()
    assert_schedule(h, net, nn, want)       # profile_step runs one more (eager) step: last
    h.close()
    return want


# ------------------------------------------------------------------ a. the boundary table
def _one(kind, H, E=6, nA=3, act=None):
    def mk(nn):
        cell = {"lstm": lambda: nn.LSTM(E, H), "gru": lambda: nn.GRU(E, H), "rnn": lambda: nn.RNN(E, H, getattr(nn, act or "tanh"))}[kind]()
        return nn.Chain(cell, nn.Dense(H, nA))
    return mk


def _case(name, kind, H, B, T, want, act=None, mfma=1, graph=1, gamma=0.95, double_q=1, seed=7):
    assert T * B <= 65536
    return Case(name=name, mk=_one(kind, H, act=act), E=6, nA=3, B=B, T=T, gamma=gamma, double_q=double_q, mfma=mfma, graph=graph, want=[want], seed=seed)


BOUNDARY = [
    # RNN: the LDS fit rule (80 KB per kernel; past 64 KB through the raised limit), whole waves and tails
    _case("rnn_h124_64k", "rnn", 124, 4, 3, "seq", act="tanh"),                          # cb 2: 63984 B, within the default 64 KB
    _case("rnn_h126_raised", "rnn", 126, 4, 3, "seq", act="relu", mfma=0, graph=0),      # cb 2: 66024 B, raised LDS limit
    _case("rnn_h141_last", "rnn", 141, 3, 4, "seq", act="sigmoid", double_q=0),         # cb 1: 81216 B, the last whole-sequence size; 51 idle lanes in wave 3
    _case("rnn_h142_step", "rnn", 142, 3, 3, "step", act="tanh", mfma=0),               # cb 1: 82360 B > 80 KB
    _case("rnn_h33_b7_tail", "rnn", 33, 7, 5, "seq", act="identity", graph=0),          # H*cb = 231: a partial last wave
    _case("rnn_h100_b3_tail", "rnn", 100, 3, 4, "seq", act="tanh", mfma=0),             # cb 1 (3 % 2): 100 of 128 lanes
    _case("rnn_t1", "rnn", 16, 4, 1, "seq", act="relu"),
    _case("rnn_t8", "rnn", 32, 8, 8, "seq", act="tanh", graph=0),                       # the prefetching form's last T
    _case("rnn_t9", "rnn", 32, 8, 9, "seq", act="sigmoid", mfma=0),                     # one step ahead
    _case("rnn_t64", "rnn", 16, 4, 64, "seq", act="tanh"),
    _case("rnn_t65", "rnn", 16, 4, 65, "step", act="tanh", graph=0),
    # GRU: cb shrinks to divide B, the % 64 rule, LDS, and the k_gru_seq<8 / 32 / 64> bounds
    _case("gru_h64_b6", "gru", 64, 6, 4, "seq"),                                        # cb 4 -> 3: H*cb = 192
    _case("gru_h80_step", "gru", 80, 4, 3, "step", mfma=0, graph=0),                    # LDS
    _case("gru_h16_b5_step", "gru", 16, 5, 4, "step"),                                  # H*cb = 80: not whole waves
    _case("gru_t1", "gru", 32, 8, 1, "seq", mfma=0),
    _case("gru_t8", "gru", 32, 8, 8, "seq", graph=0),
    _case("gru_t9", "gru", 32, 8, 9, "seq"),
    _case("gru_t64", "gru", 16, 4, 64, "seq", mfma=0),
    _case("gru_t65", "gru", 16, 4, 65, "step"),
    # LSTM (the multi-launch program: lstm_seq / lstm_step)
    _case("lstm_h32", "lstm", 32, 8, 5, "seq"),
    _case("lstm_h48_b6_step", "lstm", 48, 6, 4, "step", mfma=0),                        # cb 5 -> 3: H*cb = 144
    _case("lstm_h64_step", "lstm", 64, 4, 3, "step", graph=0),                          # LDS
    _case("lstm_t1", "lstm", 32, 8, 1, "seq", graph=0),
    _case("lstm_t8", "lstm", 32, 8, 8, "seq", mfma=0),
    _case("lstm_t9", "lstm", 32, 8, 9, "seq"),
    _case("lstm_t64", "lstm", 16, 4, 64, "seq", mfma=0, graph=0),
    _case("lstm_t65", "lstm", 16, 4, 65, "step"),
]


@pytest.mark.parametrize("c", BOUNDARY, ids=[c.name for c in BOUNDARY])
def test_boundary_case_vs_fp64_reference(mods, c, monkeypatch):
    check_case(mods, c, monkeypatch)


# ------------------------------------------------------------------ b. seeded random configs
def _random_case(nn, seed):
    """kind, H, B, T, an optional Dense before / after the recurrent layer, dueling, double_q, gamma; redrawn while a block's fp64 gradient is negligible"""
    for tries in range(20):
        rng = np.random.default_rng(1000 * seed + tries)
        kind = ["lstm", "gru", "rnn"][rng.integers(3)]
        H = int(rng.choice({"lstm": [8, 16, 24, 32, 40, 64], "gru": [8, 16, 21, 32, 48, 64], "rnn": [5, 16, 32, 47, 64, 96, 130]}[kind]))
        B, T = int(rng.integers(1, 13)), int(rng.choice([1, 2, 3, 5, 7, 8, 9, 12, 16, 32, 33]))
        E, nA = int(rng.integers(3, 10)), int(rng.integers(2, 6))
        act = int(rng.integers(4))
        pre = int(rng.integers(6, 17)) if rng.random() < 0.4 else 0
        post = int(rng.integers(6, 17)) if rng.random() < 0.4 else 0
        pre_act, post_act = int(rng.integers(4)), int(rng.integers(4))
        dueling = bool(rng.random() < 0.5)
        c = Case(name=f"random{seed}", E=E, nA=nA, B=B, T=T, gamma=float(rng.choice([0.5, 0.9, 0.99])), double_q=int(rng.integers(2)),
                 mfma=int(rng.integers(2)), graph=int(rng.integers(2)), want=None, seed=seed)

        def mk(nn, kind=kind, H=H, E=E, nA=nA, act=act, pre=pre, post=post, pre_act=pre_act, post_act=post_act, dueling=dueling):
            n_in = pre or E
            cell = {"lstm": lambda: nn.LSTM(n_in, H), "gru": lambda: nn.GRU(n_in, H), "rnn": lambda: nn.RNN(n_in, H, act)}[kind]()
            ls = ([nn.Dense(E, pre, pre_act)] if pre else []) + [cell] + ([nn.Dense(H, post, post_act), nn.Dense(post, nA)] if post else [nn.Dense(H, nA)])
            m = nn.Chain(*ls)
            return nn.create_dueling_network(m) if dueling else m
        c.mk = mk
        net = mk(nn)
        _, _, ring = _episodes(c, seed)
        p_on, p_tg = _params(nn, net, seed)
        idx, start = draws(ring, B, np.random.default_rng(seed + 100))
        g = R.train_grads(net, nn, p_on, p_tg, R.sample_batch(ring, idx, start, T, (E,)), float(np.float32(c.gamma)), bool(c.double_q))["grads"]
        if not R.dead_blocks(net, nn, g):
            c.name += f"_{kind}{H}_b{B}_t{T}"
            return c
    raise AssertionError(f"random config {seed}: no draw without a negligible gradient block")


N_RANDOM = 24


@pytest.mark.parametrize("seed", range(N_RANDOM))
def test_random_config_vs_fp64_reference(mods, seed, monkeypatch):
    c = _random_case(mods[1], seed)
    check_case(mods, c, monkeypatch)


# ------------------------------------------------------------------ c. stacks of recurrent layers
STACKS = {      # name -> (builder, E, nA, B, T, gamma, double_q)
    "gru_rnnrelu_dense": (lambda nn: nn.Chain(nn.GRU(6, 16), nn.RNN(16, 12, nn.relu), nn.Dense(12, 4)), 6, 4, 6, 5, 0.95, 1),
    "dense_lstm_gru_dense_dueling": (lambda nn: nn.create_dueling_network(nn.Chain(nn.Dense(6, 10, nn.tanh), nn.LSTM(10, 16), nn.GRU(16, 12), nn.Dense(12, 5))), 6, 5, 8, 6, 0.9, 1),
    "rnnsigmoid_rnntanh_b32": (lambda nn: nn.Chain(nn.RNN(8, 24, nn.sigmoid), nn.RNN(24, 16, nn.tanh), nn.Dense(16, 3)), 8, 3, 32, 8, 0.99, 0),
    "lstm_lstm": (lambda nn: nn.Chain(nn.LSTM(6, 16), nn.LSTM(16, 8), nn.Dense(8, 4)), 6, 4, 8, 5, 0.95, 1),
    "gru80_step_gru16_seq": (lambda nn: nn.Chain(nn.GRU(10, 80), nn.GRU(80, 16), nn.Dense(16, 3)), 10, 3, 4, 4, 0.9, 1),
    "gru_densrelu_dense": (lambda nn: nn.Chain(nn.GRU(6, 16), nn.Dense(16, 12, nn.relu), nn.Dense(12, 4)), 6, 4, 6, 4, 0.95, 0),
}


def _stack_case(name, mfma, graph=1):
    mk, E, nA, B, T, gamma, dq = STACKS[name]
    return Case(name=name, mk=mk, E=E, nA=nA, B=B, T=T, gamma=gamma, double_q=dq, mfma=mfma, graph=graph, want=None, seed=11)


@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("name", list(STACKS))
def test_stack_vs_fp64_reference_graph_eager_two_engines(mods, name, mfma, monkeypatch):
    pkg, nn = mods
    c = _stack_case(name, mfma)
    want = check_case(mods, c, monkeypatch)
    if name == "gru80_step_gru16_seq":
        assert want == {0: "step", 1: "seq"}        # one stack on both schedules
    # graph, eager and a second graph engine: the same bits
    plan = multi_launch_plan(mods, c) if any(l.kind == "lstm" for l in nn.all_layers(c.mk(nn))) else None
    res = []
    for graph in (1, 0, 1):
        net, h, ring, *_ = make_engine(mods, c, graph=graph, plan=plan)
        rng = np.random.default_rng(3)
        ls = []
        for k in range(6):
            ls.append(h.train_step_drqn(*draws(ring, c.B, rng)))
            if k == 2:
                h.sync_target()
        res.append((ls, h))
    for ls, h in res[1:]:
        assert ls == res[0][0]
        same_state(res[0][1], h)
        np.testing.assert_array_equal(h.get_params(1), res[0][1].get_params(1))
    for _, h in res:
        h.close()


# ------------------------------------------------------------------ d. the policy's per-layer state on stacks
@pytest.mark.parametrize("name", ["gru_rnnrelu_dense", "dense_lstm_gru_dense_dueling", "lstm_lstm", "gru80_step_gru16_seq"])
def test_stack_policy_state(mods, name):
    pkg, nn = mods
    c = _stack_case(name, 1)
    net, h, ring, layers, hp, eps, (p_on, p_tg) = make_engine(mods, c)
    S = 3
    rng = np.random.default_rng(23)
    xs = [rng.random((S, c.E)).astype(np.float32) for _ in range(6)]
    t64 = lambda x: torch.tensor(x, dtype=torch.float64)
    arrs = param_arrays(net, nn, p_on)
    with torch.no_grad():
        hs = R.init_state(net, nn, arrs, S)
        want = [R.q_step(net, nn, arrs, t64(x), hs).numpy() for x in xs[:4]]
    h.reset_state()
    for k in range(4):      # the carried state over several forwards
        np.testing.assert_allclose(h.forward(xs[k]), want[k], atol=1e-5, rtol=1e-5, err_msg=f"{name}: forward {k}")
    # the documented layout: per recurrent layer in layer order, (h, c) for an LSTM, h for a GRU or an RNN, each (out, streams)
    saved = h.get_hidden(S)
    ref_l = R.hidden_layout(net, nn, hs)
    rl = R.recurrent_layers(net, nn)
    kinds = [nn.all_layers(net)[i].kind for i in rl]
    assert len(saved) == len(ref_l) == len(kinds)
    assert h.hidden_size(S) == sum((2 if k == "lstm" else 1) * nn.all_layers(net)[i].n_out * S for i, k in zip(rl, kinds))
    for k, got, w in zip(kinds, saved, ref_l):
        if k == "lstm":
            assert isinstance(got, tuple) and len(got) == 2
            for a, b in zip(got, w):
                assert a.shape == b.shape; np.testing.assert_allclose(a, b, atol=1e-5, rtol=1e-5)
        else:
            assert isinstance(got, np.ndarray) and got.shape == w.shape
            np.testing.assert_allclose(got, w, atol=1e-5, rtol=1e-5)
    # set_hidden of a MODIFIED state: the next Q (and state) is the reference's step from that state
    mod = [tuple((0.5 * x + 0.1 * np.roll(x, 1, axis=1)).astype(np.float32) for x in st) if isinstance(st, tuple) else (0.5 * st - 0.2).astype(np.float32) for st in saved]
    h.set_hidden(mod)
    q = h.forward(xs[4])
    with torch.no_grad():
        hm = R.state_from_layout(net, nn, mod)
        qw = R.q_step(net, nn, arrs, t64(xs[4]), hm).numpy()
        qs = R.q_step(net, nn, arrs, t64(xs[4]), R.state_from_layout(net, nn, saved)).numpy()
    np.testing.assert_allclose(q, qw, atol=1e-5, rtol=1e-5)
    assert np.abs(qw - qs).max() > 1e-3, "the modified state must change Q"
    for k, got, w in zip(kinds, h.get_hidden(S), R.hidden_layout(net, nn, hm)):
        for a, b in zip(got if k == "lstm" else (got,), w if k == "lstm" else (w,)):
            np.testing.assert_allclose(a, b, atol=1e-5, rtol=1e-5)
    # reset_state: state0 of every layer, broadcast over the streams, and the first Q again
    h.reset_state()
    for i, k, got in zip(rl, kinds, h.get_hidden(S)):
        a = param_arrays(net, nn, h.get_params(0))[i]
        st0 = (a[3], a[4]) if k == "lstm" else (a[3],)
        for x, s0 in zip(got if k == "lstm" else (got,), st0):
            np.testing.assert_array_equal(x, np.repeat(s0.numpy().astype(np.float32)[:, None], S, axis=1))
    np.testing.assert_allclose(h.forward(xs[0]), want[0], atol=1e-5, rtol=1e-5)
    h.close()


# ------------------------------------------------------------------ e. caller-supplied summation plans (the feed-forward table: tests/plan_edges_common.py)
def _state(h):
    return [h.get_grads(), h.get_params(0)]


def plan_case_checked(mods, c, plan, default, launched=(), twin=True, steps=2):
    """the case under `plan`: against the fp64 reference; plan() returns the plan; bit for bit the C twin (LSTM networks) and the other schedule (use_graph); at least one bit
    of the gradient or the parameters differs from the run under `default`; `launched` names show in profile_step"""
    assert plan != default, c.name
    net, h, ring, out = run_checked(mods, c, steps=steps, plan=plan)
    assert h.plan() == plan, (c.name, h.plan())
    others = [make_engine(mods, c, plan=plan, graph=1 - c.graph)[1]] + ([make_engine(mods, c, plan=plan, twin=True)[1]] if twin else [])
    for o in others:
        assert replay(o, out) == [x[0] for x in out], c.name
        same_state(h, o)
        o.close()
    d = make_engine(mods, c, plan=default)[1]
    replay(d, out)
    assert any(not np.array_equal(a, b) for a, b in zip(_state(h), _state(d))), f"{c.name}: the plan gives the default plan's bits: the case tests nothing"
    d.close()
    names = {n for n, _ in h.profile_step(max_entries=4096)}
    assert set(launched) <= names, (c.name, sorted(names))
    h.close()
    return names


def default_plan_of(mods, c):
    net, h, *_ = make_engine(mods, c)
    plan = h.plan(); h.close()
    return plan


@pytest.mark.parametrize("kc", [20, 32, 24, 7])
def test_fused_column_step_with_a_chunked_head(mods, kc):
    """Chain(LSTM(6, 40), Dense(40, 3)) on the fused column-parallel step (drqn_cols.hip reads the head's chunk count and length): head chunks 20 + 20, 32 + 8, 24 + 16 and
    5 x 7 + 5.  (H = 40 is the widest LSTM whose double-Q step fits the fused launch's LDS rule, drqn_fused_cg, at these sizes; at H = 64 both networks' parameters alone pass it.)"""
    c = _case(f"lstm_cols_head_kc{kc}", "lstm", 40, 4, 3, None)
    default = default_plan_of(mods, c)
    assert all(p[2] < 0 for p in default) and default[1][0] == 0, default      # the fused step (column-group dW chunks), head unsplit
    plan = [default[0], (kc, default[1][1], default[1][2])]
    plan_case_checked(mods, c, plan, default, launched=("drqn_cols", "adam"))


@pytest.mark.parametrize("H, B, dq, groups", [(8, 12, 0, (1, 2, 3, 4, 6, 12)), (16, 8, 1, (1, 2, 4))], ids=["h8_b12", "h16_b8_doubleq"])
def test_every_admissible_column_group_size(mods, H, B, dq, groups):
    """dw_kc = -cg on every layer for each divisor cg of B with nset * 4 * H * cg <= 1024 (one thread per sequence set, gate, column and unit): group sizes the default plan
    never picks (it stops at 4), sizes that are no power of two, and the whole batch as one group.  Found here, by reading before running: the kernel's per-column tables held
    four entries while build_program admitted groups up to 16 columns; they are sized by that bound now (DRQN_COLS_MAX_CG)."""
    nset = 3 if dq else 2
    assert groups == tuple(g for g in range(1, B + 1) if B % g == 0 and nset * 4 * H * g <= 1024)
    c = _case(f"lstm_cols_h{H}_b{B}", "lstm", H, B, 3, None, double_q=dq)
    default = default_plan_of(mods, c)
    assert default[0][2] < 0 and -default[0][2] in groups, default
    for cg in groups:
        plan = [(p[0], p[1], -cg) for p in default]
        if plan == default:
            continue
        c.name = f"lstm_cols_h{H}_b{B}_cg{cg}"
        plan_case_checked(mods, c, plan, default, launched=("drqn_cols", "adam"))


def test_column_group_beyond_the_workgroups_lds_is_refused_by_name(mods):
    """a divisor of B the thread-count rule admits (2 * 4 * 8 * 16 = 1024) whose group does not fit one workgroup's LDS (T = 64 rows of 64 features for 16 columns, twice):
    refused when the program is built, before anything is launched, with the group and the bytes named -- not left to a launch that cannot be configured"""
    pkg, nn = mods
    c = Case(name="lstm_cols_lds", mk=_one("lstm", 8, E=64), E=64, nA=3, B=16, T=64, gamma=0.95, double_q=0, mfma=1, graph=1, want=None, seed=7)
    default = default_plan_of(mods, c)
    assert all(p[2] == -1 for p in default), default      # the default plan's group fits
    net, h, ring, *_ = make_engine(mods, c, plan=[(p[0], p[1], -16) for p in default])
    with pytest.raises(pkg.DQNError, match=r"column-group dW chunks \(dw_kc = -16\): a group of 16 batch columns needs \d+ bytes of LDS"):
        h.train_step_drqn(*draws(ring, c.B, np.random.default_rng(1)))
    h.close()


MULTI_LAUNCH_DW = [      # (case, dw_kc on every layer, a launch that must show)
    (_case("lstm_h64_dw32", "lstm", 64, 8, 8, None), 32, "dw_wh_dense0"),       # T * B = 64 columns in chunks of 32: Wh | junk (65 x 256 > 16384) on the LDS-tiled dW, Wi | b and the head as VALU tasks
    (_case("lstm_h16_dw24", "lstm", 16, 8, 8, None, graph=0), 24, "bwd_valu_dense0"),      # ragged: 24 + 24 + 16
    (_case("gru_h16_dw10", "gru", 16, 6, 4, None), 10, "bwd_valu_dense0"),      # 24 columns: 10 + 10 + 4; the GRU's junk row is cleared in every slab
    (_case("rnn_h32_dw32", "rnn", 32, 8, 8, None, act="tanh", mfma=0), 32, "bwd_valu_dense0"),
]


@pytest.mark.parametrize("c, kc, launch", MULTI_LAUNCH_DW, ids=[x[0].name for x in MULTI_LAUNCH_DW])
def test_multi_launch_program_with_dw_chunks(mods, c, kc, launch):
    """one LSTM, one GRU and one RNN network on the multi-launch recurrent program with dw_kc > 0: the T * B sample columns of every dW / db (Wi | b, Wh | junk, the head) in chunks"""
    pkg, nn = mods
    default = [(p[0], p[1], max(p[2], 0)) for p in default_plan_of(mods, c)]      # never the fused column step
    plan = [(p[0], p[1], kc) for p in default]
    plan_case_checked(mods, c, plan, default, launched=(launch,), twin=c.name.startswith("lstm"))
