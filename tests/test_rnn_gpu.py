"""GPU: recurrent Q-networks with Flux RNN layers (Recur(RNNCell)) through the C ABI -- one recurrent batch_train! (src/solver.jl:239-287) against an
fp64 torch reference (tests/rnn_reference.py) at fp32 round-off for each cell activation, both recurrence schedules (whole-sequence kernels / per-step
launches, DQN_RNN_STEPWISE) and both launch modes bit for bit, the policy's Recur state (hiddenstates / sethiddenstates! / resetstate!), resume, BSON
and the refusals."""
import importlib
import types

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from drqn_common import draws, feed, make_episodes
from rnn_reference import check_step, drqn_train_step, init_state, param_arrays, q_step

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    p = ge.load_package(); p.lib()
    return p, importlib.import_module(p.__name__ + ".nn")


# name -> (network builder, obs features, n_actions, B, T, kw)
NETS = {
    "cfg4_rnn_plain": (lambda nn: nn.Chain(nn.flattenbatch, nn.RNN(25, 32), nn.Dense(32, 4)), 25, 4, 32, 8, dict(gamma=0.99, double_q=1)),      # whole-sequence kernels, T <= 8
    "dense_rnn_relu_dueling": (lambda nn: nn.create_dueling_network(nn.Chain(nn.Dense(6, 12, nn.relu), nn.RNN(12, 16, nn.relu), nn.Dense(16, 5))), 6, 5, 6, 5, dict(gamma=0.95, double_q=1)),
    "rnn_sigmoid_single_q": (lambda nn: nn.Chain(nn.RNN(6, 8, nn.sigmoid), nn.Dense(8, 3)), 6, 3, 5, 3, dict(gamma=0.9, double_q=0)),
    "rnn_identity_single_q": (lambda nn: nn.Chain(nn.RNN(6, 8, nn.identity), nn.Dense(8, 3)), 6, 3, 5, 3, dict(gamma=0.9, double_q=0)),
    "rnn16_dueling_b16": (lambda nn: nn.create_dueling_network(nn.Chain(nn.RNN(16, 32), nn.Dense(32, 4))), 16, 4, 16, 10, dict(gamma=0.95, double_q=1)),   # T > 8
    "rnn128_big_lds": (lambda nn: nn.Chain(nn.RNN(8, 128), nn.Dense(128, 3)), 8, 3, 4, 3, dict(gamma=0.9, double_q=1)),      # whole-sequence kernels past 64 KB of LDS
    "rnn_wide_stepwise": (lambda nn: nn.Chain(nn.RNN(10, 160), nn.Dense(160, 3)), 10, 3, 4, 3, dict(gamma=0.9, double_q=0)),      # Wh 160 x 160 exceeds rnn_seq_fits
}
SEQ_NETS = [n for n in NETS if n != "rnn_wide_stepwise"]      # the nets whose default schedule is the whole-sequence kernels


def build(mods, name, mfma=1, graph=1, plan=None, seed=5, obs_dtype=None):
    pkg, nn = mods
    mk, E, nA, B, T, kw = NETS[name]
    net = mk(nn)
    layers, dueling = nn.lower(net)
    cap = max(12, B + 4)
    hp = pkg.default_hparams(batch_size=B, n_actions=nA, obs_c=E, dueling=int(dueling), buffer_size=cap, recurrence=1, trace_length=T, learning_rate=1e-3,
                             prioritized_replay=0, use_mfma=mfma, use_graph=graph, seed=seed, **kw)
    if obs_dtype is not None:
        hp.obs_dtype = obs_dtype
    h = pkg.Engine(layers, hp, plan=plan, device=0)
    return net, h, layers, hp


def populate(net, h, name, rng):
    mk, E, nA, B, T, kw = NETS[name]
    spec = types.SimpleNamespace(obs_shape=(E,), n_actions=nA)
    cap = max(12, B + 4)
    eps = make_episodes(spec, cap + 3, T, rng)     # more than the ring holds: the ring wraps
    feed(h, eps)
    ring = [None] * cap
    for i, ep in enumerate(eps):
        ring[i % cap] = ep
    return ring


def params(nn, net, rng):
    n = nn.glorot_params(net, seed=3).size
    p_on = (nn.glorot_params(net, seed=3) + 0.05 * rng.standard_normal(n)).astype(np.float32)      # non-zero biases and state0
    p_tg = (nn.glorot_params(net, seed=4) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return p_on, p_tg


def setup(mods, name, **kw):
    pkg, nn = mods
    net, h, layers, hp = build(mods, name, **kw)
    rng = np.random.default_rng(5)
    ring = populate(net, h, name, rng)
    p_on, p_tg = params(nn, net, rng)
    h.set_params(p_on, 0); h.set_params(p_tg, 1)
    np.testing.assert_array_equal(h.get_params(0), p_on)      # RNN block layout round trip (Wi, Wh, b, h0)
    np.testing.assert_array_equal(h.get_params(1), p_tg)
    return net, h, ring, p_on, p_tg


@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("name", list(NETS))
def test_rnn_train_step_vs_fp64_reference(mods, name, mfma):
    pkg, nn = mods
    mk, E, nA, B, T, kw = NETS[name]
    gamma, dq = float(np.float32(kw["gamma"])), bool(kw["double_q"])
    net, h, ring, p_on, p_tg = setup(mods, name, mfma=mfma)
    assert all(p[2] >= 0 for p in h.plan())
    rng = np.random.default_rng(11)
    idx, start = draws(ring, B, rng)
    check_step(h, net, nn, h.episode_get_batch(idx, start), idx, start, gamma, dq, p_on, p_tg)
    # the second step starts from the engine's own updated parameters (and Adam state): its loss and gradient are the reference's at those parameters
    p_on2 = h.get_params(0)
    idx, start = draws(ring, B, rng)
    o = drqn_train_step(net, nn, p_on2, p_tg, h.episode_get_batch(idx, start), gamma, dq)
    loss, gn = h.train_step_drqn(idx, start)
    np.testing.assert_allclose(loss, o["loss"], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(h.get_grads(), o["grads"], atol=3e-5 * (np.abs(o["grads"]).max() + 1e-30), rtol=1e-4)
    np.testing.assert_allclose(gn, o["grad_norm"], rtol=1e-4)
    h.close()


def test_rnn_schedule_follows_the_lds_fit_rule(mods, monkeypatch):
    """whole-sequence kernels where Wh and a step's state fit in LDS (past 64 KB too), per-step launches past it and under DQN_RNN_STEPWISE=1"""
    seq, step = {"rnn_seq", "rnn_bwd_seq"}, {"rnn_step", "rnn_bwd"}
    for name, want, env in (("cfg4_rnn_plain", seq, None), ("rnn128_big_lds", seq, None), ("rnn_wide_stepwise", step, None), ("cfg4_rnn_plain", step, "1")):
        if env:
            monkeypatch.setenv("DQN_RNN_STEPWISE", env)
        net, h, ring, p_on, p_tg = setup(mods, name)
        h.train_step_drqn(*draws(ring, NETS[name][3], np.random.default_rng(2)))
        names = {n.rsplit("_", 1)[0] for n, _ in h.profile_step()}
        assert want <= names and not ((seq | step) - want) & names, (name, env, names)
        h.close()
        monkeypatch.delenv("DQN_RNN_STEPWISE", raising=False)


def _run(h, ring, B, n, sync_at=None, seed=3):
    rng = np.random.default_rng(seed); out = []
    for step in range(n):
        idx, start = draws(ring, B, rng)
        out.append(h.train_step_drqn(idx, start))
        if sync_at is not None and step == sync_at:
            h.sync_target()
    return out


@pytest.mark.parametrize("name", SEQ_NETS)
def test_rnn_stepwise_schedule_is_bit_identical(mods, name, monkeypatch):
    """DQN_RNN_STEPWISE=1 (per-step recurrence / BPTT launches) and the default whole-sequence kernels: one canonical order, the same bits"""
    B = NETS[name][3]
    res = []
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("DQN_RNN_STEPWISE", env)
        net, h, ring, p_on, p_tg = setup(mods, name)
        res.append((_run(h, ring, B, 5), h.get_grads(), h.get_params(0), h.get_adam_state()))
        h.close()
        monkeypatch.delenv("DQN_RNN_STEPWISE", raising=False)
    (la, ga, pa, sa), (lb, gb, pb, sb) = res
    assert la == lb
    np.testing.assert_array_equal(ga, gb); np.testing.assert_array_equal(pa, pb)
    for x, y in zip(sa, sb):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", ["cfg4_rnn_plain", "dense_rnn_relu_dueling", "rnn_wide_stepwise"])
def test_rnn_graph_and_eager_and_two_engines_are_bit_identical(mods, name):
    B = NETS[name][3]
    res = []
    for graph in (0, 1, 1):      # eager, graph, and a second graph engine from the same seed
        net, h, ring, p_on, p_tg = setup(mods, name, graph=graph)
        res.append((_run(h, ring, B, 20, sync_at=7), h.get_params(0), h.get_params(1), h.get_grads()))
        h.close()
    for r in res[1:]:
        assert r[0] == res[0][0]
        for x, y in zip(r[1:], res[0][1:]):
            np.testing.assert_array_equal(x, y)


def test_rnn_policy_recur_state(mods):
    """hiddenstates / sethiddenstates! / resetstate! (src/helpers.jl:61-79, src/policy.jl:32-46) on 3 streams: a bare h per RNN layer"""
    pkg, nn = mods
    name = "dense_rnn_relu_dueling"
    net, h, ring, p_on, p_tg = setup(mods, name)
    ri = [i for i, l in enumerate(nn.all_layers(net)) if l.kind == "rnn"][0]
    rng = np.random.default_rng(23)
    xs = [rng.random((3, 6)).astype(np.float32) for _ in range(6)]
    with torch.no_grad():
        arrs = param_arrays(net, nn, p_on)
        hs = init_state(net, nn, arrs, 3)
        want = [q_step(net, nn, arrs, torch.tensor(x, dtype=torch.float64), hs).numpy() for x in xs[:3]]
    h.reset_state()
    for k in range(3):
        q = h.forward(xs[k])
        np.testing.assert_allclose(q, want[k], atol=1e-5, rtol=1e-5)
        assert np.array_equal(np.argmax(q, axis=1), np.argmax(want[k], axis=1))      # the actions of the reference rollout
    assert h.hidden_size(3) == 16 * 3
    saved = h.get_hidden(3)
    assert len(saved) == 1 and isinstance(saved[0], np.ndarray) and saved[0].shape == (16, 3)
    np.testing.assert_allclose(saved[0], hs[ri].numpy().T, atol=1e-5, rtol=1e-5)
    # a train step between forwards leaves the policy state untouched (the reference saves / restores it around batch_train!, src/solver.jl:137-139)
    h.train_step_drqn(*draws(ring, NETS[name][3], rng))
    np.testing.assert_array_equal(h.get_hidden(3)[0], saved[0])
    q3 = h.forward(xs[3]); st3 = h.get_hidden(3)[0]
    h.forward(xs[4])
    h.set_hidden(saved)                                       # set -> forward reproduces Q and the next state bit for bit
    np.testing.assert_array_equal(h.get_hidden(3)[0], saved[0])
    np.testing.assert_array_equal(h.forward(xs[3]), q3)
    np.testing.assert_array_equal(h.get_hidden(3)[0], st3)
    with torch.no_grad():                                      # ... and it is the reference's step from the saved state with the updated parameters
        arrs = param_arrays(net, nn, h.get_params(0))
        hs = {ri: torch.tensor(saved[0].T.astype(np.float64))}
        np.testing.assert_allclose(q3, q_step(net, nn, arrs, torch.tensor(xs[3], dtype=torch.float64), hs).numpy(), atol=1e-5, rtol=1e-5)
        np.testing.assert_allclose(st3, hs[ri].numpy().T, atol=1e-5, rtol=1e-5)
    h.reset_state()                                            # resetstate!: state0 of the online net, broadcast over the streams
    h0 = param_arrays(net, nn, h.get_params(0))[ri][3].numpy().astype(np.float32)
    np.testing.assert_array_equal(h.get_hidden(3)[0], np.repeat(h0[:, None], 3, axis=1))
    with pytest.raises(pkg.DQNError, match="buffer too small"):
        h.set_hidden([np.zeros((16, 2), np.float32)])
    h.close()


def test_rnn_checkpoint_resume_is_bit_exact(mods, tmp_path):
    pkg, nn = mods
    name = "cfg4_rnn_plain"
    net, a, ring, p_on, p_tg = setup(mods, name)
    for _ in range(3):
        a.train_step_drqn()
    ck = a.checkpoint()
    np.savez(tmp_path / "ck.npz", **ck)
    want = [a.train_step_drqn() for _ in range(4)]
    _, b, _, _ = build(mods, name)
    b.restore(dict(np.load(tmp_path / "ck.npz")))
    assert b.episode_count() == a.episode_count()
    got = [b.train_step_drqn() for _ in range(4)]
    assert got == want, (got, want)
    np.testing.assert_array_equal(a.get_params(0), b.get_params(0)); np.testing.assert_array_equal(a.get_params(1), b.get_params(1))
    for x, y in zip(a.get_adam_state(), b.get_adam_state()):
        np.testing.assert_array_equal(x, y)
    a.close(); b.close()


def test_rnn_solve_end_to_end_and_bson_round_trip(mods, tmp_path):
    """test/runtests.jl:115-129 with an RNN: TestMDP((5,5),1,6), Chain(flattenbatch, RNN(25,8), Dense(8,4)), recurrence=true, double_q; return >= 0;
    then save_model / restore_best_model (src/solver.jl:290-318) round-trip the RNN's arrays through qnetwork.bson"""
    pkg, nn = mods
    envs = importlib.import_module(pkg.__name__ + ".envs"); S = importlib.import_module(pkg.__name__ + ".solver"); bson = importlib.import_module(pkg.__name__ + ".bson")
    env = envs.TestMDP((5, 5), 1, 6, n=1, seed=7)
    model = nn.Chain(nn.flattenbatch, nn.RNN(25, 8), nn.Dense(8, env.n_actions))
    max_steps = 4000
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.01, steps=max_steps / 2), rng=np.random.default_rng(1))
    solver = S.DeepQLearningSolver(qnetwork=model, max_steps=max_steps, learning_rate=0.005, exploration_policy=expl, eval_freq=2000, num_ep_eval=20,
                                   log_freq=500, double_q=True, dueling=False, recurrence=True, verbose=False, logdir=None)
    policy = S.solve(solver, env)
    tot = 0.0
    for _ in range(50):
        env.reset(); policy.resetstate()
        r, step = 0.0, 0
        while not env.terminated()[0] and step < 100:
            r += float(env.act(np.array([policy.action(env.observe()[0])]))[0]); step += 1
        tot += r
    assert tot / 50 >= 0.0
    policy.resetstate()
    assert len(policy.engine.get_hidden()) == 1 and policy.engine.get_hidden()[0].shape == (8, 1)
    solver.logdir = str(tmp_path / "log")
    w = policy.engine.get_params(pkg.NET_ONLINE)
    S.save_model(solver, policy, 1.0, -np.inf, False)
    got, sizes = bson.load_qnetwork(str(tmp_path / "log" / "qnetwork.bson"))
    np.testing.assert_array_equal(got, w)
    assert sizes == [(8, 25), (8, 8), (8,), (8, 1), (4, 8), (4,)]
    policy.engine.set_params(w * np.float32(0.5), pkg.NET_ONLINE)
    S.restore_best_model(solver, policy)
    np.testing.assert_array_equal(policy.engine.get_params(pkg.NET_ONLINE), w)
    policy.engine.close()


def test_rnn_refusals(mods):
    pkg, nn = mods
    # recurrence = false: the reference's string (src/solver.jl:45-47)
    layers, _ = nn.lower(nn.Chain(nn.RNN(6, 8), nn.Dense(8, 3)))
    hp = pkg.default_hparams(batch_size=4, n_actions=3, obs_c=6, dueling=0, recurrence=0, prioritized_replay=0, buffer_size=8)
    with pytest.raises(pkg.DQNError, match="recurrent model but recurrence is set to false"):
        pkg.Engine(layers, hp, device=0)
    # an RNN in the advantage stream
    d = nn.DuelingNetwork(nn.Chain(nn.Dense(6, 8)), nn.Chain(nn.Dense(8, 1)), nn.Chain(nn.RNN(8, 3)))
    layers, _ = nn.lower(d)
    hp = pkg.default_hparams(batch_size=4, n_actions=3, obs_c=6, dueling=1, recurrence=1, trace_length=3, prioritized_replay=0, buffer_size=8)
    with pytest.raises(pkg.DQNError, match="base chain only"):
        pkg.Engine(layers, hp, device=0)
    # u8 replay: the episode replay stores Float32 rows
    with pytest.raises(pkg.DQNError, match="u8 is not supported with recurrence"):
        build(mods, "rnn_sigmoid_single_q", obs_dtype=pkg.OBS_U8)
    # a column-group dW plan: the fused column-parallel step covers LSTM networks only
    net, h, layers, hp = build(mods, "cfg4_rnn_plain")
    plan = [(p[0], p[1], -4) for p in h.plan()]
    h.close()
    net, h, layers, hp = build(mods, "cfg4_rnn_plain", plan=plan)
    populate(net, h, "cfg4_rnn_plain", np.random.default_rng(0))
    with pytest.raises(pkg.DQNError, match="column-group dW chunks"):
        h.train_step_drqn()
    h.close()
