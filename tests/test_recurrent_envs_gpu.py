"""GPU (-m gpu): the device environment loop on recurrent engines (DRQN) -- acting with per-copy Recur state, per-copy resetstate!, add_exp! into the episode replay
on the device, interleaved training, evaluation, lifecycle.  The reference is the shadow engine + NumPy ring model of tests/recurrent_envs_common.py; every comparison
is bit for bit."""
import math

import numpy as np
import pytest

import __graft_entry__ as ge
import recurrent_envs_common as RC

pytestmark = pytest.mark.gpu
CASES = ["lstm", "gru_duel", "rnn_conv"]


@pytest.fixture(scope="module")
def mods():
    p = ge.load_package(); p.lib()
    return (p,) + RC.load(p)


def setup(mods, name, shadow=True, mfma=1, graph=1, n=None, **ls_kw):
    pkg, nn, envs, S = mods
    case = RC.cases(nn, envs)[name]
    spec, net, n0, T, cap, B, max_len = case
    n = n or n0
    g, _ = RC.make_engine(pkg, nn, case, mfma=mfma, graph=graph)
    p = RC.noisy_params(nn, net)
    g.set_params(p, 0); g.set_params((p * 0.9).astype(np.float32), 1)
    sh = None
    if shadow:
        e2, _ = RC.make_engine(pkg, nn, case, mfma=mfma, graph=graph)
        e2.set_params(p, 0); e2.set_params((p * 0.9).astype(np.float32), 1)
        sh = RC.Shadow(e2, nn, net, n)
    g.envs_create(spec, n_envs=n, max_episode_length=max_len, seed=RC.ENV_SEED[name])
    model = RC.RingModel(n, T, cap, spec.obs_shape)
    ls = RC.LockStep(g, spec, n, max_len, RC.ENV_SEED[name], model, shadow=sh, B=B, **ls_kw)
    np.testing.assert_array_equal(g.envs_peek()[0].reshape(n, -1), ls.mirror.observe().reshape(n, -1))
    return g, sh, model, ls


def state_of(g, n):
    return dict(peek=g.envs_peek(), hidden=g.get_hidden(n), ring=g.episode_export(), count=g.episode_count(), ctr=g.get_counters(),
                p0=g.get_params(0), p1=g.get_params(1), adam=g.get_adam_state())


def assert_same_state(a, b):
    for k in ("peek", "ring", "adam"):
        for x, y in zip(a[k], b[k]):
            np.testing.assert_array_equal(x, y, err_msg=k)
    RC.hidden_equal(a["hidden"], b["hidden"])
    assert a["count"] == b["count"] and a["ctr"] == b["ctr"]
    np.testing.assert_array_equal(a["p0"], b["p0"]); np.testing.assert_array_equal(a["p1"], b["p1"])


@pytest.mark.parametrize("name", CASES)
def test_greedy_trajectory_and_state(mods, name):
    """eps = 0: every step's actions are the shadow's greedy actions on the previous observations, the Recur state equals the shadow's (columns of ended copies at
    state0), rewards / terminals / observations follow the mirror env, and the ring follows the model"""
    g, sh, model, ls = setup(mods, name, eps=(0.0, 0.0, 1.0))
    ended_any = False
    for _ in range(25):
        _, _, _, _, ended = ls.step()
        ended_any |= bool(ended.any())
    assert ended_any and ls.explored == 0 and model.size > 0


@pytest.mark.parametrize("name", CASES)
def test_dynamics_and_draws_equal_the_feed_forward_path(mods, name):
    """eps = 1: the draws are keyed by (seed, step, copy, purpose), not by the network -- a recurrent engine and a feed-forward engine (small MLP) walk the same trajectory"""
    pkg, nn, envs, S = mods
    g, _, model, ls = setup(mods, name, shadow=False, eps=(1.0, 1.0, 1.0))
    case = RC.cases(nn, envs)[name]
    spec, n = case[0], case[2]
    E = int(np.prod(spec.obs_shape))
    mlp = nn.Chain(nn.flattenbatch, nn.Dense(E, 8, nn.relu), nn.Dense(8, 4))
    f, _ = RC.make_engine(pkg, nn, case, recurrence=0, net=mlp)
    f.set_params(RC.noisy_params(nn, mlp), 0)
    f.envs_create(spec, n_envs=n, max_episode_length=case[6], seed=RC.ENV_SEED[name])
    for t in range(1, 21):
        ls.step(check_ring=False)
        f.rollout(1, t0=t, train_freq=0, target_update_freq=0, eps=(1.0, 1.0, 1.0))
        for x, y in zip(g.envs_peek(), f.envs_peek()):
            np.testing.assert_array_equal(x, y)
    assert ls.explored == 20 * n


@pytest.mark.parametrize("name,want", [("lstm", ("wrap", "prefix", "multi")), ("gru_duel", ("wrap", "open_across_reset", "multi")), ("rnn_conv", ("wrap", "short", "multi"))])
def test_episode_replay_equals_the_ring_model(mods, name, want):
    """after every step episode_export / episode_count / get_counters equal the model fed with the peeked transitions; the run reaches ring wrap, prefix truncation,
    masked rows, truncated-but-open episodes and two copies finishing in one step (seeds chosen on the CPU model, tests/test_recurrent_envs_cpu.py)"""
    g, _, model, ls = setup(mods, name, shadow=False, eps=(1.0, 1.0, 1.0))
    for _ in range(30):
        ls.step()
    for k in want:
        assert model.seen[k], (k, model.seen)


def run_training(mods, name, cadence, steps=24, shadow=True, **kw):
    g, sh, model, ls = setup(mods, name, shadow=shadow, eps=(1.0, 1.0, 1.0), **kw)
    for _ in range(RC.WARM[name]):      # random steps without training until batch_size episodes are committed (counted on the CPU model): every later train point trains
        ls.step()
    assert model.size >= ls.B and ls.trained == 0
    ls.eps, ls.tf, ls.tu, ls.cadence, ls.explored = (0.8, 0.1, 60.0), 2, 5, cadence, 0
    checked = 0
    for _ in range(steps):
        before = ls.trained
        st = ls.step()[0]
        if shadow and ls.trained > before:
            loss, gn = ls.last_scalars
            assert (st["loss"], st["grad_norm"]) == (loss, gn) and math.isfinite(loss)
            np.testing.assert_array_equal(g.get_params(0), sh.e.get_params(0))
            assert g.get_counters()["sample_ctr"] == sh.e.get_counters()["sample_ctr"]
            checked += 1
    return g, sh, model, ls, checked


@pytest.mark.parametrize("name,cadence", [("lstm", False), ("gru_duel", False), ("rnn_conv", False), ("gru_duel", True)])
def test_interleaved_training_equals_the_shadow(mods, name, cadence):
    """train_freq = 2, target_update_freq = 5, eps between 0 and 1: at each train point the shadow imports the model's ring and runs the sampled recurrent step; online
    and target parameters, Adam state, loss / grad_norm and the draw counter are bit-identical, and the shadow's greedy actions and Recur state keep matching"""
    g, sh, model, ls, checked = run_training(mods, name, cadence)
    assert checked == 24 if cadence else checked == 12      # every train point of the 24 steps trained and was compared
    assert 0 < ls.explored < ls.n * 24
    for which in (0, 1):
        np.testing.assert_array_equal(g.get_params(which), sh.e.get_params(which))
    for x, y in zip(g.get_adam_state(), sh.e.get_adam_state()):
        np.testing.assert_array_equal(x, y)
    cg, cs = g.get_counters(), sh.e.get_counters()
    assert cg["sample_ctr"] == cs["sample_ctr"] and cg["train_steps"] == cs["train_steps"] == ls.trained
    ls.eps, ls.tf = (0.0, 0.0, 1.0), 0      # greedy from here: the trained policy's actions are the shadow's
    for _ in range(4):
        ls.step()


@pytest.mark.parametrize("name", ["lstm", "gru_duel"])
def test_build_modes_give_identical_bits(mods, name):
    """use_graph 0 / 1 and use_mfma 0 / 1: parameters, ring and Recur state after the interleaved run are bit-identical"""
    outs = []
    for graph, mfma in ((1, 1), (0, 1), (1, 0)):
        g, _, _, ls, _ = run_training(mods, name, False, steps=16, shadow=False, graph=graph, mfma=mfma)
        outs.append(state_of(g, ls.n))
    assert outs[0]["ctr"]["train_steps"] > 0
    assert_same_state(outs[0], outs[1]); assert_same_state(outs[0], outs[2])


def test_evaluation_equals_the_shadow_and_leaves_training_untouched(mods):
    pkg, nn, envs, S = mods
    case = RC.cases(nn, envs)["lstm"]
    spec, net = case[0], case[1]
    g, _, _, ls, _ = run_training(mods, "lstm", False, steps=7, shadow=False)
    h, _, _, ls2, _ = run_training(mods, "lstm", False, steps=7, shadow=False)      # the same engine, which never evaluates
    for n_eval in (5, 9):
        before = state_of(g, ls.n)
        got_r, got_steps = g.evaluate(n_eval, 100, seed=3)
        assert_same_state(before, state_of(g, ls.n))
        e2, _ = RC.make_engine(pkg, nn, case)
        e2.set_params(g.get_params(0), 0)
        mir = RC.make_mirror(spec, n_eval, 3)
        tot, steps, alive = np.zeros(n_eval, np.float64), np.zeros(n_eval, np.int64), np.ones(n_eval, bool)
        while alive.any():
            a = e2.greedy_action(mir.observe())
            r, d = mir.step(0, a)
            tot[alive] += r[alive].astype(np.float64); steps[alive] += 1
            alive &= ~((d != 0) | (steps > 100))
        want_r = 0.0
        for i in range(n_eval):      # Float64 sum of the Float32 rewards, copy order
            want_r += tot[i]
        assert got_r == want_r / n_eval and got_steps == steps.sum() / n_eval
    for _ in range(6):
        ls.step(); ls2.step()
    assert_same_state(state_of(g, ls.n), state_of(h, ls2.n))


def test_lifecycle_and_refusals(mods, monkeypatch):
    pkg, nn, envs, S = mods
    g, _, model, ls = setup(mods, "lstm", shadow=False, eps=(1.0, 1.0, 1.0))
    for _ in range(7):      # 3 episodes committed at step 5, two transitions open
        ls.step()
    before = state_of(g, ls.n)
    g.rollout(0, t0=ls.t, train_freq=2, target_update_freq=5, eps=(1.0, 1.0, 1.0))      # a zero-step rollout
    assert_same_state(before, state_of(g, ls.n))
    spec, net, n0, T, cap, B, max_len = RC.cases(nn, envs)["lstm"]
    g.envs_create(spec, n_envs=6, max_episode_length=max_len, seed=23)      # another n: committed episodes stay, open ones go
    for x, y in zip(before["ring"], g.episode_export()):
        np.testing.assert_array_equal(x, y)
    assert g.episode_count() == before["count"] and g.get_hidden(6)[0][0].shape == (8, 6)
    model.recreate(6)
    ls6 = RC.LockStep(g, spec, 6, max_len, 23, model, eps=(1.0, 1.0, 1.0))
    for _ in range(6):
        ls6.step()
    assert model.len[:model.size].max() == 5      # no commit carries transitions of the discarded open episodes
    # refusals
    z = np.zeros((1,) + spec.obs_shape, np.float32)
    with pytest.raises(pkg.DQNError, match="cannot be mixed"):
        g.episode_add(z, [0], [0.0], z, [0])
    with pytest.raises(pkg.DQNError, match="cannot be mixed"):
        g.episode_commit()
    with pytest.raises(pkg.DQNError, match="n_envs must be in 1..1024"):
        g.envs_create(spec, n_envs=1025, max_episode_length=max_len, seed=1)
    with pytest.raises(pkg.DQNError, match="has device environments"):
        g.comm_init(b"\0" * 128, 0, 1)
    h, _ = RC.make_engine(pkg, nn, RC.cases(nn, envs)["lstm"])
    h.episode_add(z, [0], [0.0], z, [0])
    with pytest.raises(pkg.DQNError, match="an episode is open on the host side"):
        h.envs_create(spec, n_envs=3, max_episode_length=max_len, seed=1)
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    s, _ = RC.make_engine(pkg, nn, RC.cases(nn, envs)["lstm"])
    monkeypatch.delenv("DQN_SIM_WORLD")
    with pytest.raises(pkg.DQNError, match="DQN_SIM_WORLD"):
        s.envs_create(spec, n_envs=3, max_episode_length=max_len, seed=1)


def test_solve_with_recurrence_on_device_envs(mods):
    pkg, nn, envs, S = mods
    env = envs.TestMDP((5, 5), 1, 6, n=4)
    model = nn.Chain(nn.flattenbatch, nn.LSTM(25, 8), nn.Dense(8, 4))
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.05, steps=60))
    solver = S.DeepQLearningSolver(qnetwork=model, max_steps=80, learning_rate=0.005, exploration_policy=expl, eval_freq=40, num_ep_eval=4, train_freq=2, log_freq=40,
                                   target_update_freq=20, double_q=True, dueling=False, recurrence=True, trace_length=4, buffer_size=16, batch_size=4, train_start=20,
                                   verbose=False, logdir=None, device_envs=True, prioritized_replay=False)
    policy = S.solve(solver, env)
    r, steps = policy.engine.evaluate(4, 100, seed=3)
    assert math.isfinite(r) and steps == 5.0
    assert policy.engine.get_counters()["train_steps"] == 40 and policy.engine.episode_count()[0] == 16
