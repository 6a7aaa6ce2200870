"""GPU (-m gpu): MountainCar and InvertedPendulum on the device loop (dqn_envs_create_control), all through the C ABI.  The reference is the CPU twin's law
(envs.MountainCar / envs.InvertedPendulum) applied to the device's own pre-step state under the comparison rule of tests/control_envs_common.py: Float64 states to
1e-12 * max(1, |value|), everything downstream bit for bit.  Without dqn_envs_create_control every test here fails."""
import math

import numpy as np
import pytest

import __graft_entry__ as ge
import control_envs_common as CC

pytestmark = pytest.mark.gpu
SEED = 7


@pytest.fixture(scope="module")
def mods():
    p = ge.load_package(); p.lib()
    return (p,) + CC.load(p)


def pair(mods, net, **kw):
    """an engine and its shadow: the same layers, hparams and parameters"""
    pkg, nn, envs, S = mods
    p = CC.noisy_params(nn, net)
    def engine():
        e = CC.make_engine(pkg, nn, net, **kw)
        e.set_params(p, 0); e.set_params((p * 0.9).astype(np.float32), 1)
        return e
    return engine(), engine()


@pytest.mark.parametrize("name,n,dueling", [("mc_goal", 5, 1), ("mc_wall", 32, 0), ("mc_clamp", 5, 0), ("pend", 5, 0), ("pend", 32, 1)])
def test_lock_step_feed_forward(mods, name, n, dueling):
    """40 vector steps with training on (train_freq = 4, B = 4) and eps-greedy at 0.3: states under the comparison rule; observations, rewards, dones, greedy and
    explored actions, the pendulum's noise and reset draws and the ring rows bit for bit; the case's branches are all met.  The feed-forward train steps are
    counted, not compared (ControlLockStep's LIMITATION)"""
    pkg, nn, envs, S = mods
    spec, max_len = CC.cases(envs)[name]
    g, sh = pair(mods, CC.ff_net(nn, dueling), cap=2048)      # 40 * 32 experiences: no wrap, slot order is step order
    g.envs_create(spec, n_envs=n, max_episode_length=max_len, seed=SEED)
    assert g.envs_info() == (n, False)      # the general four-launch tail
    model = CC.FFRing(2048, (2,))
    ls = CC.ControlLockStep(g, spec, n, max_len, SEED, model, CC.Shadow(sh, nn, CC.ff_net(nn, dueling), n), eps=(0.3, 0.3, 1.0), train_freq=4, B=4)
    for _ in range(40):
        ls.step()
    want = {"mc_goal": ("goal", "reset"), "mc_wall": ("wall", "truncated"), "mc_clamp": ("clamp", "truncated"), "pend": ("fall", "reset")}[name]
    for k in want:
        assert ls.seen[k], (k, ls.seen)
    assert ls.trained == 10 and 0 < ls.explored < 40 * n
    print(f"{name} n={n}: smallest branch margin {ls.min_margin:.3e}")
    s, sp, a, r, d, _ = g.replay_export()
    k = model.size
    assert g.replay_size()[0] == k == 40 * n
    for got, w in ((s, model.s), (sp, model.sp), (a, model.a), (r, model.r), (d, model.d)):
        np.testing.assert_array_equal(got.reshape(k, -1), w[:k].reshape(k, -1))


@pytest.mark.parametrize("name,rewards", [("mc_goal", (-1.0, 99.0)), ("pend", (-1.0, 0.0))])
def test_leaf_priorities_without_training(mods, name, rewards):
    """add_exp!(replay, exp, abs(exp.r)): the jackpot's 99 and the step cost's 1, the pendulum's fall (1) and its free steps (0), as leaf priorities"""
    pkg, nn, envs, S = mods
    spec, max_len = CC.cases(envs)[name]
    g, _ = pair(mods, CC.ff_net(nn, 0))
    g.envs_create(spec, n_envs=5, max_episode_length=max_len, seed=SEED)
    g.rollout(12, t0=1, train_freq=0, target_update_freq=0, eps=(0.3, 0.3, 1.0))
    r, pr = g.replay_export()[3], g.replay_export()[5]
    assert set(np.unique(r)) == {np.float32(x) for x in rewards}
    np.testing.assert_array_equal(pr, ((np.abs(r) + np.float32(1e-3)).astype(np.float64) ** np.float64(np.float32(0.6))).astype(np.float32))


def snapshot(g, n, rec):
    d = dict(state=g.envs_peek_state(), peek=g.envs_peek(), ctr=g.get_counters(), p0=g.get_params(0), p1=g.get_params(1), adam=g.get_adam_state())
    d["ring"] = g.episode_export() if rec else g.replay_export()
    d["hidden"] = g.get_hidden(n) if rec else []
    return d


def assert_same(a, b):
    for k in ("state", "peek", "ring", "adam"):
        for x, y in zip(a[k], b[k]):
            np.testing.assert_array_equal(x, y, err_msg=k)
    CC.hidden_equal(a["hidden"], b["hidden"])
    assert a["ctr"] == b["ctr"]
    np.testing.assert_array_equal(a["p0"], b["p0"]); np.testing.assert_array_equal(a["p1"], b["p1"])


@pytest.mark.parametrize("name", ["mc_wall", "pend"])
def test_schedules_give_identical_bits(mods, name):
    """graph and eager runs, use_mfma 0 and 1, and a softmax table: peeked Float64 states, rings, parameters and counters are bit for bit the same between engines"""
    pkg, nn, envs, S = mods
    spec, max_len = CC.cases(envs)[name]
    for kw in (dict(), dict(explore=("softmax", [0.5]))):
        outs = []
        for graph, mfma in ((1, 1), (0, 1), (1, 0)):
            g, _ = pair(mods, CC.ff_net(nn, 1), graph=graph, mfma=mfma)
            g.envs_create(spec, n_envs=5, max_episode_length=max_len, seed=SEED)
            st = g.rollout(12, t0=1, train_freq=2, target_update_freq=5, eps=(0.8, 0.1, 60.0), **kw)
            assert g.envs_info() == (5, False) and st["train_steps"] > 0
            outs.append(snapshot(g, 5, False))
        assert_same(outs[0], outs[1]); assert_same(outs[0], outs[2])


@pytest.mark.parametrize("name,n", [("pend", 32), ("mc_goal", 5)])
def test_softmax_table_against_the_model(mods, name, n):
    """dqn_rollout_explore with a softmax table (tau cycling through 1, 0.3, 0.1) on the new kinds, 16 vector steps in lock step.  Every pick is judged against the
    fp64 softmax of the shadow's own forward and the purpose-11 draw, intervals widened by the derived delta (the rule and its derivation:
    test_exploration_gpu.py::test_softmax_interior) -- expf on the device and np.exp need not agree to the last bit, so the picks are not held bit for bit; the count
    of picks that equal the fp32 restatement of the law is printed.  States, rewards, dones, observations and ring rows follow the device's action bit for bit"""
    pkg, nn, envs, S = mods
    spec, max_len = CC.cases(envs)[name]
    g, sh = pair(mods, CC.ff_net(nn, 1))
    g.envs_create(spec, n_envs=n, max_episode_length=max_len, seed=SEED)
    taus = (1.0, 0.3, 0.1)
    table = lambda t: ("softmax", [np.float32(taus[(t - 1) % 3])])
    ls = CC.ControlLockStep(g, spec, n, max_len, SEED, CC.FFRing(1024, (2,)), CC.Shadow(sh, nn, CC.ff_net(nn, 1), n), explore_table=table)
    for _ in range(16):
        ls.step()
    tl = ls.tally
    print(f"softmax {name}: {tl.draws} draws, {tl.near} within delta of a boundary, {tl.widened} needed the widening, largest delta {tl.max_delta:.3e}, "
          f"{ls.law32_agree} equal the fp32 law, {ls.off_greedy} off the greedy action")
    assert tl.draws == 16 * n and tl.near <= max(1, tl.draws // 100) and ls.off_greedy > 0
    assert len(tl.picks[1.0]) >= 2, tl.picks      # at tau = 1 the draw spreads over the actions
    assert g.envs_info() == (n, False)


def test_exploration_table_equals_the_model(mods):
    """dqn_rollout_explore with an eps table (a different eps per vector step) on the pendulum: actions bit for bit the keyed draws of the model"""
    pkg, nn, envs, S = mods
    spec, max_len = CC.cases(envs)["pend"]
    g, sh = pair(mods, CC.ff_net(nn, 0))
    g.envs_create(spec, n_envs=5, max_episode_length=max_len, seed=SEED)
    table = lambda t: ("eps", [np.float32(0.1 + 0.05 * (t % 10))])
    ls = CC.ControlLockStep(g, spec, 5, max_len, SEED, CC.FFRing(256, (2,)), CC.Shadow(sh, nn, CC.ff_net(nn, 0), 5), eps=(0.0, 0.0, 1.0), explore_table=table)
    for _ in range(16):
        ls.step()
    assert 0 < ls.explored < 16 * 5


@pytest.mark.parametrize("name", ["mc_goal", "mc_wall", "pend"])
def test_lock_step_recurrent(mods, name):
    """LSTM(2, 4) -> Dense(4, 3), T = 4, n = 5, train_freq = 2: open episodes, commits on done, no commit on truncation, per-copy resetstate!, the sampled recurrent
    train step -- ring, hidden state, loss, gradient norm and parameters equal the episode-ring model and the shadow after every step"""
    pkg, nn, envs, S = mods
    spec, max_len = CC.cases(envs)[name]
    net = nn.Chain(nn.LSTM(2, 4), nn.Dense(4, 3))
    g, sh = pair(mods, net, rec=1, T=4, cap=6, B=2)
    g.envs_create(spec, n_envs=5, max_episode_length=max_len, seed=SEED)
    assert g.envs_info() == (5, False)
    model = CC.RingModel(5, 4, 6, (2,))
    ls = CC.ControlLockStep(g, spec, 5, max_len, SEED, model, CC.Shadow(sh, nn, net, 5), eps=(0.3, 0.3, 1.0), train_freq=2, target_update_freq=5, B=2, rec=True)
    for _ in range(24):
        ls.step()
    if name == "mc_wall":
        assert model.size == 0 and ls.seen["truncated"] and model.seen["open_across_reset"]      # truncation never commits
    else:
        assert model.size > 0 and ls.trained > 0


def test_evaluation_is_a_known_answer_of_the_whole_loop(mods):
    """dqn_evaluate under the linear controllers (Dense(2, 3), identity): MountainCar pushed with its velocity reaches the goal -- avg_reward and avg_steps equal the
    twin's basic_evaluation exactly (the env is deterministic, the Float64 sum of Float32 rewards is exact); the pendulum's controller keeps it up for 300 steps
    (avg_reward == 0), always-left drops it (avg_reward == -1).  Every other state of the engine is as it was before the call"""
    pkg, nn, envs, S = mods
    net = nn.Chain(nn.Dense(2, 3))
    probe = np.array([[0.25, -0.5]], np.float32)
    for env, kind, max_len, want_r in ((envs.MountainCar(), "mc", 200, None), (envs.InvertedPendulum(), "pend", 300, 0.0), (envs.InvertedPendulum(), "left", 300, -1.0)):
        g = CC.make_engine(pkg, nn, net)
        g.set_params(CC.linear_params(kind), 0); g.sync_target()
        np.testing.assert_array_equal(g.forward(probe), CC.linear_q(kind, probe))
        g.envs_create(env, n_envs=5, max_episode_length=50, seed=SEED)
        g.rollout(3, t0=1, train_freq=0, target_update_freq=0, eps=(0.5, 0.5, 1.0))
        before = snapshot(g, 5, False)
        got_r, got_s = g.evaluate(8, max_len, seed=11)
        assert_same(before, snapshot(g, 5, False))
        tw_r, tw_s, margin = CC.twin_evaluation(env, kind, 8, max_len, 11)
        assert margin > CC.MARGIN
        print(f"{kind}: device ({got_r}, {got_s}), twin ({tw_r}, {tw_s}), smallest branch margin {margin:.3e}")
        assert (got_r, got_s) == (tw_r, tw_s)
        if want_r is not None:
            assert got_r == want_r
        else:
            assert got_s < 200 and got_r == 100.0 - got_s      # the goal, on the step the twin reaches it


def test_engine_group_equals_the_members_alone(mods):
    """K = 3 members with different seeds (two pendulums and a MountainCar): dqn_rollout_many for 12 vector steps and dqn_evaluate_many are bit for bit the members
    run alone"""
    pkg, nn, envs, S = mods
    net = CC.ff_net(nn, 1)
    specs = [envs.InvertedPendulum(init_half=1.5), envs.MountainCar(x0=0.45, v0=0.05), envs.InvertedPendulum()]
    def members():
        out = []
        for k, spec in enumerate(specs):
            e = CC.make_engine(pkg, nn, net)
            p = CC.noisy_params(nn, net, seed=3 + k)
            e.set_params(p, 0); e.set_params((p * 0.9).astype(np.float32), 1)
            e.envs_create(spec, n_envs=8, max_episode_length=20, seed=SEED + k)
            out.append(e)
        return out
    alone, grouped = members(), members()
    grp = pkg._abi.EngineGroup(grouped)
    try:
        sts = grp.rollout(12, t0=1, train_freq=4, target_update_freq=8, eps=[(0.5, 0.5, 1.0)] * 3, explore=[None] * 3)
        for k, e in enumerate(alone):
            st = e.rollout(12, t0=1, train_freq=4, target_update_freq=8, eps=(0.5, 0.5, 1.0))
            assert st["train_steps"] == sts[k]["train_steps"] == 3 and st["loss"] == sts[k]["loss"]
            assert_same(snapshot(e, 8, False), snapshot(grouped[k], 8, False))
        got = grp.evaluate(6, 30, [21, 22, 23])
        for k, e in enumerate(alone):
            assert tuple(got[k]) == e.evaluate(6, 30, seed=21 + k)
            assert_same(snapshot(e, 8, False), snapshot(grouped[k], 8, False))
    finally:
        grp.close()


def test_refusals(mods, monkeypatch):
    pkg, nn, envs, S = mods
    net = CC.ff_net(nn, 0)
    g = CC.make_engine(pkg, nn, net)
    g.envs_create(envs.MountainCar(), n_envs=4, max_episode_length=9, seed=1)
    g.rollout(2, t0=1, train_freq=0, target_update_freq=0, eps=(0.5, 0.5, 1.0))
    before = snapshot(g, 4, False)
    def bad(match, kind=3, eng=None, n_envs=4, max_episode_length=9, **c):
        with pytest.raises(pkg.DQNError, match=match):
            (eng or g).envs_create_control(kind, n_envs=n_envs, max_episode_length=max_episode_length, seed=1, **c)
    bad(r"unknown kind 2", kind=2)
    bad(r"unknown kind 5", kind=5)
    bad(r"n_envs must be in 1\.\.min\(1024, replay capacity\)", n_envs=0)
    bad(r"n_envs must be in 1\.\.min\(1024, replay capacity\)", n_envs=1025)
    bad(r"max_episode_length must be >= 1", max_episode_length=0)
    bad(r"gravity = nan is not finite", gravity=np.nan)
    bad(r"noise = inf is not finite", kind=3, noise=np.inf)      # the other member's constants are checked for finiteness too
    bad(r"theta_max = -inf is not finite", kind=4, theta_max=-np.inf)
    bad(r"dt = 0 must be > 0", kind=4, dt=0.0)
    bad(r"dt = -0\.1 must be > 0", kind=4, dt=-0.1)
    bad(r"v_max = 0 must be > 0", v_max=0.0)
    bad(r"x_min = 0\.5 must lie below goal = 0\.5", x_min=0.5)
    bad(r"alpha \* m = 1\.5 must lie below 4/3", kind=4, alpha=0.75, m=2.0)
    bad(r"l = 0 must be > 0", kind=4, l=0.0)
    assert_same(before, snapshot(g, 4, False))      # a refused call leaves the env set as it was
    with pytest.raises(pkg.DQNError, match="control device environments"):
        g.comm_init(b"\0" * 128, 0, 1)
    with pytest.raises(pkg.DQNError, match="unknown environment kind 3"):      # dqn_envs_create keeps refusing the kind
        sp = pkg._abi.EnvSpec(); sp.kind, sp.n_envs, sp.max_episode_length = 3, 4, 9
        g._check(g.f["envs_create"](g._h, pkg._abi.C.byref(sp)))
    four = CC.make_engine(pkg, nn, nn.Chain(nn.Dense(2, 8, nn.tanh), nn.Dense(8, 4)), n_actions=4)
    bad(r"observation of 2 floats and 3 actions \(network: 2 in, 4 out\)", eng=four)
    four.envs_create(envs.SimpleGridWorld(), n_envs=4, max_episode_length=9, seed=1)
    with pytest.raises(pkg.DQNError, match=r"dqn_envs_peek_state: the env set is of kind 1"):
        four.envs_peek_state()
    wide = CC.make_engine(pkg, nn, nn.Chain(nn.Dense(3, 8, nn.tanh), nn.Dense(8, 3)), obs_c=3)
    bad(r"network: 3 in, 3 out", eng=wide)
    u8 = CC.make_engine(pkg, nn, net, obs_dtype=pkg.OBS_U8)
    bad(r"stores observations as u8", eng=u8)
    c = CC.make_engine(pkg, nn, net)
    c.comm_init(pkg.comm_unique_id(), 0, 1)
    bad(r"control env: .*this engine has a communicator \(dqn_comm_init\)", eng=c)
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    s = CC.make_engine(pkg, nn, net)
    monkeypatch.delenv("DQN_SIM_WORLD")
    bad(r"DQN_SIM_WORLD", eng=s)


def test_solver_runs_on_the_device_loop(mods):
    """solve(device_envs=True) on InvertedPendulum returns a policy with finite parameters (no learning claim), feed-forward and recurrent; solve_many of 4 seeds runs"""
    pkg, nn, envs, S = mods
    def solver(seed=0, rec=False, **kw):
        env = envs.InvertedPendulum(n=8, seed=seed)
        model = nn.Chain(nn.LSTM(2, 4), nn.Dense(4, 3)) if rec else nn.Chain(nn.Dense(2, 8, nn.tanh), nn.Dense(8, 3))
        expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.05, steps=100))
        return S.DeepQLearningSolver(qnetwork=model, max_steps=200, learning_rate=1e-3, exploration_policy=expl, eval_freq=100, num_ep_eval=4, log_freq=500, recurrence=rec,
                                     trace_length=4, prioritized_replay=not rec, target_update_freq=50, verbose=False, logdir=None, buffer_size=64 if rec else 512, train_start=32,
                                     batch_size=4, max_episode_length=50, seed=seed, device_envs=True, **kw), env
    for rec in (False, True):
        sv, env = solver(rec=rec)
        policy = S.solve(sv, env)
        assert np.all(np.isfinite(policy.engine.get_params(0))) and policy.engine.envs_info() == (8, False)
        assert policy.engine.get_counters()["train_steps"] > 0
        assert policy.actionvalues(env.observe()[0]).shape == (3,)
    pairs = [solver(seed=k) for k in range(4)]
    policies = S.solve_many([p[0] for p in pairs], [p[1] for p in pairs])
    assert len(policies) == 4 and all(np.all(np.isfinite(p.engine.get_params(0))) for p in policies)
    assert all(math.isfinite(p.scores_eval) for p in policies)
