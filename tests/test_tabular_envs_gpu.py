"""GPU (-m gpu): tabular (PO)MDP environments on the device loop (dqn_envs_create_tabular), all through the C ABI.  The reference is the NumPy model of the sampling law
in tests/tabular_envs_common.py beside the shadow engine and the episode-ring model of the recurrent env tests; every comparison of dynamics, draws, rings, hidden
state and recurrent training is bit for bit.  Env seeds come from the CPU model (tests/test_tabular_envs_cpu.py); the coverage flags are asserted here again."""
import math

import numpy as np
import pytest

import __graft_entry__ as ge
import tabular_envs_common as TC

pytestmark = pytest.mark.gpu
CASES = ["tiger", "sparse", "wide_mdp"]


@pytest.fixture(scope="module")
def mods():
    p = ge.load_package(); p.lib()
    return (p,) + TC.load(p)


def create(g, case, name, **kw):
    args = dict(n_envs=case["n"], max_episode_length=case["max_len"], seed=TC.ENV_SEED[name])
    args.update(kw)
    g.envs_create_tabular(**case["tab"].kwargs(), **args)


def setup(mods, name, shadow=True, mfma=1, graph=1, prefill=None, **ls_kw):
    pkg, nn, envs, S = mods
    case = TC.cases(nn)[name]
    tab, net, n = case["tab"], case["net"], case["n"]
    p = TC.noisy_params(nn, net)
    def engine():
        e = TC.make_engine(pkg, nn, case, mfma=mfma, graph=graph)
        e.set_params(p, 0); e.set_params((p * 0.9).astype(np.float32), 1)
        return e
    g = engine()
    sh = TC.Shadow(engine(), nn, net, n) if shadow else None
    model = TC.RingModel(n, case["T"], case["cap"], tab.obs_shape) if case["rec"] else TC.FFRing(case["cap"], tab.obs_shape)
    if prefill:      # a host-prefilled episode ring (a model without terminal states never commits an episode from the loop)
        rng = np.random.default_rng(11)
        for k in range(prefill):
            o = rng.integers(0, tab.O, case["T"] + 1)
            model.s[k], model.sp[k] = tab.features[o[:-1]], tab.features[o[1:]]
            model.a[k], model.r[k], model.len[k] = rng.integers(0, tab.A, case["T"]), rng.standard_normal(case["T"]).astype(np.float32), case["T"]
        model.size = model.widx = prefill
        g.episode_import(*model.export())
    create(g, case, name)
    ls = TC.TabLockStep(g, tab, n, case["max_len"], TC.ENV_SEED[name], model, shadow=sh, B=case["B"], rec=bool(case["rec"]), **ls_kw)
    np.testing.assert_array_equal(g.envs_peek()[0].reshape(n, -1), ls.mirror.observe().reshape(n, -1))
    return g, sh, model, ls, case


def state_of(g, n, rec):
    d = dict(peek=g.envs_peek(), ctr=g.get_counters(), p0=g.get_params(0), p1=g.get_params(1), adam=g.get_adam_state())
    if rec:
        d.update(hidden=g.get_hidden(n), ring=g.episode_export(), count=g.episode_count())
    else:
        d.update(hidden=[], ring=g.replay_export(), count=g.replay_size())
    return d


def assert_same_state(a, b):
    for k in ("peek", "ring", "adam"):
        for x, y in zip(a[k], b[k]):
            np.testing.assert_array_equal(x, y, err_msg=k)
    TC.hidden_equal(a["hidden"], b["hidden"])
    assert a["count"] == b["count"] and a["ctr"] == b["ctr"]
    np.testing.assert_array_equal(a["p0"], b["p0"]); np.testing.assert_array_equal(a["p1"], b["p1"])


@pytest.mark.parametrize("name", CASES)
def test_dynamics_and_draws_equal_the_model(mods, name):
    """eps = 0.5: every vector step's actions are the shadow's greedy action or the keyed random one; rewards, dones and next observations (dqn_envs_peek) equal the
    model bit for bit; on the recurrent cases the episode ring equals RingModel and the hidden state the shadow's after every step"""
    g, sh, model, ls, case = setup(mods, name, eps=(0.5, 0.5, 1.0))
    ended_any = False
    for _ in range(20):
        ended_any |= bool(ls.step()[4].any())
    assert ended_any and 0 < ls.explored < 20 * ls.n
    assert g.envs_info() == (case["n"], False)      # the general four-launch tail


@pytest.mark.parametrize("name", CASES)
def test_rings_and_branch_coverage_under_random_actions(mods, name):
    """eps = 1 with the seeds chosen on the CPU model: the run reaches every branch TC.WANT names (the fallback pick, zero-probability neighbours on both sides, first
    and last index, ring wrap, two finishers in one step, an episode open across a truncation).  Recurrent cases: ring arrays, true lengths, cursor and count equal
    RingModel after every step.  wide_mdp (train_freq = 0): the exported replay rows, actions, rewards, dones and leaf priorities equal the model's ring, and
    dqn_envs_info reports fused_tail = 0; then a short run with training on keeps loss and gradient norm finite and moves the parameters.  (A bit-exact training
    reference for the feed-forward path would need the CPU twin to step tabular envs, which it does not.)"""
    g, _, model, ls, case = setup(mods, name, shadow=False, eps=(1.0, 1.0, 1.0))
    for _ in range(TC.STEPS[name]):
        ls.step()
    flags = ls.flags()
    for k in TC.WANT[name]:
        assert flags[k], (k, flags)
    if case["rec"]:
        return
    s, sp, a, r, d, pr = g.replay_export()
    k = model.size
    assert g.replay_size() == (k, case["cap"]) and k == TC.STEPS[name] * case["n"]
    for got, want in ((s, model.s), (sp, model.sp), (a, model.a), (r, model.r), (d, model.d)):
        np.testing.assert_array_equal(got.reshape(k, -1), want[:k].reshape(k, -1))
    want_pr = ((np.abs(model.r[:k]) + np.float32(1e-3)).astype(np.float64) ** np.float64(np.float32(0.6))).astype(np.float32)      # add_exp!(replay, exp, abs(exp.r))
    np.testing.assert_array_equal(pr, want_pr)
    assert g.envs_info() == (case["n"], False)
    p0 = g.get_params(0)
    st = g.rollout(8, t0=ls.t, train_freq=2, target_update_freq=4, eps=(0.5, 0.5, 1.0))
    assert st["train_steps"] == 4 and math.isfinite(st["loss"]) and math.isfinite(st["grad_norm"]) and st["grad_norm"] > 0
    assert np.all(np.isfinite(g.get_params(0))) and not np.array_equal(p0, g.get_params(0))


def run_training(mods, name, steps, shadow=True, **kw):
    prefill = 3 if name == "tiger" else None
    g, sh, model, ls, case = setup(mods, name, shadow=shadow, eps=(1.0, 1.0, 1.0), prefill=prefill, **kw)
    for _ in range(TC.WARM.get(name, 0)):
        ls.step()
    assert model.size >= ls.B and ls.trained == 0
    ls.eps, ls.tf, ls.tu, ls.explored = (0.8, 0.1, 60.0), 2, 5, 0
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


@pytest.mark.parametrize("name", ["tiger", "sparse"])
def test_interleaved_training_equals_the_shadow(mods, name):
    """train_freq = 2, target_update_freq = 5, eps between 0 and 1: loss, grad_norm, parameters, Adam state and the draw counter equal the shadow's sampled recurrent
    step at every train point; `tiger` (no terminal state: the loop commits nothing) trains from a host-prefilled ring, which stays as imported"""
    g, sh, model, ls, checked = run_training(mods, name, 16)
    assert checked == 8 and 0 < ls.explored < ls.n * 16
    for which in (0, 1):
        np.testing.assert_array_equal(g.get_params(which), sh.e.get_params(which))
    for x, y in zip(g.get_adam_state(), sh.e.get_adam_state()):
        np.testing.assert_array_equal(x, y)
    if name == "tiger":
        assert g.episode_count()[0] == 3 and model.size == 3


@pytest.mark.parametrize("name", ["sparse", "wide_mdp"])
def test_build_modes_give_identical_bits(mods, name):
    """use_graph 0 / 1 and use_mfma 0 / 1: env state, ring, parameters, Adam state, counters (and the Recur state) after an interleaved run are bit-identical"""
    outs = []
    for graph, mfma in ((1, 1), (0, 1), (1, 0)):
        if name == "sparse":
            g, _, _, ls, _ = run_training(mods, name, 12, shadow=False, graph=graph, mfma=mfma)
        else:
            g, _, _, ls, case = setup(mods, name, shadow=False, graph=graph, mfma=mfma)
            g.rollout(12, t0=1, train_freq=2, target_update_freq=5, eps=(0.8, 0.1, 60.0))
        outs.append(state_of(g, ls.n, name == "sparse"))
    assert outs[0]["ctr"]["train_steps"] > 0
    assert_same_state(outs[0], outs[1]); assert_same_state(outs[0], outs[2])


def test_evaluation_equals_the_model_and_leaves_training_untouched(mods):
    pkg, nn, envs, S = mods
    g, _, _, ls, _ = run_training(mods, "sparse", 6, shadow=False)
    h, _, _, ls2, _ = run_training(mods, "sparse", 6, shadow=False)      # the same engine, which never evaluates
    case = TC.cases(nn)["sparse"]
    for n_eval in (5, 8):
        before = state_of(g, ls.n, True)
        got_r, got_steps = g.evaluate(n_eval, 100, seed=3)
        assert_same_state(before, state_of(g, ls.n, True))
        e2 = TC.make_engine(pkg, nn, case)
        e2.set_params(g.get_params(0), 0)
        mir = TC.TabMirror(case["tab"], n_eval, 3)
        tot, steps, alive, t = np.zeros(n_eval, np.float64), np.zeros(n_eval, np.int64), np.ones(n_eval, bool), 0
        while alive.any():
            t += 1
            a = e2.greedy_action(mir.observe())
            r, d = mir.step(t, a)
            tot[alive] += r[alive].astype(np.float64); steps[alive] += 1
            alive &= ~((d != 0) | (steps > 100))
        want_r = 0.0
        for i in range(n_eval):
            want_r += tot[i]
        assert got_r == want_r / n_eval and got_steps == steps.sum() / n_eval
    for _ in range(4):
        ls.step(); ls2.step()
    assert_same_state(state_of(g, ls.n, True), state_of(h, ls2.n, True))


def test_refusals(mods, monkeypatch):
    pkg, nn, envs, S = mods
    case = TC.cases(nn)["sparse"]
    tab = case["tab"]
    g = TC.make_engine(pkg, nn, case)
    k = tab.kwargs()
    def bad(match, eng=None, **chg):
        args = dict(n_envs=5, max_episode_length=6, seed=1)
        kw = {**k, **chg}
        for key in ("n_envs", "max_episode_length", "n_states", "n_obs"):
            if key in kw:
                args[key] = kw.pop(key)
        with pytest.raises(pkg.DQNError, match=match):
            (eng or g).envs_create_tabular(**kw, **args)
    bad(r"n_states = 0 must be in 1\.\.1024", n_states=0)
    bad(r"n_states = 1025 must be in 1\.\.1024", n_states=1025)
    bad(r"n_obs = 1025 must be in 0\.\.1024", n_obs=1025)
    bad(r"n_obs = -1 must be in 0\.\.1024", n_obs=-1)
    bad(r"n_envs must be in 1\.\.1024", n_envs=1025)
    bad(r"n_envs must be in 1\.\.1024", n_envs=0)
    bad(r"max_episode_length must be >= 1", max_episode_length=0)
    for name in ("T", "R", "terminal", "b0", "features", "Z", "Z0"):
        bad(name + r" .*is NULL", n_states=5, n_obs=3, **{name: None})
    bad(r"Z is given with n_obs = 0", n_obs=0, features=np.zeros((5, 6), np.float32))
    bad(r"Z0 is given with n_obs = 0", n_obs=0, Z=None, features=np.zeros((5, 6), np.float32))
    T = tab.T.copy(); T[2, 1, 3] = -0.25
    bad(r"T\[2\]\[1\]\[3\] = -0\.25 is negative or not finite", T=T)
    Z = tab.Z.copy(); Z[1, 4, 0] = np.inf
    bad(r"Z\[1\]\[4\]\[0\] = inf is negative or not finite", Z=Z)
    b0 = tab.b0.copy(); b0[3] = np.nan
    bad(r"env: b0\[3\] = nan is negative or not finite", b0=b0)
    T = tab.T.copy(); T[3, 2, 0] += 0.002
    bad(r"row T\[3\]\[2\] sums to 1\.002", T=T)
    Z0 = tab.Z0.copy(); Z0[2, 0] -= 0.002
    bad(r"row Z0\[2\] sums to 0\.998", Z0=Z0)
    Z0 = tab.Z0.copy(); Z0[4, 1] = -1.0
    bad(r"env: Z0\[4\]\[1\] = -1 is negative or not finite", Z0=Z0)
    b0 = tab.b0.copy(); b0[0] += 0.003      # 0.9990 + 0.003
    bad(r"row b0 sums to 1\.002", b0=b0)
    R = tab.R.copy(); R[4, 2, 1] = np.nan
    bad(r"R\[4\]\[2\]\[1\] = nan is not finite", R=R)
    F = tab.features.copy(); F[2, 5] = -np.inf
    bad(r"features\[2\]\[5\] = -inf is not finite", features=F)
    T = tab.T.copy(); T[4] = 0.0      # rows of T at a terminal state are exempt from the sum check
    g.envs_create_tabular(**{**k, "T": T}, n_envs=5, max_episode_length=6, seed=1)
    with pytest.raises(pkg.DQNError, match="tabular device environments"):
        g.comm_init(b"\0" * 128, 0, 1)
    # feed-forward engines: the transition-ring capacity bounds n_envs; a u8 replay is refused
    wide = TC.cases(nn)["wide_mdp"]
    f = TC.make_engine(pkg, nn, wide, buffer_size=4, batch_size=4)
    with pytest.raises(pkg.DQNError, match=r"n_envs must be in 1\.\.min\(1024, replay capacity\)"):
        f.envs_create_tabular(**wide["tab"].kwargs(), n_envs=8, max_episode_length=5, seed=1)
    u = TC.make_engine(pkg, nn, wide, obs_dtype=pkg.OBS_U8)
    with pytest.raises(pkg.DQNError, match="stores observations as u8"):
        u.envs_create_tabular(**wide["tab"].kwargs(), n_envs=8, max_episode_length=5, seed=1)
    c = TC.make_engine(pkg, nn, wide)      # a feed-forward engine with a real communicator (world 1): only the tabular refusal can fire
    c.comm_init(pkg.comm_unique_id(), 0, 1)
    with pytest.raises(pkg.DQNError, match=r"tabular env: .*this engine has a communicator \(dqn_comm_init\)"):
        c.envs_create_tabular(**wide["tab"].kwargs(), n_envs=8, max_episode_length=5, seed=1)
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    s = TC.make_engine(pkg, nn, wide)
    monkeypatch.delenv("DQN_SIM_WORLD")
    with pytest.raises(pkg.DQNError, match="DQN_SIM_WORLD"):
        s.envs_create_tabular(**wide["tab"].kwargs(), n_envs=8, max_episode_length=5, seed=1)


def test_solve_tiger_on_device_envs(mods):
    """test/runtests.jl:149-163 on the device loop, 8 copies: a policy whose actionvalues has shape (3,); the replay stays at the host prefill's size"""
    pkg, nn, envs, S = mods
    env = envs.TigerPOMDP(0.01, -1.0, 0.1, 0.8, 0.95, n=8, seed=1)
    model = nn.Chain(nn.flattenbatch, nn.LSTM(1, 4), nn.Dense(4, env.n_actions))
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.01, steps=150))
    solver = S.DeepQLearningSolver(qnetwork=model, prioritized_replay=False, max_steps=300, learning_rate=0.0001, exploration_policy=expl, log_freq=500, eval_freq=150,
                                   num_ep_eval=4, target_update_freq=1000, recurrence=True, trace_length=10, double_q=True, dueling=True, max_episode_length=100,
                                   train_start=8, buffer_size=16, batch_size=4, verbose=False, logdir=None, device_envs=True)
    policy = S.solve(solver, env)
    assert policy.actionvalues(env.observe()[0]).shape == (3,)
    assert policy.engine.episode_count()[0] == 8 and policy.engine.get_counters()["train_steps"] == 300 // 4
    assert policy.engine.envs_info() == (8, False)


def optimal_return(tab, horizon):
    """the best expected undiscounted return of one evaluation episode (at most `horizon` steps) from b0: backward induction on the tables in fp64"""
    T, R = tab.T.astype(np.float64), tab.R.astype(np.float64)
    T = T / T.sum(-1, keepdims=True)
    live = (tab.terminal == 0).astype(np.float64)
    V = np.zeros(tab.S)
    for _ in range(horizon):
        V = (T * (R + (V * live)[None, None, :])).sum(-1).max(1)
    b0 = tab.b0.astype(np.float64)
    return float(b0 / b0.sum() @ V)


def test_solve_wide_mdp_reaches_a_fraction_of_the_optimal_return(mods):
    """wide_mdp with the goal reward (+1 on entering state 69, -1 on entering state 33, -0.01 per step): the optimal return of an evaluation episode (101 steps at most)
    is 0.7954 by value iteration on the tables.  solve() on the device loop must reach 0.75 of it under dqn_evaluate (256 episodes).
    Where 0.75 comes from: the HOST loop on the CPU twin engine for this configuration (8 copies, 4000 vector steps, one train step per vector step) returned 0.716 =
    0.90 of the optimum at seed 0, and 0.672 .. 0.728 (0.845 .. 0.915 of it) over seeds 0 .. 4; 0.75 leaves 0.15 of the optimum under the seed-0 figure and 0.095
    under the worst of the five seeds -- the device loop draws its exploration and dynamics from another generator, so it is one more sample of that spread."""
    pkg, nn, envs, S = mods
    tab = TC.wide_tables("goal")
    opt = optimal_return(tab, 101)
    assert abs(opt - 0.7954) < 1e-3
    env = envs.TabularPOMDP(n=8, seed=0, discount=0.95, **tab.kwargs())
    model = nn.Chain(nn.Dense(8, 16, nn.relu), nn.Dense(16, 4))
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.05, steps=2000))
    solver = S.DeepQLearningSolver(qnetwork=model, max_steps=4000, learning_rate=0.002, exploration_policy=expl, eval_freq=10 ** 6, num_ep_eval=8, train_freq=1, log_freq=500,
                                   target_update_freq=200, double_q=True, dueling=True, prioritized_replay=True, verbose=False, logdir=None, buffer_size=8192,
                                   train_start=64, batch_size=32, max_episode_length=100, seed=0, device_envs=True)
    policy = S.solve(solver, env)
    got, steps = policy.engine.evaluate(256, 100, seed=99)
    print(f"wide_mdp goal: optimal {opt:.4f}, device loop {got:.4f} ({got / opt:.3f} of it), {steps:.1f} steps per episode")
    assert policy.engine.envs_info() == (8, False)
    assert got >= 0.75 * opt, (got, opt)
