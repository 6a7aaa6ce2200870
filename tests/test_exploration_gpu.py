"""GPU (-m gpu): exploration by table on the device env loop (dqn_rollout_explore): an eps table against the engine's own linear law (GPU against GPU, bit for bit),
the exact exploring set of an eps table, the softmax law at its exact ends and in its interior (against an fp64 model with a derived tolerance), both on feed-forward
and recurrent engines, every refusal by its message, and solve(device_envs=True) with a SoftmaxPolicy and with a callable eps.  The references live in
tests/exploration_common.py; seeds and scales are chosen on the CPU twin (tests/test_exploration_cpu.py)."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as ge
import envs_common as EC
import exploration_common as XC
import ref

pytestmark = pytest.mark.gpu
TC, RC = XC.TC, XC.RC


@pytest.fixture(scope="module")
def mods():
    p = ge.load_package(); p.lib()
    return (p,) + XC.load(p)


# ------------------------------------------------------------------ 1. an eps table of the linear law's values walks the linear law's trajectory
@pytest.mark.parametrize("case", ["gridworld", "wide_fc_dueling"])
def test_eps_table_equals_the_linear_law(mods, case):
    """two engines with the same network, seed and parameters: one runs rollout(eps=(1, 0, 64)), the other a table of the same values 1 - t / 64 (exact in fp32, so the
    linear law's own arithmetic rounds nowhere).  48 single vector steps with train_freq = 4, then 16 more in chunks of 5 and 11 (the table indexed by t - t0 inside
    one call, whole cycles replayed as one graph); once with the vector-step cadence and once with cadence_env_steps = 1.  dqn_envs_peek after every call, then the
    replay export with its priorities, the counters and both parameter vectors: bit for bit.  wide_fc_dueling is a fused-tail shape: the linear engine runs
    k_act_head, the table engine the general four-launch tail"""
    pkg, nn, envs, S = mods
    net = {"gridworld": EC.gridworld_mlp_dueling, "wide_fc_dueling": EC.testmdp_wide_fc_dueling}[case]()
    grid = case == "gridworld"
    for cadence in (False, True):
        hp = ref.hparams_for(net, batch_size=32 if grid else 8, buffer_size=1024 if grid else 160)
        layers = ref.layers_from_network(net)
        a, b = pkg.Engine(layers, hp), pkg.Engine(layers, hp)
        EC.same_params([a, b], net)
        spec = envs.SimpleGridWorld(n=8) if grid else envs.TestMDP((20, 20), 4, 6, n=8, seed=3)
        for h in (a, b):
            h.envs_create(spec, max_episode_length=20 if grid else 100, seed=17)
        if not grid:
            assert a.envs_info() == (8, True) and b.envs_info() == (8, True)      # (what dqn_rollout uses: the table engine reports it too)
        table = lambda t0, k: np.array([1.0 - t / 64.0 for t in range(t0, t0 + k)], np.float32)
        t0 = 1
        for chunk in [1] * 48 + [5, 11]:
            kw = dict(t0=t0, train_freq=4, target_update_freq=10, env_step_cadence=cadence)
            sa = a.rollout(chunk, eps=(1.0, 0.0, 64.0), **kw)
            sb = b.rollout(chunk, explore=("eps", table(t0, chunk)), **kw)
            t0 += chunk
            assert sa == sb, (t0, sa, sb)
            for x, y in zip(a.envs_peek(), b.envs_peek()):
                np.testing.assert_array_equal(x, y, err_msg=f"peek after step {t0 - 1}")
        assert sa["train_steps"] > 0 and sa["episodes"] > 0
        for x, y in zip(a.replay_export(), b.replay_export()):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(a.replay_priorities(), b.replay_priorities())
        assert a.get_counters() == b.get_counters() and a.replay_size() == b.replay_size()
        for which in (0, 1):
            np.testing.assert_array_equal(a.get_params(which), b.get_params(which))
        if not grid:
            assert b.envs_info() == (8, True)      # the fused program survived beside the general one
        a.close(); b.close()


# ------------------------------------------------------------------ set-ups of the lock-step tests
def ff_setup(mods, n, seed, scale=1.0, **kw):
    pkg, nn, envs, S = mods
    case = XC.wide_case(nn, n)
    p = (XC.noisy_params(nn, case["net"]) * scale).astype(np.float32)
    g, sh = TC.make_engine(pkg, nn, case, **kw), TC.make_engine(pkg, nn, case, **kw)
    for e in (g, sh):
        e.set_params(p, 0); e.sync_target()
    g.envs_create_tabular(**case["tab"].kwargs(), n_envs=n, max_episode_length=case["max_len"], seed=seed)
    ls = XC.XLockStep(g, TC.TabMirror(case["tab"], n, seed), n, 4, case["max_len"], seed, sh)
    np.testing.assert_array_equal(g.envs_peek()[0].reshape(n, -1), ls.mirror.observe().reshape(n, -1))
    return g, ls


def rec_setup(mods, name, n):
    pkg, nn, envs, S = mods
    case = RC.cases(nn, envs)[name]
    spec, net, _, T, cap, B, max_len = case
    seed = RC.ENV_SEED[name]
    p = RC.noisy_params(nn, net)
    g, _ = RC.make_engine(pkg, nn, case)
    e2, _ = RC.make_engine(pkg, nn, case)
    for e in (g, e2):
        e.set_params(p, 0); e.set_params((p * 0.9).astype(np.float32), 1)
    g.envs_create(spec, n_envs=n, max_episode_length=max_len, seed=seed)
    ls = XC.XLockStep(g, RC.make_mirror(spec, n, seed), n, 4, max_len, seed, e2, rec=True, shadow=RC.Shadow(e2, nn, net, n), model=RC.RingModel(n, T, cap, spec.obs_shape))
    np.testing.assert_array_equal(g.envs_peek()[0].reshape(n, -1), ls.mirror.observe().reshape(n, -1))
    return g, ls


def eps_judge(ls, eps, count):
    def judge(t, q, a):
        greedy = XC.first_max(q)
        want = [XC.eps_explore(ls.seed, t, i, eps, ls.nA) for i in range(ls.n)]
        count[0] += sum(x is not None for x in want)
        np.testing.assert_array_equal(a, np.array([greedy[i] if want[i] is None else want[i] for i in range(ls.n)], np.int32), err_msg=f"actions at step {t} (eps {eps})")
    return judge


# ------------------------------------------------------------------ 2. the exact exploring set of an eps table
@pytest.mark.parametrize("which", ["tabular_ff", "lstm"])
def test_eps_table_exact_exploring_set(mods, which):
    """a table drawn from {0, 1, 0.5, 2^-24, 0.25}, in blocks and alternating, 20 vector steps: where the Philox model says "explore" (u01(philox(.., 1)) < eps) the action
    is philox(.., 2) % nA, elsewhere the shadow's greedy action -- so eps = 1 explores on every copy and eps = 0 on none; rewards, dones and observations follow the
    mirror; on the recurrent case the Recur state equals the shadow's and the episode ring the model's after every step"""
    g, ls = ff_setup(mods, 8, TC.ENV_SEED["wide_mdp"]) if which == "tabular_ff" else rec_setup(mods, "lstm", 4)
    table = XC.eps_blocks(20)
    per_value = {}
    for eps in table:
        cnt = [0]
        ls.step("eps", eps, eps_judge(ls, eps, cnt))
        per_value.setdefault(float(eps), []).append(cnt[0])
    assert all(c == ls.n for c in per_value[1.0]) and all(c == 0 for c in per_value[0.0]) and all(c == 0 for c in per_value[2.0 ** -24])
    assert 0 < sum(per_value[0.5]) < ls.n * len(per_value[0.5])


# ------------------------------------------------------------------ 3. softmax, exact ends
def test_softmax_exact_ends(mods):
    """tau = 1e30: every weight is exactly 1 whatever the network says, so c_k = k + 1 and target = fp32(u * nA): the action equals the model's pick for every copy
    and step, bit for bit.  tau = 1e-3 on parameters scaled (XC.GREEDY_SCALE) so that the shadow's greedy margin exceeds 0.2 (asserted per draw): every other weight
    is expf of less than -200, which is zero, and the action is the greedy one"""
    g, ls = ff_setup(mods, 8, TC.ENV_SEED["wide_mdp"])
    def hot(t, q, a):
        for i in range(ls.n):
            target = np.float32(XC.u01(XC.philox(ls.seed, t, i, XC.P_SOFTMAX)) * np.float32(ls.nA))
            assert a[i] == XC.cum_pick(np.arange(1, ls.nA + 1, dtype=np.float32), target), (t, i)
    seen = set()
    for _ in range(12):
        a, _, _ = ls.step("softmax", 1e30, hot)
        seen |= set(a.tolist())
    assert seen == {0, 1, 2, 3}
    g.close()
    g, ls = ff_setup(mods, 8, TC.ENV_SEED["wide_mdp"], scale=XC.GREEDY_SCALE)
    def cold(t, q, a):
        s = np.sort(q, axis=1)
        assert (s[:, -1] - s[:, -2]).min() > 0.2
        np.testing.assert_array_equal(a, XC.first_max(q), err_msg=f"actions at step {t}")
    for _ in range(12):
        ls.step("softmax", 1e-3, cold)


# ------------------------------------------------------------------ 4. softmax, the interior
def softmax_judge(ls, tau, tally):
    def judge(t, q, a):
        for i in range(ls.n):
            u = XC.u01(XC.philox(ls.seed, t, i, XC.P_SOFTMAX))
            assert tally.add(q[i], tau, u, a[i]), (t, i, tau, float(u), int(a[i]), XC.softmax_model64(q[i], tau), XC.delta_for(q[i], tau))
    return judge


def test_softmax_interior(mods):
    """the feed-forward tabular case (nA = 4) with 32 copies over 16 vector steps, tau cycling through 10, 1, 0.3, 0.05: 512 draws.  q = the shadow's forward on the
    pre-step observations.  A pick a is accepted if u lies in [b_a - delta, b_{a+1} + delta), b = the cumulative probabilities of the fp64 softmax on the same fp32 q and tau.

    delta.  With e = 2^-24 (fp32 unit roundoff), Z = max_k |q_k / tau| and D = max_k (m - z_k) of the draw, to first order:
      division      z_k = (q_k / tau)(1 + e1), |e1| <= e: an absolute error of at most Z e in z_k and in m = max z (the maximum itself is exact);
      subtraction   d_k = (z_k - m)(1 + e2): against the exact (q_k - q_max) / tau, an absolute error of at most 2 Z e + D e;
      expf          w_k = exp(d_k)(1 + e3).  The bound of the device library's expf is not documented on the build machine, so 2 ulp is ASSUMED (not measured): one
                    ulp is at most 2 e relative, |e3| <= 4 e.  exp turns d_k's absolute error into a relative one: w_k is off by at most (2 Z + D + 4) e relative;
      additions     c_k is a sum of positive terms with at most nA - 1 roundings that matter: (2 Z + D + 4 + nA - 1) e relative;
      product       target = u c_last (1 + e5), |e5| <= e.
    The device decides target < c_k, that is u < (c_k / c_last) / (1 + e5): the ratio carries twice c's relative error, the product one more e, and b <= 1 turns
    the relative bound into an absolute one: |shift of a boundary| <= [2 (2 Z + D + 4) + 2 (nA - 1) + 1] e = [2 (2 Z + D + 4) + 2 nA - 1] e.  (Errors common to every
    w_k cancel in the ratio; the bound does not count on that.)  DOUBLED: delta = 2 [2 (2 Z + D + 2 * 2) + 2 nA - 1] 2^-24, per draw (XC.delta_for); over this test's
    draws it stays below 3.5e-5 (tau = 0.05 with |q| up to 2.5).

    At most 1 % of the 512 draws may lie within delta of a boundary (the seed was chosen so that the fp64 model alone meets this on the CPU twin's Q values:
    tests/test_exploration_cpu.py), and each of the 4 actions is picked at least once per temperature >= 0.3.  Measured on an MI355X: docs/history/exploration.md"""
    g, ls = ff_setup(mods, XC.INTERIOR_N, XC.INTERIOR_SEED)
    tally = XC.InteriorTally()
    for t in range(1, XC.INTERIOR_STEPS + 1):
        tau = XC.interior_tau(t)
        ls.step("softmax", tau, softmax_judge(ls, tau, tally))
    print(f"softmax interior: {tally.draws} draws, {tally.near} within delta of a boundary, {tally.widened} needed the widening "
          f"(largest |u - boundary| among them {tally.max_widened_dist:.3e}), largest delta {tally.max_delta:.3e}")
    assert tally.draws == 512
    tally.check()


# ------------------------------------------------------------------ 5. softmax on a recurrent engine
def test_softmax_recurrent(mods):
    """the GRU dueling case with 4 copies, 12 vector steps at tau = 1: picks accepted as in the interior test against the shadow's Q column (forward on 4 streams with
    carried state); the Recur state equals the shadow's and the episode ring the model's after every step -- every vector step advances every copy's state"""
    g, ls = rec_setup(mods, "gru_duel", 4)
    tally = XC.InteriorTally()
    for _ in range(12):
        ls.step("softmax", 1.0, softmax_judge(ls, 1.0, tally))
    print(f"softmax recurrent: {tally.draws} draws, {tally.near} within delta, {tally.widened} needed the widening, largest delta {tally.max_delta:.3e}")
    assert tally.draws == 48 and len(tally.picks[1.0]) >= 2


# ------------------------------------------------------------------ 6. refusals
def test_refusals_by_message_and_a_refused_call_leaves_no_trace(mods):
    pkg, nn, envs, S = mods
    abi = pkg._abi
    g, _ = ff_setup(mods, 8, 3)
    h, _ = ff_setup(mods, 8, 3)      # the twin that is never refused
    def bad(match, kind, values, n_steps=4):
        with pytest.raises(pkg.DQNError, match=match):
            g.rollout(n_steps, t0=1, train_freq=2, explore=(kind, values))
    bad(r"unknown kind 2", 2, [0.5])
    bad(r"unknown kind -1", -1, [0.5])
    bad(r"n_values = 3 is neither 1 nor n_vector_steps = 4", "eps", [0.1, 0.2, 0.3])
    bad(r"n_values = 5 is neither 1 nor n_vector_steps = 4", "softmax", [1.0] * 5)
    bad(r"eps values\[2\] = 1\.5 is outside \[0, 1\]", "eps", [0.0, 1.0, 1.5, 0.5])
    bad(r"eps values\[0\] = -0\.25 is outside \[0, 1\]", "eps", [-0.25])
    bad(r"eps values\[3\] = nan is outside \[0, 1\]", "eps", [0.0, 1.0, 0.5, np.nan])
    bad(r"temperature values\[1\] = 0 is not a finite positive number", "softmax", [1.0, 0.0, 1.0, 1.0])
    bad(r"temperature values\[0\] = -2 is not a finite positive number", "softmax", [-2.0])
    bad(r"temperature values\[3\] = inf is not a finite positive number", "softmax", [1.0, 1.0, 1.0, np.inf])
    bad(r"temperature values\[2\] = nan is not a finite positive number", "softmax", [1.0, 1.0, np.nan, 1.0])
    cfg = abi.RolloutCfg(2, 0, 0.0, 0.0, 1.0, 0, 1)
    for kind in (0, 1):      # NULL values: below the wrapper, which always has an array
        x = abi.Exploration(kind, 1, None)
        assert g.f["rollout_explore"](g._h, 4, ctypes.byref(cfg), ctypes.byref(x), None) != 0
        assert "values is NULL" in g.f["last_error"]().decode()
    for step, (kind, vals) in enumerate([("eps", [1.0, 0.5, 0.0, 0.25]), ("softmax", [0.5]), ("eps", [0.5])]):
        kw = dict(t0=1 + 4 * step, train_freq=2, target_update_freq=3, explore=(kind, vals))
        assert g.rollout(4, **kw) == h.rollout(4, **kw)
        for x, y in zip(g.envs_peek(), h.envs_peek()):
            np.testing.assert_array_equal(x, y)
    for x, y in zip(g.replay_export(), h.replay_export()):
        np.testing.assert_array_equal(x, y)
    assert g.get_counters() == h.get_counters()
    np.testing.assert_array_equal(g.get_params(0), h.get_params(0))


# ------------------------------------------------------------------ 7. solve(device_envs=True)
def test_solve_with_a_softmax_policy_reaches_the_return_bar(mods):
    """the known-optimum tabular MDP of test_tabular_envs_gpu (wide_mdp with the goal reward, optimal return 0.7954 by value iteration) under solve() on the device loop
    with a SoftmaxPolicy whose temperature decays linearly from 1 to 0.005 over 2000 vector steps: the same bar as that test's eps-greedy run, 0.75 of the optimum
    under dqn_evaluate (256 episodes).  The schedule is a hyper-parameter of this run, not a bound: the final temperature sits below the model's per-step cost of
    0.01, the scale of the Q gaps between the four actions of a state.  Over seeds 0 .. 4 on the device loop this schedule returned 0.823 .. 0.944 of the optimum (0.873
    at seed 0, which the test runs), 1 -> 0.02 returned 0.743 .. 0.906 (seed 0 the lowest, under the bar) and the eps-greedy configuration of test_tabular_envs_gpu
    0.833 .. 0.912 (docs/history/exploration.md)"""
    pkg, nn, envs, S = mods
    from test_tabular_envs_gpu import optimal_return
    tab = TC.wide_tables("goal")
    opt = optimal_return(tab, 101)
    env = envs.TabularPOMDP(n=8, seed=0, discount=0.95, **tab.kwargs())
    model = nn.Chain(nn.Dense(8, 16, nn.relu), nn.Dense(16, 4))
    expl = S.SoftmaxPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.005, steps=2000))
    solver = S.DeepQLearningSolver(qnetwork=model, max_steps=4000, learning_rate=0.002, exploration_policy=expl, eval_freq=10 ** 6, num_ep_eval=8, train_freq=1, log_freq=500,
                                   target_update_freq=200, double_q=True, dueling=True, prioritized_replay=True, verbose=False, logdir=None, buffer_size=8192,
                                   train_start=64, batch_size=32, max_episode_length=100, seed=0, device_envs=True)
    policy = S.solve(solver, env)
    got, steps = policy.engine.evaluate(256, 100, seed=99)
    print(f"wide_mdp goal under SoftmaxPolicy: optimal {opt:.4f}, device loop {got:.4f} ({got / opt:.3f} of it), {steps:.1f} steps per episode")
    assert got >= 0.75 * opt, (got, opt)


def test_solve_honours_a_callable_eps(mods):
    """eps = t -> 1 if t <= 8 else 0 over 16 vector steps (the parent froze any non-linear schedule at eps(1) without a word).  A recording engine shows the table
    dqn_train_device built; the replay shows the first 8 vector steps' actions are all the keyed random ones; and the same table, passed step by step through the
    engine, gives the exact exploring set: every copy for t <= 8, none after"""
    pkg, nn, envs, S = mods
    calls = []

    class Recording(pkg.Engine):
        def rollout(self, n_steps, **kw):
            calls.append((n_steps, dict(kw)))
            return super().rollout(n_steps, **kw)

    tab = TC.wide_tables("goal")
    env = envs.TabularPOMDP(n=8, seed=0, discount=0.95, **tab.kwargs())
    sched = lambda t: 1.0 if t <= 8 else 0.0
    solver = S.DeepQLearningSolver(qnetwork=nn.Chain(nn.Dense(8, 16, nn.relu), nn.Dense(16, 4)), max_steps=16, learning_rate=0.002, exploration_policy=S.EpsGreedyPolicy(env, sched),
                                   eval_freq=10 ** 6, train_freq=4, log_freq=10 ** 6, save_freq=10 ** 6, target_update_freq=200, verbose=False, logdir=None, buffer_size=512,
                                   train_start=64, batch_size=32, max_episode_length=100, seed=5, device_envs=True)
    policy = S.solve(solver, env, engine_cls=Recording)
    assert len(calls) == 1 and calls[0][0] == 16 and calls[0][1]["t0"] == 1 and "eps" not in calls[0][1]
    kind, vals = calls[0][1]["explore"]
    assert kind == "eps" and vals.dtype == np.float32
    np.testing.assert_array_equal(vals, np.array([1.0] * 8 + [0.0] * 8, np.float32))
    a = policy.engine.replay_export()[2]
    assert a.size == 64 + 16 * 8
    want = np.array([XC.philox(5, t, i, XC.P_RANDOM) % 4 for t in range(1, 9) for i in range(8)], np.int32)
    np.testing.assert_array_equal(a[64:128], want)
    g, ls = ff_setup(mods, 8, 5)
    for t in range(1, 17):
        cnt = [0]
        ls.step("eps", vals[t - 1], eps_judge(ls, vals[t - 1], cnt))
        assert cnt[0] == (8 if t <= 8 else 0)
