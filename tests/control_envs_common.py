"""Shared pieces of the control device-environment tests (TEST INFRASTRUCTURE): MountainCar and InvertedPendulum on the device loop (dqn_envs_create_control).

The comparison rule.  The device's cos / sin and NumPy's are both close to correctly rounded but are not the same function, so a Float64 state is compared with
the tolerance 1e-12 * max(1, |value|): at most ~30 double operations on values of order 1-10 plus library functions accurate to a few ulp give an error near 1e-14;
the tolerance leaves two orders of margin and sits five orders below the Float32 observation's resolution, so a wrong constant or a wrong order of the update cannot
hide under it.  After each vector step the device's (prev -> state) pairs are checked against the twin's law applied to the DEVICE'S OWN prev, then the device's
state is adopted; everything downstream (observations, rewards, dones, actions, draws, ring rows, priorities, episode commits, hidden state) is bit for bit.
Every branch quantity must lie further than 1e-9 from its switch point at every step (asserted on whatever states the driver sees).

Philox, u01, the eps schedule, the episode-ring model and the shadow engine are those of the recurrent env tests; FFRing is the tabular tests'.
"""
import numpy as np

from recurrent_envs_common import RingModel, Shadow, explore, hidden_equal, load, noisy_params, philox, u01      # noqa: F401
from tabular_envs_common import FFRing      # noqa: F401
from exploration_common import InteriorTally, P_SOFTMAX, softmax_law32      # noqa: F401

P_NOISE, P_THETA0, P_OMEGA0 = 12, 13, 14      # DQN_ENV_RAND_PEND_*
TOL, MARGIN = 1e-12, 1e-9


def draws(seed, t, n, purpose):
    """Float64(u01(philox(seed, t, i, purpose))) for i < n, from the tests' own scalar Philox"""
    return np.array([np.float64(u01(philox(seed, t, i, purpose))) for i in range(n)], np.float64)


def close(got, want):
    return np.all(np.abs(got - want) <= TOL * np.maximum(1.0, np.abs(want)))


def cases(envs):
    """name -> (env spec, max_episode_length): the smallest starts that reach the goal with its jackpot, the wall, the clamp, truncation, and the pendulum's fall"""
    return {
        "mc_goal": (envs.MountainCar(x0=0.45, v0=0.05), 100),      # reaches the goal, the jackpot and the reset within two steps
        "mc_wall": (envs.MountainCar(x0=-1.19, v0=-0.07), 3),       # hits the wall in its first step; truncated after three
        "mc_clamp": (envs.MountainCar(x0=0.0, v0=-0.07), 2),        # gravity pulls v below -v_max: the clamp
        "pend": (envs.InvertedPendulum(init_half=1.5), 100),        # falls (the terminal and its cost), then the random reset
    }


def ff_net(nn, dueling):
    net = nn.Chain(nn.Dense(2, 8, nn.tanh), nn.Dense(8, 3))
    return nn.create_dueling_network(net) if dueling else net


def make_engine(pkg, nn, net, B=4, cap=256, rec=0, T=1, mfma=1, graph=1, **hp_kw):
    layers, dueling = nn.lower(net)
    kw = dict(batch_size=B, n_actions=3, obs_c=2, obs_h=1, obs_w=1, dueling=int(dueling), buffer_size=cap, recurrence=rec, trace_length=T, learning_rate=1e-2,
              prioritized_replay=0 if rec else 1, use_mfma=mfma, use_graph=graph, seed=3, gamma=0.99, double_q=1)
    kw.update(hp_kw)
    return pkg.Engine(layers, pkg.default_hparams(**kw))


def linear_params(kind):
    """Dense(2, 3), identity: the flat vector is W[in][out] then the bias.  mc: Q = [-v, 0, +v]; pend: Q = [-(theta + omega), 0, theta + omega]; left: Q = [1, 0, 0]"""
    return np.array({"mc": [0, 0, 0, -1, 0, 1, 0, 0, 0], "pend": [-1, 0, 1, -1, 0, 1, 0, 0, 0], "left": [0, 0, 0, 0, 0, 0, 1, 0, 0]}[kind], np.float32)


def linear_q(kind, obs):
    """the Q columns of linear_params(kind) on Float32 observations, as an fma chain from +0 gives them (every product is exact)"""
    z = {"mc": obs[:, 1], "pend": obs[:, 0] + obs[:, 1], "left": None}[kind]
    if z is None:
        return np.tile(np.array([1, 0, 0], np.float32), (len(obs), 1))
    return np.stack([-z, np.zeros_like(z), z], 1).astype(np.float32)


def twin_evaluation(env_spec, kind, n_eval, max_len, seed):
    """basic_evaluation on the CPU twin under the linear controller: (avg_reward, avg_steps), the Float64 sums in copy order, and the smallest branch margin met"""
    env = env_spec.host_copy(n_eval, seed=seed)
    tot, steps, alive, margin = np.zeros(n_eval, np.float64), np.zeros(n_eval, np.int64), np.ones(n_eval, bool), np.inf
    while alive.any():
        a = np.argmax(linear_q(kind, env.observe()), axis=1)
        r = env.act(a)
        margin = min(margin, float(env.margin[alive].min()))
        tot[alive] += r[alive].astype(np.float64); steps[alive] += 1
        alive &= ~(env.terminated() | (steps > max_len))
    want = 0.0
    for i in range(n_eval):
        want += tot[i]
    return want / n_eval, steps.sum() / n_eval, margin


class ControlLockStep:
    """advances `g` (an engine with a control env set) one vector step at a time beside the twin's law, the ring model (RingModel for a recurrent engine, FFRing
    for a feed-forward one) and the shadow engine.

    LIMITATION (feed-forward engines).  They train inside the rollout and the shadow takes g's online parameters before every step, so its greedy actions are those
    of the network that acts -- but the feed-forward train step itself (the prioritized draw from the ring these kinds wrote, the update) is NOT compared with
    anything here; only the number of train steps is.  The recurrent lock step does compare loss, gradient norm and parameters with the shadow's sampled step.

    explore_table(t) -> ("eps", [eps]) or ("softmax", [tau]) runs the step through dqn_rollout_explore.  An eps table is held bit for bit.  A softmax pick is judged
    as the exploration tests judge it (exploration_common.judge_softmax): against the fp64 softmax of the SHADOW's forward on the pre-step observations and the
    purpose-11 draw, each interval widened by the derived delta (the device's expf and NumPy's exp need not agree to the last bit, so bit for bit cannot be held);
    the device's action is then taken as given"""

    def __init__(self, g, spec, n, max_len, seed, model, shadow, eps=(0.0, 0.0, 1.0), train_freq=0, target_update_freq=0, B=1, rec=False, explore_table=None):
        self.g, self.spec, self.n, self.max_len, self.seed, self.model, self.shadow, self.eps = g, spec, n, max_len, seed, model, shadow, eps
        self.tf, self.tu, self.B, self.rec, self.xt = train_freq, target_update_freq, B, rec, explore_table
        self.law = spec.host_copy(n, seed=seed)      # used for its laws only
        self.ep_step = np.zeros(n, np.int64)
        self.t, self.trained, self.explored = 1, 0, 0
        self.seen = dict(goal=False, wall=False, clamp=False, fall=False, truncated=False, reset=False)
        self.min_margin = np.inf
        self.tally, self.law32_agree, self.off_greedy = InteriorTally(), 0, 0
        self.s = self.law.reset_law(draws(seed, 0, n, P_THETA0), draws(seed, 0, n, P_OMEGA0))
        state, prev = g.envs_peek_state()
        np.testing.assert_array_equal(state, self.s, err_msg="the first reset"); np.testing.assert_array_equal(prev, 0.0)
        np.testing.assert_array_equal(g.envs_peek()[0].reshape(n, 2), self.s.astype(np.float32))

    def step(self):
        t, n, g, seed = self.t, self.n, self.g, self.seed
        obs_prev = self.s.astype(np.float32)
        if not self.rec:
            self.shadow.e.set_params(g.get_params(0), 0)
        greedy = self.shadow.greedy(obs_prev)
        softmax = bool(self.xt) and self.xt(t)[0] == "softmax"
        q_model = self.shadow.e.forward(obs_prev) if softmax else None      # (feed-forward shadows only: a forward would advance a recurrent one's state twice)
        kw = dict(explore=self.xt(t)) if self.xt else {}
        st = g.rollout(1, t0=t, train_freq=self.tf, target_update_freq=self.tu, eps=self.eps, **kw)
        obs, a, r, d = g.envs_peek()
        q, gr = g.envs_peek_q()
        state, prev = g.envs_peek_state()
        np.testing.assert_array_equal(prev, self.s, err_msg=f"the pre-step state at step {t}")
        np.testing.assert_array_equal(gr, np.argmax(q, axis=1)); np.testing.assert_array_equal(gr, greedy, err_msg=f"greedy actions at step {t}")
        eps = self.eps
        if softmax:
            tau = float(np.float32(self.xt(t)[1][0]))
            for i in range(n):
                u = u01(philox(seed, t, i, P_SOFTMAX))
                assert self.tally.add(q_model[i], tau, u, a[i]), (t, i, tau, float(u), int(a[i]), q_model[i])
                self.law32_agree += int(softmax_law32(q_model[i], tau, u) == a[i]); self.off_greedy += int(a[i] != greedy[i])
        elif self.xt:      # an eps table (dqn_rollout_explore): values[0] is this step's eps, the linear law is ignored
            v = np.float32(self.xt(t)[1][0]); eps = (v, v, 0.0)
        if not softmax:
            ex = [explore(seed, t, i, eps, 3) for i in range(n)]
            self.explored += sum(x is not None for x in ex)
            want_a = np.array([greedy[i] if ex[i] is None else ex[i] for i in range(n)], np.int32)
            np.testing.assert_array_equal(a, want_a, err_msg=f"actions at step {t}")
        # the law on the device's own prev
        s2, r_m, d_m, margin = self.law.step_law(prev, a, draws(seed, t, n, P_NOISE))
        assert margin.min() > MARGIN, (t, margin)
        self.min_margin = min(self.min_margin, float(margin.min()))
        np.testing.assert_array_equal(r, r_m.astype(np.float32), err_msg=f"rewards at step {t}"); np.testing.assert_array_equal(d, d_m.astype(np.uint8), err_msg=f"dones at step {t}")
        self.ep_step += 1
        ended = d_m | (self.ep_step >= self.max_len)
        assert close(state[~ended], s2[~ended]), (t, state[~ended] - s2[~ended])
        fresh = self.law.reset_law(draws(seed, t, n, P_THETA0), draws(seed, t, n, P_OMEGA0))
        np.testing.assert_array_equal(state[ended], fresh[ended], err_msg=f"reset states at step {t}")      # no library function in a reset: exact
        post = np.where(ended[:, None], s2, state)      # an ended copy's post-step state is visible as its Float32 ring row only: the twin's stands in
        if self.law.KIND == 3:
            c = self.law.c
            self.seen["goal"] |= bool(d_m.any()); self.seen["wall"] |= bool(((post[:, 0] == c["x_min"]) & (post[:, 1] == 0)).any())
            self.seen["clamp"] |= bool((np.abs(post[:, 1]) == c["v_max"]).any())
        else:
            self.seen["fall"] |= bool(d_m.any())
        self.seen["truncated"] |= bool((ended & ~d_m).any()); self.seen["reset"] |= bool(ended.any())
        sp = post.astype(np.float32)
        self.model.add(obs_prev, a, r_m.astype(np.float32), sp, d_m.astype(np.uint8))
        if self.rec:
            for i in np.nonzero(ended & ~d_m)[0]:
                self.model.note_truncated(int(i))
            if self.tf > 0 and t % self.tf == 0 and self.model.size >= self.B:
                loss, gn = self.shadow.train(self.model, 1)
                self.trained += 1
                assert st["train_steps"] == 1 and (st["loss"], st["grad_norm"]) == (loss, gn)
                np.testing.assert_array_equal(g.get_params(0), self.shadow.e.get_params(0))
            else:
                assert st["train_steps"] == 0
            if self.tu > 0 and t % self.tu == 0:
                self.shadow.e.sync_target()
            self.shadow.reset_columns(ended)
        else:
            self.trained += st["train_steps"]
        self.s = state.copy()
        self.ep_step[ended] = 0
        np.testing.assert_array_equal(obs.reshape(n, 2), self.s.astype(np.float32), err_msg=f"observations after step {t}")
        if self.rec:
            self.model.check(g)
            hidden_equal(g.get_hidden(n), self.shadow.e.get_hidden(n))
        self.t += 1
        return st, a, ended
