"""Shared pieces of the exploration tests (TEST INFRASTRUCTURE): dqn_rollout_explore's two laws restated without the code under test.

  softmax_law32    the softmax law of include/dqn_mi355x.h in NumPy fp32, operation by operation (np.exp in fp32 stands where the device calls expf: the two need not
                   agree to the last bit, which is why only the exact ends of the temperature range are compared bit for bit)
  softmax_model64  an fp64 model of it on the same fp32 q and tau: the cumulative probabilities b_0 = 0 <= b_1 <= ... <= b_nA = 1
  delta_for        the half-width by which an interval of the fp64 model is widened before a device pick is judged against it (derived in
                   tests/test_exploration_gpu.py::test_softmax_interior)
  XLockStep        a lock-step driver that takes the device's peeked action AS GIVEN for the mirror env, so one accepted near-boundary pick cannot derail the rest of
                   the trajectory; what the action should have been is decided by a `judge` the test passes in

Philox, u01, the mirrors, the ring model and the shadow engine are those of the recurrent / tabular env tests.
"""
import numpy as np

from recurrent_envs_common import RingModel, Shadow, hidden_equal, load, make_mirror, noisy_params, philox, u01      # noqa: F401
import recurrent_envs_common as RC      # noqa: F401
import tabular_envs_common as TC        # noqa: F401

P_EXPLORE, P_RANDOM, P_SOFTMAX = 1, 2, 11      # Philox purposes: explore or not, the random action, the softmax draw (DQN_ENV_RAND_SOFTMAX)
EPS32 = 2.0 ** -24                             # unit roundoff of fp32
EXPF_ULP = 2.0                                 # expf's error bound in ulp: no accuracy table of the device library is installed beside the compiler, so 2 ulp is ASSUMED (unmeasured)


# ------------------------------------------------------------------ the eps law
def eps_explore(seed, t, i, eps, n_actions):
    """None (greedy) or the random action of copy i at vector step t under eps = the fp32 table value"""
    if u01(philox(seed, t, i, P_EXPLORE)) < np.float32(eps):
        return philox(seed, t, i, P_RANDOM) % n_actions
    return None


# ------------------------------------------------------------------ the softmax law
def softmax_law32(q, tau, u, seen=None):
    """z = q / tau; m = max z; w = exp(z - m); c_k = c_{k-1} + w_k ascending; target = u * c_last; the first k with target < c_k, else the last k with c_k > c_{k-1}"""
    q = np.asarray(q, np.float32)
    tau, u = np.float32(tau), np.float32(u)
    z = (q / tau).astype(np.float32)
    m = np.float32(z.max())
    w = np.exp((z - m).astype(np.float32)).astype(np.float32)
    c, acc = np.empty(q.size, np.float32), np.float32(0)
    for k in range(q.size):
        acc = np.float32(acc + w[k])
        c[k] = acc
    return cum_pick(c, np.float32(u * c[-1]), seen)


def cum_pick(c, target, seen=None):
    for k in range(len(c)):
        if target < c[k]:
            return k
    rose = [k for k in range(len(c)) if c[k] > (c[k - 1] if k else np.float32(0))]
    if seen is not None:
        seen["fallback"] = True
    return rose[-1] if rose else 0


def softmax_model64(q, tau):
    """boundaries b[0 .. nA] of the fp64 softmax on the fp32 q and tau: action k owns [b[k], b[k + 1])"""
    z = np.asarray(q, np.float32).astype(np.float64) / np.float64(np.float32(tau))
    w = np.exp(z - z.max())
    b = np.concatenate([[0.0], np.cumsum(w)])
    return b / b[-1]


def delta_for(q, tau):
    """the widening of one draw's intervals: 2 * [2 * (2 Z + D + 2 * EXPF_ULP) + 2 nA - 1] * 2^-24 with Z = max |q_k / tau|, D = max (m - z_k) (the derivation is in
    the docstring of tests/test_exploration_gpu.py::test_softmax_interior)"""
    z = np.asarray(q, np.float32).astype(np.float64) / np.float64(np.float32(tau))
    Z, D, nA = np.abs(z).max(), z.max() - z.min(), z.size
    return 2.0 * (2.0 * (2.0 * Z + D + 2.0 * EXPF_ULP) + 2.0 * nA - 1.0) * EPS32


def judge_softmax(q, tau, u, a):
    """(accepted, needed_widening, distance of u to the nearest inner boundary, delta) of the device's pick a"""
    b, d = softmax_model64(q, tau), delta_for(q, tau)
    u = float(u)
    exact = b[a] <= u < b[a + 1]
    ok = b[a] - d <= u < b[a + 1] + d
    inner = b[1:-1]
    dist = float(np.abs(inner - u).min()) if inner.size else 1.0
    return ok, ok and not exact, dist, d


# ------------------------------------------------------------------ the lock-step driver
class XLockStep:
    """advances `g` one vector step at a time under dqn_rollout_explore beside a mirror env (TabMirror or the built-in kinds' mirrors), a shadow engine that supplies the Q
    column of the pre-step observations (forward on n streams: on a recurrent engine that call also advances the shadow's Recur state, as the acting step advances the
    device's) and, for a recurrent engine, the episode-ring model.  No training: train_freq = 0"""

    def __init__(self, g, mirror, n, n_actions, max_len, seed, shadow_engine, rec=False, shadow=None, model=None):
        self.g, self.mirror, self.n, self.nA, self.max_len, self.seed = g, mirror, n, n_actions, max_len, seed
        self.se, self.rec, self.shadow, self.model = shadow_engine, rec, shadow, model
        self.ep_step = np.zeros(n, np.int64)
        self.t = 1

    def step(self, kind, value, judge):
        """judge(t, q [n, nA], a [n]) asserts what it must about the device's actions"""
        t, n, g = self.t, self.n, self.g
        obs_prev = self.mirror.observe()
        q = self.se.forward(obs_prev)
        g.rollout(1, t0=t, train_freq=0, target_update_freq=0, explore=(kind, [value]), stats=False)
        obs, a, r, d = g.envs_peek()
        assert a.min() >= 0 and a.max() < self.nA
        judge(t, q, a)
        r_m, d_m = self.mirror.step(t, a)
        sp = self.mirror.observe()
        np.testing.assert_array_equal(r, r_m, err_msg=f"rewards at step {t}"); np.testing.assert_array_equal(d, d_m, err_msg=f"dones at step {t}")
        if self.model is not None:
            self.model.add(obs_prev, a, r_m, sp, d_m)
        self.ep_step += 1
        ended = (d_m != 0) | (self.ep_step >= self.max_len)
        if self.rec and self.model is not None:
            for i in np.nonzero(ended & (d_m == 0))[0]:
                self.model.note_truncated(int(i))
        self.mirror.reset(ended, t)
        self.ep_step[ended] = 0
        if self.rec:
            self.shadow.reset_columns(ended)
        np.testing.assert_array_equal(obs.reshape(n, -1), self.mirror.observe().reshape(n, -1), err_msg=f"observations after step {t}")
        if self.rec:
            if self.model is not None:
                self.model.check(g)
            hidden_equal(g.get_hidden(n), self.se.get_hidden(n))
        self.t += 1
        return a, q, ended


def first_max(q):
    """the greedy action: the first maximum of each row"""
    return np.argmax(np.asarray(q), axis=1).astype(np.int32)


# ------------------------------------------------------------------ cases
def wide_case(nn, n):
    """the feed-forward tabular case of the tabular env tests (S = 70, nA = 4, E = 8, dueling MLP) with n copies"""
    c = dict(TC.cases(nn)["wide_mdp"])
    c["n"] = n
    return c


def eps_blocks(steps):
    """a table drawn from {0, 1, 0.5, 2^-24, 0.25}: blocks of three, then alternating"""
    vals = [0.0, 1.0, 0.5, 2.0 ** -24, 0.25]
    out = []
    for v in vals:
        out += [v] * 3
    k = 0
    while len(out) < steps:
        out.append(vals[k % len(vals)]); k += 1
    return np.array(out[:steps], np.float32)


GREEDY_SCALE = 8.0                 # the wide case's noisy parameters times this: the greedy margin of every one of the 70 states is 1.59 or more on the CPU twin (asserted > 0.2 in tests/test_exploration_cpu.py)
TAUS = (10.0, 1.0, 0.3, 0.05)      # the interior test cycles through these
INTERIOR_N, INTERIOR_STEPS = 32, 16
INTERIOR_SEED = 7                  # env seed of the interior test: chosen on the CPU twin (tests/test_exploration_cpu.py) so that the fp64 model alone keeps <= 1 % of the draws within delta of a boundary


def interior_tau(t):
    return TAUS[(t - 1) % len(TAUS)]


class InteriorTally:
    """what the interior test counts over its draws: picks per temperature, draws within delta of an inner boundary, draws that needed the widening"""

    def __init__(self):
        self.draws = self.near = self.widened = 0
        self.max_delta = self.max_widened_dist = 0.0
        self.picks = {}

    def add(self, q, tau, u, a):
        ok, widened, dist, d = judge_softmax(q, tau, u, a)
        self.draws += 1
        self.near += dist <= d
        self.max_delta = max(self.max_delta, d)
        if widened:
            self.widened += 1
            self.max_widened_dist = max(self.max_widened_dist, dist)
        self.picks.setdefault(tau, set()).add(int(a))
        return ok

    def check(self):
        assert self.near <= self.draws // 100, (self.near, self.draws)      # at most 1 % of the draws within delta of a boundary
        for tau, got in self.picks.items():
            if tau >= 0.3:
                assert len(got) == 4, (tau, sorted(got))
