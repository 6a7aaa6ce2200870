"""Shared pieces of the tabular device-environment tests (TEST INFRASTRUCTURE).

There is no CPU twin of this path.  The reference is a NumPy restatement of the sampling law of include/dqn_mi355x.h that owes nothing to the code under test:
cumulative rows by an explicit np.float32 loop, u = u01(philox(seed, t, i, purpose)), np.searchsorted(cdf, u, side="right") plus the fallback (the last index at
which the row still rose).  Philox, u01, the eps schedule, the episode-ring model and the shadow engine are those of the recurrent env tests; the lock-step driver
is this file's own (the recurrent one hard-codes 4 actions and picks its mirror by attribute).
"""
import numpy as np

from recurrent_envs_common import RingModel, Shadow, eps_at, explore, hidden_equal, load, noisy_params, philox, u01      # noqa: F401

P_NEXT, P_OBS, P_INIT, P_INIT_OBS = 7, 8, 9, 10      # the four purposes of the tabular kind (DQN_ENV_RAND_TAB_*)


def cumrows(p):
    """cumulative rows along the last axis: acc = acc + p in fp32, ascending index order"""
    p = np.asarray(p, np.float32)
    out = np.empty_like(p)
    flat_p, flat_o = p.reshape(-1, p.shape[-1]), out.reshape(-1, p.shape[-1])
    for r in range(flat_p.shape[0]):
        acc = np.float32(0)
        for j in range(flat_p.shape[1]):
            acc = np.float32(acc + flat_p[r, j])
            flat_o[r, j] = acc
    return out


FLAGS = ("fallback", "zero_left", "zero_right", "first", "last")


def pick(cdf, u, seen=None):
    """the first j with u < cdf[j]; if none, the last j with cdf[j] > cdf[j - 1] (cdf[0] > 0 for j = 0)"""
    K = len(cdf)
    j = int(np.searchsorted(cdf, u, side="right"))
    fb = j == K
    if fb:
        rose = [k for k in range(K) if cdf[k] > (cdf[k - 1] if k else np.float32(0))]
        j = rose[-1] if rose else 0
    if seen is not None:
        prob = lambda k: cdf[k] - (cdf[k - 1] if k else np.float32(0))
        seen["fallback"] |= fb
        seen["zero_left"] |= j > 0 and prob(j - 1) == 0
        seen["zero_right"] |= j + 1 < K and prob(j + 1) == 0
        seen["first"] |= j == 0
        seen["last"] |= j == K - 1
    return j


class Tables:
    """a tabular (PO)MDP: T[S, A, S], R[S, A, S], terminal[S], b0[S], features[O or S, E], Z[A, S, O] / Z0[S, O] or None"""

    def __init__(self, T, R, terminal, b0, features, Z=None, Z0=None):
        self.T, self.R = np.ascontiguousarray(T, np.float32), np.ascontiguousarray(R, np.float32)
        self.terminal, self.b0 = np.ascontiguousarray(terminal, np.uint8), np.ascontiguousarray(b0, np.float32)
        self.features = np.ascontiguousarray(features, np.float32)
        self.Z = None if Z is None else np.ascontiguousarray(Z, np.float32)
        self.Z0 = None if Z0 is None else np.ascontiguousarray(Z0, np.float32)
        self.S, self.A = self.T.shape[0], self.T.shape[1]
        self.O = 0 if self.Z is None else self.Z.shape[-1]
        self.obs_shape = self.features.shape[1:]
        self.cT, self.cb0 = cumrows(self.T), cumrows(self.b0)
        self.cZ, self.cZ0 = (cumrows(self.Z), cumrows(self.Z0)) if self.O else (None, None)

    def kwargs(self):
        return dict(T=self.T, R=self.R, terminal=self.terminal, b0=self.b0, features=self.features, Z=self.Z, Z0=self.Z0)


class TabMirror:
    """n copies stepped by the law, draws keyed by (seed, vector step, copy, purpose)"""

    def __init__(self, tab, n, seed):
        self.tab, self.n, self.seed = tab, n, seed
        self.s, self.o = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.seen = dict.fromkeys(FLAGS, False)
        self.counts = dict(T=np.zeros(tab.T.shape, np.int64), b0=np.zeros(tab.S, np.int64),
                           Z=None if not tab.O else np.zeros(tab.Z.shape, np.int64), Z0=None if not tab.O else np.zeros(tab.Z0.shape, np.int64))
        self.reset(np.ones(n, bool), 0)

    def u(self, t, i, purpose):
        return u01(philox(self.seed, t, int(i), purpose))

    def reset(self, mask, t):
        tb = self.tab
        for i in np.nonzero(mask)[0]:
            s = pick(tb.cb0, self.u(t, i, P_INIT), self.seen)
            self.counts["b0"][s] += 1
            o = s
            if tb.O:
                o = pick(tb.cZ0[s], self.u(t, i, P_INIT_OBS), self.seen)
                self.counts["Z0"][s, o] += 1
            self.s[i], self.o[i] = s, o

    def observe(self):
        return self.tab.features[self.o]

    def step(self, t, a):
        tb = self.tab
        r, d = np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)
        for i in range(self.n):
            s, ai = int(self.s[i]), int(a[i])
            sp = pick(tb.cT[s, ai], self.u(t, i, P_NEXT), self.seen)
            self.counts["T"][s, ai, sp] += 1
            o = sp
            if tb.O:
                o = pick(tb.cZ[ai, sp], self.u(t, i, P_OBS), self.seen)
                self.counts["Z"][ai, sp, o] += 1
            r[i], d[i] = tb.R[s, ai, sp], tb.terminal[sp]
            self.s[i], self.o[i] = sp, o
        return r, d


# ------------------------------------------------------------------ the three cases
def tiger_tables(r_listen=-1.0, r_findtiger=-100.0, r_escapetiger=10.0, p=0.85):
    """POMDPModels.TigerPOMDP, recalled, written out entry by entry.  State / observation index = the Bool (0 tiger right, 1 tiger left); actions listen, open-left,
    open-right"""
    T = [[[1.0, 0.0], [0.5, 0.5], [0.5, 0.5]],
         [[0.0, 1.0], [0.5, 0.5], [0.5, 0.5]]]
    Z = [[[p, 1.0 - p], [1.0 - p, p]],
         [[0.5, 0.5], [0.5, 0.5]],
         [[0.5, 0.5], [0.5, 0.5]]]
    R = [[[r_listen] * 2, [r_escapetiger] * 2, [r_findtiger] * 2],
         [[r_listen] * 2, [r_findtiger] * 2, [r_escapetiger] * 2]]
    return Tables(T, R, [0, 0], [0.5, 0.5], [[0.0], [1.0]], Z=Z, Z0=Z[0])


def sparse_tables():
    """S = 5, O = 3, A = 3, E = 6.  Zero entries at the front, in the middle and at the end of rows; one row per table (two of T) sums to 0.9990 (0.99905: safely inside the 1e-3 the creation call allows); state 4 is terminal and absorbing"""
    S, A, O = 5, 3, 3
    T = np.zeros((S, A, S), np.float32)
    pat = [[0.0, 0.3, 0.0, 0.3, 0.4],      # zero at the front and in the middle
           [0.25, 0.0, 0.25, 0.5, 0.0],     # zero in the middle and at the end
           [0.0, 0.0, 0.6, 0.0, 0.4],
           [0.2, 0.2, 0.2, 0.2, 0.2],
           [0.5, 0.0, 0.0, 0.0, 0.5]]
    for s in range(S - 1):
        for a in range(A):
            T[s, a] = pat[(s + a) % len(pat)]
    T[0, 0] = [0.5, 0.0, 0.29905, 0.0, 0.2]      # double sum 0.9990, the last entry positive
    T[1, 1] = [0.0, 0.4, 0.59905, 0.0, 0.0]      # double sum 0.9990, the row ends in zeros: the fallback lands on index 2
    T[S - 1, :, S - 1] = 1.0                    # absorbing
    Z = np.zeros((A, S, O), np.float32)
    zp = [[0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0], [0.2, 0.3, 0.5], [1.0, 0.0, 0.0]]
    for a in range(A):
        for s in range(S):
            Z[a, s] = zp[(a + 2 * s) % len(zp)]
    Z[0, 2] = [0.0, 0.99905, 0.0]                 # double sum 0.9990: every u at or above it falls back to index 1
    Z0 = np.array([[0.5, 0.0, 0.5], [0.0, 0.99905, 0.0], [0.3, 0.3, 0.4], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], np.float32)
    b0 = np.array([0.3, 0.39905, 0.0, 0.3, 0.0], np.float32)      # double sum 0.9990; never starts terminal
    R = (np.arange(S * A * S, dtype=np.float32).reshape(S, A, S) % 7 - 3) * np.float32(0.25)
    feat = (np.arange(O * 6, dtype=np.float32).reshape(O, 6) * np.float32(0.125) - np.float32(1.0))
    return Tables(T, R, [0, 0, 0, 0, 1], b0, feat, Z=Z, Z0=Z0)


def wide_tables(reward="dense"):
    """an MDP (n_obs = 0) with S = 70, A = 4, E = 8: a ring walk -- action k moves k + 1 places with probability 0.7, stays with 0.2, moves back one with 0.1; states 33
    and 69 are terminal.  reward "goal": +1 on entering state 69, -1 on entering state 33, -0.01 per step otherwise (a known-optimum problem for value iteration)"""
    S, A, E = 70, 4, 8
    T = np.zeros((S, A, S), np.float32)
    for s in range(S):
        for a in range(A):
            T[s, a, (s + a + 1) % S] += 0.7
            T[s, a, s] += 0.2
            T[s, a, (s - 1) % S] += 0.1
    term = np.zeros(S, np.uint8); term[[33, 69]] = 1
    b0 = np.zeros(S, np.float32); b0[:32] = 1.0 / 32      # a front block of mass, the rest zero
    if reward == "goal":
        R = np.full((S, A, S), -0.01, np.float32); R[:, :, 69] = 1.0; R[:, :, 33] = -1.0
    else:
        R = ((np.arange(S * A * S, dtype=np.float32).reshape(S, A, S) % 11) - 5) * np.float32(0.125)
    idx = np.arange(S)
    feat = np.stack([np.sin(2 * np.pi * idx * (k + 1) / S) if k % 2 == 0 else np.cos(2 * np.pi * idx * (k + 1) / S) for k in range(E)], 1).astype(np.float32)
    return Tables(T, R, term, b0, feat)


def cases(nn):
    """name -> dict(tab, net, n, T (trace length), cap (episodes; transitions for the feed-forward case), B, max_len, rec)"""
    return {
        "tiger": dict(tab=tiger_tables(), net=nn.create_dueling_network(nn.Chain(nn.LSTM(1, 4), nn.Dense(4, 3))), n=3, T=4, cap=6, B=2, max_len=3, rec=1),
        "sparse": dict(tab=sparse_tables(), net=nn.Chain(nn.GRU(6, 8), nn.Dense(8, 3)), n=5, T=4, cap=4, B=2, max_len=6, rec=1),
        "wide_mdp": dict(tab=wide_tables(), net=nn.create_dueling_network(nn.Chain(nn.Dense(8, 16, nn.relu), nn.Dense(16, 4))), n=8, T=1, cap=256, B=8, max_len=12, rec=0),
    }


STEPS = {"tiger": 20, "sparse": 40, "wide_mdp": 24}      # vector steps of the eps = 1 coverage runs (CPU model and GPU alike)
# env seeds chosen on the CPU model (tests/test_tabular_envs_cpu.py) so that, under eps = 1 and within STEPS, every flag of WANT happens
ENV_SEED = {"tiger": 1, "sparse": 13, "wide_mdp": 10}
WANT = {
    "tiger": ("first", "last", "open_across_reset"),
    "sparse": ("fallback", "zero_left", "zero_right", "first", "last", "wrap", "multi", "open_across_reset"),
    "wide_mdp": ("zero_left", "zero_right", "first", "last"),
}
WARM = {"sparse": 2}      # vector steps under eps = 1 after which batch_size episodes are committed, counted on the CPU model


def make_engine(pkg, nn, case, mfma=1, graph=1, seed=3, engine_cls=None, **hp_kw):
    tab = case["tab"]
    layers, dueling = nn.lower(case["net"])
    E = int(np.prod(tab.obs_shape))
    kw = dict(batch_size=case["B"], n_actions=tab.A, obs_c=E, obs_h=1, obs_w=1, dueling=int(dueling), buffer_size=case["cap"], recurrence=case["rec"],
              trace_length=case["T"], learning_rate=1e-2, prioritized_replay=0 if case["rec"] else 1, use_mfma=mfma, use_graph=graph, seed=seed, gamma=0.95, double_q=1)
    kw.update(hp_kw)
    return (engine_cls or pkg.Engine)(layers, pkg.default_hparams(**kw))


class FFRing:
    """the transition ring of a feed-forward engine as the device env loop fills it: the n experiences of a vector step at consecutive slots from the cursor, copy order"""

    def __init__(self, cap, obs_shape):
        self.cap, self.widx, self.size = cap, 0, 0
        self.s = np.zeros((cap,) + tuple(obs_shape), np.float32); self.sp = np.zeros_like(self.s)
        self.a, self.r, self.d = np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(cap, np.uint8)

    def add(self, s, a, r, sp, done):
        for i in range(len(a)):
            k = self.widx
            self.s[k], self.a[k], self.r[k], self.sp[k], self.d[k] = s[i], a[i], r[i], sp[i], done[i]
            self.widx, self.size = (k + 1) % self.cap, min(self.cap, self.size + 1)


class TabLockStep:
    """advances `g` (an engine with a tabular env set, or None for a CPU-only simulation under eps = 1) one vector step at a time beside the mirror, the ring model
    (RingModel for a recurrent engine, FFRing for a feed-forward one) and the shadow engine"""

    def __init__(self, g, tab, n, max_len, seed, model, shadow=None, eps=(0.0, 0.0, 1.0), train_freq=0, target_update_freq=0, B=1, rec=True):
        self.g, self.tab, self.n, self.max_len, self.seed, self.model, self.shadow, self.eps = g, tab, n, max_len, seed, model, shadow, eps
        self.tf, self.tu, self.B, self.rec = train_freq, target_update_freq, B, rec
        self.mirror = TabMirror(tab, n, seed)
        self.ep_step = np.zeros(n, np.int64)
        self.t, self.trained, self.explored, self.last_scalars = 1, 0, 0, None

    def flags(self):
        out = dict(self.mirror.seen)
        out.update(getattr(self.model, "seen", {}))
        return out

    def step(self, check_ring=True, check_hidden=True):
        t, n, g, A = self.t, self.n, self.g, self.tab.A
        obs_prev = self.mirror.observe()
        greedy = self.shadow.greedy(obs_prev) if self.shadow else None
        st = None
        if g is not None:
            st = g.rollout(1, t0=t, train_freq=self.tf, target_update_freq=self.tu, eps=self.eps)
            obs, a, r, d = g.envs_peek()
            q, gr = g.envs_peek_q()      # the step's own Q columns and greedy actions: the shadow's, explored copies included
            np.testing.assert_array_equal(gr, np.argmax(q, axis=1), err_msg=f"greedy vs the argmax of q at step {t}")
            if greedy is not None:
                np.testing.assert_array_equal(gr, greedy, err_msg=f"greedy actions at step {t}")
        else:
            a = np.array([explore(self.seed, t, i, (1.0, 1.0, 1.0), A) for i in range(n)], np.int32)
        want_a = [explore(self.seed, t, i, self.eps, A) for i in range(n)]
        self.explored += sum(x is not None for x in want_a)
        if greedy is not None:
            np.testing.assert_array_equal(a, np.array([greedy[i] if want_a[i] is None else want_a[i] for i in range(n)], np.int32), err_msg=f"actions at step {t}")
        elif g is not None:
            assert all(x is None or x == a[i] for i, x in enumerate(want_a)), f"random actions at step {t}"
        r_m, d_m = self.mirror.step(t, a)
        sp = self.mirror.observe()
        if g is not None:
            np.testing.assert_array_equal(r, r_m, err_msg=f"rewards at step {t}"); np.testing.assert_array_equal(d, d_m, err_msg=f"dones at step {t}")
        if self.model is not None:
            self.model.add(obs_prev, a, r_m, sp, d_m)
        self.ep_step += 1
        ended = (d_m != 0) | (self.ep_step >= self.max_len)
        if self.rec and self.model is not None:
            for i in np.nonzero(ended & (d_m == 0))[0]:
                self.model.note_truncated(int(i))
        due = int(self.tf > 0 and t % self.tf == 0)
        if self.rec:
            if due and self.model.size >= self.B:
                if self.shadow:
                    self.last_scalars = self.shadow.train(self.model, 1)
                self.trained += 1
                assert st is None or st["train_steps"] == 1
            else:
                assert st is None or st["train_steps"] == 0
            if self.tu > 0 and t % self.tu == 0 and self.shadow:
                self.shadow.e.sync_target()
        self.mirror.reset(ended, t)
        self.ep_step[ended] = 0
        if self.shadow and self.rec:
            self.shadow.reset_columns(ended)
        if g is not None:
            np.testing.assert_array_equal(obs.reshape(n, -1), self.mirror.observe().reshape(n, -1), err_msg=f"observations after step {t}")
            if self.rec and check_ring:
                self.model.check(g)
            if self.rec and self.shadow and check_hidden:
                hidden_equal(g.get_hidden(n), self.shadow.e.get_hidden(n))
        self.t += 1
        return st, a, r_m, d_m, ended


def simulate(name, nn, seed=None, steps=None):
    """the CPU model alone under eps = 1: (driver, flags) after STEPS[name] vector steps"""
    c = cases(nn)[name]
    model = RingModel(c["n"], c["T"], c["cap"], c["tab"].obs_shape) if c["rec"] else FFRing(c["cap"], c["tab"].obs_shape)
    ls = TabLockStep(None, c["tab"], c["n"], c["max_len"], ENV_SEED[name] if seed is None else seed, model, eps=(1.0, 1.0, 1.0), rec=bool(c["rec"]))
    first_batch = None
    for k in range(STEPS[name] if steps is None else steps):
        ls.step()
        if first_batch is None and c["rec"] and model.size >= c["B"]:
            first_batch = k + 1
    return ls, ls.flags(), first_batch
