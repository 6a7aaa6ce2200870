"""Shared pieces of the recurrent device-environment tests (TEST INFRASTRUCTURE).

There is no CPU twin of the recurrent env loop, so the reference is a SHADOW: a second engine with the same layers, hparams, seed and parameters but no env set,
driven from Python through the host entry points (greedy_action on n streams, get_hidden / set_hidden for the per-copy resetstate!, episode_import + set_counters +
train_step_drqn at the train points).  Around it sit
  RingModel   a NumPy model of the episode ring: per-copy open lists, the prefix of T, commit on `done` in ascending copy order, ring wrap, the true length;
  mirrors     of the two built-in MDPs driven by the peeked actions (TestMDP: the package's envs.TestMDP; SimpleGridWorld: the device's Philox-keyed dynamics restated here);
  LockStep    the driver that advances the device rollout one vector step at a time and checks it against all of the above.
"""
import importlib
import types

import numpy as np

M32 = 0xFFFFFFFF


# ------------------------------------------------------------------ the device's keyed draws: Philox4x32-10, counter (vector step, copy, purpose), key = seed
def philox(seed, t, env, purpose):
    k0, k1 = seed & M32, (seed >> 32) & M32
    c = [t & M32, (t >> 32) & M32, env & M32, purpose & M32]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c[0]


def u01(r):
    return np.float32(r >> 8) * np.float32(1.0 / 16777216.0)


def eps_at(eps, t):
    """LinearDecaySchedule in fp32, as the env step computes it"""
    start, stop, steps = (np.float32(x) for x in eps)
    if not steps > 0:
        return stop
    e = start - np.float32(t) * ((start - stop) / steps)
    return stop if e < stop else e


def explore(seed, t, i, eps, n_actions):
    """None (greedy) or the random action of copy i at vector step t"""
    if u01(philox(seed, t, i, 1)) < eps_at(eps, t):
        return philox(seed, t, i, 2) % n_actions
    return None


class GridMirror:
    """SimpleGridWorld as the device steps it (defaults recalled from POMDPModels): draws keyed by (seed, step, copy, purpose)"""

    def __init__(self, spec, n, seed):
        self.spec, self.n, self.seed = spec, n, seed
        self.pos = np.zeros((n, 2), np.int64)
        self.reset(np.ones(n, bool), 0)

    def reset(self, mask, t):
        for i in np.nonzero(mask)[0]:
            self.pos[i] = (1 + philox(self.seed, t, int(i), 5) % self.spec.size[0], 1 + philox(self.seed, t, int(i), 6) % self.spec.size[1])

    def observe(self):
        return self.pos.astype(np.float32)

    def step(self, t, a):
        r, d = np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)
        for i in range(self.n):
            rv = np.float32(0)
            for (x, y), v in self.spec.reward_cells.items():
                if (self.pos[i, 0], self.pos[i, 1]) == (x, y):
                    rv = np.float32(v)
            at_reward = rv != 0
            intended = u01(philox(self.seed, t, i, 3)) < np.float32(self.spec.tprob)
            other = philox(self.seed, t, i, 4) % 3
            eff = int(a[i]) if intended else (int(a[i]) + 1 + other) % 4
            dx, dy = {0: (0, 1), 1: (0, -1), 2: (-1, 0), 3: (1, 0)}[eff]
            nx, ny = self.pos[i, 0] + dx, self.pos[i, 1] + dy
            if not at_reward and 1 <= nx <= self.spec.size[0] and 1 <= ny <= self.spec.size[1]:
                self.pos[i] = (nx, ny)
            r[i], d[i] = rv, at_reward
        return r, d


class TestMDPMirror:
    """the package's vectorised TestMDP (envs.TestMDP) behind the same interface"""
    __test__ = False

    def __init__(self, spec, n, seed):
        self.env = type(spec)(spec.shape, spec.o_stack, spec.max_time, n=n, seed=7)
        self.env.images = spec.images
        self.n = n

    def reset(self, mask, t):
        self.env.reset(np.asarray(mask, bool))

    def observe(self):
        return self.env.observe()

    def step(self, t, a):
        r = self.env.act(np.asarray(a))
        return r, self.env.terminated().astype(np.uint8)


def make_mirror(spec, n, seed):
    return (TestMDPMirror if hasattr(spec, "images") else GridMirror)(spec, n, seed)


# ------------------------------------------------------------------ the episode ring
class RingModel:
    """EpisodeReplayBuffer as the device env loop fills it.  A transition goes to position open_len of the copy's open episode only while open_len < T (only the prefix
    can ever be sampled) and the length counts on; truncation does not close an episode; on `done` the staged prefix is committed with the TRUE length to slot
    (widx + k) % cap, k = rank of the copy among this step's finishers in ascending copy index.  Storage starts zeroed; a commit writes the prefix only."""

    def __init__(self, n, T, cap, obs_shape):
        self.T, self.cap, self.obs_shape = T, cap, tuple(obs_shape)
        self.s = np.zeros((cap, T) + self.obs_shape, np.float32); self.sp = np.zeros_like(self.s)
        self.a, self.r, self.d = np.zeros((cap, T), np.int32), np.zeros((cap, T), np.float32), np.zeros((cap, T), np.uint8)
        self.len = np.zeros(cap, np.int32)
        self.widx = self.size = 0
        self.seen = dict(wrap=False, prefix=False, short=False, open_across_reset=False, multi=False)
        self.recreate(n)

    def recreate(self, n):
        """a new env set: open episodes go, committed ones stay"""
        self.n = n
        self.open = [[] for _ in range(n)]
        self.open_len = [0] * n

    def note_truncated(self, i):
        """copy i was reset by length without `done`: its episode stays open"""
        if self.open_len[i] > 0:
            self.seen["open_across_reset"] = True

    def add(self, s, a, r, sp, done):
        fin = []
        for i in range(self.n):
            if self.open_len[i] < self.T:
                self.open[i].append((np.array(s[i], np.float32), int(a[i]), np.float32(r[i]), np.array(sp[i], np.float32), 1 if done[i] else 0))
            self.open_len[i] += 1
            if done[i]:
                fin.append(i)
        self.seen["multi"] |= len(fin) >= 2
        for i in fin:                                   # ascending copy index, one after the other
            k = self.widx
            for t, (s_, a_, r_, sp_, d_) in enumerate(self.open[i]):
                self.s[k, t], self.a[k, t], self.r[k, t], self.sp[k, t], self.d[k, t] = s_.reshape(self.obs_shape), a_, r_, sp_.reshape(self.obs_shape), d_
            self.len[k] = self.open_len[i]
            self.seen["prefix"] |= self.open_len[i] > self.T
            self.seen["short"] |= self.open_len[i] < self.T
            self.seen["wrap"] |= self.size == self.cap
            self.widx = (self.widx + 1) % self.cap
            self.size = min(self.cap, self.size + 1)
            self.open[i], self.open_len[i] = [], 0

    def export(self):
        k = self.size
        return self.s[:k], self.sp[:k], self.a[:k], self.r[:k], self.d[:k], self.len[:k]

    def check(self, h, sample_ctr=None, counters=True):
        """episode_export / episode_count / get_counters of a handle equal this model, every array bit for bit (counters=False: the CPU twin keeps counters of the
        transition replay only, its cursor shows in where the next episode lands)"""
        assert h.episode_count() == (self.size, self.cap)
        for got, want in zip(h.episode_export(), self.export()):      # (a handle reports observations as (C, H, W): a flat observation comes back as (E, 1, 1))
            assert got.size == want.size and got.shape[:2] == want.shape[:2], (got.shape, want.shape)
            np.testing.assert_array_equal(got.reshape(want.shape), want)
        if not counters:
            return
        c = h.get_counters()
        assert (c["size"], c["widx"]) == (self.size, self.widx), (c, self.size, self.widx)
        if sample_ctr is not None:
            assert c["sample_ctr"] == sample_ctr


# ------------------------------------------------------------------ cases (smallest shapes that reach every branch)
def cases(nn, envs):
    """name -> (env spec, network, n, T, ep_cap, B, max_episode_length)"""
    return {
        # n off a multiple of 4, T shorter than an episode (5 steps)
        "lstm": (envs.TestMDP((5, 5), 1, 6), nn.Chain(nn.flattenbatch, nn.LSTM(25, 8), nn.Dense(8, 4)), 3, 4, 5, 2, 100),
        # episodes truncated by length: open episodes cross resets
        "gru_duel": (envs.SimpleGridWorld(), nn.create_dueling_network(nn.Chain(nn.GRU(2, 8), nn.Dense(8, 4))), 8, 10, 6, 4, 7),
        # T longer than an episode: masked rows
        "rnn_conv": (envs.TestMDP((6, 6), 1, 6), nn.Chain(nn.Conv(3, 1, 2, nn.relu), nn.flattenbatch, nn.RNN(32, 8, nn.tanh), nn.Dense(8, 4)), 5, 8, 4, 2, 100),
    }


WARM = {"lstm": 5, "gru_duel": 7, "rnn_conv": 5}      # vector steps under eps = 1 (network-independent) after which batch_size episodes are committed, counted on the CPU model (test_recurrent_envs_cpu)
ENV_SEED = {"lstm": 17, "gru_duel": 1, "rnn_conv": 5}      # gru_duel: chosen on the CPU model so that wrap, a truncated-but-open episode and two finishers in one step all happen (test_recurrent_envs_cpu)


def make_engine(pkg, nn, case, mfma=1, graph=1, seed=3, engine_cls=None, recurrence=1, net=None):
    spec, cnet, n, T, cap, B, max_len = case
    net = cnet if net is None else net
    layers, dueling = nn.lower(net)
    shp = spec.obs_shape
    c, h, w = shp if len(shp) == 3 else (int(np.prod(shp)), 1, 1)
    hp = pkg.default_hparams(batch_size=B, n_actions=4, obs_c=c, obs_h=h, obs_w=w, dueling=int(dueling), buffer_size=cap if recurrence else 64, recurrence=recurrence,
                             trace_length=T, learning_rate=1e-2, prioritized_replay=0 if recurrence else 1, use_mfma=mfma, use_graph=graph, seed=seed, gamma=0.95, double_q=1)
    return (engine_cls or pkg.Engine)(layers, hp), net


def noisy_params(nn, net, seed=3):
    """glorot weights plus noise everywhere: non-zero biases and a non-zero, trainable state0"""
    p = nn.glorot_params(net, seed=seed)
    return (p + 0.1 * np.random.default_rng(seed).standard_normal(p.size)).astype(np.float32)


def state0_slices(nn, net):
    """per recurrent layer in chain order: (slice of h0, slice of c0 or None) in the flat Flux.params vector"""
    out, off = [], 0
    for l in nn.all_layers(net):
        if l.kind in ("maxpool", "meanpool"):
            continue
        sizes = [int(np.prod(s)) for s in l.shapes()]
        if l.kind == "lstm":
            o = off + sum(sizes[:3]); out.append((slice(o, o + sizes[3]), slice(o + sizes[3], o + sizes[3] + sizes[4])))
        elif l.kind in ("gru", "rnn"):
            o = off + sum(sizes[:3]); out.append((slice(o, o + sizes[3]), None))
        off += sum(sizes)
    return out


class Shadow:
    """the host-driven reference engine: n observation streams with carried state, reset per column"""

    def __init__(self, engine, nn, net, n):
        self.e, self.n, self.sl = engine, n, state0_slices(nn, net)

    def greedy(self, obs):
        return self.e.greedy_action(obs)

    def reset_columns(self, mask):
        """resetstate! of the copies in mask: their columns become state0 of the online net as it is now"""
        if not np.any(mask):
            return
        hs, p, out = self.e.get_hidden(self.n), self.e.get_params(0), []
        for st, (h0, c0) in zip(hs, self.sl):
            if c0 is not None:
                h, c = st
                h[:, mask] = p[h0][:, None]; c[:, mask] = p[c0][:, None]
                out.append((h, c))
            else:
                st[:, mask] = p[h0][:, None]
                out.append(st)
        self.e.set_hidden(out)

    def train(self, model, k=1):
        """a train point: the model's ring goes in, the draw counter and the step count stay"""
        c = self.e.get_counters()
        self.e.episode_import(*model.export())
        self.e.set_counters(model.size, model.widx, c["sample_ctr"], c["train_steps"])
        out = None
        for _ in range(k):
            out = self.e.train_step_drqn()
        return out


def hidden_equal(a, b):
    for x, y in zip(a, b):
        for u, v in zip(x if isinstance(x, tuple) else (x,), y if isinstance(y, tuple) else (y,)):
            np.testing.assert_array_equal(u, v)


class LockStep:
    """advances `g` (an engine with a recurrent env set, or None for a CPU-only simulation under eps = 1) one vector step at a time beside the mirror env, the ring
    model and the shadow"""

    def __init__(self, g, spec, n, max_len, seed, model, shadow=None, eps=(0.0, 0.0, 1.0), train_freq=0, target_update_freq=0, cadence=False, B=1):
        self.g, self.spec, self.n, self.max_len, self.seed, self.model, self.shadow, self.eps = g, spec, n, max_len, seed, model, shadow, eps
        self.tf, self.tu, self.cadence, self.B = train_freq, target_update_freq, cadence, B
        self.mirror = make_mirror(spec, n, seed)
        self.ep_step = np.zeros(n, np.int64)
        self.t = 1
        self.trained = 0
        self.explored = 0
        self.last_scalars = None

    def step(self, check_ring=True, check_hidden=True):
        t, n, g = self.t, self.n, self.g
        obs_prev = self.mirror.observe()
        greedy = self.shadow.greedy(obs_prev) if self.shadow else None
        if g is not None:
            st = g.rollout(1, t0=t, train_freq=self.tf, target_update_freq=self.tu, eps=self.eps, env_step_cadence=self.cadence)
            obs, a, r, d = g.envs_peek()
            q, gr = g.envs_peek_q()      # what the recurrent tail left in pol_q / pol_a: the shadow's greedy actions, explored copies included, and the first-max argmax of q
            np.testing.assert_array_equal(gr, np.argmax(q, axis=1), err_msg=f"greedy vs the argmax of q at step {t}")
            if greedy is not None:
                np.testing.assert_array_equal(gr, greedy, err_msg=f"greedy actions at step {t}")
        else:
            st, a = None, np.array([explore(self.seed, t, i, (1.0, 1.0, 1.0), 4) for i in range(n)], np.int32)
        want_a = np.array([explore(self.seed, t, i, self.eps, 4) for i in range(n)], object)
        self.explored += sum(x is not None for x in want_a)
        if greedy is not None:
            np.testing.assert_array_equal(a, np.array([greedy[i] if want_a[i] is None else want_a[i] for i in range(n)], np.int32), err_msg=f"actions at step {t}")
        r_m, d_m = self.mirror.step(t, a)
        sp = self.mirror.observe()
        if g is not None:
            np.testing.assert_array_equal(r, r_m); np.testing.assert_array_equal(d, d_m)
        self.model.add(obs_prev, a, r_m, sp, d_m)
        self.ep_step += 1
        ended = (d_m != 0) | (self.ep_step >= self.max_len)
        for i in np.nonzero(ended & (d_m == 0))[0]:
            self.model.note_truncated(int(i))
        # train point(s) of this vector step, then the target sync (src/solver.jl:136-145)
        due = 0
        if self.tf > 0:
            due = (t * n) // self.tf - ((t - 1) * n) // self.tf if self.cadence else int(t % self.tf == 0)
        if due and self.model.size >= self.B:
            if self.shadow:
                self.last_scalars = self.shadow.train(self.model, due)
            self.trained += due
            if st is not None:
                assert st["train_steps"] == due
        elif st is not None:
            assert st["train_steps"] == 0
        if self.tu > 0 and ((t * n) // self.tu != ((t - 1) * n) // self.tu if self.cadence else t % self.tu == 0) and self.shadow:
            self.shadow.e.sync_target()
        self.mirror.reset(ended, t)
        self.ep_step[ended] = 0
        if self.shadow:
            self.shadow.reset_columns(ended)      # after the train step: state0 of the online net as it is THEN
        if g is not None:
            np.testing.assert_array_equal(obs.reshape(n, -1), self.mirror.observe().reshape(n, -1), err_msg=f"observations after step {t}")
            if check_ring:
                self.model.check(g)
            if self.shadow and check_hidden:
                hidden_equal(g.get_hidden(n), self.shadow.e.get_hidden(n))
        self.t += 1
        return st, a, r_m, d_m, ended


def load(pkg):
    return importlib.import_module(pkg.__name__ + ".nn"), importlib.import_module(pkg.__name__ + ".envs"), importlib.import_module(pkg.__name__ + ".solver")


def stub_namespace(**kw):
    return types.SimpleNamespace(**kw)
