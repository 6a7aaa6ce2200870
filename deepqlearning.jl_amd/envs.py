"""
Vectorised host-side environments used by the tests, the bench and the solve() mirror.

TestMDP        restatement of the reference's own image-observation test MDP (test/test_env.jl:10-87):
               state = (last `stack`=4 actions in {1,2,3}, t); observation = stack of `o_stack` fixed random integer
               images / 255 (:54-60); reward [-0.1, 0, +0.1][sp[end]] times -10 if s[end] == 2 (:77-83); terminal when
               t >= max_time (:85-87); 4 actions, action 4 repeats the previous element (:66-75); discount 0.99.
               Known answer (test/test_env.jl:7-8): optimal return 2.1, optimal policy [2,1,2,1,3].
               TestMDP((84,84),4,6) yields exactly the 84x84x4 observation of BASELINE configs 2/3/5.
SimpleGridWorld  POMDPModels.SimpleGridWorld defaults (third-party; recalled): 10x10 grid, 4 actions,
               rewards (4,3)=-10 (4,6)=-5 (9,3)=+10 (8,8)=+3 which are terminal, 70 % intended-move probability,
               discount 0.95, observation Float32[x, y].

TabularPOMDP  any discrete MDP / POMDP given as its matrices T[s, a, sp], Z[a, sp, o], R[s, a, sp], terminal[s], b0[s] and one feature row
               per observation index (per state index for an MDP: Z = Z0 = None); stepped as POMDPTools' MDPCommonRLEnv /
               POMDPCommonRLEnv step a POMDPs.jl problem (third-party; recalled): sp ~ T[s, a], o ~ Z[a, sp], r = R[s, a, sp],
               done = terminal[sp]; reset s ~ b0, o ~ Z0[s].  The device loop steps the same tables (dqn_envs_create_tabular).
TigerPOMDP     POMDPModels.TigerPOMDP as tables (third-party; recalled, not executed): 2 states (index = Bool: 0 tiger right,
               1 tiger left), actions listen / open-left / open-right, 2 observations, listening reports the side correctly with
               p_listen_correctly, opening re-draws the state, no terminal state, observation Float32[o].
MountainCar, InvertedPendulum  POMDPModels' two continuous-state control problems (third-party; recalled, not executed): two Float64 state
               values per copy, three actions, observation Float32[state[1], state[2]], discount 0.99.  These are the CPU twins of the device's
               control kinds (dqn_envs_create_control): the header's laws expression by expression in NumPy float64, and the device's own
               Philox draws keyed by (seed, vector step, copy, purpose) -- unlike the classes above, which draw from a NumPy generator.

Actions are 0-based here.  `n` environments step in lock-step as NumPy arrays (BASELINE config 3 shards 256 of
them over 8 ranks).
"""
from __future__ import annotations

import numpy as np


class TestMDP:
    __test__ = False  # not a pytest class

    def __init__(self, shape=(6,), stack=4, max_time=6, discount=0.99, n=1, seed=7, u8=False):
        rng = np.random.default_rng(seed)
        self.shape = tuple(shape)
        self.stack = 4              # hard-coded field (constructor quirk, test/test_env.jl:31)
        self.o_stack = stack        # the `stack` ARGUMENT becomes o_stack
        self.max_time = max_time
        self.discount = discount
        img_shape = self.shape[::-1]  # Julia (W,H) -> C order (H,W)
        self.images = np.stack([rng.integers(1, 51, img_shape), rng.integers(100, 151, img_shape),
                                rng.integers(150, 201, img_shape)]).astype(np.uint8)   # bad, normal, good (:26-28)
        self.rewards = np.array([-0.1, 0.0, 0.1], np.float32)
        self.n = n
        self.u8 = u8
        self.rng = np.random.default_rng(seed + 1)
        self.n_actions = 4
        self.obs_shape = (self.o_stack,) + img_shape
        self.reset()

    def reset(self, mask=None):
        if mask is None:
            self.s = np.ones((self.n, self.stack), np.int32)
            self.t = np.ones(self.n, np.int32)
        else:
            self.s[mask] = 1
            self.t[mask] = 1

    def observe(self):
        # obs[.., i] = observations[s[end-i+1]]  (test/test_env.jl:56-58)
        sel = self.s[:, ::-1][:, :self.o_stack] - 1            # (n, o_stack)
        o = self.images[sel]                                    # (n, o_stack, H, W) uint8
        return o if self.u8 else o.astype(np.float32) / np.float32(255.0)

    def terminated(self):
        return self.t >= self.max_time

    def act(self, a):
        a = np.asarray(a)
        was_second = self.s[:, -1] == 2
        s_new = np.roll(self.s, -1, axis=1)
        s_new[:, -1] = np.where(a < 3, a + 1, s_new[:, -2])
        r = self.rewards[s_new[:, -1] - 1] * np.where(was_second, np.float32(-10), np.float32(1))
        self.s, self.t = s_new, self.t + 1
        return r.astype(np.float32)


class SimpleGridWorld:
    def __init__(self, size=(10, 10), n=1, seed=0, tprob=0.7, discount=0.95):
        self.size = size
        self.reward_cells = {(4, 3): -10.0, (4, 6): -5.0, (9, 3): 10.0, (8, 8): 3.0}
        self.tprob, self.discount = tprob, discount
        self.n, self.n_actions, self.obs_shape = n, 4, (2,)
        self.dirs = np.array([[0, 1], [0, -1], [-1, 0], [1, 0]], np.int32)   # up, down, left, right
        self.rng = np.random.default_rng(seed)
        self.rmap = np.zeros((size[0] + 1, size[1] + 1), np.float32)
        for (x, y), v in self.reward_cells.items():
            self.rmap[x, y] = v
        self.reset()

    def reset(self, mask=None):
        new = np.stack([self.rng.integers(1, self.size[0] + 1, self.n), self.rng.integers(1, self.size[1] + 1, self.n)], 1).astype(np.int32)
        if mask is None:
            self.pos = new
            self.done = np.zeros(self.n, bool)
        else:
            self.pos[mask] = new[mask]
            self.done[mask] = False

    def observe(self):
        return self.pos.astype(np.float32)

    def terminated(self):
        return self.done

    def act(self, a):
        a = np.asarray(a)
        r = self.rmap[self.pos[:, 0], self.pos[:, 1]].copy()     # reward for acting from a reward cell, then terminal
        at_reward = r != 0
        rnd = self.rng.random(self.n) < self.tprob
        other = self.rng.integers(0, 3, self.n)
        eff = np.where(rnd, a, (a + 1 + other) % 4)
        new = self.pos + self.dirs[eff]
        inb = (new[:, 0] >= 1) & (new[:, 0] <= self.size[0]) & (new[:, 1] >= 1) & (new[:, 1] <= self.size[1])
        self.pos = np.where((inb & ~at_reward)[:, None], new, self.pos)
        self.done = at_reward
        return r.astype(np.float32)


class TabularPOMDP:
    def __init__(self, T, R, terminal, b0, features, Z=None, Z0=None, discount=0.95, n=1, seed=0):
        self.T, self.R = np.ascontiguousarray(T, np.float32), np.ascontiguousarray(R, np.float32)
        self.terminal, self.b0 = np.ascontiguousarray(terminal, np.uint8), np.ascontiguousarray(b0, np.float32)
        self.features = np.ascontiguousarray(features, np.float32)
        if (Z is None) != (Z0 is None):
            raise ValueError("TabularPOMDP: Z and Z0 come together (both None for an MDP)")
        self.Z = None if Z is None else np.ascontiguousarray(Z, np.float32)
        self.Z0 = None if Z0 is None else np.ascontiguousarray(Z0, np.float32)
        if self.T.ndim != 3 or self.T.shape[0] != self.T.shape[2]:
            raise ValueError(f"TabularPOMDP: T has shape {self.T.shape}, expected (S, A, S)")
        S, A, _ = self.T.shape
        O = 0 if self.Z is None else self.Z.shape[-1]
        self.n_states, self.n_obs, self.n_actions = S, O, A
        want = dict(R=(S, A, S), terminal=(S,), b0=(S,))
        if O:
            want.update(Z=(A, S, O), Z0=(S, O))
        for name, shp in want.items():
            if getattr(self, name).shape != shp:
                raise ValueError(f"TabularPOMDP: {name} has shape {getattr(self, name).shape}, expected {shp}")
        if self.features.ndim < 2 or self.features.shape[0] != (O or S):
            raise ValueError(f"TabularPOMDP: features has shape {self.features.shape}, expected ({O or S}, ...): one row per {'observation' if O else 'state'}")
        if not (1 <= S <= 1024 and 0 <= O <= 1024):
            raise ValueError(f"TabularPOMDP: n_states = {S} must be in 1..1024 and n_obs = {O} in 0..1024")
        rows = [("T", self.T, ~self.terminal.astype(bool)[:, None]), ("b0", self.b0, None)]
        if O:
            rows += [("Z", self.Z, None), ("Z0", self.Z0, None)]
        for name, p, need in rows:      # a row is named by the table's own leading indices: T[s][a], Z[a][sp], Z0[s], b0
            if not np.all(np.isfinite(p)) or np.any(p < 0):
                raise ValueError(f"TabularPOMDP: {name} has a negative or non-finite probability")
            off = np.abs(p.astype(np.float64).sum(-1) - 1.0) > 1e-3          # rows of T at terminal states are exempt
            if need is not None:
                off &= need
            if off.any():
                at = "".join(f"[{int(i)}]" for i in np.argwhere(off)[0])
                raise ValueError(f"TabularPOMDP: row {name}{at} sums to {float(p.astype(np.float64).sum(-1)[off][0]):.6f}, further than 1e-3 from 1")
        if not np.all(np.isfinite(self.R)) or not np.all(np.isfinite(self.features)):
            raise ValueError("TabularPOMDP: R and features must be finite")
        self.discount, self.n = discount, n
        self.obs_shape = tuple(self.features.shape[1:])
        self.rng = np.random.default_rng(seed)
        self.reset()

    def host_copy(self, n, seed=0):
        """another host instance of the same model (the tables are shared) with n copies"""
        return TabularPOMDP(self.T, self.R, self.terminal, self.b0, self.features, Z=self.Z, Z0=self.Z0, discount=self.discount, n=n, seed=seed)

    def _draw(self, p):
        """one index per row of p (n, K) by inversion; an entry of probability zero is never drawn.  An all-zero row (T at a terminal state) gives index 0, as on
        the device"""
        c = np.cumsum(p.astype(np.float64), axis=1)
        j = (self.rng.random(p.shape[0])[:, None] * c[:, -1:] >= c).sum(1)
        last = np.where((p > 0).any(axis=1), p.shape[1] - 1 - np.argmax(p[:, ::-1] > 0, axis=1), 0)
        return np.minimum(j, last).astype(np.int64)

    def reset(self, mask=None):
        s = self._draw(np.broadcast_to(self.b0, (self.n, self.n_states)))
        o = self._draw(self.Z0[s]) if self.n_obs else s
        if mask is None:
            self.s, self.o = s, o
            self.done = np.zeros(self.n, bool)
        else:
            self.s[mask], self.o[mask] = s[mask], o[mask]
            self.done[mask] = False

    def observe(self):
        return self.features[self.o]

    def terminated(self):
        return self.done

    def act(self, a):
        a = np.asarray(a).astype(np.int64)
        sp = self._draw(self.T[self.s, a])
        r = self.R[self.s, a, sp]
        self.o = self._draw(self.Z[a, sp]) if self.n_obs else sp
        self.s, self.done = sp, self.terminal[sp] != 0
        return r.astype(np.float32)


def is_tabular(env):
    """the env spec carries tables: the device loop steps it through dqn_envs_create_tabular"""
    return isinstance(env, TabularPOMDP)


def philox_u32(seed, t, env, purpose):
    """the device's keyed draw: word 0 of Philox4x32-10 under key = seed and counter (t low, t high, env, purpose).  `env` may be an array of copy indices"""
    env = np.asarray(env, np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    c = [np.full(env.shape, int(t) & 0xFFFFFFFF, np.uint64), np.full(env.shape, (int(t) >> 32) & 0xFFFFFFFF, np.uint64), env & m32, np.full(env.shape, int(purpose), np.uint64)]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]      # 32 x 32 bits: no overflow in 64
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & m32, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c[0]


def u01(r):
    """the device's 24-bit uniform in [0, 1): Float32(r >> 8) * 2^-24"""
    return (np.asarray(r, np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


class _ControlEnv:
    """Two Float64 state values per copy, three actions, observation Float32[state[1], state[2]]: the CPU twin of the device's control kinds (dqn_envs_create_control).
    The laws are the header's, expression by expression, in NumPy float64; the draws are the device's: u = Float64(u01(philox(seed, t, copy, purpose))), t = the vector
    step (the number of act() calls so far; a reset draws at the step it follows, 0 at construction)."""
    KIND = None      # DQN_ENV_MOUNTAINCAR / DQN_ENV_PENDULUM
    FIELDS = ("force", "freq", "gravity", "v_max", "x_min", "goal", "cost", "jackpot", "x0", "v0", "g", "m", "l", "M", "alpha", "dt", "u_max", "noise", "theta_max", "init_half")
    ALL_DEFAULTS = dict(force=0.001, freq=3.0, gravity=0.0025, v_max=0.07, x_min=-1.2, goal=0.5, cost=-1.0, jackpot=100.0, x0=-0.5, v0=0.0,
                        g=9.81, m=2.0, l=8.0, M=8.0, alpha=None, dt=0.1, u_max=50.0, noise=20.0, theta_max=np.pi / 2, init_half=0.1)
    P_NOISE, P_THETA0, P_OMEGA0 = 12, 13, 14      # DQN_ENV_RAND_PEND_*

    def __init__(self, n=1, seed=0, discount=0.99, **constants):
        name = type(self).__name__
        for k in constants:
            if k not in self.FIELDS:
                raise ValueError(f"{name}: unknown constant {k!r} (the fields of dqn_control_env: {', '.join(self.FIELDS)})")
        c = {**self.ALL_DEFAULTS, **constants}
        if c["alpha"] is None:
            c["alpha"] = 1.0 / (float(c["m"]) + float(c["M"]))
        self.c = {k: np.float64(c[k]) for k in self.FIELDS}
        for k, v in self.c.items():
            if not np.isfinite(v):
                raise ValueError(f"{name}: {k} = {float(v):g} is not finite")
        self.check()
        self.n, self.seed, self.discount = int(n), int(seed), discount
        self.n_actions, self.obs_shape = 3, (2,)
        self.kwargs = dict(constants)
        self.t = 0
        self.s = np.zeros((self.n, 2), np.float64)
        self.reset()

    def constants(self):
        """the spec's constants as Python floats, in the struct's order"""
        return {k: float(self.c[k]) for k in self.FIELDS}

    def host_copy(self, n, seed=0):
        """another host instance of the same model with n copies"""
        return type(self)(n=n, seed=seed, discount=self.discount, **self.kwargs)

    def u(self, t, purpose, idx=None):
        return u01(philox_u32(self.seed, t, np.arange(self.n) if idx is None else idx, purpose)).astype(np.float64)

    def reset(self, mask=None):
        new = self.reset_law(self.u(self.t, self.P_THETA0), self.u(self.t, self.P_OMEGA0))
        if mask is None:
            self.s = new
            self.done = np.zeros(self.n, bool)
        else:
            mask = np.asarray(mask, bool)
            self.s[mask] = new[mask]
            self.done[mask] = False

    def observe(self):
        return self.s.astype(np.float32)

    def terminated(self):
        return self.done

    def act(self, a):
        self.t += 1
        self.s, r, self.done, self.margin = self.step_law(self.s, np.asarray(a), self.u(self.t, self.P_NOISE))
        return r.astype(np.float32)


class MountainCar(_ControlEnv):
    """POMDPModels.MountainCar (third-party; recalled, not executed).  State (x, v); actions 0, 1, 2 push -1, 0, +1; reset to (x0, v0)."""
    KIND = 3

    def check(self):
        c = self.c
        if not c["v_max"] > 0:
            raise ValueError(f"MountainCar: v_max = {float(c['v_max']):g} must be > 0")
        if not c["x_min"] < c["goal"]:
            raise ValueError(f"MountainCar: x_min = {float(c['x_min']):g} must lie below goal = {float(c['goal']):g}")

    def reset_law(self, u13, u14):
        return np.stack([np.full(len(u13), self.c["x0"]), np.full(len(u13), self.c["v0"])], 1)

    def step_law(self, s, a, u12=None):
        """(state', Float64 reward, done, margin): margin = per copy the smallest distance of a branch quantity from its switch point (x' - goal, x' - x_min before the
        wall rule, |v'| - v_max before the clamp)"""
        c = self.c
        x, v, push = s[:, 0], s[:, 1], np.asarray(a).astype(np.float64) - 1.0
        vp = v + push * c["force"] + np.cos(c["freq"] * x) * (-c["gravity"])
        m_v = np.abs(np.abs(vp) - c["v_max"])
        vp = np.maximum(np.minimum(c["v_max"], vp), -c["v_max"])
        xp = x + vp
        m_w = np.abs(xp - c["x_min"])
        wall = xp < c["x_min"]
        xp, vp = np.where(wall, c["x_min"], xp), np.where(wall, 0.0, vp)
        done = xp >= c["goal"]
        r = c["cost"] + np.where(done, c["jackpot"], 0.0)
        return np.stack([xp, vp], 1), r, done, np.minimum(np.minimum(m_v, m_w), np.abs(xp - c["goal"]))


class InvertedPendulum(_ControlEnv):
    """POMDPModels.InvertedPendulum, Lagoudakis & Parr's pendulum (third-party; recalled, not executed).  State (theta, omega); actions 0, 1, 2 apply -u_max, 0, +u_max
    plus uniform noise; explicit Euler from the pre-step state; falls at |theta| > theta_max; reset uniform in [-init_half, init_half)^2."""
    KIND = 4

    def check(self):
        c = self.c
        if not c["dt"] > 0:
            raise ValueError(f"InvertedPendulum: dt = {float(c['dt']):g} must be > 0")
        if not c["l"] > 0:
            raise ValueError(f"InvertedPendulum: l = {float(c['l']):g} must be > 0")
        if not c["alpha"] * c["m"] < 4.0 / 3.0:
            raise ValueError(f"InvertedPendulum: alpha * m = {float(c['alpha'] * c['m']):g} must lie below 4/3: the denominator (4/3) l - alpha m l cos^2(theta) can reach 0")

    def reset_law(self, u13, u14):
        c = self.c
        return np.stack([(u13 - 0.5) * 2.0 * c["init_half"], (u14 - 0.5) * 2.0 * c["init_half"]], 1)

    def step_law(self, s, a, u12):
        """(state', Float64 reward, done, margin): margin = | |theta'| - theta_max | per copy"""
        c = self.c
        th, om, push = s[:, 0], s[:, 1], np.asarray(a).astype(np.float64) - 1.0
        g, m, l, al, dt = c["g"], c["m"], c["l"], c["alpha"], c["dt"]
        u = push * c["u_max"] + c["noise"] * (u12 - 0.5)
        sn, cs, s2 = np.sin(th), np.cos(th), np.sin(2.0 * th)
        acc = (g * sn - al * m * l * om * om * s2 * 0.5 - al * cs * u) / ((4.0 / 3.0) * l - al * m * l * cs * cs)
        thp, omp = th + om * dt, om + acc * dt
        done = np.abs(thp) > c["theta_max"]
        return np.stack([thp, omp], 1), np.where(done, c["cost"], 0.0), done, np.abs(np.abs(thp) - c["theta_max"])


def is_control(env):
    """the env spec is one of the continuous-state control problems: the device loop steps it through dqn_envs_create_control"""
    return isinstance(env, _ControlEnv)


class TigerPOMDP(TabularPOMDP):
    """POMDPModels.TigerPOMDP (third-party; recalled, not executed).  State / observation index = the Bool (0: tiger right, 1: tiger left); actions 0 listen,
    1 open-left, 2 open-right; opening the tiger's door costs r_findtiger, the other door pays r_escapetiger; observation Float32[o]."""

    def __init__(self, r_listen=-1.0, r_findtiger=-100.0, r_escapetiger=10.0, p_listen_correctly=0.85, discount=0.95, n=1, seed=0):
        self.r_listen, self.r_findtiger, self.r_escapetiger, self.p_listen_correctly = r_listen, r_findtiger, r_escapetiger, p_listen_correctly
        p = p_listen_correctly
        T = np.zeros((2, 3, 2), np.float32); Z = np.zeros((3, 2, 2), np.float32); R = np.zeros((2, 3, 2), np.float32)
        for s in range(2):
            T[s, 0, s] = 1.0                       # listening keeps the state
            T[s, 1:, :] = 0.5                      # opening a door re-draws it uniformly
            Z[0, s, s], Z[0, s, 1 - s] = p, 1.0 - p
            Z[1:, s, :] = 0.5                      # ... and yields a uniform observation
            R[s, 0, :] = r_listen
            R[s, 1, :] = r_findtiger if s == 1 else r_escapetiger      # open-left: the tiger is left in state 1
            R[s, 2, :] = r_findtiger if s == 0 else r_escapetiger
        super().__init__(T, R, np.zeros(2, np.uint8), np.full(2, 0.5, np.float32), np.array([[0.0], [1.0]], np.float32), Z=Z, Z0=Z[0].copy(),
                         discount=discount, n=n, seed=seed)
