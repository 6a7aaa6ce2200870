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
