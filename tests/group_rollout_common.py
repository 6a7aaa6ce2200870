"""Shared cases of the grouped-acting tests (TEST INFRASTRUCTURE): the heterogeneous members of dqn_rollout_many, how a member and its twin-constructed reference
are built (same layers, plan, hyper-parameters, parameters, replay prefill and env set), and every observable THE LAW of include/dqn_mi355x.h (grouped acting)
names.  Comparisons are np.array_equal throughout."""
import numpy as np

import dqn_oracle as O
import ref
from engine_group_common import assert_same, observables as step_observables
from envs_common import gridworld_mlp_dueling
from tabular_envs_common import tiger_tables

R, I, T = O.ACT_RELU, O.ACT_IDENTITY, O.ACT_TANH
abi = ref.abi
N_STEPS, TRAIN_FREQ, TARGET_FREQ = 12, 4, 8
EPS = (1.0, 0.1, 10.0)


def _duel(obs_shape, layers):
    b, v, a = O.create_dueling_network(layers)
    return O.Network(obs_shape, b, v, a)


def member_specs():
    """name -> dict(net, env, n, B, cap, n_fill, u8, fwd_kc, max_len, hp, eps), in group order.  Ring branches of add_exp!'s tree rebuild: `grid` wraps inside the run
    with cap not a multiple of n (e0 < s0), `deep` has n == cap, `plain` and `one` never wrap; `mdp` wraps too, with u8 rows."""
    return {
        # BASELINE config 1's network on its environment: four columns per item, the two dueling heads share an item loop
        "grid": dict(net=gridworld_mlp_dueling(), env="grid", n=32, B=8, cap=100, n_fill=10, u8=False, max_len=5, eps=EPS,
                     hp=dict(double_q=1, gamma=0.95, learning_rate=1e-3, seed=21)),
        # the same trunk without the dueling split, three copies: the scalar column loop, fewer copies than a wave
        "plain": dict(net=O.Network((2,), [O.Dense(2, 32, R), O.Dense(32, 4, I)]), env="grid", n=3, B=4, cap=64, n_fill=8, u8=False, max_len=4, eps=(0.8, 0.2, 6.0),
                      hp=dict(double_q=0, gamma=0.9, learning_rate=1e-2, seed=22)),
        "one": dict(net=O.Network((2,), [O.Dense(2, 4, T), O.Dense(4, 4, I)]), env="grid", n=1, B=4, cap=32, n_fill=6, u8=False, max_len=3, eps=(0.5, 0.5, 1.0),
                    hp=dict(double_q=1, gamma=0.99, learning_rate=3e-3, seed=23)),
        # two hidden layers under a plan that cuts both contractions: K = 24 -> 16 + 8, K = 40 -> 16 + 16 + 8; 100 copies: above one wave, no multiple of 64; n == cap
        "deep": dict(net=_duel((2,), [O.Dense(2, 24, R), O.Dense(24, 40, T), O.Dense(40, 4, I)]), env="grid", n=100, B=8, cap=100, n_fill=20, u8=False, fwd_kc=16, max_len=6,
                     eps=(1.0, 0.05, 8.0), hp=dict(double_q=1, gamma=0.97, learning_rate=5e-4, seed=24)),
        # TestMDP on 3 x 3 images, two stacked: E = 18, byte rows
        "mdp": dict(net=O.Network((2, 3, 3), [O.Dense(18, 8, R), O.Dense(8, 4, I)]), env="mdp", n=5, B=4, cap=37, n_fill=9, u8=True, max_len=7, eps=(0.9, 0.1, 9.0),
                    hp=dict(double_q=1, gamma=0.9, learning_rate=2e-3, seed=25)),
        # TigerPOMDP from its tables: the observation is not the state
        "tiger": dict(net=_duel((1,), [O.Dense(1, 8, R), O.Dense(8, 3, I)]), env="tiger", n=6, B=4, cap=48, n_fill=8, u8=False, max_len=3, eps=(1.0, 0.3, 12.0),
                      hp=dict(double_q=0, gamma=0.95, learning_rate=1e-2, seed=26)),
    }


def env_spec(envs, spec):
    if spec["env"] == "grid":
        return envs.SimpleGridWorld(n=spec["n"], seed=5)
    if spec["env"] == "mdp":
        return envs.TestMDP((3, 3), 2, 6, n=spec["n"], seed=3)
    return None


def replay_rows(spec, n=None, seed=0):
    """prefill rows with non-zero rewards (a zero reward under prio_eps = 0 is the assertion case, not the prefill's)"""
    net, n = spec["net"], spec["n_fill"] if n is None else n
    rng = np.random.default_rng(2000 + seed + spec["hp"]["seed"])
    if spec["u8"]:
        s, sp = (rng.integers(0, 256, (n,) + net.obs_shape).astype(np.uint8) for _ in range(2))
    else:
        s, sp = (rng.random((n,) + net.obs_shape, dtype=np.float32) for _ in range(2))
    r = (rng.standard_normal(n) * 2).astype(np.float32)
    r[r == 0] = 1.0
    return s, rng.integers(0, net.n_actions, n).astype(np.int32), r, sp, (rng.random(n) < 0.2).astype(np.uint8)


def build(spec, factory, default_plan, envs, env_seed=17, **factory_kw):
    """one engine of the spec with its env set -- the group member and its twin-constructed reference come from two calls of this"""
    net = spec["net"]
    hp = ref.hparams_for(net, batch_size=spec["B"], buffer_size=spec["cap"], obs_dtype=abi.OBS_U8 if spec["u8"] else abi.OBS_F32, **spec["hp"])
    layers = ref.layers_from_network(net)
    plan = default_plan(layers, hp)
    if spec.get("fwd_kc"):
        plan = [(spec["fwd_kc"], 0, w) for _, _, w in plan]
    h = factory(layers, hp, plan=plan, **factory_kw)
    p = O.Network.flatten(O.init_params(net, seed=spec["hp"]["seed"]))
    p = (p + 0.05 * np.random.default_rng(spec["hp"]["seed"]).standard_normal(p.shape)).astype(np.float32)      # non-zero biases
    h.set_params(p, 0); h.sync_target()
    h.replay_add(*replay_rows(spec))
    if spec["env"] == "tiger":
        h.envs_create_tabular(n_envs=spec["n"], max_episode_length=spec["max_len"], seed=env_seed + spec["hp"]["seed"], **tiger_tables().kwargs())
    else:
        h.envs_create(env_spec(envs, spec), max_episode_length=spec["max_len"], seed=env_seed + spec["hp"]["seed"])
    return h


def observables(h, stats=None, td=True, trained=True):
    """everything THE LAW names, as a flat dict of arrays: the train step's observables and checkpoint() field by field (engine_group_common), what dqn_envs_peek and
    dqn_envs_peek_q return, the replay size, and the call's statistics.  The engine has taken a vector step (dqn_envs_peek_q is refused before the first)"""
    if trained:
        out = step_observables(h, td=td)
    else:      # nothing trained yet: the last-step getters have nothing to show
        m, v, bp = h.get_adam_state()
        out = dict(p_on=h.get_params(0), p_tg=h.get_params(1), adam_m=m, adam_v=v, adam_bp=np.asarray(bp, np.float64), priorities=h.replay_priorities())
        out.update({"counters." + k: np.asarray(x) for k, x in h.get_counters().items()})
        out.update({"ck." + k: np.asarray(x) for k, x in h.checkpoint().items()})
    out.update({"peek." + k: x for k, x in zip(("obs", "actions", "rewards", "dones"), h.envs_peek())})
    out.update({"peekq." + k: x for k, x in zip(("q", "greedy"), h.envs_peek_q())})      # the last vector step's Q columns and greedy actions: pol_q / pol_a
    out["replay_size"] = np.asarray(h.replay_size())
    if stats is not None:
        out.update({"stats." + k: np.asarray(x) for k, x in stats.items()})
    return out


def rollout_alone(h, spec, n_steps, t0=1, explore=None, train_freq=TRAIN_FREQ, target_update_freq=TARGET_FREQ):
    return h.rollout(n_steps, t0=t0, train_freq=train_freq, target_update_freq=target_update_freq, eps=spec["eps"], explore=explore)


__all__ = ["assert_same", "build", "member_specs", "observables", "replay_rows", "rollout_alone", "N_STEPS", "TRAIN_FREQ", "TARGET_FREQ"]
