"""Shared cases of the grouped-evaluation tests (TEST INFRASTRUCTURE): how members of dqn_evaluate_many and their twin-constructed standalone references are built
(group_rollout_common's six heterogeneous members, read-only, plus the members the launch-boundary and tile-edge cases need), and the observables that must not move
under an evaluation.  Comparisons are == on the doubles or np.array_equal throughout."""
import re

import numpy as np

import dqn_oracle as O
import ref
from engine_group_common import observables as step_observables
from group_rollout_common import assert_same, build, member_specs

R, I, T = O.ACT_RELU, O.ACT_IDENTITY, O.ACT_TANH
abi = ref.abi
N_EVALS = (1, 3, 37, 100)      # one copy; fewer than a wave on the scalar path; ragged above a wave (a multiple-of-4 tile and a scalar tail); a multiple of 4
LENGTHS = (1, 7)
WARM_STEPS = 3                 # train steps before any evaluation: the networks are not at their initial values


def seeds_for(n_members, n_eval, length):
    """a different seed per member (and per case)"""
    return [10_000 * (k + 1) + 100 * n_eval + length for k in range(n_members)]


def wide_spec(mid):
    """Dense(2, 128, relu) -> Dense(128, mid, tanh) -> Dense(mid, 4) on the grid world.  mid = 96 (13 156 parameters) is the network the tile-edge case was first written
    for; the single-workgroup TRAIN step keeps three parameter-sized arrays in LDS (3 * 13 156 floats > 144 KB), so dqn_group_create refuses it, and mid = 80
    (11 028 parameters: 3 P + activations = 139 KB at batch_size 2) is the widest middle layer in steps of 8 a group accepts.  one_dx_chunk: dx_kc = 0, the plan the
    single-workgroup step takes"""
    return dict(net=O.Network((2,), [O.Dense(2, 128, R), O.Dense(128, mid, T), O.Dense(mid, 4, I)]), env="grid", n=2, B=2, cap=16, n_fill=8, u8=False, fwd_kc=128,
                max_len=5, eps=(1.0, 0.1, 10.0), hp=dict(double_q=1, gamma=0.95, learning_rate=1e-4, seed=31))


def one_tile_floats(mid, n_eval):
    """floats of LDS the policy input and the activations of wide_spec(mid) need when ONE tile holds all n_eval copies: a launch whose dynamic LDS (evaluate_info) is
    smaller than 4 bytes of each ran more than one tile"""
    return (2 + 128 + mid + 4) * n_eval


def tiger_spec(seed=41):
    """TigerPOMDP has no terminal state: an episode ends at max_episode_length alone"""
    b, v, a = O.create_dueling_network([O.Dense(1, 8, R), O.Dense(8, 3, I)])
    return dict(net=O.Network((1,), b, v, a), env="tiger", n=2, B=4, cap=16, n_fill=8, u8=False, max_len=3, eps=(1.0, 0.3, 12.0),
                hp=dict(double_q=0, gamma=0.95, learning_rate=1e-2, seed=seed))


def long_mdp_spec(max_time, seed=42):
    """TestMDP whose only terminal condition, t >= max_time, lies beyond every episode bound of the launch-boundary case"""
    return dict(net=O.Network((2, 3, 3), [O.Dense(18, 8, R), O.Dense(8, 4, I)]), env="mdp", n=3, B=4, cap=16, n_fill=8, u8=True, max_len=7, eps=(0.9, 0.1, 9.0),
                max_time=max_time, hp=dict(double_q=1, gamma=0.9, learning_rate=2e-3, seed=seed))


class _LongMDP:
    """the envs module with TestMDP's max_time replaced: group_rollout_common.build creates the member's env set through it"""

    def __init__(self, envs, max_time):
        self._envs, self._max_time = envs, max_time

    def TestMDP(self, shape, stack, max_time, **kw):
        return self._envs.TestMDP(shape, stack, self._max_time, **kw)

    def __getattr__(self, name):
        return getattr(self._envs, name)


def build_member(spec, pkg, envs, env_seed=17):
    """group_rollout_common.build; a spec with max_time gets a TestMDP of that max_time"""
    return build(spec, pkg.Engine, pkg.default_plan, _LongMDP(envs, spec["max_time"]) if "max_time" in spec else envs, env_seed=env_seed)


def build_pair(spec, pkg, envs):
    return build_member(spec, pkg, envs), build_member(spec, pkg, envs)


def warm(group, alone, n=WARM_STEPS):
    """the same n train steps on the members (one group launch each) and on the references"""
    group.train_steps(n)
    for h in alone:
        h.train_steps(n)


def still(h):
    """what an evaluation must leave alone, as a flat dict: the train step's observables and the checkpoint field by field, what dqn_envs_peek returns (training copies),
    the replay size.  (dqn_envs_peek_q is refused after an evaluation -- that is part of the law, tested by itself)"""
    out = step_observables(h)
    out.update({"peek." + k: x for k, x in zip(("obs", "actions", "rewards", "dones"), h.envs_peek())})
    out["replay_size"] = np.asarray(h.replay_size())
    return out


def header_arity(hdr_text, name):
    """number of parameters of a prototype in the C header (comments stripped)"""
    txt = re.sub(r"/\*.*?\*/", "", hdr_text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


__all__ = ["assert_same", "build", "build_member", "build_pair", "header_arity", "long_mdp_spec", "member_specs", "one_tile_floats", "seeds_for", "still", "tiger_spec", "warm", "wide_spec",
           "N_EVALS", "LENGTHS", "WARM_STEPS"]
