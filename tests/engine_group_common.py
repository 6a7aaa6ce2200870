"""Shared cases of the engine-group tests (TEST INFRASTRUCTURE): the five heterogeneous members, how a member and its twin-constructed
reference are built (same layers, hyper-parameters, seed, parameters and replay), every observable THE LAW of include/dqn_mi355x.h
(engine groups) names, and the pure-Python refusal cases of solver.solve_many.  Comparisons are np.array_equal throughout."""
import numpy as np

import dqn_oracle as O
import ref
from nets import cfg1_mlp_dueling

R, I, T = O.ACT_RELU, O.ACT_IDENTITY, O.ACT_TANH
abi = ref.abi


def _duel(obs_shape, layers):
    b, v, a = O.create_dueling_network(layers)
    return O.Network(obs_shape, b, v, a)


def member_specs():
    """name -> dict(net, B, cap, n_fill, u8, hp): the members of the heterogeneous group, in group order a..e"""
    return {
        "a": dict(net=O.Network((2,), [O.Dense(2, 4, R), O.Dense(4, 2, I)]), B=4, cap=16, n_fill=12, u8=False,
                  hp=dict(double_q=0, gamma=0.9, learning_rate=1e-2, seed=11)),
        "b": dict(net=cfg1_mlp_dueling(), B=32, cap=128, n_fill=100, u8=False,
                  hp=dict(double_q=1, gamma=0.95, learning_rate=1e-3, seed=22)),
        # B = 5: not a multiple of four, the scalar item loops of the step; distinct draws
        "c": dict(net=_duel((3,), [O.Dense(3, 8, T), O.Dense(8, 8, R), O.Dense(8, 3, I)]), B=5, cap=32, n_fill=20, u8=False,
                  hp=dict(double_q=0, gamma=0.99, learning_rate=3e-3, seed=33, sample_distinct=1, adam_beta1=0.8, adam_eps=1e-6)),
        "d": dict(net=O.Network((1, 2, 2), [O.Dense(4, 8, R), O.Dense(8, 3, I)]), B=8, cap=64, n_fill=40, u8=True,
                  hp=dict(double_q=1, gamma=0.9, learning_rate=2e-3, seed=44)),
        # 3 * 8836 parameters' worth of floats in LDS alone: above 64 KB, the launch must raise the function's dynamic-LDS limit.  one_dx_chunk: the default plan cuts
        # the dX sum of a 128-wide Dense layer into four chunks for the multi-launch program's tiles, and the single-workgroup step takes plans with one chunk only --
        # so this member is created with the default plan's dx_kc set to 0 (a caller-supplied plan; the FIRST layer has no dX at all, no arithmetic depends on it)
        "e": dict(net=O.Network((64,), [O.Dense(64, 128, R), O.Dense(128, 4, I)]), B=8, cap=64, n_fill=48, u8=False, one_dx_chunk=True,
                  hp=dict(double_q=1, gamma=0.97, learning_rate=5e-4, seed=55)),
    }


def replay_rows(spec, n=None, seed=0):
    net, n = spec["net"], spec["n_fill"] if n is None else n
    rng = np.random.default_rng(1000 + seed + spec["hp"]["seed"])
    if spec["u8"]:
        s, sp = (rng.integers(0, 256, (n,) + net.obs_shape).astype(np.uint8) for _ in range(2))
    else:
        s, sp = (rng.random((n,) + net.obs_shape, dtype=np.float32) for _ in range(2))
    return s, rng.integers(0, net.n_actions, n).astype(np.int32), (rng.standard_normal(n) * 2).astype(np.float32), sp, (rng.random(n) < 0.2).astype(np.uint8)


def initial_params(spec):
    net, seed = spec["net"], spec["hp"]["seed"]
    p_on = O.Network.flatten(O.init_params(net, seed=seed))
    p_on = (p_on + 0.01 * np.random.default_rng(seed).standard_normal(p_on.shape)).astype(np.float32)      # non-zero biases
    return p_on, O.Network.flatten(O.init_params(net, seed=seed + 100)).astype(np.float32)


def build(spec, factory, default_plan, **factory_kw):
    """one engine of the spec -- the group member and its twin-constructed reference come from two calls of this"""
    net = spec["net"]
    hp = ref.hparams_for(net, batch_size=spec["B"], buffer_size=spec["cap"], obs_dtype=abi.OBS_U8 if spec["u8"] else abi.OBS_F32, **spec["hp"])
    layers = ref.layers_from_network(net)
    plan = default_plan(layers, hp)
    if spec.get("one_dx_chunk"):
        plan = [(f, 0, w) for f, _, w in plan]
    h = factory(layers, hp, plan=plan, **factory_kw)
    p_on, p_tg = initial_params(spec)
    h.set_params(p_on, 0); h.set_params(p_tg, 1)
    s, a, r, sp, d = replay_rows(spec)
    h.replay_add(s, a, r, sp, d)
    return h


def observables(h, td=True):
    """everything THE LAW names, as a flat dict of arrays; checkpoint() field by field (ck.*)"""
    m, v, bp = h.get_adam_state()
    out = dict(p_on=h.get_params(0), p_tg=h.get_params(1), grads=h.get_grads(), adam_m=m, adam_v=v, adam_bp=np.asarray(bp, np.float64),
               priorities=h.replay_priorities(), last_indices=h.last_indices())
    out.update({"counters." + k: np.asarray(x) for k, x in h.get_counters().items()})
    out.update({"last_q." + k: x for k, x in h.last_q().items()})
    if td:      # (the CPU twin exports no dqn_get_last_td)
        out["td"], out["is_weights"] = h.last_td()
    out.update({"ck." + k: np.asarray(x) for k, x in h.checkpoint().items()})
    return out


def assert_same(got, want, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for k in want:
        assert np.asarray(got[k]).dtype == np.asarray(want[k]).dtype and np.array_equal(got[k], want[k], equal_nan=True), (what, k, got[k], want[k])


# ---- solver.solve_many: the refusals made in pure Python, before any engine exists.  (field the message must name, the solver indices it must name, overrides per solver)
def many_refusal_cases():
    eq = ("train_freq", "target_update_freq", "max_steps", "train_start", "buffer_size", "batch_size", "eval_freq", "log_freq", "save_freq")
    cases = [(f, (0, 2), {2: {f: 7}}) for f in eq]
    cases += [
        ("env.n", (0, 1), {1: {"_env_n": 3}}),
        ("device_envs", (1,), {1: {"device_envs": False}}),
        ("recurrence", (2,), {2: {"recurrence": True}}),
        ("recurrence", (1,), {1: {"_lstm": True}}),
        ("logdir", (0, 2), {0: {"logdir": "log/x"}, 2: {"logdir": "log/x"}}),
    ]
    return cases
