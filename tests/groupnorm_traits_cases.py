"""The networks behind tests/golden/groupnorm_traits_gpu.json (TEST INFRASTRUCTURE): kind_traits_cases' recording -- the launch names of one train step and of a middle
step, the acting program's fused_tail, the dqn_comm_init / DQN_SIM_WORLD refusal texts -- for networks with a GroupNorm layer, in a module of its own (kind_traits_cases.py
and its goldens are not edited).  `observe` is kind_traits_cases.observe_gpu on a case of THIS table; nothing here computes an expected value."""
import importlib

import kind_traits_cases as K

nn, pkg = K.nn, K.pkg
relu = nn.relu


def _cases():
    c = {}
    case = lambda name, net, obs=K.IMG, B=8, env=None, envs=False, refuse=False, **hp: c.__setitem__(name, dict(net=net, obs=obs, B=B, hp=hp, env=env or {}, envs=envs, refuse=refuse))
    case("gn", nn.Chain(nn.Conv(3, 2, 8, relu), nn.GroupNorm(8, 2, relu), nn.Dense(288, 16, relu), nn.Dense(16, 4)), prioritized_replay=0)
    case("gn_prio_u8", nn.Chain(nn.Conv(3, 2, 8, relu), nn.GroupNorm(8, 2, relu), nn.Dense(288, 16, relu), nn.Dense(16, 4)), B=32, obs_dtype=K.abi.OBS_U8)
    # every map kind around the layer: padded conv -> GroupNorm -> pool -> GroupNorm -> convolutional block -> GroupNorm; the heads' producers would take k_head_cols4 without it
    case("gn_all_maps", nn.Chain(nn.Conv(3, 2, 8, relu, pad=1), nn.GroupNorm(8, 1), nn.MaxPool(2), nn.GroupNorm(8, 8, relu),
                                 nn.SkipConnection(nn.Chain(nn.Conv(3, 8, 8, relu, pad=1), nn.Conv(3, 8, 8, pad=1)), "+"), nn.GroupNorm(8, 4, relu),
                                 nn.Dense(128, 128, relu), nn.Dense(128, 4)), prioritized_replay=0)
    case("gn_dueling_b128", nn.create_dueling_network(nn.Chain(nn.Conv(3, 2, 16, relu), nn.GroupNorm(16, 4, relu), nn.Conv(3, 16, 16, relu), nn.Dense(256, 32, relu), nn.Dense(32, 4))), B=128, dueling=1)
    case("gn_lstm", nn.Chain(nn.Conv(3, 2, 4, relu), nn.GroupNorm(4, 2, relu), nn.LSTM(144, 8), nn.Dense(8, 4)), B=4, recurrence=1, trace_length=3, prioritized_replay=0)
    case("act_gn", nn.Chain(nn.Conv(3, 4, 8, relu), nn.GroupNorm(8, 2, relu), nn.Dense(72, 128, relu), nn.Dense(128, 4)), obs=K.ENVOBS, envs=True)
    case("refuse_gn", nn.Chain(nn.Conv(3, 2, 8, relu), nn.GroupNorm(8, 2), nn.Dense(288, 4)), refuse=True, prioritized_replay=0)
    # the kinds in the table's order: a pool at layer 3 is named in front of the GroupNorm at layer 1, a GroupNorm behind every other own-level kind is named last
    case("refuse_gn1_pool3", nn.Chain(nn.Conv(3, 2, 8, relu), nn.GroupNorm(8, 2), nn.Conv(3, 8, 8, relu), nn.MaxPool(2), nn.Dense(32, 4)), refuse=True, prioritized_replay=0)
    return c


CASES = _cases()


def observe(name):
    c = CASES[name]
    if c["refuse"]:
        h, _ = K._engine(c, c["env"])
        out = {"comm_init": K._refusal(lambda: h.comm_init(bytes(128), 0, 1))}
        h.close()
        out["sim_world"] = K._refusal(lambda: K._engine(c, c["env"] | {"DQN_SIM_WORLD": "2"})[0].close())
        return out
    h, hp = K._engine(c, c["env"])
    if c["envs"]:
        envs = importlib.import_module(pkg.__name__ + ".envs")
        h.envs_create(envs.TestMDP((5, 5), 4, 6, n=8, seed=3), max_episode_length=100, seed=17)
        out = {"fused_tail": h.envs_info()[1]}
    else:
        K._fill(h, hp, c)
        out = {"step": [n for n, _ in h.profile_step(max_entries=512)]}
        if not hp.recurrence:
            out["steady"] = [n for n, _ in h.profile_step(max_entries=512, steady=True)]
    h.close()
    return out
