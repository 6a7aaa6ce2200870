"""The networks behind tests/golden/activation_traits_gpu.json (TEST INFRASTRUCTURE): kind_traits_cases' recording -- the launch names of one train step and of a middle
step, the acting program's fused_tail, the dqn_comm_init / DQN_SIM_WORLD refusal texts -- for networks with a standalone Activation layer (kind 14), in a module of its own
(kind_traits_cases.py, groupnorm_traits_cases.py and their goldens are not edited).  Nothing here computes an expected value."""
import importlib

import kind_traits_cases as K

nn, pkg = K.nn, K.pkg
relu = nn.relu
A = nn.Activation


def _cases():
    c = {}
    case = lambda name, net, obs=K.IMG, B=8, env=None, envs=False, refuse=False, **hp: c.__setitem__(name, dict(net=net, obs=obs, B=B, hp=hp, env=env or {}, envs=envs, refuse=refuse))
    # (its recorded step shows `bwd_valu_act2` behind `bwd_act2`: the Activation has no VALU task -- it is the head's deferred dW task table, flushed at that level and named
    #  after the level's layer, as `bwd_valu_pool3` / `bwd_valu_ln1` are in kind_traits_gpu.json)
    # without the layer this trunk takes the fused heads (k_red_head / k_head_cols4) and, when acting, the fused tail: with it every fusion declines
    case("act_vec", nn.Chain(nn.Conv(3, 2, 8, relu), nn.Dense(288, 128), A(nn.gelu), nn.Dense(128, 4)), prioritized_replay=0)
    case("act_map_prio_u8", nn.Chain(nn.Conv(3, 2, 8), A(nn.swish), nn.Dense(288, 16, relu), nn.Dense(16, 4)), B=32, obs_dtype=K.abi.OBS_U8)
    # every map kind around the layer, and the post-add relu between two convolutional blocks
    case("act_all_maps", nn.Chain(nn.Conv(3, 2, 8, pad=1), A(nn.mish), nn.MaxPool(2), A(relu), nn.GroupNorm(8, 2), A(nn.hardswish),
                                  nn.SkipConnection(nn.Chain(nn.Conv(3, 8, 8, relu, pad=1), nn.Conv(3, 8, 8, pad=1)), "+"), A(relu),
                                  nn.SkipConnection(nn.Chain(nn.Conv(3, 8, 8, relu, pad=1), nn.Conv(3, 8, 8, pad=1)), "+"), nn.Dense(128, 128, relu), nn.Dense(128, 4)), prioritized_replay=0)
    # a first-layer pool: nothing between the observation and the conv at layer 2 has parameters, so neither bwd_act1 nor bwd_pool0 nor the conv's dX is emitted
    case("act_behind_first_pool", nn.Chain(nn.MeanPool(2), A(nn.tanh), nn.Conv(2, 2, 4, relu), nn.Dense(36, 4)), prioritized_replay=0)
    case("act_dueling_b128", nn.create_dueling_network(nn.Chain(nn.Conv(3, 2, 16, relu), nn.Dense(576, 32), A(nn.swish), nn.Dense(32, 32, relu), nn.Dense(32, 4))), B=128, dueling=1)
    case("act_lstm", nn.Chain(nn.Conv(3, 2, 4), A(nn.gelu), nn.LSTM(144, 8), A(nn.tanh), nn.Dense(8, 4)), B=4, recurrence=1, trace_length=3, prioritized_replay=0)
    case("acting_act", nn.Chain(nn.Conv(3, 4, 8, relu), nn.Dense(72, 128), A(relu), nn.Dense(128, 4)), obs=K.ENVOBS, envs=True)
    case("refuse_act", nn.Chain(nn.Dense(128, 16), A(nn.gelu), nn.Dense(16, 4)), refuse=True, prioritized_replay=0)
    # the kinds in the table's order: the Activation row is the last, so a GroupNorm at layer 3 is named in front of the Activation at layer 1
    case("refuse_act1_gn3", nn.Chain(nn.Conv(3, 2, 8), A(relu), nn.Conv(3, 8, 8, relu), nn.GroupNorm(8, 2), nn.Dense(128, 4)), refuse=True, prioritized_replay=0)
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
