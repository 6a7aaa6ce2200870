"""The networks behind tests/golden/conv_dg_traits_gpu.json (TEST INFRASTRUCTURE): kind_traits_cases' recording -- the launch names of one train step and of a middle step,
the acting program's fused_tail, the dqn_comm_init / DQN_SIM_WORLD refusal texts -- for networks with a dilated / grouped / depthwise Conv (kind 15), in a module of its own
(kind_traits_cases.py, groupnorm_traits_cases.py, activation_traits_cases.py and their goldens are not edited).  Nothing here computes an expected value."""
import activation_traits_cases as AT
import kind_traits_cases as K

nn, pkg = K.nn, K.pkg
relu = nn.relu
C, DW = nn.Conv, nn.DepthwiseConv


def _cases():
    c = {}
    case = lambda name, net, obs=K.IMG, B=8, env=None, envs=False, refuse=False, **hp: c.__setitem__(name, dict(net=net, obs=obs, B=B, hp=hp, env=env or {}, envs=envs, refuse=refuse))
    # the first layer on a u8 replay: the byte arena, no input gradient; the heads keep their fusion (the kind declines the acting tail only, as the padded Conv does)
    case("cdg_first_u8", nn.Chain(C(3, 2, 16, relu, pad=2, dilation=2), nn.Dense(1024, 128, relu), nn.Dense(128, 4)), B=32, obs_dtype=K.abi.OBS_U8)
    # the depthwise-separable stem, and a grouped layer with a dX in front of a pool
    case("cdg_separable_gn", nn.Chain(DW(3, 2, 4, pad=1), C(1, 4, 8), nn.GroupNorm(8, 2, relu), C(3, 8, 8, relu, groups=2), nn.MaxPool(2), nn.Dense(72, 4)), prioritized_replay=0)
    # the entry of a convolutional skip block, then an Activation
    case("cdg_skip_entry", nn.Chain(C(3, 2, 8, nn.tanh, pad=2, dilation=2, groups=2), nn.SkipConnection(nn.Chain(C(3, 8, 8, relu, pad=1), C(3, 8, 8, pad=1)), "+"),
                                    nn.Activation(relu), nn.Dense(512, 4)), prioritized_replay=0)
    case("cdg_dueling_b128", nn.create_dueling_network(nn.Chain(C(1, 2, 16, relu), C(3, 16, 16, relu, pad=2, dilation=2), nn.Dense(1024, 32, relu), nn.Dense(32, 4))), B=128, dueling=1)
    case("cdg_lstm", nn.Chain(C(3, 2, 4, relu, dilation=2), nn.LSTM(64, 8), nn.Dense(8, 4)), B=4, recurrence=1, trace_length=3, prioritized_replay=0)
    case("acting_cdg", nn.Chain(DW(3, 4, 8, relu), nn.Dense(72, 128, relu), nn.Dense(128, 4)), obs=K.ENVOBS, envs=True)
    case("refuse_cdg", nn.Chain(DW(3, 2, 4, relu), nn.Dense(144, 4)), refuse=True, prioritized_replay=0)
    # the kinds in the table's order: the new row is the last, so an Activation at layer 1 is named in front of the dilated Conv at layer 0
    case("refuse_cdg0_act1", nn.Chain(C(3, 2, 4, dilation=2), nn.Activation(relu), nn.Dense(64, 4)), refuse=True, prioritized_replay=0)
    return c


CASES = _cases()


def observe(name):
    """activation_traits_cases.observe on this module's table"""
    saved = AT.CASES
    AT.CASES = CASES
    try:
        return AT.observe(name)
    finally:
        AT.CASES = saved
