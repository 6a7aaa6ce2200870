"""The case table of networks with a PADDED convolution -- Flux Conv((kh, kw), cin => cout, act; stride, pad = (ph, pw)), symmetric zero padding -- (TEST
INFRASTRUCTURE): tests/test_conv_pad_cpu.py and tests/test_conv_pad_gpu.py.  The fp64 reference with its two legs and the margin rule is tests/feedforward_reference.py;
data, the per-step checker and its tolerances are tests/feedforward_edges_common.py.  Every case draws from its FIXED seed and prepare() asserts the margins (no redraw,
no skip at run time); the seeds were found on the CPU with the reference alone (feedforward_edges_common.find_seed)."""
import types

import numpy as np

import dqn_oracle as O
import feedforward_edges_common as E
from feedforward_reference import MaxPool, MeanPool, PConv, abi, is_pool, layer_descs, pad_of      # noqa: F401  (re-exported for the test files)

I, RELU, TANH, SIG = O.ACT_IDENTITY, O.ACT_RELU, O.ACT_TANH, O.ACT_SIGMOID


def extended(c, net, D):
    """the exact check's second network: the case's first (padded) conv with pad 0 on observations zero-extended by (ph, pw) -- a 0 byte border for u8.  -> (layer descs, the
    hyper-parameter view with the extended observation shape, s, sp)"""
    ph, pw = pad_of(net.base[0]); C, H, W = net.obs_shape
    ext = lambda x: np.pad(x, ((0, 0), (0, 0), (ph, ph), (pw, pw)))
    view = types.SimpleNamespace(obs_shape=(C, H + 2 * ph, W + 2 * pw), n_actions=net.n_actions, dueling=net.dueling)
    return layer_descs(net, pad=False), view, ext(D["s"]), ext(D["sp"])


# ------------------------------------------------------------------ the table: the smallest shapes at which the index math of conv_own.hip / the program can go wrong
# seeds: found with find_seed on the CPU, with the reference alone; fixed here
SEEDS = {'same3': 1, 'all_border': 1, 'rect': 1, 'one_axis': 2, 'stride2': 1, 'aniso': 1, 'interior': 683, 'interior_tanh': 1, 'stack_same': 1, 'pool_after': 1, 'pool_before': 1, 'dueling_u8': 13}


def _c(name, obs, layers, B, **kw):
    return E.case(name, obs, layers, B, seed=SEEDS.get(name, 1), draws=1, **kw)


CASES = [
    # the basic border, an odd batch (ten columns, the target pass starts at column 5)
    _c("same3", (1, 5, 5), lambda: [PConv(3, 1, 4, RELU, pad=1), O.Dense(100, 4)], 5),
    # every window touches padding: 2x2 map, 3x3 kernel, pad 1 -> 2x2
    _c("all_border", (2, 2, 2), lambda: [PConv(3, 2, 3, TANH, pad=1), O.Dense(12, 4)], 8),
    # ph != pw, rectangular kernel and map: 6x7 -> 6x7
    _c("rect", (2, 6, 7), lambda: [PConv((3, 5), 2, 4, RELU, pad=(1, 2)), O.Dense(168, 4)], 16),
    # an unpadded axis beside a padded one: 6x6 -> 6x4
    _c("one_axis", (1, 6, 6), lambda: [PConv(3, 1, 4, RELU, pad=(1, 0)), O.Dense(96, 4)], 8),
    # stride 2: the extended map is 9x10, the last column of the trailing padding is dropped; dX tap divisibility.  7x8 -> 4x4
    _c("stride2", (2, 7, 8), lambda: [PConv(3, 2, 4, RELU, stride=2, pad=1), O.Dense(64, 4)], 16),
    # anisotropic stride with pad: kernel (4,3), stride (2,1), pad (1,1): 8x6 -> 4x6
    _c("aniso", (1, 8, 6), lambda: [PConv((4, 3), 1, 4, RELU, stride=(2, 1), pad=(1, 1)), O.Dense(96, 4)], 8),
    # dX THROUGH a padded conv into a relu epilogue; 16-channel MFMA tiles: 8x8 -> 6x6 -> 6x6
    _c("interior", (1, 8, 8), lambda: [O.Conv(3, 1, 16, RELU), PConv(3, 16, 16, RELU, pad=1), O.Dense(576, 4)], 32),
    # the dact_f kinds, cout 32, stride 2 on the padded layer: 8x8 -> 6x6 -> 3x3
    _c("interior_tanh", (1, 8, 8), lambda: [O.Conv(3, 1, 16, TANH), PConv(3, 16, 32, SIG, stride=2, pad=1), O.Dense(288, 4)], 16),
    # three pad-1 3x3 convs at B = 128: the dW sample-chunk path.  (smooth activations: 128 x 720 relu units per step leave no seed with every unit off its kink;
    # the relu epilogues are the other cases')
    _c("stack_same", (4, 6, 6), lambda: [PConv(3, 4, 4, TANH, pad=1), PConv(3, 4, 8, SIG, pad=1), PConv(3, 8, 8, TANH, pad=1), O.Dense(288, 4)], 128),
    # the neighbours that launch alone
    _c("pool_after", (1, 6, 6), lambda: [PConv(3, 1, 4, RELU, pad=1), MaxPool(2), O.Dense(36, 4)], 16),
    _c("pool_before", (2, 8, 8), lambda: [MeanPool(2), PConv(3, 2, 4, RELU, pad=1), O.Dense(64, 4)], 16),
    # first-layer pad 1, dueling streams, u8 replay: the byte arena, the dueling join's dX.  cout 16, K = 36: the MFMA forms read bytes
    _c("dueling_u8", (4, 6, 6), lambda: [PConv(3, 4, 16, RELU, pad=1), O.Dense(576, 16, RELU), O.Dense(16, 4)], 32, dueling=True, u8=1),
    # beyond the issue's table: 16 output channels at B = 128 -- the default plan cuts the dW chains in SAMPLES (32-aligned chunks that start inside a position) and the
    # MFMA dW walks them; smooth activation for the reason given at stack_same
    _c("b128_c16", (4, 6, 6), lambda: [PConv(3, 4, 16, TANH, pad=1), O.Dense(576, 4)], 128),
]
BY_NAME = {c.name: c for c in CASES}
FIRST_LAYER = ["same3", "all_border", "rect", "one_axis", "stride2", "aniso", "dueling_u8", "b128_c16"]      # the padded conv is the first layer: the exact check's cases


# ------------------------------------------------------------------ recurrent: Conv(3, 1=>8, relu; pad=1) -> LSTM -> Dense, T = 3, B = 4 (package nn descriptors; feedforward_reference.rec_*)
def rec_net(nn):
    return nn.Chain(nn.Conv(3, 1, 8, nn.relu, pad=1), nn.LSTM(200, 8), nn.Dense(8, REC.nA))


REC = types.SimpleNamespace(obs=(1, 5, 5), nA=4, B=4, T=3, gamma=0.95, double_q=1, seed=1, steps=3, net=rec_net)
