"""The case table of networks with Flux MaxPool / MeanPool layers (TEST INFRASTRUCTURE): tests/test_pool_cpu.py and tests/test_pool_gpu.py.  The fp64 reference
with its two legs and the margin rule is tests/feedforward_reference.py; data, the per-step checker and its tolerances are tests/feedforward_edges_common.py.
A MaxPool is a second non-smooth point beside relu (feedforward_reference.margins): every case draws from its FIXED seed and prepare() asserts the margins (no redraw,
no skip at run time); the seeds were found on the CPU with the reference alone (feedforward_edges_common.find_seed)."""
import types

import dqn_oracle as O
import feedforward_edges_common as E
from feedforward_reference import MaxPool, MeanPool, abi, is_pool      # noqa: F401  (abi: re-exported for the test files)

I, RELU = O.ACT_IDENTITY, O.ACT_RELU


# ------------------------------------------------------------------ the table: the smallest shapes at which each path of pool.hip / the program can go wrong
# seeds: found with find_seed on the CPU, with the reference alone; fixed here
SEEDS = {'max_c16': 2400, 'max_c3': 2, 'mean_c16': 1584, 'between': 303, 'overlap_max': 3, 'overlap_mean': 2, 'gaps_max': 1, 'gaps_mean': 2, 'whole_max': 1, 'whole_mean': 1,
         'one_max': 1, 'one_mean': 1, 'first_max_f32': 3, 'first_mean_u8': 1, 'dueling_max': 21, 'b5_max': 1, 'b5_mean': 1, 'b16_max': 2, 'b128_max': 6, 'b128_mean': 4, 'ties': 1}


def _net(conv, pool, feat, nA=4, hidden=32):
    """Conv -> pool -> Dense(feat, hidden, relu) -> Dense(hidden, nA)"""
    return lambda: [conv(), pool(), O.Dense(feat, hidden, RELU), O.Dense(hidden, nA)]


def _c(name, obs, layers, B, **kw):
    return E.case(name, obs, layers, B, seed=SEEDS.get(name, 1), draws=1, **kw)


c3 = lambda cin, cout, act=RELU: (lambda: O.Conv(3, cin, cout, act))
CASES = [
    # 1. Conv(3, 1=>16, relu) -> pool(2) -> Dense -> Dense on 1x10x10 (8x8 map -> 4x4), B = 32: the LDS / MFMA conv family; cout = 3: the VALU family; MeanPool
    _c("max_c16", (1, 10, 10), _net(c3(1, 16), lambda: MaxPool(2), 256), 32),
    _c("max_c3", (1, 10, 10), _net(c3(1, 3), lambda: MaxPool(2), 48), 32),
    _c("mean_c16", (1, 10, 10), _net(c3(1, 16), lambda: MeanPool(2), 256), 32),
    # 2. pools between convs on 2x15x14: 13x12 -> 6x6 -> 4x4 -> 2x2; the upper conv's dX lands in a pool's dY
    _c("between", (2, 15, 14), lambda: [O.Conv(3, 2, 8, RELU), MaxPool(2), O.Conv(3, 8, 8, RELU), MeanPool(2), O.Dense(32, 4)], 32),
    # 3. overlapping rectangular windows and an uncovered edge behind a conv whose map is 8x7 (MaxPool (3,2)/(2,1): row 7 is in no window)
    _c("overlap_max", (1, 10, 9), _net(c3(1, 4), lambda: MaxPool((3, 2), (2, 1)), 4 * 3 * 6), 32),
    _c("overlap_mean", (1, 10, 9), _net(c3(1, 4), lambda: MeanPool((2, 3), (1, 2)), 4 * 7 * 3), 32),
    # 4. gaps: window 2, stride 3 (8x8 -> 3x3; rows / columns 2 and 5 are in no window)
    _c("gaps_max", (1, 10, 10), _net(c3(1, 4), lambda: MaxPool(2, 3), 36), 32),
    _c("gaps_mean", (1, 10, 10), _net(c3(1, 4), lambda: MeanPool(2, 3), 36), 32),
    # 5. the window is the whole map: 1x1 output
    _c("whole_max", (1, 10, 10), _net(c3(1, 4), lambda: MaxPool(8), 4), 32),
    _c("whole_mean", (1, 10, 10), _net(c3(1, 4), lambda: MeanPool(8), 4), 32),
    # 6. window 1x1, stride 1: bit for bit the network without the layer (test_pool_gpu.py)
    _c("one_max", (1, 10, 10), _net(c3(1, 4), lambda: MaxPool(1), 256), 32),
    _c("one_mean", (1, 10, 10), _net(c3(1, 4), lambda: MeanPool(1), 256), 32),
    # 7. a pool as the first layer (fp32 arena; no input gradient), with an f32 and with a u8 replay
    _c("first_max_f32", (2, 8, 8), lambda: [MaxPool(2), O.Conv(3, 2, 4, RELU), O.Dense(16, 4)], 32),
    _c("first_mean_u8", (2, 8, 8), lambda: [MeanPool(2), O.Conv(3, 2, 4, RELU), O.Dense(16, 4)], 32, u8=1),
    # 8. dueling: the pool is the last base layer, the join's summed dX is its dY
    _c("dueling_max", (1, 10, 10), lambda: [O.Conv(3, 1, 4, RELU), MaxPool(2), O.Dense(64, 16, RELU), O.Dense(16, 4)], 32, dueling=True),
    # 9. column edges: B = 5 (ten columns, the target pass starts at column 5: the scalar path), 16, and 128 (the large-batch schedule)
    _c("b5_max", (1, 6, 6), _net(c3(1, 3), lambda: MaxPool(2), 12, hidden=16), 5),
    _c("b5_mean", (1, 6, 6), _net(c3(1, 3), lambda: MeanPool(2), 12, hidden=16), 5),
    _c("b16_max", (1, 6, 6), _net(c3(1, 3), lambda: MaxPool(2), 12, hidden=16), 16),
    _c("b128_max", (1, 6, 6), _net(c3(1, 3), lambda: MaxPool(2), 12, hidden=16), 128),
    _c("b128_mean", (1, 6, 6), _net(c3(1, 3), lambda: MeanPool(2), 12, hidden=16), 128),
    # 10. exact ties: an all-zero conv with a non-zero bias and identity activation -- every MaxPool window ties in both precisions.  This case PINS the tie
    #     rule: both legs (np.argmax, torch) route dY to the first tap, and the conv's dW / db must match them
    _c("ties", (1, 10, 10), _net(c3(1, 4, I), lambda: MaxPool(2), 64), 32, zero_conv=True),
]
BY_NAME = {c.name: c for c in CASES}


def without_pool(c):
    """the network of a 1x1-window case with the pool layer taken out (same parameters, same data)"""
    ls = [l for l in c.layers() if not is_pool(l)]
    return O.Network(c.obs, *O.create_dueling_network(ls)) if c.dueling else O.Network(c.obs, ls)


# ------------------------------------------------------------------ recurrent: Conv -> pool -> LSTM -> Dense (package nn descriptors; feedforward_reference.rec_*)
def rec_net(nn):
    return nn.Chain(nn.Conv(2, 1, 8, nn.relu), nn.MaxPool(2), nn.LSTM(32, 8), nn.Dense(8, REC.nA))


REC = types.SimpleNamespace(obs=(1, 5, 5), nA=4, B=4, T=3, gamma=0.95, double_q=1, seed=3, steps=3, net=rec_net)      # case 11: Conv(2, 1=>8, relu) -> MaxPool(2) -> LSTM(32, 8) -> Dense(8, 4)
