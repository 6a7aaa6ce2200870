"""The case table of networks with Flux GlobalMaxPool / GlobalMeanPool / AdaptiveMaxPool / AdaptiveMeanPool layers (TEST INFRASTRUCTURE): tests/test_adaptive_pool_cpu.py and
tests/test_adaptive_pool_gpu.py.  The fp64 reference is the two-legged tests/feedforward_reference.py, unedited: the reference network holds FR.Pool(kind, k, stride)
with the geometry resolve() gives -- Flux's rule, restated here from the law and not from the engine --, the engine receives kinds 12 / 13 with the OUTPUT size
(descs()), and the exact companion is the same network through FR.layer_descs (kinds 5 / 6 with the resolved window: pool.hip).  Data, the per-step checker and its
tolerances are tests/feedforward_edges_common.py; no constant is added.  Every case draws from its FIXED seed and prepare() asserts the relu, MaxPool and argmax margins
(no redraw, no skip at run time); the seeds were found on the CPU with the reference alone (feedforward_edges_common.find_seed)."""
import types

import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_reference as FR

abi = FR.abi
I, RELU = O.ACT_IDENTITY, O.ACT_RELU


def resolve(n_in, n_out):
    """Flux's adaptive rule on one axis -> (k, stride): stride = in ÷ out, k = in - (out - 1) * stride, pad 0"""
    assert 1 <= n_out <= n_in
    s = n_in // n_out
    return n_in - (n_out - 1) * s, s


def windows(n_in, n_out):
    """[(first, last)] of the resolved windows on one axis, inclusive"""
    k, s = resolve(n_in, n_out)
    assert (n_in - k) // s + 1 == n_out
    return [(i * s, i * s + k - 1) for i in range(n_out)]


class APool(FR.Pool):
    """an adaptive / global pool on a known (h, w) map: for the reference an ordinary FR.Pool with the resolved geometry; `out` = (oh, ow) is what the engine is told"""

    def __init__(self, kind, hw, out=(1, 1)):
        (kh, sh), (kw, sw) = resolve(hw[0], out[0]), resolve(hw[1], out[1])
        super().__init__(kind, (kh, kw), (sh, sw))
        self.hw, self.out = tuple(hw), tuple(out)
        assert self.out_shape((1,) + self.hw)[1:] == self.out

    @property
    def is_global(self):
        return self.out == (1, 1)


gmax = lambda hw: (lambda: APool("maxpool", hw))
gmean = lambda hw: (lambda: APool("meanpool", hw))
amax = lambda hw, out: (lambda: APool("maxpool", hw, out))
amean = lambda hw, out: (lambda: APool("meanpool", hw, out))


def descs(net):
    """the network as the engine receives it: every APool as kind 12 / 13 with kh, kw = the OUTPUT size, sh = sw = n_in = n_out = 0; everything else as FR.layer_descs"""
    out = FR.layer_descs(net)
    for d, l in zip(out, net.base):      # base layers come first in ABI order
        if isinstance(l, APool):
            d.kind = abi.LAYER_ADAPTIVEMAXPOOL if l.kind == "maxpool" else abi.LAYER_ADAPTIVEMEANPOOL
            d.kh, d.kw, d.sh, d.sw = l.out[0], l.out[1], 0, 0
    return out


def pools(net):
    return [(i, l) for i, l in enumerate(net.base) if isinstance(l, APool)]


def exact(net):
    """the kinds 5 / 6 network with the resolved window gives the same bits: always for a MaxPool and off the whole-map kernels; for a global MeanPool only where n <= 16
    (every slot of pool_global.hip then holds at most one row and the two summation orders coincide)"""
    return all(l.kind == "maxpool" or not l.is_global or l.hw[0] * l.hw[1] <= 16 for _, l in pools(net))


# ------------------------------------------------------------------ the table: the smallest shapes at which each path of pool_global.hip / the dispatch can go wrong
# seeds: found with find_seed on the CPU, with the reference alone; fixed here
SEEDS = {'g88_max': 1, 'g88_mean': 1, 'g57_max_c3': 2, 'g57_mean_c3': 4, 'g117_max': 1, 'g117_mean': 3, 'g44_max_c16': 3, 'g44_mean_c16': 3, 'g11_max': 1, 'g11_mean': 1, 'g57_b5_max': 1,
         'g57_b5_mean': 1, 'g57_b16_max': 2, 'g57_b16_mean': 2, 'g57_b128_max': 13, 'g57_b128_mean': 35, 'first_gmax_f32': 1, 'first_amean_u8': 1, 'dueling_gmax': 11, 'dueling_gmean': 3, 'g88_ties': 1,
         'a8to3_max': 3, 'a8to3_mean': 2, 'a5to3_max': 2, 'a5to3_mean': 2, 'a7to2_max': 1, 'a78to23_mean': 3, 'a_out_is_in_max': 2, 'a_out13_mean': 3}


def _net(conv, pool, feat, nA=4, hidden=32):
    """Conv -> pool -> Dense(feat, hidden, relu) -> Dense(hidden, nA)"""
    return lambda: [conv(), pool(), O.Dense(feat, hidden, RELU), O.Dense(hidden, nA)]


def _c(name, obs, layers, B, **kw):
    return E.case(name, obs, layers, B, seed=SEEDS.get(name, 1), draws=1, **kw)


c3 = lambda cin, cout, act=RELU: (lambda: O.Conv(3, cin, cout, act))
GLOBAL = [
    # 1. rows per slot (16 slots): 8x8 = 64 rows, four per slot; 5x7 = 35 rows, slots of 3 and 2; 1x17, slot 0 alone holds two; 4x4 = 16, one each; 1x1.  c = 4, 3, 16
    _c("g88_max", (1, 10, 10), _net(c3(1, 4), gmax((8, 8)), 4), 32),
    _c("g88_mean", (1, 10, 10), _net(c3(1, 4), gmean((8, 8)), 4), 32),
    _c("g57_max_c3", (1, 7, 9), _net(c3(1, 3), gmax((5, 7)), 3), 32),
    _c("g57_mean_c3", (1, 7, 9), _net(c3(1, 3), gmean((5, 7)), 3), 32),
    _c("g117_max", (1, 3, 19), _net(c3(1, 4), gmax((1, 17)), 4), 32),
    _c("g117_mean", (1, 3, 19), _net(c3(1, 4), gmean((1, 17)), 4), 32),
    _c("g44_max_c16", (1, 6, 6), _net(c3(1, 16), gmax((4, 4)), 16), 32),
    _c("g44_mean_c16", (1, 6, 6), _net(c3(1, 16), gmean((4, 4)), 16), 32),
    _c("g11_max", (1, 3, 3), _net(c3(1, 4), gmax((1, 1)), 4), 32),
    _c("g11_mean", (1, 3, 3), _net(c3(1, 4), gmean((1, 1)), 4), 32),
    # 2. column edges: B = 5 (ten columns, the target pass starts at column 5: one column a piece), 16 (one partly filled tile of 64), 128 (several column tiles)
    _c("g57_b5_max", (1, 7, 9), _net(c3(1, 3), gmax((5, 7)), 3, hidden=16), 5),
    _c("g57_b5_mean", (1, 7, 9), _net(c3(1, 3), gmean((5, 7)), 3, hidden=16), 5),
    _c("g57_b16_max", (1, 7, 9), _net(c3(1, 3), gmax((5, 7)), 3, hidden=16), 16),
    _c("g57_b16_mean", (1, 7, 9), _net(c3(1, 3), gmean((5, 7)), 3, hidden=16), 16),
    _c("g57_b128_max", (1, 7, 9), _net(c3(1, 3), gmax((5, 7)), 3, hidden=16), 128),
    _c("g57_b128_mean", (1, 7, 9), _net(c3(1, 3), gmean((5, 7)), 3, hidden=16), 128),
    # 3. placement: the first layer (fp32 arena; no input gradient) with an f32 and with a u8 replay -- a global one, and an adaptive 8 -> 3 in front of a Conv;
    #    the last base layer of a dueling network (the join's summed dX is its dY)
    _c("first_gmax_f32", (2, 8, 8), lambda: [APool("maxpool", (8, 8)), O.Dense(2, 16, RELU), O.Dense(16, 4)], 32),
    _c("first_amean_u8", (2, 8, 8), lambda: [APool("meanpool", (8, 8), (3, 3)), O.Conv(3, 2, 4, RELU), O.Dense(4, 4)], 32, u8=1),
    _c("dueling_gmax", (1, 10, 10), lambda: [O.Conv(3, 1, 4, RELU), APool("maxpool", (8, 8)), O.Dense(4, 16, RELU), O.Dense(16, 4)], 32, dueling=True),
    _c("dueling_gmean", (1, 7, 9), lambda: [O.Conv(3, 1, 4, RELU), APool("meanpool", (5, 7)), O.Dense(4, 16, RELU), O.Dense(16, 4)], 32, dueling=True),
    # 4. exact ties: pool_reference's case `ties` under GlobalMaxPool -- an all-zero conv with a non-zero bias and identity activation: all 64 rows of a channel tie in both
    #    precisions, row 0 takes dY (both legs: np.argmax, torch), and the conv's dW / db must match them
    _c("g88_ties", (1, 10, 10), _net(c3(1, 4, I), gmax((8, 8)), 4), 32, zero_conv=True),
]
ADAPTIVE = [
    # 5. adaptive outputs (pool.hip on the resolved geometry): 8 -> 3 (k 4, stride 2), 5 -> 3 (k 3, stride 1: overlapping), 7 -> 2 (k 4, stride 3),
    #    (7, 8) -> (2, 3) (rectangular: (4, 4) / (3, 2)), out = in (k 1, stride 1), out = (1, 3) on 5x7 (a whole axis: (5, 3) / (5, 2))
    _c("a8to3_max", (1, 10, 10), _net(c3(1, 4), amax((8, 8), (3, 3)), 36), 32),
    _c("a8to3_mean", (1, 10, 10), _net(c3(1, 4), amean((8, 8), (3, 3)), 36), 32),
    _c("a5to3_max", (1, 7, 7), _net(c3(1, 4), amax((5, 5), (3, 3)), 36), 32),
    _c("a5to3_mean", (1, 7, 7), _net(c3(1, 4), amean((5, 5), (3, 3)), 36), 32),
    _c("a7to2_max", (1, 9, 9), _net(c3(1, 4), amax((7, 7), (2, 2)), 16), 32),
    _c("a78to23_mean", (1, 9, 10), _net(c3(1, 4), amean((7, 8), (2, 3)), 24), 32),
    _c("a_out_is_in_max", (1, 6, 6), _net(c3(1, 4), amax((4, 4), (4, 4)), 64), 32),
    _c("a_out13_mean", (1, 7, 9), _net(c3(1, 4), amean((5, 7), (1, 3)), 12), 32),
]
CASES = GLOBAL + ADAPTIVE
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def without_pool(c):
    """the network of a 1x1-map case with the pool layer taken out (same parameters, same data)"""
    ls = [l for l in c.layers() if not FR.is_pool(l)]
    return O.Network(c.obs, *O.create_dueling_network(ls)) if c.dueling else O.Network(c.obs, ls)


# ------------------------------------------------------------------ recurrent: Conv -> GlobalMeanPool -> flattenbatch -> LSTM -> Dense (package nn descriptors; feedforward_reference.rec_*)
def rec_net(nn):
    """the chain as the REFERENCE reads it: MeanPool with the resolved whole-map window (feedforward_reference knows MaxPool / MeanPool only)"""
    return nn.Chain(nn.Conv(2, 1, 8, nn.relu), nn.MeanPool((4, 4)), nn.flattenbatch, nn.LSTM(8, 8), nn.Dense(8, REC.nA))


def rec_engine_net(nn):
    """the same chain as the ENGINE receives it"""
    return nn.Chain(nn.Conv(2, 1, 8, nn.relu), nn.GlobalMeanPool(), nn.flattenbatch, nn.LSTM(8, 8), nn.Dense(8, REC.nA))


def rec_nn(nn):
    """the package's nn module with `lower` redirected: feedforward_gpu_common.recurrent_chain lowers the chain it was given (the reference's) -- hand it the engine's"""
    return types.SimpleNamespace(lower=lambda net: nn.lower(rec_engine_net(nn)), **{k: getattr(nn, k) for k in dir(nn) if not k.startswith("__") and k != "lower"})


REC = types.SimpleNamespace(obs=(1, 5, 5), nA=4, B=4, T=3, gamma=0.95, double_q=1, seed=1, steps=3, net=rec_net)      # Conv(2, 1=>8, relu) -> GlobalMeanPool() -> LSTM(8, 8) -> Dense(8, 4)


# ------------------------------------------------------------------ the engine's refusals, by raw descriptors: make(layers, obs, **hparams) plans on the host or creates an engine
def L(kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, kh=0, kw=0, sh=0, sw=0):
    d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, kh, kw, sh, sw
    return d


def engine_accepts_and_refuses(make, raises):
    """build_layers on kinds 12 / 13.  make(layers, obs=(1, 6, 6), **hparams) -> whatever; raises(regex) -> a context manager"""
    AMAX, AMEAN, D, CV = abi.LAYER_ADAPTIVEMAXPOOL, abi.LAYER_ADAPTIVEMEANPOOL, abi.LAYER_DENSE, abi.LAYER_CONV
    conv = lambda co=2: L(CV, act=1, cin=1, cout=co, kh=3, kw=3, sh=1, sw=1)      # (1, 6, 6) -> (co, 4, 4)
    head = lambda n: L(D, n_in=n, n_out=4)
    # accepted: the output size decides the feature count the next layer must state
    make([conv(), L(AMAX, kh=1, kw=1), head(2)])                                  # global: (2, 1, 1)
    make([conv(), L(AMEAN, kh=2, kw=3, cin=2, cout=2), head(12)])                 # (2, 2, 3); the channels stated
    make([conv(), L(AMAX, kh=4, kw=4), head(32)])                                 # out = in
    make([L(AMEAN, kh=1, kw=1), head(1)])                                         # the first layer
    make([conv(), L(AMAX, kh=1, kw=1), L(CV, cin=2, cout=4, kh=1, kw=1, sh=1, sw=1), head(4)])      # a 1x1-fitting Conv behind it
    make([conv(4), L(AMEAN, kh=1, kw=1), L(abi.LAYER_GROUPNORM, cin=4, cout=4, kh=1), head(4)])     # a GroupNorm behind it: n_g = 4 >= 2
    make([conv(), L(AMAX, kh=2, kw=2), L(abi.LAYER_MAXPOOL, kh=2, kw=2, sh=2, sw=2), L(AMEAN, kh=1, kw=1), head(2)])      # pools behind pools
    blk = [L(CV, act=1, cin=2, cout=2, kh=3, kw=3, sh=1, sw=1, n_in=1, n_out=1), L(CV, cin=2, cout=2, kh=3, kw=3, sh=1, sw=1, n_in=1, n_out=1), L(abi.LAYER_SKIPADD_MAP, cin=2)]
    make([conv(), L(AMAX, kh=3, kw=3)] + blk + [head(18)])                        # the entry of a convolutional skip block
    make([conv(), L(AMEAN, kh=1, kw=1), L(abi.LAYER_LSTM, n_in=2, n_out=8), L(D, n_in=8, n_out=4)], recurrence=1, trace_length=3)
    make([conv(), L(AMAX, kh=1, kw=1), L(D, stream=1, n_in=2, n_out=1), L(D, stream=2, n_in=2, n_out=4)], dueling=1)      # the last base layer of a dueling network
    with raises(r"layer 2: dense n_in 8 != incoming features 12"):                # the resolved map is (2, 2, 3)
        make([conv(), L(AMEAN, kh=2, kw=3), head(8)])
    # refused, by layer index and value
    for kh, kw in ((0, 1), (1, 0), (-1, 2)):
        with raises(r"layer 1: AdaptiveMaxPool output size \(%d, %d\) must be at least \(1, 1\)" % (kh, kw)):
            make([conv(), L(AMAX, kh=kh, kw=kw), head(2)])
    with raises(r"layer 1: AdaptiveMeanPool output size \(5, 2\) is larger than the 4x4 input map"):
        make([conv(), L(AMEAN, kh=5, kw=2), head(2)])
    with raises(r"layer 1: AdaptiveMaxPool output size \(1, 5\) is larger than the 4x4 input map"):
        make([conv(), L(AMAX, kh=1, kw=5), head(2)])
    for slot in ("sh", "sw", "n_in", "n_out"):
        vals = {k: (1 if k == slot else 0) for k in ("sh", "sw", "n_in", "n_out")}
        with raises(r"layer 1: AdaptiveMaxPool uses cin, cout, kh and kw \(the OUTPUT size \(oh, ow\)\) only; sh / sw / n_in / n_out = %d / %d / %d / %d must be 0" % tuple(vals.values())):
            make([conv(), L(AMAX, kh=1, kw=1, **vals), head(2)])
    with raises(r"layer 1: AdaptiveMeanPool has no activation \(act must be DQN_ACT_IDENTITY, got 1\)"):
        make([conv(), L(AMEAN, act=1, kh=1, kw=1), head(2)])
    for stream in (1, 2):
        with raises(r"layer 2: AdaptiveMaxPool layers are supported in the base chain only \(not in a value / advantage stream; stream = %d\)" % stream):
            make([conv(), L(D, stream=stream, n_in=32, n_out=16), L(AMAX, stream=stream, kh=1, kw=1), L(D, stream=3 - stream, n_in=32, n_out=4)], dueling=1)
    with raises(r"layer 1: AdaptiveMeanPool must be the first layer or follow a layer whose output is a \(c, h, w\) map \(layer 0 is a Dense layer, whose output is a feature vector of 16\)"):
        make([L(D, n_in=36, n_out=16), L(AMEAN, kh=1, kw=1), head(16)])
    with raises(r"layer 1: AdaptiveMaxPool must be the first layer or follow .* \(layer 0 is a recurrent layer"):
        make([L(abi.LAYER_LSTM, n_in=36, n_out=8), L(AMAX, kh=1, kw=1), head(8)], recurrence=1, trace_length=3)
    with raises(r"layer 1: AdaptiveMaxPool cin 3 / cout 3 != incoming channels 2"):
        make([conv(), L(AMAX, cin=3, cout=3, kh=1, kw=1), head(2)])
    with raises(r"layer 1: a MaxPool / MeanPool layer cannot be the network's output layer"):      # the pool row of the traits table
        make([conv(4), L(AMAX, kh=1, kw=1)])
    with raises(r"layer 2: GroupNorm\(2, 2\) on a \(2, 1, 1\) map normalises over n_g = 1 element"):      # the existing n_g >= 2 rule, behind a global pool
        make([conv(), L(AMEAN, kh=1, kw=1), L(abi.LAYER_GROUPNORM, cin=2, cout=2, kh=2), head(2)])
    with raises(r"layer 3: the convolutional skip block holds a MaxPool / MeanPool layer \(layer 2\)"):      # an inner layer: refused as a pool is
        make([conv(), blk[0], L(AMAX, kh=4, kw=4), L(abi.LAYER_SKIPADD_MAP, cin=2), head(32)])
    with raises(r"layer 2: conv kernel/stride does not fit the 1x1 input"):      # what may follow a pool may follow these -- and nothing more
        make([conv(), L(AMAX, kh=1, kw=1), L(CV, cin=2, cout=4, kh=2, kw=2, sh=1, sw=1), head(4)])
