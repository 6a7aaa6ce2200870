"""CPU: Flux Dropout layers in the Python mirror, the ABI header, the library's host-side validation (no GPU: dqn_plan_default), BSON and the Julia shim, and the fp64
reference the GPU tests (test_dropout_gpu.py) stand on: the mask law's keep rate, its two legs against each other on every case, the margin seeds of the table, and the
proof that the tests can tell -- one flipped mask element, or the layer active in a pass where Flux leaves it inactive, is off by hundreds of tolerances on every case."""
import importlib
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import dropout_reference as DR
import layernorm_reference as LR

ROOT = ge.ROOT
ALL = DR.CASES + DR.REC_CASES
IDS = lambda cs: [c.name for c in cs]


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "_abi", "bson"))


def _bits(p):
    b = int(np.float64(p).view(np.uint64))
    return int(np.uint32(b & 0xFFFFFFFF).view(np.int32)), int(np.uint32(b >> 32).view(np.int32))


def test_enum_value_matches_the_header(mods):
    nn, abi, _ = mods
    hdr = open(os.path.join(ROOT, "include", "dqn_mi355x.h")).read()
    assert int(re.search(r"DQN_LAYER_DROPOUT\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_DROPOUT == 8
    assert int(re.search(r"#define DQN_PLAN_VERSION\s+(\d+)", hdr).group(1)) == 3      # no struct and no exported symbol changed


def test_lowering(mods):
    """kind 8, p's Float64 bits in cin (low word) / cout (high word) -- 0.1 is 0x3FB999999999999A, not the Float32 0.1 --, n_in = n_out = 0 for the engine to fill in"""
    nn, abi, _ = mods
    net = nn.Chain(nn.Dense(6, 16, nn.relu), nn.Dropout(0.1), nn.Dense(16, 8, nn.tanh), nn.Dropout(0.5), nn.Dense(8, 4))
    layers, dueling = nn.lower(net)
    assert not dueling and [l.kind for l in layers] == [abi.LAYER_DENSE, abi.LAYER_DROPOUT, abi.LAYER_DENSE, abi.LAYER_DROPOUT, abi.LAYER_DENSE]
    a, b = layers[1], layers[3]
    assert (a.cin & 0xFFFFFFFF, a.cout & 0xFFFFFFFF) == (0x9999999A, 0x3FB99999) and (a.cin, a.cout) == _bits(0.1)
    assert (b.cin & 0xFFFFFFFF, b.cout & 0xFFFFFFFF) == (0x00000000, 0x3FE00000)
    for l in (a, b):
        assert (l.n_in, l.n_out, l.act, l.stream, l.kh, l.kw, l.sh, l.sw) == (0, 0, abi.ACT_IDENTITY, abi.STREAM_BASE, 0, 0, 0, 0)
    z = nn.lower(nn.Chain(nn.Dense(6, 16), nn.Dropout(0), nn.Dense(16, 4)))[0][1]
    assert (z.kind, z.cin, z.cout) == (8, 0, 0)


def test_no_parameters_in_the_layout_the_initialisation_or_the_bson_file(mods, tmp_path):
    nn, abi, bson = mods
    net = nn.Chain(nn.Dense(6, 5, nn.relu), nn.Dropout(0.5), nn.Dense(5, 4))
    assert net.layers[1].shapes() == []
    p = nn.glorot_params(net, seed=3)
    assert p.size == 6 * 5 + 5 + 5 * 4 + 4
    np.testing.assert_array_equal(p, nn.glorot_params(nn.Chain(nn.Dense(6, 5, nn.relu), nn.Dense(5, 4)), seed=3))
    shapes = bson.julia_param_shapes(net)
    assert shapes == [((5, 6), 30), ((5,), 5), ((4, 5), 20), ((4,), 4)]      # Flux.params skips the layer
    path = str(tmp_path / "qnetwork.bson")
    bson.save_qnetwork(path, p, shapes)
    flat, sizes = bson.load_qnetwork(path)
    np.testing.assert_array_equal(flat, p)
    assert [tuple(s) for s in sizes] == [s for s, _ in shapes]


def test_dueling_split_leaves_the_layer_in_the_base_chain(mods):
    nn, abi, _ = mods
    d = nn.create_dueling_network(nn.Chain(nn.Dense(6, 16, nn.relu), nn.Dropout(0.5), nn.Dense(16, 4)))      # the trailing Dense run stops at the layer: the join sits on it
    assert [l.kind for l in d.base] == ["dense", "dropout"] and d.val.layers[0].n_out == 1
    layers, dueling = nn.lower(d)
    assert dueling and [(l.kind, l.stream) for l in layers] == [(0, 0), (8, 0), (0, 1), (0, 2)]


def test_the_mirror_refuses_by_name(mods):
    nn, abi, _ = mods
    for bad in (-0.1, 1.0, 1.5, float("inf"), float("nan")):
        with pytest.raises(abi.DQNError, match=r"Dropout\(.*\): p must be finite with 0 <= p < 1"):
            nn.Dropout(bad)
    with pytest.raises(abi.DQNError, match=r"p = 1 drops every feature: Q would be constant"):
        nn.Dropout(1.0)
    with pytest.raises(abi.DQNError, match=r"Dropout\(0.5; dims=1\) is not supported; .*dims = :"):
        nn.Dropout(0.5, dims=1)
    nn.Dropout(0.5, dims=":")
    with pytest.raises(abi.DQNError, match=r"unsupported layer .*Dense / Dropout / LSTM.*RNN / LayerNorm / flattenbatch only"):
        nn.lower(nn.Chain(object()))
    # two in a row: the engine refuses it by index (build_layers), the mirror by name -- across the edge of a skip block too
    with pytest.raises(abi.DQNError, match=r"Dropout\(0.5\) cannot directly follow Dropout\(0.1\): two Dropout layers in a row are not supported"):
        nn.lower(nn.Chain(nn.Dense(6, 16), nn.Dropout(0.1), nn.Dropout(0.5), nn.Dense(16, 4)))
    with pytest.raises(abi.DQNError, match=r"two Dropout layers in a row are not supported, as the first inner layer of a SkipConnection neither"):
        nn.lower(nn.Chain(nn.Dense(6, 16), nn.Dropout(0.1), nn.SkipConnection(nn.Chain(nn.Dropout(0.5), nn.Dense(16, 16)), "+"), nn.Dense(16, 4)))
    assert len(nn.lower(nn.Chain(nn.Dense(6, 16), nn.Dropout(0.1), nn.LayerNorm(16), nn.Dropout(0.5), nn.Dense(16, 4)))[0]) == 5      # a LayerNorm between them: accepted, as before


def _L(abi, kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, k=0, s=0):
    d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, k, k, s, s
    return d


def test_host_side_validation_accepts_and_refuses_without_a_gpu(pkg, mods):
    """dqn_plan_default runs build_layers on the host: the supported placements get a plan (the layer's entry all zero), every refusal names the layer index and the value"""
    nn, abi, _ = mods
    D, LN, DO = abi.LAYER_DENSE, abi.LAYER_LAYERNORM, abi.LAYER_DROPOUT
    plan = lambda layers, obs=(6, 1, 1), **kw: pkg.default_plan(layers, pkg.default_hparams(batch_size=8, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], buffer_size=64, **({"dueling": 0} | kw)))

    def do(p=0.5, n=0, **kw):
        lo, hi = _bits(p)
        return _L(abi, DO, n_in=n, n_out=n, cin=lo, cout=hi, **kw)
    ln = lambda n=16, **kw: _L(abi, LN, n_in=n, n_out=n, **kw)
    head = _L(abi, D, n_in=16, n_out=4)
    assert tuple(plan([_L(abi, D, act=1, n_in=6, n_out=16), do(), head])[1]) == (0, 0, 0)
    assert tuple(plan([_L(abi, D, act=1, n_in=6, n_out=16), do(n=16), head])[1]) == (0, 0, 0)      # n given, equal to the incoming feature count
    assert tuple(plan([_L(abi, D, act=1, n_in=6, n_out=2048), do(0.0), _L(abi, D, n_in=2048, n_out=4)])[1]) == (0, 0, 0)
    plan([_L(abi, D, n_in=6, n_out=16), do(), ln(act=1), head])                           # Dense -> Dropout -> LayerNorm(relu) -> Dense: LayerNorm accepts the layer in front of it
    plan([_L(abi, D, n_in=6, n_out=16), ln(act=1), do(), head])                           # ... and behind it
    plan([_L(abi, D, n_in=6, n_out=16), do(), _L(abi, D, stream=1, n_in=16, n_out=1), _L(abi, D, stream=2, n_in=16, n_out=4)], dueling=1)      # the join sits on the layer
    plan([_L(abi, abi.LAYER_LSTM, n_in=6, n_out=8), do(), _L(abi, D, n_in=8, n_out=4)], recurrence=1, trace_length=3)      # behind a recurrent layer
    plan([_L(abi, D, n_in=6, n_out=8), do(), _L(abi, abi.LAYER_GRU, n_in=8, n_out=8), _L(abi, D, n_in=8, n_out=4)], recurrence=1, trace_length=3)
    with pytest.raises(abi.DQNError, match=r"layer 0: Dropout cannot be the first layer"):
        plan([do(), _L(abi, D, n_in=6, n_out=4)])
    with pytest.raises(abi.DQNError, match=r"layer 1: Dropout must directly follow a Dense, recurrent or LayerNorm layer \(layer 0 is a Conv / MaxPool / MeanPool layer, whose output is a \(2, 4, 4\) map\)"):
        plan([_L(abi, abi.LAYER_CONV, cin=1, cout=2, k=3, s=1), do(), _L(abi, D, n_in=32, n_out=4)], obs=(1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"layer 2: Dropout must directly follow a Dense, recurrent or LayerNorm layer \(layer 1 is a Dropout layer\)"):
        plan([_L(abi, D, n_in=6, n_out=16), do(), do(), head])
    for stream in (1, 2):
        with pytest.raises(abi.DQNError, match=r"layer 2: Dropout layers are supported in the base chain only \(not in a value / advantage stream; stream = %d\)" % stream):
            plan([_L(abi, D, n_in=6, n_out=16), _L(abi, D, stream=stream, n_in=16, n_out=16), do(stream=stream), _L(abi, D, stream=3 - stream, n_in=16, n_out=4)], dueling=1)
    with pytest.raises(abi.DQNError, match=r"layer 1: a Dropout layer cannot be the network's output layer"):
        plan([_L(abi, D, n_in=6, n_out=4), do()])
    with pytest.raises(abi.DQNError, match=r"layer 1: Dropout size n = 12 != incoming features 16"):
        plan([_L(abi, D, n_in=6, n_out=16), do(n=12), _L(abi, D, n_in=12, n_out=4)])
    with pytest.raises(abi.DQNError, match=r"layer 1: Dropout n_in 16 != n_out 0"):
        plan([_L(abi, D, n_in=6, n_out=16), _L(abi, DO, n_in=16, n_out=0, cout=_bits(0.5)[1]), head])
    with pytest.raises(abi.DQNError, match=r"layer 1: Dropout has no activation \(act must be DQN_ACT_IDENTITY, got 1\)"):
        plan([_L(abi, D, n_in=6, n_out=16), do(act=1), head])
    for bad, shown in ((-0.25, "-0.25"), (1.0, "p = 1 drops every feature: Q would be constant"), (1.5, "1.5"), (float("inf"), "inf"), (float("nan"), "nan")):
        with pytest.raises(abi.DQNError, match=r"layer 1: Dropout p = .* \(bit pattern 0x[0-9a-f]{16}\) must be finite with 0 <= p < 1") as ei:
            plan([_L(abi, D, n_in=6, n_out=16), do(bad), head])
        assert shown in str(ei.value)
    with pytest.raises(abi.DQNError, match=r"layer 1: Dropout uses n_in, n_out, cin and cout .* kh / kw / sh / sw = 3 / 3 / 0 / 0 must be 0"):
        plan([_L(abi, D, n_in=6, n_out=16), do(k=3), head])
    # the LayerNorm refusals keep their words for the cases they covered before
    with pytest.raises(abi.DQNError, match=r"layer 2: LayerNorm must directly follow a Dense or recurrent layer \(layer 1 is a LayerNorm layer\)"):
        plan([_L(abi, D, n_in=6, n_out=16), ln(), ln(), head])


def test_julia_shim_maps_the_layer_and_refuses_dims_and_a_forced_mode():
    src = open(os.path.join(ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    assert re.search(r"elseif l isa Flux\.Dropout\b", src)
    assert re.search(r"l\.dims === Colon\(\) \|\| throw\(\"DeepQLearningError: [^\"]*Dropout with dims = : only", src)
    assert re.search(r"l\.active === nothing \|\| throw\(\"DeepQLearningError: [^\"]*automatic mode only", src)
    assert re.search(r"bits = reinterpret\(UInt64, Float64\(l\.p\)\)", src)
    assert re.search(r"return LayerDesc\(8, 0, stream, 0, 0, reinterpret\(Int32, UInt32\(bits & 0xffffffff\)\), reinterpret\(Int32, UInt32\(bits >> 32\)\), 0, 0, 0, 0\)", src)
    assert 'throw("DeepQLearningError: unsupported layer' in src and "Dense / Dropout / LSTM" in src and "RNN / LayerNorm / flattenbatch only" in src
    for a, b in (("(", ")"), ("[", "]")):
        assert src.count(a) == src.count(b)
    assert len(re.findall(r"\bend\b", src)) >= len(re.findall(r"^\s*(?:function|if|for|begin|struct|mutable struct|module|let|while|try)\b", src, re.M))


# ------------------------------------------------------------------ the mask law
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_rate_is_binomial(p):
    """N = 2^16 elements (n = 256 features, C = 256 columns): the kept fraction within 4 sqrt(p (1 - p) / N) of 1 - p"""
    n = C = 256; N = n * C
    for k, layer in ((0, 1), (7, 3)):
        keep = DR.keep_mask(DR.ENGINE_SEED, k, layer, n, C, p)
        assert keep.shape == (C, n)
        assert abs(keep.mean() - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / N), (p, k, layer, keep.mean())


def test_p0_keeps_everything_and_the_stream_moves_with_step_layer_and_seed():
    assert DR.keep_mask(DR.ENGINE_SEED, 0, 1, 33, 10, 0.0).all() and DR.do_scale(0.0) == 1.0
    base = DR.uniforms(5, 0, 1, 33, 12)
    assert base.min() >= 0.0 and base.max() < 1.0 and np.unique(base).size > 0.99 * base.size
    for other in (DR.uniforms(5, 1, 1, 33, 12), DR.uniforms(5, 0, 2, 33, 12), DR.uniforms(6, 0, 1, 33, 12), DR.uniforms(5 + (1 << 32), 0, 1, 33, 12), DR.uniforms(5, 1 << 32, 1, 33, 12)):
        assert (other != base).mean() > 0.99
    # q = f * ceil(C / 4) + col / 4: the quads of C = 6 are not those of C = 8 beyond feature 0, and a column's word is its position in its quad
    np.testing.assert_array_equal(DR.uniforms(5, 0, 1, 1, 6), DR.uniforms(5, 0, 1, 1, 8)[:6])
    assert (DR.uniforms(5, 0, 1, 2, 6)[:, 1] != DR.uniforms(5, 0, 1, 2, 12)[:6, 1]).all()
    np.testing.assert_array_equal(DR.uniforms(5, 0, 1, 3, 6)[:, 1], DR.uniforms(5, 0, 1, 3, 8)[:6, 1])      # ceil(6 / 4) == ceil(8 / 4)
    # the scale is Float32(1 / (1 - p)) with the quotient in Float64: 0.1 gives 1.1111112, not the 1.1111113 of Float32 arithmetic on Float32(0.1)
    assert DR.do_scale(0.1) == float(np.float32(1.0 / 0.9)) and DR.do_scale(0.5) == 2.0
    assert DR.DO_TAG == 0x44520000 and (DR.DO_TAG | 31) != DR.RR.TAG


# ------------------------------------------------------------------ the fp64 reference
@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_reference_legs_agree_and_the_seed_keeps_the_margins(c):
    """torch autograd through the law written out and the hand-written NumPy layer: 1e-10 relative on every quantity; the case's fixed seed keeps the margins of the
    LayerNorm table (SIGMA_MIN, RELU_MARGIN, GAP) on the masked s pass and the unmasked s' passes, and no gradient block is dead"""
    D, batch, masks = DR.first_step(c)
    a, b = DR.step(c, D, batch, masks, leg="law"), DR.step(c, D, batch, masks, leg="numpy")
    LR.legs_agree(a, b)
    sg, rm, gap = DR.case_margins(c)
    assert sg >= LR.SIGMA_MIN and rm > LR.RELU_MARGIN and gap > LR.GAP, (c.name, sg, rm, gap)
    DR.check_grads(D.net, a["grads"], b["grads"], live=True)
    for l, m in masks.items():      # the masks of the table do something: both kinds of element where p > 0
        p = DR.nn.all_layers(D.net)[l].p
        assert m.all() if p == 0 else (m.any() and not m.all()), (c.name, l)


@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_the_tests_can_tell(c):
    """one flipped mask element moves a compared quantity by >= 100 tolerances; the layer active on s' or in the target pass moves y / td of every double-Q case likewise"""
    flip, sp, tg = DR.tell_distances(c)
    assert flip >= DR.TELL, (c.name, flip)
    assert bool(c.dq) == (sp is not None)
    if c.dq:
        assert sp >= DR.TELL and tg >= DR.TELL, (c.name, sp, tg)
    else:
        assert all(p == 0 for p in c.ps) or c.name == "single_q_b6"      # every p = 0 case is single-Q


def test_an_inactive_reference_is_the_network_without_the_layer():
    """masks = None (every inactive pass): bit for bit the Q of the chain with the Dropout layers taken out"""
    c = DR.BY_NAME["two_do"]; D = DR.ff_data(c); nn = DR.nn
    bare = nn.Chain(*[l for l in D.net.layers if l.kind != "dropout"])
    x = D.s[:7]
    np.testing.assert_array_equal(DR.q_values(D.net, D.p_on, x), LR.q_values(bare, D.p_on, x))
    masks = DR.masks_for(D.net, 0, 7)
    assert np.abs(DR.q_values(D.net, D.p_on, x, masks) - LR.q_values(bare, D.p_on, x)).max() > 1e-2


def test_exact_readout_network_in_fp64():
    """the GPU readout network in the reference: Dense(n, n) = I, b = 1 -> Dropout(p) -> Dense(n, n) = I on zero observations gives Q = 0 or scale, element for element"""
    nn = DR.nn; n, B, p = 7, 5, 0.25
    net = nn.Chain(nn.Dense(n, n), nn.Dropout(p), nn.Dense(n, n))
    flat = np.concatenate([np.eye(n).ravel(), np.ones(n), np.eye(n).ravel(), np.zeros(n)])
    masks = DR.masks_for(net, 0, B)
    q = DR.q_values(net, flat, np.zeros((B, n)), masks)
    np.testing.assert_array_equal(q, np.where(masks[1], DR.do_scale(p), 0.0))
