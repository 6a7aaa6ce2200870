"""CPU: CONVOLUTIONAL Flux SkipConnection(layers, +) blocks -- x + Conv(Conv(x)) on a (c, h, w) map, descriptor kind DQN_LAYER_SKIPADD_MAP = 10 -- in the Python mirror,
the ABI header, the library's host-side validation (no GPU: dqn_plan_default runs build_layers) and the Julia shim, and the fp64 reference the GPU tests
(test_conv_skip_gpu.py) stand on: its two legs against each other on every case, the margin seeds of the table along the three-step trajectory, and the proof that the
tests can tell -- each wrong engine (the entry gradient without + dY, the entry's derivative before the sum or twice, the last inner layer's derivative omitted at the join,
the skip read from the first inner layer's output) is off by hundreds of tolerances on every case it applies to.  The kind-9 refusals on maps stay what they were
(test_skip_cpu.py holds their words; here: that they still apply next to the new kind)."""
import importlib
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import conv_skip_reference as CR

ROOT = ge.ROOT
IDS = lambda cs: [c.name for c in cs]


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "_abi", "bson"))


def test_enum_value_matches_the_header(mods):
    nn, abi, _ = mods
    hdr = open(os.path.join(ROOT, "include", "dqn_mi355x.h")).read()
    assert int(re.search(r"DQN_LAYER_SKIPADD_MAP\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_SKIPADD_MAP == 10
    assert int(re.search(r"DQN_LAYER_SKIPADD\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_SKIPADD == 9
    assert int(re.search(r"#define DQN_PLAN_VERSION\s+(\d+)", hdr).group(1)) == 3      # no struct and no exported symbol changed, no summation order either
    assert "SKIPADD_MAP, the join of a CONVOLUTIONAL SkipConnection(layers, +) block" in hdr


# ------------------------------------------------------------------ lowering
def _blk(nn, c=16, k=3, pad=1, act_k=None):
    return nn.SkipConnection(nn.Chain(nn.Conv(k, c, c, nn.relu, 1, pad), nn.Conv(k, c, c, act_k or nn.identity, 1, pad)), "+")


def test_lowering_to_kind_10_behind_a_map_and_to_kind_9_behind_a_vector(mods):
    nn, abi, _ = mods
    C, D, MP, SK, SKM = abi.LAYER_CONV, abi.LAYER_DENSE, abi.LAYER_MAXPOOL, abi.LAYER_SKIPADD, abi.LAYER_SKIPADD_MAP
    net = nn.Chain(nn.Conv(3, 2, 16, nn.relu, 1, 1), _blk(nn), nn.MaxPool(2), nn.SkipConnection(nn.Conv((3, 5), 16, 16, nn.tanh, 1, (1, 2)), "+"), _blk(nn), nn.flattenbatch,
                   nn.Dense(144, 32, nn.relu), nn.SkipConnection(nn.Dense(32, 32), "+"), nn.Dense(32, 4))
    layers, dueling = nn.lower(net)
    assert not dueling and [l.kind for l in layers] == [C, C, C, SKM, MP, C, SKM, C, C, SKM, D, D, SK, D]
    for j, m in ((3, 2), (6, 1), (9, 2), (12, 1)):      # the join: the descriptor shape of kind 9
        l = layers[j]
        assert (l.cin, l.n_in, l.n_out, l.act, l.stream, l.cout, l.kh, l.kw, l.sh, l.sw) == (m, 0, 0, abi.ACT_IDENTITY, abi.STREAM_BASE, 0, 0, 0, 0, 0), j
    assert (layers[5].kh, layers[5].kw, layers[5].n_in, layers[5].n_out, layers[5].act) == (3, 5, 1, 2, abi.ACT_TANH)      # the inner conv keeps its pad in n_in / n_out
    # a block in the last place of a dueling base chain
    d = nn.create_dueling_network(nn.Chain(nn.Conv(3, 2, 16, nn.relu, 1, 1), _blk(nn), nn.flattenbatch, nn.Dense(576, 4)))
    assert [(l.kind, l.stream) for l in nn.lower(d)[0]] == [(C, 0), (C, 0), (C, 0), (SKM, 0), (D, 1), (D, 2)]


def test_parameter_order_walks_into_the_block(mods, tmp_path):
    """Flux.params of the block = the inner layers' arrays in order: all_layers, glorot_params, julia_param_shapes and the BSON round trip see the same chain without it"""
    nn, abi, bson = mods
    net = nn.Chain(nn.Conv(3, 2, 4, nn.relu, 1, 1), _blk(nn, 4), nn.flattenbatch, nn.Dense(100, 4))
    flat = nn.Chain(nn.Conv(3, 2, 4, nn.relu, 1, 1), nn.Conv(3, 4, 4, nn.relu, 1, 1), nn.Conv(3, 4, 4, nn.identity, 1, 1), nn.flattenbatch, nn.Dense(100, 4))
    assert [l.kind for l in nn.all_layers(net)] == ["conv", "conv", "conv", "dense"]
    p = nn.glorot_params(net, seed=3)
    np.testing.assert_array_equal(p, nn.glorot_params(flat, seed=3))
    assert p.size == 72 + 4 + 2 * (144 + 4) + 400 + 4
    shapes = bson.julia_param_shapes(net)
    assert shapes == bson.julia_param_shapes(flat) and [n for _, n in shapes] == [72, 4, 144, 4, 144, 4, 400, 4]
    path = str(tmp_path / "qnetwork.bson")
    bson.save_qnetwork(path, p, shapes)
    np.testing.assert_array_equal(bson.load_qnetwork(path)[0], p)


def test_the_mirror_refuses_by_name(mods):
    nn, abi, _ = mods
    stem, head = nn.Conv(3, 2, 16, nn.relu, 1, 1), nn.Dense(576, 4)
    low = lambda *ls: nn.lower(nn.Chain(*ls))
    with pytest.raises(abi.DQNError, match=r"a Conv with pad 0 inside a convolutional SkipConnection is not supported \(its inner layers are Conv layers with pad != 0 only"):
        low(stem, nn.SkipConnection(nn.Chain(nn.Conv(3, 16, 16, nn.relu, 1, 1), nn.Conv(1, 16, 16)), "+"), head)
    with pytest.raises(abi.DQNError, match=r"a MaxPool / MeanPool layer inside a convolutional SkipConnection is not supported"):
        low(stem, nn.SkipConnection(nn.Chain(nn.Conv(3, 16, 16, nn.relu, 1, 1), nn.MeanPool(1)), "+"), head)
    with pytest.raises(abi.DQNError, match=r"maps 16 channels to 8; SkipConnection\(layers, \+\) needs layers: \(c, h, w\) -> \(c, h, w\)"):
        low(stem, nn.SkipConnection(nn.Chain(nn.Conv(3, 16, 8, nn.relu, 1, 1)), "+"), nn.Dense(288, 4))
    with pytest.raises(abi.DQNError, match=r"cannot be the network's output layer"):
        low(stem, _blk(nn))
    with pytest.raises(abi.DQNError, match=r"cannot be the first layer: a skip block's input is never the observation"):
        low(_blk(nn), head)
    # the kind-9 refusals on maps keep their words
    with pytest.raises(abi.DQNError, match=r"cannot follow a Conv / MaxPool / MeanPool layer: a skip block stands on a feature vector \(convolutional residual blocks are not supported\)"):
        low(stem, nn.flattenbatch, nn.SkipConnection(nn.Dense(576, 576), "+"), head)
    with pytest.raises(abi.DQNError, match=r"cannot follow a Conv / MaxPool / MeanPool layer: a skip block stands on a feature vector"):
        low(stem, _blk(nn), nn.SkipConnection(nn.Dense(576, 576), "+"), head)      # ... behind a convolutional block's join too
    with pytest.raises(abi.DQNError, match=r"a Conv / MaxPool / MeanPool layer inside a SkipConnection is not supported"):
        low(stem, nn.flattenbatch, nn.Dense(576, 16), nn.SkipConnection(nn.Chain(nn.Conv(3, 1, 1, nn.relu, 1, 1)), "+"), nn.Dense(16, 4))
    with pytest.raises(abi.DQNError, match=r"cannot follow a Conv / MaxPool / MeanPool layer"):      # a mixed block behind a map is no convolutional block
        low(stem, nn.SkipConnection(nn.Chain(nn.Conv(3, 16, 16, nn.relu, 1, 1), nn.Dense(576, 576)), "+"), head)
    with pytest.raises(abi.DQNError, match=r"is supported in the base chain only"):
        nn.lower(nn.DuelingNetwork(nn.Chain(stem), nn.Chain(_blk(nn), nn.Dense(576, 1)), nn.Chain(nn.Dense(576, 4))))


def _L(abi, kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, k=0, s=0, kw=None):
    d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, k, kw or k, s, s
    return d


def test_host_side_validation_accepts_and_refuses_without_a_gpu(pkg, mods):
    """dqn_plan_default runs build_layers on the host: the supported placements get a plan (the join's entry all zero), every refusal names the layer index"""
    nn, abi, _ = mods
    C, D, SK, SKM = abi.LAYER_CONV, abi.LAYER_DENSE, abi.LAYER_SKIPADD, abi.LAYER_SKIPADD_MAP
    plan = lambda layers, obs=(2, 6, 6), **kw: pkg.default_plan(layers, pkg.default_hparams(batch_size=8, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], buffer_size=64, **({"dueling": 0} | kw)))
    cv = lambda cin=16, cout=16, k=3, pad=1, **kw: _L(abi, C, cin=cin, cout=cout, k=k, s=1, n_in=pad, n_out=pad, **kw)
    pool = lambda kind=abi.LAYER_MAXPOOL, k=2: _L(abi, kind, k=k, s=k)
    dn = lambda a, b, **kw: _L(abi, D, n_in=a, n_out=b, **kw)
    skm = lambda m, n=0, **kw: _L(abi, SKM, cin=m, n_in=n, n_out=n, **kw)
    stem, head = cv(2, 16, act=1), dn(576, 4)
    for c in CR.ALL:      # every case of the table lowers and gets a plan
        layers, dueling = nn.lower(c.mk())
        got = pkg.default_plan(layers, pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=c.obs[0], obs_h=c.obs[1], obs_w=c.obs[2], buffer_size=64, dueling=int(dueling),
                                                           recurrence=int(bool(c.T)), trace_length=c.T or 1, prioritized_replay=0 if c.T else 1))
        assert all(tuple(p) == (0, 0, 0) for p, l in zip(got, layers) if l.kind == SKM), c.name
    assert tuple(plan([stem, cv(act=1), cv(), skm(2), head])[3]) == (0, 0, 0)
    plan([stem, cv(), skm(1, 576), head])                                                  # one inner layer; n given
    plan([cv(2, 16, pad=0, act=2), cv(), skm(1), dn(256, 4)])                              # P a pad-0 Conv
    plan([stem, pool(), cv(), skm(1), dn(144, 4)]); plan([stem, pool(abi.LAYER_MEANPOOL), cv(), skm(1), dn(144, 4)])      # P a pool
    plan([pool(), cv(2, 2), skm(1), dn(18, 4)])                                            # P a pool on the observation: no input gradient behind the block
    plan([stem, cv(), skm(1), cv(act=3), skm(1), head])                                    # P a join
    plan([stem, cv(), skm(1), cv(16, 8, pad=0), dn(128, 4)]); plan([stem, cv(), skm(1), pool(), dn(144, 4)])      # a Conv / a pool consumes the join
    plan([stem, _L(abi, C, cin=16, cout=16, k=3, kw=5, s=1, n_in=1, n_out=2), skm(1), head])      # a rectangular kernel, pad (1, 2)
    plan([stem, _L(abi, C, cin=16, cout=16, k=1, kw=3, s=1, n_in=0, n_out=1), skm(1), head])      # pad != 0 on ONE axis is a padded conv
    plan([stem, cv(), skm(1), _L(abi, D, stream=1, n_in=576, n_out=1), _L(abi, D, stream=2, n_in=576, n_out=4)], dueling=1)      # directly in front of the dueling split
    plan([stem, cv(), skm(1), _L(abi, abi.LAYER_LSTM, n_in=576, n_out=8), dn(8, 4)], recurrence=1, trace_length=3)
    with pytest.raises(abi.DQNError, match=r"layer 2: a convolutional skip block holds at least one inner layer \(cin = m = 0 must be >= 1\)"):
        plan([stem, cv(), skm(0), head])
    with pytest.raises(abi.DQNError, match=r"layer 2: the convolutional skip block's 3 inner layers would start before the first layer"):
        plan([stem, cv(), skm(3), head])
    with pytest.raises(abi.DQNError, match=r"layer 1: the convolutional skip block's first inner layer \(layer 0\) reads the observation; a skip block cannot be the first layer"):
        plan([cv(2, 2), skm(1), dn(72, 4)])
    with pytest.raises(abi.DQNError, match=r"layer 2: the convolutional skip block holds a Conv with pad 0 \(layer 1, kernel \(1, 1\)\); its inner layers are Conv layers with pad != 0 only"):
        plan([stem, cv(k=1, pad=0), skm(1), head])
    with pytest.raises(abi.DQNError, match=r"layer 3: the convolutional skip block holds a MaxPool / MeanPool layer \(layer 2\)"):
        plan([stem, cv(), _L(abi, abi.LAYER_MAXPOOL, k=1, s=1), skm(2), head])
    with pytest.raises(abi.DQNError, match=r"layer 3: the convolutional skip block holds a Dense layer \(layer 2\)"):
        plan([stem, cv(), dn(576, 576), skm(2), head])
    with pytest.raises(abi.DQNError, match=r"layer 3: the convolutional skip block holds a recurrent layer \(layer 2\)"):
        plan([stem, cv(), _L(abi, abi.LAYER_GRU, n_in=576, n_out=576), skm(2), head], recurrence=1, trace_length=3)
    with pytest.raises(abi.DQNError, match=r"layer 4: the convolutional skip block's 3 inner layers reach across the join of another skip block \(layer 2\); nested skip blocks are not supported"):
        plan([stem, cv(), skm(1), cv(), skm(3), head])
    with pytest.raises(abi.DQNError, match=r"layer 3: the convolutional skip block's input is the feature vector of layer 1 \(a Dense layer\); a convolutional skip block stands on the \(c, h, w\) map"):
        plan([dn(72, 16), dn(16, 16), cv(), skm(1), dn(16, 4)])      # (a Conv behind a Dense layer reads its n features as an (n, 1, 1) map)
    with pytest.raises(abi.DQNError, match=r"layer 5: the convolutional skip block's input is the feature vector of layer 3 \(the join of a skip block on a feature vector\)"):
        plan([dn(72, 16), dn(16, 16), dn(16, 16), _L(abi, SK, cin=1), cv(), skm(1), dn(16, 4)])
    with pytest.raises(abi.DQNError, match=r"layer 2: the convolutional skip block maps a \(16, 6, 6\) map to a \(8, 6, 6\) map; SkipConnection\(layers, \+\) needs layers: \(c, h, w\) -> \(c, h, w\)"):
        plan([stem, cv(16, 8), skm(1), dn(288, 4)])
    with pytest.raises(abi.DQNError, match=r"layer 2: the convolutional skip block maps a \(16, 6, 6\) map to a \(16, 4, 4\) map"):
        plan([stem, cv(k=5, pad=1), skm(1), dn(256, 4)])
    with pytest.raises(abi.DQNError, match=r"layer 2: a convolutional skip block's join has no activation \(act must be DQN_ACT_IDENTITY, got 1\)"):
        plan([stem, cv(), skm(1, act=1), head])
    with pytest.raises(abi.DQNError, match=r"layer 2: convolutional skip block size n = 12 != the block's features 16 \* 6 \* 6 = 576"):
        plan([stem, cv(), skm(1, 12), head])
    with pytest.raises(abi.DQNError, match=r"layer 2: a convolutional skip block's join uses n_in, n_out and cin .* cout / kh / kw / sh / sw = 0 / 3 / 3 / 0 / 0 must be 0"):
        plan([stem, cv(), skm(1, k=3), head])
    with pytest.raises(abi.DQNError, match=r"layer 2: a skip block cannot be the network's output layer"):
        plan([cv(2, 4), cv(4, 4), skm(1)], obs=(2, 1, 1))
    with pytest.raises(abi.DQNError, match=r"layer 2: a convolutional skip block is supported in the base chain only \(not in a value / advantage stream; stream = 1\)"):
        plan([stem, cv(), skm(1, stream=1), _L(abi, D, stream=1, n_in=576, n_out=1), _L(abi, D, stream=2, n_in=576, n_out=4)], dueling=1)
    # kind 9 keeps its refusals on maps, word for word (test_skip_cpu.py holds the rest) -- also behind a convolutional block's join
    with pytest.raises(abi.DQNError, match=r"layer 2: the skip block holds a Conv / MaxPool / MeanPool layer \(layer 1\).*convolutional residual blocks are not supported"):
        plan([stem, cv(), _L(abi, SK, cin=1), head])
    with pytest.raises(abi.DQNError, match=r"layer 4: the skip block's input is the \(c, h, w\) map of layer 2 \(a Conv / MaxPool / MeanPool layer\); a skip block stands on a feature vector"):
        plan([stem, cv(), skm(1), dn(576, 576), _L(abi, SK, cin=1), head])


def test_julia_shim_lowers_the_block_and_refuses_the_rest():
    src = open(os.path.join(ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    assert re.search(r"is_map_desc\(d\) = d\.kind == 1 \|\| d\.kind == 5 \|\| d\.kind == 6 \|\| d\.kind == 10", src)
    assert re.search(r"if !isempty\(descs\) && is_map_desc\(descs\[end\]\) && !isempty\(real\) && all\(is_map_layer, real\)\s+return lower_skip_map!\(descs, l, stream, inner\)", src)
    assert re.search(r"x isa Conv \|\| throw\(\"DeepQLearningError: a MaxPool / MeanPool layer inside a convolutional SkipConnection is not supported", src)
    assert re.search(r"all\(==\(0\), x\.pad\) && throw\(\"DeepQLearningError: a Conv with pad 0 inside a convolutional SkipConnection is not supported", src)
    assert re.search(r"c_in == c_out \|\| throw\(\"DeepQLearningError: the convolutional SkipConnection maps \$\(c_in\) channels to \$\(c_out\)", src)
    assert re.search(r"push!\(descs, LayerDesc\(10, 0, stream, 0, 0, m, 0, 0, 0, 0, 0\)\)", src)      # the join: kind 10, act 0, n_in = n_out = 0, cin = m
    body = src[src.index("function lower_skip_map!"):src.index("function lower_skip!")]
    assert body.index("push!(descs, lower_layer(x, stream)); m += 1") < body.index("push!(descs, LayerDesc(10,")      # the inner descriptors first, then the join
    assert src.index("l.connection === (+) || throw(") < src.index("return lower_skip_map!(descs, l, stream, inner)")      # the connection is checked for both kinds
    assert re.search(r"push!\(descs, LayerDesc\(9, 0, stream, 0, 0, m, 0, 0, 0, 0, 0\)\)", src)      # kind 9 stays
    for a, b in (("(", ")"), ("[", "]")):
        assert src.count(a) == src.count(b)
    assert len(re.findall(r"\bend\b", src)) >= len(re.findall(r"^\s*(?:function|if|for|begin|struct|mutable struct|module|let|while|try)\b", src, re.M))


# ------------------------------------------------------------------ the fp64 reference
def test_program_and_engine_indices():
    """the reference's program is the lowered descriptor list: same length, joins where the descriptors have kind 10, P / K as build_layers takes them"""
    nn = CR.nn
    for c in CR.ALL:
        net = c.mk(); prog = CR.program(net); layers, _ = nn.lower(net)
        assert [e.kind == "join" for e in prog] == [l.kind == nn._abi.LAYER_SKIPADD_MAP for l in layers], c.name
        for j, e in enumerate(prog):
            if e.kind == "join":
                m = layers[j].cin
                assert e.src == j - 1 and prog[j - m].src == e.P and CR._first_inner(prog, j) == j - m, (c.name, j)
    assert len(CR.CASES) == 11 and len(CR.REC_CASES) == 1


@pytest.mark.parametrize("c", CR.ALL, ids=IDS(CR.ALL))
def test_reference_legs_agree_and_the_seed_keeps_the_margins(c):
    """torch autograd through F.conv2d(padding) and layers(x) + x against the hand-written NumPy step (recurrent: the NumPy join): 1e-10 relative on every quantity, on
    each of the three steps of the fp64 trajectory; the case's fixed seed keeps the margins there -- every relu pre-activation RELU_MARGIN off the kink, every MaxPool
    window off a tie, every argmax column GAP clear --, no gradient block is dead, nothing is skipped or masked, and find_seed reaches the seed inside its cap"""
    D, batch = CR.first_step(c)
    a, b = CR.step(c, D, batch, leg="law"), CR.step(c, D, batch, leg="numpy")
    CR.legs_agree(a, b)
    CR.check_grads(D.net, a["grads"], b["grads"], live=True)
    for k, ((rm, pm, gap), o) in enumerate(CR.trajectory(c)):
        assert rm > CR.RELU_MARGIN and pm > CR.RELU_MARGIN and gap > CR.GAP, (c.name, k, rm, pm, gap)
        assert np.isfinite(o["grads"]).all() and np.isfinite(o["loss"])
    rm, pm, gap = CR.case_margins(c)
    assert rm > 2 * CR.RELU_MARGIN and pm > 2 * CR.RELU_MARGIN and gap > 2 * CR.GAP, (c.name, rm, pm, gap)
    if c.name == "p_maxpool_c16_b32":
        assert np.isfinite(pm)      # the MaxPool margin is a measured one, not the empty case's inf
    assert CR.find_seed(c) == c.seed      # twice the margins on the first step, the margins on the next two, twice the tell distances: the smallest such seed


def test_later_steps_of_the_trajectory_agree_between_the_legs():
    """the legs at the trajectory's THIRD parameters (after two fp64 Adam steps), on the dueling / prioritized / u8 case and the tanh-join case"""
    for name in ("dueling_prio_u8", "k_tanh_c16_b32"):
        c = CR.BY_NAME[name]; D = CR.ff_data(c); p = D.p_on.astype(np.float64); adam = CR.Adam(p.size, lr=CR.LR.LR)
        for k in range(3):
            batch = CR.ff_batch(c, D, D.idx[k])
            a, b = CR.step(c, D, batch, p_on=p, leg="law"), CR.step(c, D, batch, p_on=p, leg="numpy")
            CR.legs_agree(a, b)
            p = adam.step(p, a["grads"])


@pytest.mark.parametrize("c", CR.CASES, ids=IDS(CR.CASES))
def test_the_tests_can_tell(c):
    """each wrong engine moves some compared quantity (Q, y, td, loss, a gradient block) by >= TELL tolerances on every case it applies to"""
    d = CR.tell_distances(c)
    assert "entry_without_dY" in d and "skip_read_from_f" in d
    for w, v in d.items():
        assert v >= CR.TELL, (c.name, w, v)


def test_every_wrong_engine_is_shown_by_some_case():
    seen = {w for c in CR.CASES for w, _ in CR.WRONG if CR.applies(c, w)}
    assert seen == {w for w, _ in CR.WRONG} and CR.TELL == 100.0
    for w, fwd in CR.WRONG:      # the backward-only ones leave every forward quantity alone
        c = next(c for c in CR.CASES if CR.applies(c, w)); D, batch = CR.first_step(c); g = float(np.float32(c.gamma))
        a = CR.np_step(D.net, D.p_on, D.p_tg, batch, g, bool(c.dq)); b = CR.np_step(D.net, D.p_on, D.p_tg, batch, g, bool(c.dq), wrong=w)
        assert np.array_equal(a["q_on_s"], b["q_on_s"]) == (not fwd), w


def test_centre_tap_identity_blocks_double_the_map_in_fp64():
    """Conv(1x1 centre tap, I) -> two blocks of centre-tap identity convs with zero bias -> Dense(I): Q = 4x exactly (the GPU readout network in the reference)"""
    net, flat, n = CR.readout_net(c=4, hw=(3, 3), blocks=2)
    x = np.arange(-7, 3 * n - 7, dtype=np.float64).reshape((3, 4, 3, 3))
    np.testing.assert_array_equal(CR.q_values(net, flat, x), 4 * x.reshape(3, -1))
