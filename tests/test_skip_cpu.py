"""CPU: Flux SkipConnection(layers, +) blocks in the Python mirror, the ABI header, the library's host-side validation (no GPU: dqn_plan_default runs build_layers), BSON
and the Julia shim, and the fp64 reference the GPU tests (test_skip_gpu.py) stand on: its two legs against each other on every case, the margin seeds of the table, and
the proof that the tests can tell -- each wrong engine (the entry gradient without + dY, the entry's derivative before the sum or twice, the last inner layer's derivative
omitted at the join, its pre-activation added instead of its output, the skip read from the first inner layer's output) is off by hundreds of tolerances on every case
it applies to."""
import importlib
import operator
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import layernorm_reference as LR
import skip_reference as SR

ROOT = ge.ROOT
ALL = SR.CASES + SR.REC_CASES
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
    assert int(re.search(r"DQN_LAYER_SKIPADD\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_SKIPADD == 9
    assert int(re.search(r"#define DQN_PLAN_VERSION\s+(\d+)", hdr).group(1)) == 3      # no struct and no exported symbol changed
    assert "SkipConnection" in hdr and "cin = m" in hdr


# ------------------------------------------------------------------ lowering
def _prenorm(nn, n=16):
    return nn.SkipConnection(nn.Chain(nn.LayerNorm(n), nn.Dense(n, 4 * n, nn.relu), nn.Dense(4 * n, n)), "+")


def test_lowering_puts_one_join_directly_behind_the_inner_descriptors(mods):
    nn, abi, _ = mods
    net = nn.Chain(nn.Dense(6, 16, nn.relu), _prenorm(nn), nn.SkipConnection(nn.Dense(16, 16, nn.tanh), operator.add), nn.Dense(16, 4))
    layers, dueling = nn.lower(net)
    D, LN, SK = abi.LAYER_DENSE, abi.LAYER_LAYERNORM, abi.LAYER_SKIPADD
    assert not dueling and [l.kind for l in layers] == [D, LN, D, D, SK, D, SK, D]
    for j, m in ((4, 3), (6, 1)):
        l = layers[j]
        assert (l.cin, l.n_in, l.n_out, l.act, l.stream, l.cout, l.kh, l.kw, l.sh, l.sw) == (m, 0, 0, abi.ACT_IDENTITY, abi.STREAM_BASE, 0, 0, 0, 0, 0)
    assert [(l.n_in, l.n_out) for l in layers if l.kind == D] == [(6, 16), (16, 64), (64, 16), (16, 16), (16, 4)]
    assert repr(net.layers[2]).startswith("SkipConnection(Chain(Dense") or "SkipConnection" in repr(net.layers[2])


def test_parameters_are_the_inner_layers_in_flux_params_order(mods, tmp_path):
    nn, abi, bson = mods
    net = nn.Chain(nn.Dense(6, 8, nn.relu), nn.SkipConnection(nn.Chain(nn.LayerNorm(8), nn.Dense(8, 12, nn.relu), nn.Dropout(0.5), nn.Dense(12, 8)), "+"), nn.Dense(8, 4))
    flat = nn.Chain(nn.Dense(6, 8, nn.relu), nn.LayerNorm(8), nn.Dense(8, 12, nn.relu), nn.Dropout(0.5), nn.Dense(12, 8), nn.Dense(8, 4))
    assert net.layers[1].shapes() == []      # the join holds nothing
    assert [l.kind for l in nn.all_layers(net)] == ["dense", "layernorm", "dense", "dropout", "dense", "dense"]
    p = nn.glorot_params(net, seed=3)
    np.testing.assert_array_equal(p, nn.glorot_params(flat, seed=3))
    assert p.size == 6 * 8 + 8 + 16 + 8 * 12 + 12 + 12 * 8 + 8 + 8 * 4 + 4
    shapes = bson.julia_param_shapes(net)
    assert shapes == bson.julia_param_shapes(flat) == [((8, 6), 48), ((8,), 8), ((8,), 8), ((8,), 8), ((12, 8), 96), ((12,), 12), ((8, 12), 96), ((8,), 8), ((4, 8), 32), ((4,), 4)]
    path = str(tmp_path / "qnetwork.bson")
    bson.save_qnetwork(path, p, shapes)
    got, sizes = bson.load_qnetwork(path)
    np.testing.assert_array_equal(got, p)
    assert [tuple(s) for s in sizes] == [s for s, _ in shapes]
    assert not nn.isrecurrent(net)
    assert nn.isrecurrent(nn.Chain(nn.LSTM(6, 8), nn.SkipConnection(nn.Dense(8, 8), "+"), nn.Dense(8, 4)))


def test_create_dueling_network_treats_the_block_as_a_non_dense_layer(mods):
    nn, abi, _ = mods
    d = nn.create_dueling_network(nn.Chain(nn.Dense(6, 16, nn.relu), _prenorm(nn), nn.Dense(16, 4)))      # the trailing Dense run stops at the block: the split sits on the join
    assert [l.kind for l in d.base] == ["dense", "skip"] and d.val.layers[0].n_out == 1 and len(d.adv.layers) == 1
    layers, dueling = nn.lower(d)
    assert dueling and [(l.kind, l.stream) for l in layers] == [(0, 0), (7, 0), (0, 0), (0, 0), (9, 0), (0, 1), (0, 2)]
    d2 = nn.create_dueling_network(nn.Chain(nn.Dense(6, 16, nn.relu), _prenorm(nn), nn.Dense(16, 16, nn.relu), nn.Dense(16, 4)))
    assert [l.kind for l in d2.base] == ["dense", "skip"] and len(d2.val.layers) == len(d2.adv.layers) == 2
    with pytest.raises(abi.DQNError, match="the qnetwork provided is incompatible with dueling"):      # a chain that ends in a block, as in the reference
        nn.create_dueling_network(nn.Chain(nn.Dense(6, 4), nn.SkipConnection(nn.Dense(4, 4), "+")))


def test_the_mirror_refuses_by_name(mods):
    nn, abi, _ = mods
    inner = lambda: nn.Chain(nn.Dense(16, 16))
    for conn, shown in (("vcat", "vcat"), ("*", r"\*"), (operator.mul, "mul"), (lambda a, b: a + b, "<lambda>")):
        with pytest.raises(abi.DQNError, match=r"SkipConnection\(layers, %s\) is not supported; .* connection \+ only \(vcat, \*, closures and Parallel are not supported\)" % shown):
            nn.SkipConnection(inner(), conn)
    with pytest.raises(abi.DQNError, match=r"Parallel is not supported; .*SkipConnection\(layers, \+\) only"):
        nn.lower(nn.Chain(nn.Dense(6, 16), nn.Parallel("+", nn.Dense(16, 16), nn.Dense(16, 16)), nn.Dense(16, 4)))
    with pytest.raises(abi.DQNError, match=r"holds no layer"):
        nn.SkipConnection(nn.Chain(), "+")
    head = nn.Dense(16, 4)
    low = lambda *ls: nn.lower(nn.Chain(*ls))
    with pytest.raises(abi.DQNError, match=r"cannot be the first layer: a skip block's input is never the observation"):
        low(nn.SkipConnection(nn.Dense(16, 16), "+"), head)
    with pytest.raises(abi.DQNError, match=r"cannot follow a Conv / MaxPool / MeanPool layer: a skip block stands on a feature vector \(convolutional residual blocks are not supported\)"):
        low(nn.Conv(3, 1, 4, nn.relu), nn.flattenbatch, nn.SkipConnection(nn.Dense(64, 64), "+"), nn.Dense(64, 4))
    with pytest.raises(abi.DQNError, match=r"cannot be the network's output layer"):
        low(nn.Dense(6, 4), nn.SkipConnection(nn.Dense(4, 4), "+"))
    with pytest.raises(abi.DQNError, match=r"a SkipConnection inside a SkipConnection is not supported \(nested skip blocks\)"):
        low(nn.Dense(6, 16), nn.SkipConnection(nn.Chain(nn.Dense(16, 16), nn.SkipConnection(nn.Dense(16, 16), "+")), "+"), head)
    with pytest.raises(abi.DQNError, match=r"a recurrent layer inside a SkipConnection is not supported"):
        low(nn.Dense(6, 16), nn.SkipConnection(nn.GRU(16, 16), "+"), head)
    with pytest.raises(abi.DQNError, match=r"a Conv / MaxPool / MeanPool layer inside a SkipConnection is not supported"):
        low(nn.Dense(6, 16), nn.SkipConnection(nn.Chain(nn.Conv(3, 1, 1)), "+"), head)
    with pytest.raises(abi.DQNError, match=r"maps 16 features to 12; SkipConnection\(layers, \+\) needs layers: n -> n"):
        low(nn.Dense(6, 16), nn.SkipConnection(nn.Chain(nn.Dense(16, 32, nn.relu), nn.Dense(32, 12)), "+"), nn.Dense(12, 4))
    with pytest.raises(abi.DQNError, match=r"is supported in the base chain only"):
        nn.lower(nn.DuelingNetwork(nn.Chain(nn.Dense(6, 16)), nn.Chain(nn.SkipConnection(nn.Dense(16, 16), "+"), nn.Dense(16, 1)), nn.Chain(nn.Dense(16, 4))))
    with pytest.raises(abi.DQNError, match=r"unsupported layer .*SkipConnection\(\+\) / Conv / MaxPool"):
        nn.lower(nn.Chain(object()))
    # the relaxed rules, and a block in a dueling base chain's last place, lower
    low(nn.Dense(6, 16), nn.SkipConnection(nn.Chain(nn.Dropout(0.5), nn.Dense(16, 16)), "+"), nn.LayerNorm(16), nn.SkipConnection(nn.Dense(16, 16), "+"), nn.Dropout(0.1), head)


def _L(abi, kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, k=0, s=0):
    d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, k, k, s, s
    return d


def test_host_side_validation_accepts_and_refuses_without_a_gpu(pkg, mods):
    """dqn_plan_default runs build_layers on the host: the supported placements get a plan (the join's entry all zero), every refusal names the layer index"""
    nn, abi, _ = mods
    D, LN, DO, SK = abi.LAYER_DENSE, abi.LAYER_LAYERNORM, abi.LAYER_DROPOUT, abi.LAYER_SKIPADD
    plan = lambda layers, obs=(6, 1, 1), **kw: pkg.default_plan(layers, pkg.default_hparams(batch_size=8, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], buffer_size=64, **({"dueling": 0} | kw)))
    dn = lambda a, b, **kw: _L(abi, D, n_in=a, n_out=b, **kw)
    sk = lambda m, n=0, **kw: _L(abi, SK, cin=m, n_in=n, n_out=n, **kw)
    ln = lambda n=16, **kw: _L(abi, LN, n_in=n, n_out=n, **kw)
    do = lambda **kw: _L(abi, DO, cout=0x3FE00000, **kw)      # p = 0.5
    first, head = dn(6, 16, act=1), dn(16, 4)
    assert tuple(plan([first, dn(16, 16), sk(1), head])[2]) == (0, 0, 0)
    assert tuple(plan([first, ln(), dn(16, 64, act=1), dn(64, 16), sk(3, 16), head])[4]) == (0, 0, 0)      # the pre-norm block; n given
    assert tuple(plan(nn.lower(nn.Chain(nn.Dense(6, 2048, nn.relu), nn.SkipConnection(nn.Dense(2048, 2048), "+"), nn.Dense(2048, 4)))[0])[2]) == (0, 0, 0)
    plan([first, do(), dn(16, 16), sk(2), head])                                  # Dropout first in the block: it reads the block's input
    plan([first, dn(16, 16), do(), sk(2), head])                                  # ... and last
    plan([first, dn(16, 16), sk(1), ln(), head]); plan([first, dn(16, 16), sk(1), do(), head])      # LayerNorm / Dropout directly behind a block
    plan([first, dn(16, 16), sk(1), dn(16, 16, act=2), sk(1), head])              # block behind block
    plan([first, ln(act=2), dn(16, 16), sk(1), head]); plan([first, do(), dn(16, 16), do(), sk(2), head])      # P a LayerNorm; P a Dropout (the first Dropout stands in FRONT of the block: m = 2)
    plan([first, dn(16, 16), sk(1), _L(abi, D, stream=1, n_in=16, n_out=1), _L(abi, D, stream=2, n_in=16, n_out=4)], dueling=1)      # directly in front of the dueling split
    plan([_L(abi, abi.LAYER_LSTM, n_in=6, n_out=8), dn(8, 8), sk(1), dn(8, 4)], recurrence=1, trace_length=3)
    plan([dn(6, 8, act=1), dn(8, 8), sk(1), _L(abi, abi.LAYER_GRU, n_in=8, n_out=8), dn(8, 4)], recurrence=1, trace_length=3)
    with pytest.raises(abi.DQNError, match=r"layer 2: a skip block holds at least one inner layer \(cin = m = 0 must be >= 1\)"):
        plan([first, dn(16, 16), sk(0), head])
    with pytest.raises(abi.DQNError, match=r"layer 2: the skip block's 3 inner layers would start before the first layer"):
        plan([first, dn(16, 16), sk(3), head])
    with pytest.raises(abi.DQNError, match=r"layer 0: .*before the first layer"):
        plan([sk(1), dn(6, 4)])
    with pytest.raises(abi.DQNError, match=r"layer 1: the skip block's first inner layer \(layer 0\) reads the observation; a skip block cannot be the first layer"):
        plan([dn(6, 6), sk(1), dn(6, 4)])
    with pytest.raises(abi.DQNError, match=r"layer 4: the skip block's 3 inner layers reach across the join of another skip block \(layer 2\); nested skip blocks are not supported"):
        plan([first, dn(16, 16), sk(1), dn(16, 16), sk(3), head])
    with pytest.raises(abi.DQNError, match=r"layer 2: the skip block holds a recurrent layer \(layer 1\)"):
        plan([dn(6, 8), _L(abi, abi.LAYER_GRU, n_in=8, n_out=8), sk(1), dn(8, 4)], recurrence=1, trace_length=3)
    with pytest.raises(abi.DQNError, match=r"layer 2: the skip block holds a Conv / MaxPool / MeanPool layer \(layer 1\).*convolutional residual blocks are not supported"):
        plan([_L(abi, abi.LAYER_CONV, cin=1, cout=2, k=3, s=1), _L(abi, abi.LAYER_CONV, cin=2, cout=2, k=1, s=1), sk(1), dn(32, 4)], obs=(1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"layer 2: the skip block's input is the \(c, h, w\) map of layer 0 \(a Conv / MaxPool / MeanPool layer\); a skip block stands on a feature vector"):
        plan([_L(abi, abi.LAYER_CONV, cin=1, cout=2, k=3, s=1), dn(32, 32), sk(1), dn(32, 4)], obs=(1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"layer 3: the skip block maps 16 features to 12; SkipConnection\(layers, \+\) needs layers: n -> n"):
        plan([first, dn(16, 32, act=1), dn(32, 12), sk(2), dn(12, 4)])
    with pytest.raises(abi.DQNError, match=r"layer 2: a skip block's join has no activation \(act must be DQN_ACT_IDENTITY, got 1\)"):
        plan([first, dn(16, 16), sk(1, act=1), head])
    for stream in (1, 2):
        with pytest.raises(abi.DQNError, match=r"layer 2: a skip block is supported in the base chain only \(not in a value / advantage stream; stream = %d\)" % stream):
            plan([first, _L(abi, D, stream=stream, n_in=16, n_out=16), sk(1, stream=stream), _L(abi, D, stream=stream, n_in=16, n_out=1 if stream == 1 else 4), _L(abi, D, stream=3 - stream, n_in=16, n_out=4 if stream == 1 else 1)], dueling=1)
    with pytest.raises(abi.DQNError, match=r"layer 2: a skip block cannot be the network's output layer"):
        plan([dn(6, 4), dn(4, 4), sk(1)])
    with pytest.raises(abi.DQNError, match=r"layer 2: skip block size n = 12 != the block's features 16"):
        plan([first, dn(16, 16), sk(1, 12), head])
    with pytest.raises(abi.DQNError, match=r"layer 2: a skip block's join uses n_in, n_out and cin .* cout / kh / kw / sh / sw = 0 / 3 / 3 / 0 / 0 must be 0"):
        plan([first, dn(16, 16), sk(1, k=3), head])
    # the LayerNorm and Dropout refusals keep their words for the cases they covered before
    with pytest.raises(abi.DQNError, match=r"layer 1: LayerNorm must directly follow a Dense or recurrent layer \(layer 0 is a LayerNorm layer\)|layer 2: LayerNorm must directly follow"):
        plan([first, ln(), ln(), dn(16, 16), sk(2), head])
    with pytest.raises(abi.DQNError, match=r"layer 0: Dropout cannot be the first layer"):
        plan([do(), dn(6, 4)])


def test_julia_shim_lowers_the_block_and_refuses_the_rest():
    src = open(os.path.join(ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    assert re.search(r"l isa Flux\.SkipConnection \? lower_skip!\(descs, l, stream\)", src)
    assert re.search(r"l\.connection === \(\+\) \|\| throw\(\"DeepQLearningError: SkipConnection\(layers, \$\(l\.connection\)\) is not supported; [^\"]*connection \+ only \(vcat, \*, closures and Parallel are not supported\)", src)
    assert re.search(r"x isa Flux\.SkipConnection && throw\(\"DeepQLearningError: a SkipConnection inside a SkipConnection is not supported", src)
    assert re.search(r"\(x isa Dense \|\| x isa Flux\.LayerNorm \|\| x isa Flux\.Dropout\) \|\| throw\(", src)
    assert re.search(r"push!\(descs, lower_layer\(x, stream\)\); m \+= 1", src)      # the inner descriptors first ...
    assert re.search(r"push!\(descs, LayerDesc\(9, 0, stream, 0, 0, m, 0, 0, 0, 0, 0\)\)", src)      # ... then the join: kind 9, act 0, n_in = n_out = 0, cin = m
    assert src.index("push!(descs, lower_layer(x, stream)); m += 1") < src.index("push!(descs, LayerDesc(9, 0, stream, 0, 0, m, 0, 0, 0, 0, 0))")
    assert re.search(r"l isa Flux\.Parallel && throw\(\"DeepQLearningError: Parallel is not supported", src)
    assert "lower_into!(descs, l, Int32(s))" in src and "lower_into!(descs, l, Int32(0))" in src
    assert "flatparams(q) = reduce(vcat, [vec(Float32.(w)) for w in Flux.params(q)])" in src      # Flux.params walks into the block: the inner layers' arrays in order
    for a, b in (("(", ")"), ("[", "]")):
        assert src.count(a) == src.count(b)
    assert len(re.findall(r"\bend\b", src)) >= len(re.findall(r"^\s*(?:function|if|for|begin|struct|mutable struct|module|let|while|try)\b", src, re.M))


# ------------------------------------------------------------------ the fp64 reference
def test_program_and_engine_indices():
    """the reference's program is the lowered descriptor list: same length, joins where the descriptors have kind 9, P / K as build_layers takes them"""
    nn = SR.nn
    for c in ALL:
        net = c.mk(); prog = SR.program(net); layers, _ = nn.lower(net)
        assert [e.kind == "join" for e in prog] == [l.kind == nn._abi.LAYER_SKIPADD for l in layers], c.name
        for j, e in enumerate(prog):
            if e.kind == "join":
                m = layers[j].cin
                assert e.src == j - 1 and prog[j - m].src == e.P and SR._first_inner(prog, j) == j - m, (c.name, j)
    net = SR.BY_NAME["two_blocks_n33_b32"].mk()
    assert SR.engine_index(net) == {0: 0, 1: 1, 2: 2, 3: 4, 4: 5, 5: 6, 6: 8}
    c = SR.BY_NAME["p_dropout_n64_b32"]; m = SR.masks_for(c.mk(), 0, c.B)
    assert list(m) == [1] and m[1].shape == (32, 64)
    c = SR.BY_NAME["do_last_n8_b5"]; m = SR.masks_for(c.mk(), 0, c.B)
    np.testing.assert_array_equal(m[3], SR.DR.keep_mask(SR.ENGINE_SEED, 0, 3, 8, 5, 0.5))


@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_reference_legs_agree_and_the_seed_keeps_the_margins(c):
    """torch autograd through layers(x) + x and the hand-written NumPy step (recurrent: the NumPy join): 1e-10 relative on every quantity; the case's fixed seed keeps
    the margins of the LayerNorm table on the masked s pass and the unmasked s' passes, no gradient block is dead, and find_seed reaches it inside its cap"""
    D, batch, masks = SR.first_step(c)
    a, b = SR.step(c, D, batch, masks, leg="law"), SR.step(c, D, batch, masks, leg="numpy")
    SR.legs_agree(a, b)
    sg, rm, gap = SR.case_margins(c)
    assert sg >= LR.SIGMA_MIN and rm > LR.RELU_MARGIN and gap > LR.GAP, (c.name, sg, rm, gap)
    SR.check_grads(D.net, a["grads"], b["grads"], live=True)
    assert SR.margins_ok(c) and SR.tells_ok(c) and SR.find_seed(c) == c.seed      # twice the margins, twice the tell distances, the smallest such seed


@pytest.mark.parametrize("c", SR.CASES, ids=IDS(SR.CASES))
def test_the_tests_can_tell(c):
    """each wrong engine moves some compared quantity (Q, y, td, loss, a gradient block) by >= TELL tolerances on every case it applies to"""
    d = SR.tell_distances(c)
    assert "entry_without_dY" in d
    for w, v in d.items():
        assert v >= SR.TELL, (c.name, w, v)


def test_every_wrong_engine_is_shown_by_some_case():
    seen = {w for c in SR.CASES for w, _ in SR.WRONG if SR.applies(c, w)}
    assert seen == {w for w, _ in SR.WRONG}
    for w, fwd in SR.WRONG:      # the backward-only ones leave every forward quantity alone
        c = next(c for c in SR.CASES if SR.applies(c, w)); D, batch, masks = SR.first_step(c); g = float(np.float32(c.gamma))
        a = SR.np_step(D.net, D.p_on, D.p_tg, batch, g, bool(c.dq), masks); b = SR.np_step(D.net, D.p_on, D.p_tg, batch, g, bool(c.dq), masks, wrong=w)
        assert np.array_equal(a["q_on_s"], b["q_on_s"]) == (not fwd), w


def test_a_block_around_zero_weights_is_the_identity_and_the_exact_readout_holds_in_fp64():
    """Dense(W = I) -> block around Dense(W = 2I) -> Dense(W = I): Q = 3x exactly (the GPU readout network in the reference)"""
    nn = SR.nn; n = 5
    net = nn.Chain(nn.Dense(n, n), nn.SkipConnection(nn.Dense(n, n), "+"), nn.Dense(n, n))
    I = np.eye(n).ravel(); z = np.zeros(n)
    x = np.arange(-7, 3 * n - 7, dtype=np.float64).reshape(3, n)
    np.testing.assert_array_equal(SR.q_values(net, np.concatenate([I, z, 2 * I, z, I, z]), x), 3 * x)
    np.testing.assert_array_equal(SR.q_values(net, np.concatenate([I, z, 0 * I, z, I, z]), x), x)
