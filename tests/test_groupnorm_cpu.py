"""CPU: Flux GroupNorm layers in the Python mirror, the ABI header, the library's host-side validation (no GPU: dqn_plan_default), BSON and the Julia shim, and the fp64
reference the GPU tests (test_groupnorm_gpu.py) stand on: its two legs against each other on every case, the hand-written gradient against central differences, the cases
that tell sqrt(var + eps) from sigma + eps and the beta, gamma parameter order from gamma, beta, the dead group, and the margin seeds of the table."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import groupnorm_reference as GR

ROOT = ge.ROOT
ALL = GR.CASES + GR.REC_CASES
IDS = lambda cs: [c.name for c in cs]
nn = GR.nn


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "_abi", "bson"))


def _bits(eps):
    return int(np.float32(eps).view(np.int32))


def test_enum_value_matches_the_header(mods):
    _, abi, _ = mods
    hdr = open(os.path.join(ROOT, "include", "dqn_mi355x.h")).read()
    assert int(re.search(r"DQN_LAYER_GROUPNORM\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_GROUPNORM == 11
    assert int(re.search(r"#define DQN_PLAN_VERSION\s+(\d+)", hdr).group(1)) == 3      # no struct changed


def test_lowering_and_descriptor_slots(mods):
    _, abi, _ = mods
    net = nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.GroupNorm(4, 2), nn.Conv(3, 4, 8, nn.relu, pad=1), nn.GroupNorm(8, 8, nn.tanh, eps=0.5), nn.MaxPool(2), nn.flattenbatch, nn.Dense(32, 4))
    layers, dueling = nn.lower(net)
    assert not dueling and [l.kind for l in layers] == [abi.LAYER_CONV, abi.LAYER_GROUPNORM, abi.LAYER_CONV, abi.LAYER_GROUPNORM, abi.LAYER_MAXPOOL, abi.LAYER_DENSE]
    a, b = layers[1], layers[3]
    assert (a.act, a.stream, a.cin, a.cout, a.kh, a.kw) == (abi.ACT_IDENTITY, abi.STREAM_BASE, 4, 4, 2, _bits(1e-5)) and a.kw == 0x3727C5AC
    assert (b.act, b.stream, b.cin, b.cout, b.kh, b.kw) == (abi.ACT_TANH, abi.STREAM_BASE, 8, 8, 8, 0x3F000000)
    for l in (a, b):
        assert (l.n_in, l.n_out, l.sh, l.sw) == (0, 0, 0, 0)      # the engine fills in c * h * w; the stride slots are unused
    assert (layers[4].cin, layers[4].cout) == (8, 8)      # a pool behind the layer reads the channel count of the map in front of it


def test_shapes_initialisation_parameter_order_and_bson_round_trip(mods, tmp_path):
    _, abi, bson = mods
    net = nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.GroupNorm(4, 2), nn.flattenbatch, nn.Dense(64, 3))
    assert net.layers[1].shapes() == [(4,), (4,)]
    p = nn.glorot_params(net, seed=3)
    assert p.size == 36 + 4 + 4 + 4 + 64 * 3 + 3
    np.testing.assert_array_equal(p[40:44], np.zeros(4, np.float32)); np.testing.assert_array_equal(p[44:48], np.ones(4, np.float32))      # Flux.params: beta = zeros FIRST, then gamma = ones
    shapes = bson.julia_param_shapes(net)
    assert shapes == [((3, 3, 1, 4), 36), ((4,), 4), ((4,), 4), ((4,), 4), ((3, 64), 192), ((3,), 3)]      # W, b, beta, gamma, W, b
    assert [nm for nm, _ in GR.blocks(net)] == ["conv0.W", "conv0.b", "gn1.beta", "gn1.gamma", "dense2.W", "dense2.b"]
    p = (p + np.arange(p.size, dtype=np.float32)).astype(np.float32)
    path = str(tmp_path / "qnetwork.bson")
    bson.save_qnetwork(path, p, shapes)
    flat, sizes = bson.load_qnetwork(path)
    np.testing.assert_array_equal(flat, p)
    assert [tuple(s) for s in sizes] == [s for s, _ in shapes]


def test_dueling_split_leaves_the_layer_in_the_base_chain(mods):
    d = nn.create_dueling_network(nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.GroupNorm(4, 2, nn.relu), nn.flattenbatch, nn.Dense(64, 8, nn.relu), nn.Dense(8, 4)))
    assert [l.kind for l in d.base] == ["conv", "groupnorm"] and [l.kind for l in d.val] == ["dense", "dense"]
    layers, dueling = nn.lower(d)
    assert dueling and [(l.kind, l.stream) for l in layers] == [(1, 0), (11, 0), (0, 1), (0, 1), (0, 2), (0, 2)]


def test_the_mirror_refuses_by_name(mods):
    _, abi, _ = mods
    with pytest.raises(abi.DQNError, match=r"GroupNorm\(8, 2; affine=false\) is not supported; the MI355X engine runs the layer with its γ and β \(affine=true\)"):
        nn.GroupNorm(8, 2, affine=False)
    with pytest.raises(abi.DQNError, match=r"GroupNorm\(8, 2; track_stats=true\) is not supported; the MI355X engine keeps no running statistics"):
        nn.GroupNorm(8, 2, track_stats=True)
    for chs, G in ((8, 3), (8, 0), (4, 8)):
        with pytest.raises(abi.DQNError, match=r"GroupNorm\(%d, %d\): the number of groups G must be >= 1 and divide the channel count" % (chs, G)):
            nn.GroupNorm(chs, G)
    for bad in (0.0, -1e-5, float("inf"), float("nan"), 1e39):
        with pytest.raises(abi.DQNError, match=r"GroupNorm\(8, 2; eps=.*\): eps must be finite and > 0 in Float32"):
            nn.GroupNorm(8, 2, eps=bad)
    with pytest.raises(abi.DQNError, match=r"BatchNorm is not supported: it keeps running statistics"):
        nn.BatchNorm(8)
    with pytest.raises(abi.DQNError, match=r"InstanceNorm is not supported: its default is affine = false"):
        nn.InstanceNorm(8)
    with pytest.raises(abi.DQNError, match=r"GroupNorm\(1, 1, act=0, eps=1e-05\) cannot be the first layer: normalising the observation is not supported"):
        nn.lower(nn.Chain(nn.GroupNorm(1, 1), nn.Conv(3, 1, 4), nn.Dense(64, 4)))
    with pytest.raises(abi.DQNError, match=r"GroupNorm\(4, 2, act=0, eps=1e-05\) cannot be the network's output layer"):
        nn.lower(nn.Chain(nn.Conv(3, 1, 4), nn.GroupNorm(4, 2)))
    with pytest.raises(abi.DQNError, match=r"a GroupNorm layer inside a SkipConnection is not supported"):
        nn.lower(nn.Chain(nn.Conv(3, 1, 4), nn.SkipConnection(nn.Chain(nn.Conv(3, 4, 4, pad=1), nn.GroupNorm(4, 2)), "+"), nn.Dense(64, 4)))
    with pytest.raises(abi.DQNError, match=r"a GroupNorm layer inside a SkipConnection is not supported"):
        nn.lower(nn.Chain(nn.Dense(6, 8), nn.SkipConnection(nn.Chain(nn.GroupNorm(8, 2)), "+"), nn.Dense(8, 4)))


def test_the_unsupported_layer_vocabulary_keeps_every_existing_regex(mods):
    """the string gains GroupNorm behind MeanPool; the regexes of test_pool_cpu, test_dropout_cpu, test_layernorm_cpu, test_skip_cpu and test_rnn_cpu still match"""
    _, abi, _ = mods
    with pytest.raises(abi.DQNError) as ei:
        nn.lower(nn.Chain(object()))
    msg = str(ei.value)
    assert "(SkipConnection(+) / Conv / MaxPool / MeanPool / GroupNorm / Dense / Dropout / LSTM / GRU / RNN / LayerNorm / flattenbatch only)" in msg
    for rx in (r"unsupported layer .*MaxPool.*RNN", r"unsupported layer .*Dense / Dropout / LSTM.*RNN / LayerNorm / flattenbatch only", r"unsupported layer .*MaxPool.*RNN / LayerNorm",
               r"unsupported layer .*SkipConnection\(\+\) / Conv / MaxPool", r"unsupported layer .*RNN", "unsupported layer"):
        assert re.search(rx, msg), rx


def _L(abi, kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, kh=0, kw=0, s=0):
    d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, kh, kw, s, s
    return d


def test_host_side_validation_accepts_and_refuses_without_a_gpu(pkg, mods):
    """dqn_plan_default runs build_layers on the host: the supported placements get a plan (the layer's entry all zero), every refusal names the layer index and the value"""
    _, abi, _ = mods
    D, CV, GN, LN, DO = abi.LAYER_DENSE, abi.LAYER_CONV, abi.LAYER_GROUPNORM, abi.LAYER_LAYERNORM, abi.LAYER_DROPOUT
    plan = lambda layers, obs=(1, 6, 6), **kw: pkg.default_plan(layers, pkg.default_hparams(batch_size=8, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], buffer_size=64, **({"dueling": 0} | kw)))
    conv = lambda co=4, **kw: _L(abi, CV, act=1, cin=1, cout=co, kh=3, kw=3, s=1, **kw)      # (1, 6, 6) -> (co, 4, 4)
    gn = lambda G=2, c=4, **kw: _L(abi, GN, **({"cin": c, "cout": c, "kh": G} | kw))
    head = lambda n=64: _L(abi, D, n_in=n, n_out=4)
    assert tuple(plan([conv(), gn(), head()])[1]) == (0, 0, 0)
    assert tuple(plan([conv(), gn(cin=0, cout=0, n_in=64, n_out=64), head()])[1]) == (0, 0, 0)      # chs 0: taken from the map; n_in == n_out == c * h * w accepted
    plan([conv(), gn(kw=_bits(0.5), act=10), _L(abi, D, stream=1, n_in=64, n_out=1), _L(abi, D, stream=2, n_in=64, n_out=4)], dueling=1)      # the join sits on the layer
    plan([conv(), gn(), gn(G=1), head()])                                                          # behind another GroupNorm
    plan([conv(), _L(abi, abi.LAYER_MAXPOOL, kh=2, kw=2, s=2), gn(), head(16)])                   # behind a pool
    blk = [_L(abi, CV, act=1, cin=4, cout=4, kh=3, kw=3, s=1, n_in=1, n_out=1), _L(abi, CV, cin=4, cout=4, kh=3, kw=3, s=1, n_in=1, n_out=1), _L(abi, abi.LAYER_SKIPADD_MAP, cin=2)]
    plan([conv(), gn()] + blk + [gn(), head()])                                                    # in front of and behind a convolutional skip block
    plan([conv(), gn(), _L(abi, abi.LAYER_LSTM, n_in=64, n_out=8), _L(abi, D, n_in=8, n_out=4)], recurrence=1, trace_length=3)
    wide = plan([_L(abi, CV, act=1, cin=1, cout=512, kh=3, kw=3, s=1), gn(G=4, c=512), head(8192)])      # no chunk rule of a GEMM layer applies, at any width
    assert tuple(wide[1]) == (0, 0, 0)
    R = pytest.raises
    with R(abi.DQNError, match=r"layer 0: GroupNorm cannot be the first layer \(normalising the observation is not supported; it must directly follow a Conv, MaxPool / MeanPool or GroupNorm layer or a convolutional skip block\)"):
        plan([gn(G=1, c=1), head(36)])
    for stream in (1, 2):
        with R(abi.DQNError, match=r"layer 2: GroupNorm layers are supported in the base chain only \(not in a value / advantage stream; stream = %d\)" % stream):
            plan([conv(), _L(abi, D, stream=stream, n_in=64, n_out=16), gn(stream=stream), _L(abi, D, stream=3 - stream, n_in=64, n_out=4)], dueling=1)
    with R(abi.DQNError, match=r"layer 2: GroupNorm must directly follow a Conv, MaxPool / MeanPool or GroupNorm layer or a convolutional skip block \(layer 1 is a Dense layer, whose output is no \(c, h, w\) map\)"):
        plan([conv(), _L(abi, D, n_in=64, n_out=16), gn(c=16), head(16)])
    with R(abi.DQNError, match=r"layer 2: GroupNorm must directly follow .* \(layer 1 is a LayerNorm layer, whose output is no \(c, h, w\) map\)"):
        plan([_L(abi, D, n_in=36, n_out=16), _L(abi, LN, n_in=16, n_out=16), gn(c=16), head(16)])
    with R(abi.DQNError, match=r"layer 1: GroupNorm must directly follow .* \(layer 0 is a recurrent layer, whose output is no \(c, h, w\) map\)"):
        plan([_L(abi, abi.LAYER_LSTM, n_in=36, n_out=8), gn(c=8), head(8)], recurrence=1, trace_length=3)
    with R(abi.DQNError, match=r"layer 1: GroupNorm activation 11 is not one of DQN_ACT_\* \(0\.\.10\)"):
        plan([conv(), gn(act=11), head()])
    with R(abi.DQNError, match=r"layer 1: GroupNorm chs \(cin 8 / cout 8\) != incoming channels 4"):
        plan([conv(), gn(c=8), head()])
    with R(abi.DQNError, match=r"layer 1: GroupNorm n_in 64 != n_out 0 \(both carry the feature count c \* h \* w, or both 0\)"):
        plan([conv(), gn(n_in=64), head()])
    with R(abi.DQNError, match=r"layer 1: GroupNorm size n = 60 != incoming features 4 \* 4 \* 4 = 64"):
        plan([conv(), gn(n_in=60, n_out=60), head()])
    with R(abi.DQNError, match=r"layer 1: GroupNorm uses cin, cout, kh \(the group count G\), kw \(the bit pattern of eps\), n_in, n_out and act only; sh / sw = 1 / 1 must be 0"):
        plan([conv(), gn(s=1), head()])
    for G in (0, 3, -1):
        with R(abi.DQNError, match=r"layer 1: GroupNorm G = %d must be >= 1 and divide the channel count 4" % G):
            plan([conv(), gn(G=G), head()])
    with R(abi.DQNError, match=r"layer 1: GroupNorm\(4, 4\) on a \(4, 1, 1\) map normalises over n_g = 1 element \(n_g must be >= 2: over one element the variance is identically 0 and the output is constant\)"):
        plan([conv(), gn(G=4), head(4)], obs=(1, 3, 3))
    for bad, shown in ((0.0, None), (-1.0, "-1"), (float("inf"), "inf"), (float("nan"), "nan")):
        bits = _bits(bad) if bad != 0.0 else _bits(-0.0)      # +0 bits mean "the default": -0 is the zero that can be asked for
        with R(abi.DQNError, match=r"layer 1: GroupNorm eps = .* \(bit pattern 0x[0-9a-f]{8}\) must be finite and > 0") as ei:
            plan([conv(), gn(kw=bits), head()])
        assert shown is None or shown in str(ei.value)
    with R(abi.DQNError, match=r"layer 1: a GroupNorm layer cannot be the network's output layer"):
        plan([_L(abi, CV, cin=1, cout=4, kh=6, kw=6, s=1), gn()])      # (4, 1, 1) = n_actions
    # inside either skip-block kind
    with R(abi.DQNError, match=r"layer 3: the convolutional skip block holds a GroupNorm layer \(layer 2\); its inner layers are Conv layers with pad != 0 only"):
        plan([conv(), blk[0], gn(), _L(abi, abi.LAYER_SKIPADD_MAP, cin=2), head()])
    with R(abi.DQNError, match=r"layer 3: the skip block holds a GroupNorm layer \(layer 2\); its inner layers are Dense, LayerNorm and Dropout layers only \(GroupNorm inside a skip block is not supported\)"):
        plan([conv(), gn(), gn(G=1), _L(abi, abi.LAYER_SKIPADD, cin=1), head()])
    with R(abi.DQNError, match=r"layer 3: the skip block's input is the \(c, h, w\) map of layer 1 \(a GroupNorm layer\); a skip block stands on a feature vector"):
        plan([conv(), gn(), _L(abi, D, n_in=64, n_out=64), _L(abi, abi.LAYER_SKIPADD, cin=1), head()])
    # a LayerNorm or Dropout directly behind the layer: wording of its own
    with R(abi.DQNError, match=r"layer 2: LayerNorm must directly follow a Dense or recurrent layer \(layer 1 is a GroupNorm layer, whose output is a \(4, 4, 4\) map\)"):
        plan([conv(), gn(), _L(abi, LN, n_in=64, n_out=64), head()])
    with R(abi.DQNError, match=r"layer 2: Dropout must directly follow a Dense, recurrent or LayerNorm layer \(layer 1 is a GroupNorm layer, whose output is a \(4, 4, 4\) map\)"):
        plan([conv(), gn(), _L(abi, DO, cout=0x3FE00000), head()])


def test_julia_shim_maps_the_layer_and_refuses_its_relatives():
    src = open(os.path.join(ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    assert re.search(r"elseif l isa Flux\.GroupNorm\b", src)
    assert re.search(r"l\.affine \|\| throw\(\"DeepQLearningError: [^\"]*GroupNorm with affine=true only\"\)", src)
    assert re.search(r"l\.track_stats && throw\(\"DeepQLearningError: [^\"]*GroupNorm with track_stats=false only", src)
    assert re.search(r"return LayerDesc\(11, ACT\[l\.λ\], stream, 0, 0, l\.chs, l\.chs, l\.G, reinterpret\(Int32, Float32\(l\.ϵ\)\), 0, 0\)", src)
    assert re.search(r"l isa Flux\.BatchNorm && throw\(\"DeepQLearningError: BatchNorm is not supported: it keeps running statistics", src)
    assert re.search(r"l isa Flux\.InstanceNorm && throw\(\"DeepQLearningError: InstanceNorm is not supported: its default is affine = false", src)
    assert re.search(r"\(l isa Flux\.LayerNorm \|\| l isa Flux\.GroupNorm\) \? l\.λ", src)      # check_act sees the layer's λ
    assert re.search(r"is_map_desc\(d\) = .*d\.kind == 11", src)      # a convolutional block may stand behind the layer
    assert 'throw("DeepQLearningError: unsupported layer' in src and "MeanPool / GroupNorm / Dense / Dropout / LSTM" in src and "RNN / LayerNorm / flattenbatch only" in src
    for a, b in (("(", ")"), ("[", "]")):
        assert src.count(a) == src.count(b)
    assert len(re.findall(r"\bend\b", src)) >= len(re.findall(r"^\s*(?:function|if|for|begin|struct|mutable struct|module|let|while|try)\b", src, re.M))


def _first_step(c, leg):
    gamma = float(np.float32(c.gamma))
    if c.T:
        D = GR.rec_data(c); idx, start = D.draws[0]
        return GR.rec_step(D.net, D.p_on, D.p_tg, GR.R.sample_batch(D.ring, idx, start, c.T, c.obs), gamma, bool(c.dq), leg)
    D = GR.ff_data(c)
    return GR.ff_step(D.net, D.p_on, D.p_tg, GR.ff_batch(c, D, D.idx[0]), gamma, bool(c.dq), leg)


@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_reference_legs_agree_and_the_seed_keeps_the_margins(c):
    """F.group_norm under autograd and the hand-written NumPy layer: 1e-10 relative on every quantity.  The case's fixed seed keeps sigma >= SIGMA_MIN on every
    non-degenerate group, the relu and MaxPool margins and the argmax gap -- asserted, never redrawn, never skipped"""
    sg, rm, pm, gap = GR.case_margins(c)
    assert sg >= GR.SIGMA_MIN and rm > GR.RELU_MARGIN and pm > GR.RELU_MARGIN and gap > GR.GAP, (c.name, sg, rm, pm, gap)
    a, b = _first_step(c, "torch"), _first_step(c, "numpy")
    GR.legs_agree(a, b)
    D = GR.rec_data(c) if c.T else GR.ff_data(c)
    assert not GR.dead_blocks(D.net, a["grads"]), c.name      # every block, gn<i>.beta / gn<i>.gamma included, is live
    names = [nm for nm, _ in GR.blocks(D.net)]
    assert any(re.fullmatch(r"gn\d+\.beta", nm) for nm in names) and any(re.fullmatch(r"gn\d+\.gamma", nm) for nm in names)


def test_the_table_reaches_what_it_says():
    """the chunk cases are built around the kernel's chunk length; both column paths; the group shapes"""
    src = open(os.path.join(ROOT, "deepqlearning.jl_amd", "csrc", "common.h")).read()
    assert int(re.search(r"#define GN_R (\d+)", src).group(1)) == GR.GN_R
    def ng(name):
        c = GR.BY_NAME[name]; net = c.mk(); shp = c.obs
        for l in net.layers:
            if l.kind == "conv":
                shp = (l.cout, (shp[1] + 2 * l.ph - l.kh) // l.sh + 1, (shp[2] + 2 * l.pw - l.kw) // l.sw + 1)
            elif l.kind in ("maxpool", "meanpool"):
                shp = (shp[0], (shp[1] - l.kh) // l.sh + 1, (shp[2] - l.kw) // l.sw + 1)
            elif l.kind == "groupnorm":
                return (shp[0] // l.G) * shp[1] * shp[2], shp[1] * shp[2]
    assert ng("chunks_b5") == ng("chunks_b8") == (2 * GR.GN_R + 3, 1) and ng("one_chunk") == (GR.GN_R - 1, 9)
    assert ng("g2_b5") == (32, 16) and ng("g1") == (64, 16) and ng("gc") == (16, 16) and ng("hw_odd")[1] == 15
    assert (2 * GR.BY_NAME["g2_b5"].B) % 4 != 0 and (2 * GR.BY_NAME["chunks_b5"].B) % 4 != 0 and GR.BY_NAME["chunks_b8"].B % 4 == 0      # the one-column and the four-column path
    assert float(np.float32(GR.BY_NAME["eps_half"].mk().layers[1].eps)) == 0.5
    assert {GR.BY_NAME[n].mk().layers[1].act for n in ("act_tanh", "act_leakyrelu")} == {nn.tanh, nn.leakyrelu}
    assert GR.BY_NAME["valu"].mfma == 0 and GR.BY_NAME["b32"].B == 32 and GR.BY_NAME["u8"].u8 == 1 and GR.BY_NAME["dueling"].dueling and GR.BY_NAME["then_lstm"].T == 3


@pytest.mark.parametrize("eps", [1e-5, 0.5])
@pytest.mark.parametrize("G", [1, 2, 6])
def test_gradient_of_the_law_against_central_differences(eps, G):
    """the hand-written backward, the path through the variance included, against central differences of the hand-written forward in fp64"""
    rng = np.random.default_rng(3); B, C, H, W = 2, 6, 2, 3
    x, beta, gamma, dy = rng.standard_normal((B, C, H, W)), 0.2 * rng.standard_normal(C), 1 + 0.3 * rng.standard_normal(C), rng.standard_normal((B, C, H, W))
    loss = lambda x, b, g: float((GR.gn_forward_np(x, b, g, G, eps)[0] * dy).sum())
    dx, db, dg = GR.gn_backward_np(GR.gn_forward_np(x, beta, gamma, G, eps)[1], dy)
    h = 1e-6
    def num(arr, f):
        g = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            up, dn = arr.copy(), arr.copy(); up[i] += h; dn[i] -= h
            g[i] = (f(up) - f(dn)) / (2 * h)
        return g
    np.testing.assert_allclose(dx, num(x, lambda v: loss(v, beta, gamma)), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(db, num(beta, lambda v: loss(x, v, gamma)), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(dg, num(gamma, lambda v: loss(x, beta, v)), rtol=1e-6, atol=1e-8)
    # ... and autograd through torch's own group_norm agrees with it
    xt, bt, gt = (torch.tensor(v, requires_grad=True) for v in (x, beta, gamma))
    (GR.gn_torch(xt, bt, gt, G, eps) * torch.tensor(dy)).sum().backward()
    for got, want in ((xt.grad, dx), (bt.grad, db), (gt.grad, dg)):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-10, atol=1e-12)
    # without the path through the variance the input gradient is a different one: the check above can tell
    xh, r, _, _ = GR.gn_forward_np(x, beta, gamma, G, eps)[1]; g = (dy * gamma.reshape(1, C, 1, 1)).reshape(B, G, -1)
    assert np.abs((r * (g - g.mean(axis=2, keepdims=True))).reshape(x.shape) - dx).max() > 1e-2


def test_the_tests_can_tell_the_two_eps_laws_apart():
    """eps = 0.5: the reference's Q differs from the Q under (x - mu) / (sigma + eps) by more than 100 x TOL_Q on every column -- an engine on LayerNorm's law fails eps_half"""
    c = GR.BY_NAME["eps_half"]; D = GR.ff_data(c); s = GR.ff_batch(c, D, D.idx[0])[0]
    q, ql = GR.q_values(D.net, D.p_on, s), GR.q_values(D.net, D.p_on, s, leg="ln_law")
    tol = GR.TOL_Q["atol"] + GR.TOL_Q["rtol"] * np.abs(q)
    assert (np.abs(q - ql) / tol).max() > 1000 and (np.abs(q - ql) / tol).max(axis=1).min() > 100, (float((np.abs(q - ql) / tol).max()), float((np.abs(q - ql) / tol).max(axis=1).min()))
    c0 = GR.BY_NAME["g1"]; D0 = GR.ff_data(c0); s0 = GR.ff_batch(c0, D0, D0.idx[0])[0]      # at the default eps the two laws are close: the case above is the one that bites
    assert np.abs(GR.q_values(D0.net, D0.p_on, s0) - GR.q_values(D0.net, D0.p_on, s0, leg="ln_law")).max() < 1e-2


def test_the_tests_can_tell_beta_gamma_from_gamma_beta():
    """noisy parameters: with the two arrays of the layer swapped (gamma, beta -- LayerNorm's order) every case's Q is off by more than 100 x TOL_Q"""
    for name in ("g2_b5", "chunks_b8", "dueling"):
        c = GR.BY_NAME[name]; D = GR.ff_data(c); s = GR.ff_batch(c, D, D.idx[0])[0]
        p = D.p_on.copy(); blks = dict(GR.blocks(D.net))
        for nm, sl in blks.items():
            if nm.endswith(".beta"):
                g = blks[nm[:-4] + "gamma"]
                p[sl], p[g] = D.p_on[g], D.p_on[sl]
        q, qs = GR.q_values(D.net, D.p_on, s), GR.q_values(D.net, p, s)
        tol = GR.TOL_Q["atol"] + GR.TOL_Q["rtol"] * np.abs(q)
        assert (np.abs(q - qs) / tol).max() > 100, name


def test_dead_group_really_is_identically_zero_in_fp64():
    c = GR.BY_NAME["dead_group"]; D = GR.ff_data(c); s, _, _, sp, _, _ = GR.ff_batch(c, D, D.idx[0])
    for p, x in ((D.p_on, s), (D.p_on, sp), (D.p_tg, sp)):
        pr = GR.probe_of(D.net, p, x)
        assert pr["dead"] == c.B and pr["sigma"] >= GR.SIGMA_MIN      # group 0 of every column; the live group keeps the rule
    arrs = GR.param_arrays(D.net, nn, D.p_on.astype(np.float64))
    y = torch.relu(torch.nn.functional.conv2d(GR._t64(s), arrs[0][0].flip(2, 3), arrs[0][1]))
    assert float(y[:, :2].abs().max()) == 0.0 and float(y[:, 2:].abs().max()) > 0
    o = GR.ff_step(D.net, D.p_on, D.p_tg, GR.ff_batch(c, D, D.idx[0]), 0.95, True)
    assert np.isfinite(o["grads"]).all()
    for name in ("g2_b5", "u8"):      # no other case has one
        c2 = GR.BY_NAME[name]; D2 = GR.ff_data(c2)
        assert GR.probe_of(D2.net, D2.p_on, GR.ff_batch(c2, D2, D2.idx[0])[0])["dead"] == 0


def test_default_plans(pkg, mods):
    """the layer's entry is all zeros at every batch; the GEMM layers around it keep the plan they have without it"""
    for B in (8, 32, 128, 512):
        hp = pkg.default_hparams(batch_size=B, n_actions=4, obs_c=4, obs_h=84, obs_w=84, buffer_size=1024, dueling=0)
        plain = nn.Chain(nn.Conv(8, 4, 32, nn.relu, 4), nn.Conv(4, 32, 64, nn.relu, 2), nn.Conv(3, 64, 64, nn.relu, 1), nn.flattenbatch, nn.Dense(3136, 512, nn.relu), nn.Dense(512, 4))
        normed = nn.Chain(nn.Conv(8, 4, 32, nn.relu, 4), nn.GroupNorm(32, 4, nn.relu), nn.Conv(4, 32, 64, nn.relu, 2), nn.GroupNorm(64, 4, nn.relu), nn.Conv(3, 64, 64, nn.relu, 1),
                          nn.GroupNorm(64, 4, nn.relu), nn.flattenbatch, nn.Dense(3136, 512, nn.relu), nn.Dense(512, 4))
        a = [tuple(p) for p in pkg.default_plan(nn.lower(plain)[0], hp)]; b = [tuple(p) for p in pkg.default_plan(nn.lower(normed)[0], hp)]
        assert [b[i] for i in (1, 3, 5)] == [(0, 0, 0)] * 3 and [b[i] for i in (0, 2, 4, 6, 7)] == a, B
