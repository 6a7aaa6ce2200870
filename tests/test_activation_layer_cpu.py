"""CPU: the standalone activation layer nn.Activation(σ) (layer kind 14; Julia's Base.Broadcast.BroadcastFunction(σ)) in the fp64 reference the GPU tests
(test_activation_layer_gpu.py) stand on -- known values, the hand-written derivatives against autograd, the two legs against each other along every case, the seeds and
their margins --, then in the Python mirror, the ABI header, the parameter layout, BSON, the library's host-side validation (no GPU: dqn_plan_default runs build_layers) and
the Julia shim.  Every test here fails without the feature: nn.Activation and abi.LAYER_ACTIVATION do not exist and build_layers answers "unknown kind 14"."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import activation_layer_reference as XR

ROOT = ge.ROOT
nn = XR.nn
IDS = lambda cs: [c.name for c in cs]
ALL = XR.CASES + XR.REC_CASES + XR.EXACT_ONLY


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "_abi", "bson"))


# ------------------------------------------------------------------ the fp64 reference
KNOWN = [(XR.SWISH, 1.0, 1.0 / (1.0 + math.exp(-1.0))), (XR.SWISH, 0.0, 0.0), (XR.GELU, 1.0, 0.8411919906082768), (XR.GELU, -1.0, -0.15880800939172324),
         (XR.MISH, 1.0, 0.8650983882673103), (XR.MISH, 0.0, 0.0), (XR.HARDSWISH, 1.0, 2.0 / 3.0), (XR.HARDSWISH, -4.0, 0.0), (XR.HARDSWISH, 5.0, 5.0), (XR.HARDSWISH, -1.5, -0.375)]


@pytest.mark.parametrize("a,x,want", KNOWN, ids=[f"{XR.NAMES[a]}({x:g})" for a, x, _ in KNOWN])
def test_known_values(a, x, want):
    """both legs, to 1e-15; gelu(1) = 0.84119... is the TANH form (the erf form gives 0.84134...)"""
    assert abs(float(XR.actl_np(np.array([x]), a)[0]) - want) <= 1e-15
    assert abs(float(XR.actl_torch(torch.tensor([x], dtype=torch.float64), a)[0]) - want) <= 1e-15
    assert abs(0.8411919906082768 - 0.5 * (1.0 + math.erf(1.0 / math.sqrt(2.0)))) > 1e-4


def test_hand_written_derivatives_are_the_derivatives():
    """dactl_np -- from the output for the eleven, from the input for the four -- against torch float64 autograd on a grid that straddles every kink (off the kinks)"""
    x = np.concatenate([np.linspace(-9.0, 9.0, 721) + 1e-3, [-30.0, 30.0]])
    for a in range(15):
        t = torch.tensor(x, requires_grad=True)
        y = XR.actl_torch(t, a); y.sum().backward()
        yn = XR.actl_np(x, a)
        assert np.abs(yn - y.detach().numpy()).max() <= 1e-14, XR.NAMES[a]
        assert np.abs(XR.dactl_np(np.ones_like(x), x, yn, a) - t.grad.numpy()).max() <= 1e-13, XR.NAMES[a]


@pytest.mark.parametrize("c", XR.CASES + XR.REC_CASES, ids=IDS(XR.CASES + XR.REC_CASES))
def test_legs_agree_and_the_seed_keeps_the_margins(c):
    """torch autograd over torch.nn.functional and the NumPy closed forms with the hand-written backward: 1e-10 relative on every quantity along the case's steps; along the
    same steps every kink, every MaxPool window and every argmax column keeps its margin; no gradient block is dead on the first step"""
    D = XR.prepare(c); g = float(np.float32(c.gamma))
    for k, p, batch, o in XR.trajectory(c, D):
        o2 = XR.rec_step(D.net, p, D.p_tg, batch, g, bool(c.dq), "numpy") if c.T else XR.ff_step(D.net, p, D.p_tg, batch, g, bool(c.dq), "numpy")
        XR.legs_agree(o, o2)
        km, pm, gap = XR.margins(c, D.net, p, D.p_tg, batch)
        assert km > XR.RELU_MARGIN and pm > XR.RELU_MARGIN and gap > XR.GAP, (c.name, k, km, pm, gap)
        if k == 0:
            XR.check_grads(D.net, o["grads"], o["grads"], live=True)
    assert [code for _, code in XR.activations(D.net)] == list(c.codes)


def test_the_seeds_are_the_smallest_that_keep_twice_the_margins():
    """no case lacks a seed below 64, none is skipped; the table's seed is what find_seed returns"""
    for c in ALL:
        assert XR.find_seed(c) == c.seed, c.name


def test_the_table_covers_what_the_gpu_file_promises():
    names = set(XR.BY_NAME)
    assert {f"vec_{n}" for n in XR.NAMES} <= names and {f"vec_{XR.NAMES[a]}_b5_n7" for a in XR.NEW} <= names and "vec_gelu_b128" in names
    assert {f"map_{XR.NAMES[a]}" for a in XR.NEW + (1,)} <= names and {"map_gn_swish", "map_maxpool_mish", "map_gelu_cpad", "postadd_vec", "postadd_map", "dueling_swish", "map_gmean_hardswish", "vec_tanh_then_relu"} <= names
    assert {f"exact_map_{XR.NAMES[a]}" for a in range(11) if a != 1} <= names and "exact_cpad_tanh" in names
    assert sum(c.plain is not None for c in ALL) == 11 + 11 + 1 + 1      # Dense and Conv companions of the eleven, one padded Conv, Activation behind Activation
    assert set(XR.KINKS[XR.HARDSWISH]) == {-3.0, 3.0} and XR.KINKS[9] == (0.0, 6.0) and XR.KINKS[10] == (-1.0, 1.0)


# ------------------------------------------------------------------ the mirror, the header, the parameter layout
def test_header_and_abi_agree(mods):
    _, abi, _ = mods
    hdr = open(os.path.join(ROOT, "include", "dqn_mi355x.h")).read()
    assert int(re.search(r"DQN_LAYER_ACTIVATION\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_ACTIVATION == 14
    for code, name in zip(XR.NEW, ("GELU", "SWISH", "MISH", "HARDSWISH")):
        assert int(re.search(r"DQN_ACT_%s\s*=\s*(\d+)" % name, hdr).group(1)) == code == getattr(abi, "ACT_" + name)
    assert re.search(r"#define DQN_ACT_LAST DQN_ACT_HARDTANH\b", hdr) and re.search(r"#define DQN_ACT_LAYER_LAST DQN_ACT_HARDSWISH\b", hdr)      # every other kind keeps 0..10
    assert int(re.search(r"#define DQN_PLAN_VERSION\s+(\d+)", hdr).group(1)) == 3      # no struct changed, no summation order changed


def test_the_mirror_layer(mods):
    _, abi, _ = mods
    assert nn.ACT_NAMES == XR.AR.NAMES and nn.LAYER_ACT_NAMES == XR.NAMES      # the eleven stay the eleven
    for code, name in enumerate(XR.NAMES):
        l = XR.A(code)
        assert l.kind == "activation" and l.code == code and l.shapes() == [] and repr(l) == f"Activation({name})"
    assert nn.Activation(nn.gelu).code == 11 and nn.Activation(nn.hardswish).code == 14 and nn.Activation(nn.relu).code == 1 and nn.Activation(np.int32(7)).code == 7
    for bad in (15, -1, 2.0, "gelu", None, True, (lambda x: x)):
        with pytest.raises(abi.DQNError, match=r"DeepQLearningError: unsupported activation .* on Activation \(supported: identity / relu / .* / hardtanh / gelu / swish / mish / hardswish"):
            nn.Activation(bad)


def test_lowering_to_descriptors(mods):
    _, abi, _ = mods
    layers, dueling = nn.lower(nn.Chain(nn.Dense(6, 64), XR.A(XR.GELU), nn.Dense(64, 4)))
    assert not dueling and [(l.kind, l.act, l.stream, l.n_in, l.n_out, l.cin, l.cout, l.kh, l.kw, l.sh, l.sw) for l in layers] == \
        [(0, 0, 0, 6, 64, 0, 0, 0, 0, 0, 0), (14, 11, 0, 0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 64, 4, 0, 0, 0, 0, 0, 0)]
    blk = lambda: nn.SkipConnection(nn.Chain(nn.Conv(3, 4, 4, nn.relu, pad=1), nn.Conv(3, 4, 4, pad=1)), "+")
    layers, _ = nn.lower(nn.Chain(nn.Conv(3, 1, 4), blk(), XR.A(1), blk(), nn.flattenbatch, nn.Dense(64, 4)))
    assert [(l.kind, l.act) for l in layers] == [(1, 0), (1, 1), (1, 0), (10, 0), (14, 1), (1, 1), (1, 0), (10, 0), (0, 0)]      # the second block behind the layer is still a MAP block
    vb = lambda: nn.SkipConnection(nn.Chain(nn.Dense(16, 16, nn.relu), nn.Dense(16, 16)), "+")
    layers, _ = nn.lower(nn.Chain(nn.Dense(6, 16), vb(), XR.A(1), vb(), nn.Dense(16, 4)))
    assert [l.kind for l in layers] == [0, 0, 0, 9, 14, 0, 0, 9, 0]
    layers, _ = nn.lower(nn.Chain(nn.Conv(3, 1, 4), XR.A(12), XR.A(2), nn.MaxPool(2), XR.A(13), nn.flattenbatch, nn.Dense(16, 4)))      # a pool behind it takes the conv's channels
    assert [(l.kind, l.act, l.cin) for l in layers] == [(1, 0, 1), (14, 12, 0), (14, 2, 0), (5, 0, 4), (14, 13, 0), (0, 0, 0)]


def test_parameter_order_glorot_and_bson_round_trip(mods, tmp_path):
    _, abi, bson = mods
    net = nn.Chain(nn.Conv(3, 1, 4), XR.A(XR.MISH), nn.flattenbatch, nn.Dense(64, 3), XR.A(1), nn.Dense(3, 2))
    plain = nn.Chain(nn.Conv(3, 1, 4), nn.flattenbatch, nn.Dense(64, 3), nn.Dense(3, 2))
    assert [l.kind for l in nn.all_layers(net)] == ["conv", "activation", "dense", "activation", "dense"]
    p = nn.glorot_params(net, seed=3)
    np.testing.assert_array_equal(p, nn.glorot_params(plain, seed=3))      # the layer holds nothing and draws nothing
    shapes = bson.julia_param_shapes(net)
    assert shapes == bson.julia_param_shapes(plain) == [((3, 3, 1, 4), 36), ((4,), 4), ((3, 64), 192), ((3,), 3), ((2, 3), 6), ((2,), 2)]
    assert [nm for nm, _ in XR.blocks(net)] == ["conv0.W", "conv0.b", "dense2.W", "dense2.b", "dense4.W", "dense4.b"]
    p = (p + np.arange(p.size, dtype=np.float32)).astype(np.float32)
    path = str(tmp_path / "qnetwork.bson")
    bson.save_qnetwork(path, p, shapes)
    flat, sizes = bson.load_qnetwork(path)
    np.testing.assert_array_equal(flat, p)
    assert [tuple(s) for s in sizes] == [s for s, _ in shapes]


def test_dueling_split_ends_the_trailing_dense_run_at_the_layer(mods):
    _, abi, _ = mods
    d = nn.create_dueling_network(nn.Chain(nn.Dense(6, 16), XR.A(XR.SWISH), nn.Dense(16, 8, nn.relu), nn.Dense(8, 4)))
    assert [l.kind for l in d.base] == ["dense", "activation"] and [l.kind for l in d.val] == ["dense", "dense"] and d.val.layers[-1].n_out == 1
    layers, dueling = nn.lower(d)
    assert dueling and [(l.kind, l.stream) for l in layers] == [(0, 0), (14, 0), (0, 1), (0, 1), (0, 2), (0, 2)]
    with pytest.raises(abi.DQNError, match="incompatible with dueling"):      # a chain that ends in the layer has no trailing Dense
        nn.create_dueling_network(nn.Chain(nn.Dense(6, 4), XR.A(1)))


def test_the_mirror_refuses_by_name(mods):
    _, abi, _ = mods
    low = lambda *ls: nn.lower(nn.Chain(*ls))
    with pytest.raises(abi.DQNError, match=r"Activation\(relu\) cannot be the first layer"):
        low(XR.A(1), nn.Dense(6, 4))
    with pytest.raises(abi.DQNError, match=r"Activation\(gelu\) cannot be the network's output layer"):
        low(nn.Dense(6, 4), XR.A(11))
    d = nn.create_dueling_network(nn.Chain(nn.Dense(6, 16), nn.Dense(16, 8), nn.Dense(8, 4)))
    d.adv.layers.insert(1, XR.A(12))
    with pytest.raises(abi.DQNError, match=r"Activation\(swish\) is supported in the base chain only \(not in a value / advantage stream\)"):
        nn.lower(d)
    with pytest.raises(abi.DQNError, match=r"an Activation layer inside a SkipConnection is not supported"):
        low(nn.Dense(6, 16), nn.SkipConnection(nn.Chain(nn.Dense(16, 16), XR.A(1), nn.Dense(16, 16)), "+"), nn.Dense(16, 4))
    with pytest.raises(abi.DQNError, match=r"an Activation layer inside a SkipConnection is not supported"):
        low(nn.Conv(3, 1, 4), nn.SkipConnection(nn.Chain(nn.Conv(3, 4, 4, pad=1), XR.A(1), nn.Conv(3, 4, 4, pad=1)), "+"), nn.flattenbatch, nn.Dense(64, 4))
    with pytest.raises(abi.DQNError, match=r"LayerNorm\(16.* cannot directly follow Activation\(relu\)"):
        low(nn.Dense(6, 16), XR.A(1), nn.LayerNorm(16), nn.Dense(16, 4))
    with pytest.raises(abi.DQNError, match=r"Dropout\(0.1\) cannot directly follow Activation\(mish\)"):
        low(nn.Dense(6, 16), XR.A(13), nn.Dropout(0.1), nn.Dense(16, 4))
    # ... across the edge of a skip block too: the block's first inner layer reads the Activation's output (the engine refuses it by index, the Julia shim by the next descriptor)
    blk = lambda first: nn.SkipConnection(nn.Chain(first, nn.Dense(16, 16)), "+")
    with pytest.raises(abi.DQNError, match=r"LayerNorm\(16.* cannot directly follow Activation\(tanh\): .* as the first inner layer of a SkipConnection neither"):
        low(nn.Dense(6, 16), XR.A(2), blk(nn.LayerNorm(16)), nn.Dense(16, 4))
    with pytest.raises(abi.DQNError, match=r"Dropout\(0.5\) cannot directly follow Activation\(gelu\): .* as the first inner layer of a SkipConnection neither"):
        low(nn.Dense(6, 16), XR.A(11), blk(nn.Dropout(0.5)), nn.Dense(16, 4))
    assert len(low(nn.Dense(6, 16), XR.A(2), blk(nn.Dense(16, 16, nn.relu)), nn.Dense(16, 4))[0]) == 6      # a Dense first: accepted, as before
    assert len(low(nn.Dense(6, 16), blk(nn.LayerNorm(16)), nn.Dense(16, 4))[0]) == 5      # ... and a LayerNorm first behind a Dense
    with pytest.raises(abi.DQNError, match=r"a closure cannot be inspected; write a standalone activation as Activation\(relu\) \(Julia: Base.BroadcastFunction\(relu\)\)"):
        low(nn.Dense(6, 16), (lambda x: np.maximum(x, 0)), nn.Dense(16, 4))


def test_dense_with_gelu_is_still_refused_with_todays_text(mods):
    _, abi, _ = mods
    for bad in (nn.gelu, nn.swish, nn.mish, nn.hardswish):
        with pytest.raises(abi.DQNError, match=r"DeepQLearningError: unsupported activation %s on Dense\(6, 8, act=%s\): %s is not monotone, so its derivative needs the "
                                               r"pre-activation, and the MI355X engine keeps only each layer's output y" % (bad.name, bad.name, bad.name)):
            nn.lower(nn.Chain(nn.Dense(6, 8, bad), nn.Dense(8, 4)))
    with pytest.raises(abi.DQNError, match=r"unsupported activation swish on Conv\("):
        nn.lower(nn.Chain(nn.Conv(3, 1, 4, nn.swish), nn.flattenbatch, nn.Dense(64, 4)))


# ------------------------------------------------------------------ build_layers on the host
def _L(abi, kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, kh=0, kw=0, sh=0, sw=0):
    d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, kh, kw, sh, sw
    return d


def test_host_side_validation_without_a_gpu(pkg, mods):
    """dqn_plan_default runs build_layers on the host: every placement that is admitted, every refusal by layer index; the layer's plan entry is zeros"""
    _, abi, _ = mods
    L = lambda *a, **k: _L(abi, *a, **k)
    D, CV, ACT, LN, DO, GN, MP, AMP, SK, SKM = 0, 1, 14, abi.LAYER_LAYERNORM, abi.LAYER_DROPOUT, abi.LAYER_GROUPNORM, abi.LAYER_MAXPOOL, abi.LAYER_ADAPTIVEMEANPOOL, abi.LAYER_SKIPADD, abi.LAYER_SKIPADD_MAP

    def plan(layers, obs=(6, 1, 1), **kw):
        return pkg.default_plan(layers, pkg.default_hparams(batch_size=8, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], buffer_size=64, **({"dueling": 0} | kw)))
    img = (1, 6, 6)
    d0, head = L(D, n_in=6, n_out=16), L(D, n_in=16, n_out=4)
    conv = lambda: L(CV, cin=1, cout=4, kh=3, kw=3, sh=1, sw=1)                                   # (1, 6, 6) -> (4, 4, 4)
    cpad = lambda a=0: L(CV, act=a, cin=4, cout=4, kh=3, kw=3, sh=1, sw=1, n_in=1, n_out=1)
    mblk = lambda: [cpad(1), cpad(), L(SKM, cin=2)]
    vblk = lambda: [L(D, act=1, n_in=16, n_out=16), L(D, n_in=16, n_out=16), L(SK, cin=2)]
    # ---- admitted: all fifteen codes; the size stated or left to the engine
    for a in range(15):
        p = plan([d0, L(ACT, act=a), head])
        assert p[1] == (0, 0, 0)
        plan([d0, L(ACT, act=a, n_in=16, n_out=16), head])
        plan([conv(), L(ACT, act=a), L(D, n_in=64, n_out=4)], obs=img)
    # behind: Dense, recurrent, LayerNorm, Dropout, either join, Conv (padded or not), pools (global / adaptive too), GroupNorm, another Activation
    plan([L(abi.LAYER_LSTM, n_in=6, n_out=16), L(ACT, act=2), head], recurrence=1, trace_length=3)
    plan([L(abi.LAYER_GRU, n_in=6, n_out=16), L(ACT, act=11), head], recurrence=1, trace_length=3)
    plan([d0, L(LN, n_in=16, n_out=16), L(ACT, act=12), head])
    plan([d0, L(DO, cin=0, cout=0), L(ACT, act=1), head])
    plan([d0] + vblk() + [L(ACT, act=1)] + vblk() + [head])                                         # ... and a feature-vector block behind it
    plan([conv()] + mblk() + [L(ACT, act=1)] + mblk() + [L(D, n_in=64, n_out=4)], obs=img)          # ... and a convolutional block behind it
    plan([conv(), cpad(), L(ACT, act=13), L(D, n_in=64, n_out=4)], obs=img)
    plan([conv(), L(MP, kh=2, kw=2, sh=2, sw=2), L(ACT, act=13), L(D, n_in=16, n_out=4)], obs=img)
    plan([conv(), L(AMP, kh=1, kw=1), L(ACT, act=14), L(D, n_in=4, n_out=4)], obs=img)
    plan([conv(), L(GN, kh=2), L(ACT, act=12), L(D, n_in=64, n_out=4)], obs=img)
    plan([d0, L(ACT, act=1), L(ACT, act=11), head])
    # behind it, on a map: Conv, pools, GroupNorm; on either: a recurrent layer; the dueling split
    plan([conv(), L(ACT, act=11), cpad(), L(ACT, act=1), L(MP, kh=2, kw=2, sh=2, sw=2), L(ACT, act=2), L(GN, kh=2), L(D, n_in=16, n_out=4)], obs=img)
    plan([conv(), L(ACT, act=11), L(abi.LAYER_GRU, n_in=64, n_out=8), L(D, n_in=8, n_out=4)], obs=img, recurrence=1, trace_length=3)
    plan([d0, L(ACT, act=12), L(D, stream=1, n_in=16, n_out=1), L(D, stream=2, n_in=16, n_out=4)], dueling=1)      # the last layer of a dueling base chain
    with pytest.raises(abi.DQNError, match=r"layer 2: dense n_in 16 != incoming features 64"):      # it keeps the map: (4, 4, 4) = 64 features
        plan([conv(), L(ACT, act=1), head], obs=img)
    # ---- refused, by layer index
    with pytest.raises(abi.DQNError, match=r"layer 0: an Activation layer cannot be the first layer"):
        plan([L(ACT, act=1), L(D, n_in=6, n_out=4)])
    with pytest.raises(abi.DQNError, match=r"layer 1: an Activation layer cannot be the network's output layer"):
        plan([L(D, n_in=6, n_out=4), L(ACT, act=1)])
    for stream in (1, 2):
        with pytest.raises(abi.DQNError, match=r"layer 2: Activation layers are supported in the base chain only \(not in a value / advantage stream; stream = %d\)" % stream):
            plan([d0, L(D, stream=stream, n_in=16, n_out=16), L(ACT, stream=stream, act=1), L(D, stream=3 - stream, n_in=16, n_out=4)], dueling=1)
    with pytest.raises(abi.DQNError, match=r"layer 3: the skip block holds an Activation layer \(layer 2\)"):
        plan([d0, L(D, n_in=16, n_out=16), L(ACT, act=1), L(SK, cin=2), head])
    with pytest.raises(abi.DQNError, match=r"layer 3: the convolutional skip block holds an Activation layer \(layer 2\)"):
        plan([conv(), cpad(), L(ACT, act=1), L(SKM, cin=2), L(D, n_in=64, n_out=4)], obs=img)
    with pytest.raises(abi.DQNError, match=r"layer 2: LayerNorm must directly follow a Dense or recurrent layer \(layer 1 is an Activation layer"):
        plan([d0, L(ACT, act=1), L(LN, n_in=16, n_out=16), head])
    with pytest.raises(abi.DQNError, match=r"layer 2: Dropout must directly follow a Dense, recurrent or LayerNorm layer \(layer 1 is an Activation layer"):
        plan([d0, L(ACT, act=1), L(DO), head])
    for code in (15, -1):
        with pytest.raises(abi.DQNError, match=r"layer 1: Activation code %d is not one of DQN_ACT_\* \(0\.\.14\)" % code):
            plan([d0, L(ACT, act=code), head])
    for slot in ("cin", "cout", "kh", "kw", "sh", "sw"):
        vals = {k: (1 if k == slot else 0) for k in ("cin", "cout", "kh", "kw", "sh", "sw")}
        with pytest.raises(abi.DQNError, match=r"layer 1: Activation uses act, n_in and n_out only; cin / cout / kh / kw / sh / sw = %d / %d / %d / %d / %d / %d must be 0" % tuple(vals.values())):
            plan([d0, L(ACT, act=1, **vals), head])
    with pytest.raises(abi.DQNError, match=r"layer 1: Activation n_in 16 != n_out 0"):
        plan([d0, L(ACT, act=1, n_in=16), head])
    with pytest.raises(abi.DQNError, match=r"layer 1: Activation size n = 5 != incoming features 16"):
        plan([d0, L(ACT, act=1, n_in=5, n_out=5), head])
    # a pool / GroupNorm behind the layer on a feature vector is named as such; a vector block behind the layer on a map stays refused
    with pytest.raises(abi.DQNError, match=r"layer 2: GroupNorm must directly follow .* \(layer 1 is an Activation layer on a feature vector"):
        plan([d0, L(ACT, act=1), L(GN, kh=2), head])
    with pytest.raises(abi.DQNError, match=r"layer 5: the skip block's input is the \(c, h, w\) map of layer 1"):
        plan([conv(), L(ACT, act=1), L(D, n_in=64, n_out=64), L(D, n_in=64, n_out=64), L(D, n_in=64, n_out=64), L(SK, cin=3), L(D, n_in=64, n_out=4)], obs=img)
    # every other kind keeps refusing the codes above 10 with the message it has
    with pytest.raises(abi.DQNError, match=r"layer 0: Dense activation 11 is not one of DQN_ACT_\* \(0\.\.10\)"):
        plan([L(D, act=11, n_in=6, n_out=16), head])
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv activation 14 is not one of DQN_ACT_\* \(0\.\.10\)"):
        plan([L(CV, act=14, cin=1, cout=4, kh=3, kw=3, sh=1, sw=1), L(D, n_in=64, n_out=4)], obs=img)
    with pytest.raises(abi.DQNError, match=r"layer 1: GroupNorm activation 12 is not one of DQN_ACT_\* \(0\.\.10\)"):
        plan([conv(), L(GN, act=12, kh=2), L(D, n_in=64, n_out=4)], obs=img)


def test_n_params_skip_the_layer(pkg, mods):
    """the default plan of a network with the layer is the plan of the network without it, with a zero entry in between"""
    _, abi, _ = mods
    hp = pkg.default_hparams(batch_size=8, n_actions=4, obs_c=6, obs_h=1, obs_w=1, buffer_size=64, dueling=0)
    a = pkg.default_plan(nn.lower(nn.Chain(nn.Dense(6, 2048), XR.A(11), nn.Dense(2048, 4)))[0], hp)
    b = pkg.default_plan(nn.lower(nn.Chain(nn.Dense(6, 2048, nn.tanh), nn.Dense(2048, 4)))[0], hp)
    assert a[1] == (0, 0, 0) and [a[0], a[2]] == b


# ------------------------------------------------------------------ the Julia shim (static: Julia is not available here)
def test_julia_shim_has_the_broadcastfunction_branch_in_front_of_the_generic_throw():
    src = open(os.path.join(ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    m = re.search(r"const ACT = Dict\(([^)]*)\)", src)
    assert m and {k.strip(): int(v) for k, v in (kv.split("=>") for kv in m.group(1).split(","))} == {n: i for i, n in enumerate(XR.AR.NAMES)}      # still the eleven
    assert re.search(r"const ACT_NEEDS_X = \(gelu, swish, mish, hardswish\)", src)
    body = src[src.index("function lower_layer"):src.index("is_act_layer(l) =")]
    br, generic = body.index("if l isa Base.Broadcast.BroadcastFunction"), body.index('throw("DeepQLearningError: unsupported layer')
    assert br < generic
    branch = body[br:body.index("\n    end\n", br)]
    assert "findfirst(g -> l.f === g, ACT_NEEDS_X)" in branch and "haskey(ACT, l.f) ? ACT[l.f]" in branch and "10 + i" in branch and "LayerDesc(14, code, stream, 0, 0, 0, 0, 0, 0, 0, 0)" in branch
    assert "Base.BroadcastFunction(relu)" in body[generic:] and "x -> relu.(x)" in body[generic:]      # the refusal names the way to write it
    # Julia declares BroadcastFunction <: Function (recalled): on the path `lower` takes the layer must be recognised BEFORE anything is taken for glue, or it is dropped silently
    glue = src[src.index("is_glue(l) ="):src.index("\n", src.index("is_glue(l) ="))]
    assert "is_act_layer(l) = l isa Base.Broadcast.BroadcastFunction" in src
    assert glue.index("!is_act_layer(l) &&") < glue.index("|| l isa Function")
    # x -> flattenbatch(x), the flatten of the reference's own models, stays on the glue path: is_glue holds for EVERY other Function and nothing on the path refuses one
    assert glue.rstrip().endswith("!is_act_layer(l) && (l === identity || l === flattenbatch || l isa Function)")
    path = src[src.index("is_act_layer(l) ="):src.index("flatparams(q) =")]
    assert "nameof" not in path and "anonymous closure cannot be inspected;" not in path and "is_anonymous" not in src
    assert "x -> flattenbatch(x)" in src and "skipped as glue" in body[generic:]      # the limitation is stated where the user reads it
    assert re.search(r"lower_into!\(descs, l, stream\) = is_glue\(l\) \? descs :", src)      # every top-level layer goes through is_glue first ...
    skip = src[src.index("function lower_skip!"):src.index("lower_into!(descs, l, stream) =")]
    assert skip.index("any(is_act_layer, inner) && throw") < skip.index("real = filter(!is_glue, inner)")      # ... and inside a SkipConnection the refusal stands in front of the glue filter
    assert "is_glue(l) = l === identity" not in src      # (the parent's form, which took the layer itself for glue)
    # the placement refusals, by name, on the descriptors `lower` returns
    chk = src[src.index("function check_act_layers"):src.index("\nend\n", src.index("function check_act_layers"))]
    for text in ("cannot be the first layer", "is supported in the base chain only (not in a value / advantage stream)", "cannot be the network's output layer", "cannot directly follow"):
        assert text in chk, text
    assert "check_act_layers(descs, q isa DeepQLearning.DuelingNetwork)" in src[src.index("function lower(q)"):]
    names = re.search(r"const ACT_LAYER_NAMES = \(([^)]*)\)", src).group(1)
    assert [n.strip().strip('"') for n in names.split(",")] == list(XR.NAMES)
    assert "descs[k].kind == 14" in src      # the map test of a following SkipConnection looks through the layer
