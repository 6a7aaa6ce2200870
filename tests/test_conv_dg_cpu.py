"""CPU: dilated, grouped and depthwise convolutions (Flux Conv dilation / groups, DepthwiseConv; layer kind 15) in the Python mirror, the ABI header, the Julia shim and the
host-only entries of the library (dqn_plan_default: build_layers' geometry and refusals), and the fp64 reference the GPU tests (test_conv_dg_gpu.py) stand on: its two legs
against each other on the whole case table, the margin seeds of that table, the exact companion's algebra, and that the table can tell four wrong engines from the right one.

Without the feature every test here fails: nn.Conv(..., dilation=2) is a TypeError (conv_dg_reference builds its table at import) and kind 15 is "unknown"."""
import importlib
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import conv_dg_reference as XR

ROOT = ge.ROOT
IDS = lambda cs: [c.name for c in cs]
ALL = XR.CASES + XR.REC_CASES
nn = XR.nn
abi = nn._abi


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def bson(pkg):
    return importlib.import_module(pkg.__name__ + ".bson")


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_reference_legs_agree_along_the_trajectory(c):
    """F.conv2d(dilation, groups, padding) under autograd and the hand-written NumPy forward / backward share no conv code: 1e-10 relative on every quantity, every step"""
    D = XR.prepare(c)
    for (k, p, batch, a), (_, _, _, b) in zip(XR.trajectory(c, D, leg="torch"), XR.trajectory(c, D, leg="numpy")):
        XR.legs_agree(a, b)
        assert np.abs(a["grads"]).max() > 0, (c.name, k)


@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_the_recorded_seed_is_the_smallest_that_keeps_twice_the_margins(c):
    assert XR.find_seed(c) == c.seed
    assert XR.margins_ok(c)      # along the fp64 trajectory of the steps the GPU test runs: 2 RELU_MARGIN at every kink, 2 RELU_MARGIN in every MaxPool window, 2 GAP in every argmax


def test_the_table_holds_the_issues_cases():
    assert len(XR.CASES) == 15 and len(XR.REC_CASES) == 1
    for c in ALL:
        assert XR.general_layers(c.mk()), c.name
        assert c.wrong and set(c.wrong) <= set(XR.WRONG), c.name
    for w in XR.WRONG:
        assert sum(w in c.wrong for c in ALL) >= 3, w


def _off(c, D, a, b):
    """the largest error / tolerance between two step outputs, with the GPU test's own constants"""
    worst = 0.0
    for k, tol in (("q_on_s", XR.TOL_Q), ("q_on_sp", XR.TOL_Q), ("q_tg_sp", XR.TOL_Q), ("td", XR.TOL_TD)):
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        worst = max(worst, float((np.abs(x - y) / (tol["atol"] + tol["rtol"] * np.abs(y))).max()))
    gmax = np.abs(b["grads"]).max()
    for nm, sl in XR.blocks(D.net):
        w = b["grads"][sl]; scale = max(np.abs(w).max(), 1e-2 * gmax)
        worst = max(worst, float((np.abs(a["grads"][sl] - w) / (XR.GRAD_C * scale + XR.GRAD_RTOL * np.abs(w))).max()))
    return worst


WRONG_PAIRS = [(c, w) for c in ALL for w in c.wrong]


@pytest.mark.parametrize("c,w", WRONG_PAIRS, ids=[f"{c.name}-{w}" for c, w in WRONG_PAIRS])
def test_the_tests_can_tell_a_wrong_engine(c, w):
    """an engine that ignores the dilation, ignores the groups, interleaves the group-to-channel map or tests dX validity without the dilation lands at least 100
    tolerances off on the first step"""
    D = XR.prepare(c)
    _, _, _, good = next(XR.trajectory(c, D))
    _, _, _, bad = next(XR.trajectory(c, D, leg=w))
    if c.T:
        good = dict(good, q_on_s=good["td"], q_on_sp=np.stack(good["q_on_sp"]), q_tg_sp=np.stack(good["q_tg_sp"])); bad = dict(bad, q_on_s=bad["td"], q_on_sp=np.stack(bad["q_on_sp"]), q_tg_sp=np.stack(bad["q_tg_sp"]))
    off = _off(c, D, bad, good)
    assert off >= 100, (c.name, w, off)


@pytest.mark.parametrize("c", XR.CASES, ids=IDS(XR.CASES))
def test_the_expanded_network_computes_the_same_function_in_fp64(c):
    """the exact companion's algebra: the kind-1 network on the zero-stuffed, block-diagonal kernel; its gradient read at the live taps is the layer's own"""
    D = XR.prepare(c); ex = XR.expand(D.net)
    assert not XR.general_layers(ex) and all(d.kind != abi.LAYER_CONV_DG for d in nn.lower(ex)[0])
    p1, t1 = XR.expand_params(D.net, D.p_on), XR.expand_params(D.net, D.p_tg)
    assert p1.dtype == np.float32 and np.count_nonzero(p1) == np.count_nonzero(D.p_on)
    batch = XR.ff_batch(c, D, D.idx[0]); g32 = float(np.float32(c.gamma))
    a = XR.ff_step(D.net, D.p_on, D.p_tg, batch, g32, True); b = XR.ff_step(ex, p1, t1, batch, g32, True)
    g = XR.contract_grads(D.net, b["grads"]); b = dict(b, grads=g, grad_norm=float(np.abs(g).max()))      # (the dead taps of the expanded kernel have gradients of their own: grad_norm is taken over the live ones)
    XR.legs_agree(a, b, rel=1e-12)
    np.testing.assert_array_equal(XR.contract_grads(D.net, p1), D.p_on)


# ------------------------------------------------------------------ the Python mirror
def test_dilation_1_groups_1_keeps_lowering_to_kind_1():
    for kw in (dict(), dict(pad=1), dict(stride=2, pad=(1, 0)), dict(dilation=1, groups=1), dict(dilation=(1, 1))):
        l = nn.Conv(3, 2, 4, nn.relu, **kw); d = nn.lower(nn.Chain(l, nn.Dense(4, 4)))[0][0]
        assert not l.general and (d.kind, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw) == (abi.LAYER_CONV, l.ph, l.pw, 2, 4, 3, 3), kw
        assert "dilation" not in repr(l) and "groups" not in repr(l)
    assert repr(nn.Conv(3, 2, 4, pad=1)) == "Conv((3, 3), 2 => 4, act=0, stride=(1, 1), pad=(1, 1))"


def test_lowering_packs_pad_dilation_and_groups():
    d = nn.lower(nn.Chain(nn.Conv((3, 2), 4, 6, nn.relu, stride=(2, 1), pad=(2, 0), dilation=(2, 1), groups=2), nn.Dense(4, 4)))[0][0]
    assert (d.kind, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw, d.act, d.stream) == (15, 4, 6, 3, 2, 2, 1, 1, 0) and abi.LAYER_CONV_DG == 15
    assert (d.n_in & 0xffff, d.n_in >> 16) == (2, 0) and (d.n_out & 0xff, (d.n_out >> 8) & 0xff, d.n_out >> 16) == (2, 1, 2)
    d = nn.lower(nn.Chain(nn.DepthwiseConv(3, 4, 8, pad=(0, 1), dilation=(1, 3)), nn.Dense(4, 4)))[0][0]
    assert (d.kind, d.cin, d.cout) == (15, 4, 8) and (d.n_in, d.n_out) == (1 << 16, 1 | (3 << 8) | (4 << 16))
    l = nn.Conv(3, 2, 4, pad=nn.SamePad(), dilation=2)      # SamePad() resolves to (k - 1) d / 2
    assert (l.ph, l.pw) == (2, 2) and "dilation=(2, 2), groups=1" in repr(l)
    assert (nn.Conv((3, 5), 2, 4, pad=nn.SamePad(), dilation=(2, 1)).ph, nn.Conv((3, 5), 2, 4, pad=nn.SamePad(), dilation=(2, 1)).pw) == (2, 2)
    assert nn.Conv(2, 2, 4, pad=nn.SamePad(), dilation=2).ph == 1      # an even kernel whose dilated extent is odd pads symmetrically
    assert nn.Conv(3, 2, 4, pad=4, dilation=2).ph == 4      # the largest pad: the dilated extent minus one


def test_parameter_shapes_order_fans_and_bson_round_trip(bson, tmp_path):
    net = nn.Chain(nn.DepthwiseConv(3, 4, 8, pad=1), nn.Conv((2, 3), 8, 6, nn.relu, groups=2, dilation=(1, 2)), nn.Dense(6 * 5 * 2, 4))
    dw, gc = net.layers[0], net.layers[1]
    assert dw.shapes() == [(8, 1, 3, 3), (8,)] and gc.shapes() == [(6, 4, 2, 3), (6,)]
    assert dw.fans() == (9, 72) and gc.fans() == (24, 36)      # nfan(kw, kh, cin ÷ g, cout) = (kh kw cin/g, kh kw cout)
    shapes = bson.julia_param_shapes(net)
    assert shapes == [((3, 3, 1, 8), 72), ((8,), 8), ((3, 2, 4, 6), 144), ((6,), 6), ((4, 60), 240), ((4,), 4)]
    p = nn.glorot_params(net, seed=2)
    assert p.size == sum(n for _, n in shapes) and np.abs(p[:72]).max() <= 0.5 * np.sqrt(24.0 / 81) and np.abs(p[:72]).max() > 0.4 * np.sqrt(24.0 / 81)
    assert not p[72:80].any() and np.abs(p[80:224]).max() <= 0.5 * np.sqrt(24.0 / 60)
    path = tmp_path / "q.bson"; bson.save_qnetwork(path, p, shapes)
    w, sizes = bson.load_qnetwork(path)
    np.testing.assert_array_equal(w, p); assert [tuple(x) for x in sizes] == [s for s, _ in shapes]


def test_python_side_refusals_carry_their_messages():
    R = lambda m: pytest.raises(abi.DQNError, match=m)
    with R(r"groups must be >= 1 and divide cin = 4 and cout = 6"):
        nn.Conv(3, 4, 6, groups=4)
    with R(r"groups must be >= 1 and divide cin = 3 and cout = 6"):
        nn.Conv(3, 3, 6, groups=2)
    with R(r"groups must be >= 1"):
        nn.Conv(3, 4, 4, groups=0)
    with R(r"dilation must be at least 1 per axis"):
        nn.Conv(3, 1, 4, dilation=0)
    with R(r"dilation must be at least 1 per axis"):
        nn.Conv(3, 1, 4, dilation=(2, -1))
    with R(r"dilation must be an int or a pair"):
        nn.Conv(3, 1, 4, dilation=(1, 1, 1))
    with R(r"pad \(5, 1\) is larger than the dilated kernel extent - 1 = \(4, 4\)"):
        nn.Conv(3, 1, 4, pad=(5, 1), dilation=2)
    with R(r"SamePad\(\) on an even kernel is an asymmetric pad"):      # (k - 1) d odd: the words the mirror already uses
        nn.Conv(2, 1, 4, pad=nn.SamePad(), dilation=(1, 3))
    with R(r"DepthwiseConv\(3, 4 => 6\): groups = cin must divide cout"):
        nn.DepthwiseConv(3, 4, 6)
    with R(r"dilation <= 255 and groups <= 32767"):
        nn.Conv(3, 1, 4, dilation=256)
    blk = lambda l: nn.Chain(nn.Conv(3, 1, 4, pad=1), nn.SkipConnection(nn.Chain(l, nn.Conv(3, 4, 4, pad=1)), "+"), nn.Dense(144, 4))
    for l in (nn.Conv(3, 4, 4, nn.relu, pad=2, dilation=2), nn.Conv(3, 4, 4, pad=1, groups=2), nn.DepthwiseConv(3, 4, 4, pad=1)):
        with R(r"a Conv with dilation != 1 or groups != 1 \(DepthwiseConv included\) inside a SkipConnection is not supported"):
            nn.lower(blk(l))
    with R(r"inside a SkipConnection is not supported"):      # ... and in a block on a feature vector
        nn.lower(nn.Chain(nn.Dense(6, 16), nn.SkipConnection(nn.Chain(nn.DepthwiseConv(1, 16, 16)), "+"), nn.Dense(16, 4)))
    duel = nn.DuelingNetwork(nn.Chain(nn.Conv(3, 1, 4)), nn.Chain(nn.Conv(3, 4, 4, dilation=2), nn.Dense(4, 1)), nn.Chain(nn.Dense(64, 4)))
    with R(r"dilation=\(2, 2\), groups=1\) is supported in the base chain only \(not in a value / advantage stream\)"):
        nn.lower(duel)


# ------------------------------------------------------------------ the shim and the header (static)
def test_julia_shim_reads_dilation_and_groups_and_refuses_by_name():
    src = open(os.path.join(ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    conv = src[src.index("elseif l isa Conv"):src.index("elseif l isa Flux.MaxPool")]
    assert "dil = l.dilation; g = l.groups" in conv and "if any(!=(1), dil) || g != 1" in conv      # the silent drop ends: both fields are read, and kind 15 only when one differs from 1
    assert conv.index("if any(!=(1), dil) || g != 1") < conv.index("return LayerDesc(15,") < conv.index("return LayerDesc(1,")
    # the packed slots, (W, H) order of l.dilation as of l.stride, the FULL channel count (size(l.weight, 3) is per group)
    assert "return LayerDesc(15, ACT[l.σ], stream, p[3] | (p[1] << 16), dil[2] | (dil[1] << 8) | (g << 16), cin * g, cout, kh, kw, l.stride[2], l.stride[1])" in conv
    for words in ("the dilation must be at least 1 per axis", "groups must be >= 1 and divide cin", "is larger than the dilated kernel extent - 1", "is supported in the base chain only (not in a value / advantage stream)"):
        assert re.search(r"\|\| throw\(\"DeepQLearningError: [^\n]*" + re.escape(words), conv), words
    skip = src[src.index("function lower_skip!"):src.index("lower_into!(descs, l, stream) =")]
    assert "is_general_conv(x) = x isa Conv && (any(!=(1), x.dilation) || x.groups != 1)" in src
    assert skip.index("any(is_general_conv, real) && throw(\"DeepQLearningError: a Conv with dilation != 1 or groups != 1") < skip.index("return lower_skip_map!(descs, l, stream, inner)")
    assert re.search(r"is_map_desc\(d\) = [^\n#]*d\.kind == 15", src)      # a skip block, a GroupNorm, a pool may stand behind the layer


def test_header_documents_kind_15_and_keeps_the_plan_version():
    hdr = open(os.path.join(ROOT, "include", "dqn_mi355x.h")).read()
    assert "DQN_LAYER_CONV_DG = 15" in hdr and re.search(r"#define DQN_PLAN_VERSION 3\b", hdr)
    assert "n_in = pad_h | pad_w << 16" in hdr and "n_out = dh | dw << 8 | g << 16" in hdr
    assert "(cout, cin/g, kh, kw)" in hdr and "0 <= pad_h <= (kh-1) dh" in hdr


# ------------------------------------------------------------------ the library's host-only entries: geometry, plan, refusals by layer index
def _L(kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, k=(0, 0), s=(0, 0)):
    d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, k[0], k[1], s[0], s[1]
    return d


def _dg(cin, cout, k=(3, 3), s=(1, 1), pad=(0, 0), dil=(1, 1), g=1, stream=0, act=1):
    return _L(15, stream=stream, act=act, n_in=pad[0] | (pad[1] << 16), n_out=dil[0] | (dil[1] << 8) | (g << 16), cin=cin, cout=cout, k=k, s=s)


def _plan(pkg, layers, obs=(1, 6, 6), B=8, **kw):
    return pkg.default_plan(layers, pkg.default_hparams(batch_size=B, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], buffer_size=64, **({"dueling": 0} | kw)))


def test_geometry_reaches_the_next_layer(pkg):
    dense = lambda n: _L(abi.LAYER_DENSE, n_in=n, n_out=4)
    assert len(_plan(pkg, [_dg(1, 4, dil=(2, 2)), dense(4 * 3 * 3)], obs=(1, 7, 7))) == 2      # (7 - 4 - 1) + 1 = 3
    assert len(_plan(pkg, [_dg(2, 4, k=(3, 2), s=(2, 1), pad=(2, 0), dil=(2, 1)), dense(4 * 5 * 5)], obs=(2, 9, 6))) == 2      # (9 + 4 - 4 - 1) / 2 + 1 = 5, (6 - 1 - 1) + 1 = 5
    assert len(_plan(pkg, [_dg(4, 8, pad=(1, 1), g=4), dense(8 * 36)], obs=(4, 6, 6))) == 2
    with pytest.raises(abi.DQNError, match=r"dense n_in 37 != incoming features 36"):
        _plan(pkg, [_dg(1, 4, dil=(2, 2)), dense(37)], obs=(1, 7, 7))
    with pytest.raises(abi.DQNError, match=r"unknown kind 16"):
        _plan(pkg, [_L(16), dense(4)])


@pytest.mark.parametrize("B", [8, 32, 128, 512])
def test_plan_default_reads_the_layers_own_K_and_N(pkg, B):
    """dqn_plan_default gives kind 15 the plan of the Conv with the same K = (cin/g) kh kw, N, kernel, stride, output map and batch: the inputs it reads today"""
    tail = lambda: [_L(abi.LAYER_CONV, act=1, cin=32, cout=32, k=(1, 1), s=(1, 1)), _L(abi.LAYER_DENSE, n_in=32 * 400, n_out=4)]
    front = lambda c: _L(abi.LAYER_CONV, act=1, cin=c, cout=c, k=(1, 1), s=(1, 1))
    a = _plan(pkg, [front(32), _dg(32, 32, pad=(1, 1), g=2)] + tail(), obs=(32, 20, 20), B=B)
    b = _plan(pkg, [front(16), _L(abi.LAYER_CONV, act=1, n_in=1, n_out=1, cin=16, cout=32, k=(3, 3), s=(1, 1))] + tail(), obs=(16, 20, 20), B=B)
    assert a[1:] == b[1:], (a, b)


def test_refusals_of_build_layers(pkg):
    dense = lambda n, stream=0: _L(abi.LAYER_DENSE, stream=stream, n_in=n, n_out=4)
    R = lambda m: pytest.raises(abi.DQNError, match=m)
    with R(r"layer 0: Conv groups = 4 must be >= 1 and divide cin = 4 and cout = 6"):
        _plan(pkg, [_dg(4, 6, g=4), dense(96)], obs=(4, 6, 6))
    with R(r"layer 0: Conv groups = 2 must be >= 1 and divide cin = 3 and cout = 6"):
        _plan(pkg, [_dg(3, 6, g=2), dense(96)], obs=(3, 6, 6))
    with R(r"layer 0: Conv groups = 0 must be >= 1"):
        _plan(pkg, [_dg(4, 4, g=0), dense(64)], obs=(4, 6, 6))
    with R(r"layer 0: Conv dilation \(0, 1\) must be at least 1 per axis"):
        _plan(pkg, [_dg(1, 4, dil=(0, 1)), dense(64)])
    with R(r"layer 0: dilated / grouped Conv: the packed slots n_in = -1 .* must not be negative"):
        _plan(pkg, [_L(15, act=1, n_in=-1, n_out=1 | (1 << 8) | (1 << 16), cin=1, cout=4, k=(3, 3), s=(1, 1)), dense(64)])
    with R(r"layer 0: Conv pad \(5, 1\) is larger than the dilated kernel extent - 1 = \(4, 4\)"):
        _plan(pkg, [_dg(1, 4, pad=(5, 1), dil=(2, 2)), dense(64)])
    with R(r"layer 0: Conv kernel \(3, 3\) with dilation \(3, 3\) spans \(7, 7\) and does not fit the 6x6 input map extended by pad \(0, 0\)"):
        _plan(pkg, [_dg(1, 4, dil=(3, 3)), dense(64)])
    with R(r"layer 0: dilated / grouped Conv cin 2 != incoming channels 1"):
        _plan(pkg, [_dg(2, 4, g=2), dense(64)])
    with R(r"layer 2: a Conv with dilation \(2, 2\) / groups 1 is supported in the base chain only \(not in a value / advantage stream\)"):
        _plan(pkg, [_L(abi.LAYER_CONV, cin=1, cout=1, k=(1, 1), s=(1, 1)), _L(abi.LAYER_DENSE, 1, n_in=36, n_out=1), _dg(1, 2, dil=(2, 2), stream=2), dense(8, 2)], dueling=1)
    # inside either skip-block kind
    conv = lambda pad=1: _L(abi.LAYER_CONV, act=1, n_in=pad, n_out=pad, cin=4, cout=4, k=(3, 3), s=(1, 1))
    with R(r"layer 3: the convolutional skip block holds a Conv with dilation \(2, 2\) / groups 1 \(layer 1\); its inner layers are Conv layers with pad != 0, dilation 1 and groups 1 only"):
        _plan(pkg, [_L(abi.LAYER_CONV, n_in=1, n_out=1, cin=1, cout=4, k=(3, 3), s=(1, 1)), _dg(4, 4, pad=(2, 2), dil=(2, 2)), conv(), _L(abi.LAYER_SKIPADD_MAP, cin=2), dense(144)])
    with R(r"layer 2: the skip block holds a Conv with dilation \(1, 1\) / groups 4 \(layer 1\); its inner layers are Dense, LayerNorm and Dropout layers only"):
        _plan(pkg, [_L(abi.LAYER_CONV, n_in=1, n_out=1, cin=1, cout=4, k=(3, 3), s=(1, 1)), _dg(4, 4, pad=(1, 1), g=4), _L(abi.LAYER_SKIPADD, cin=1), dense(144)])
    # accepted: as the ENTRY of a convolutional skip block, the largest pad, the output layer of a 1x1 map
    assert len(_plan(pkg, [_dg(1, 4, pad=(2, 2), dil=(2, 2)), conv(), conv(), _L(abi.LAYER_SKIPADD_MAP, cin=2), dense(144)])) == 5
    assert len(_plan(pkg, [_dg(1, 4, pad=(4, 4), dil=(2, 2)), dense(4 * 10 * 10)])) == 2
    assert len(_plan(pkg, [_dg(2, 4, k=(3, 3), dil=(2, 2), g=2, act=0)], obs=(2, 5, 5))) == 1
