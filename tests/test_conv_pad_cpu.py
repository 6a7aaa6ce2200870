"""CPU: padded convolutions (Flux Conv pad / SamePad()) in the Python mirror, the ABI header, the Julia shim and the host-only entries of the library
(dqn_plan_default: build_layers' geometry and refusals; dqn_n_params needs an engine and is checked in test_conv_pad_gpu.py), and the fp64 reference the GPU tests (test_conv_pad_gpu.py) stand on: its two
legs against each other on the whole case table, and the margin seeds of that table."""
import importlib
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import conv_pad_reference as CR
import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_reference as FR

ROOT = ge.ROOT
IDS = lambda cs: [c.name for c in cs]


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "_abi", "bson"))


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("c", CR.CASES, ids=IDS(CR.CASES))
def test_reference_legs_agree_and_the_seed_keeps_the_margins(c):
    """NumPy (np.pad + the oracle's pad-0 conv + crop) and torch autograd (F.conv2d's padding) share no padding code: 1e-10 relative on every quantity along the
    fp64 trajectory of the case's three steps.  prepare() asserts the case's fixed seed against the argmax, relu and MaxPool margins."""
    E.check_legs_along_trajectory(c)


def test_the_table_holds_the_cases_and_every_first_layer_case_is_padded():
    assert set(CR.FIRST_LAYER) <= set(CR.BY_NAME) and len(CR.CASES) == 13
    for name in CR.FIRST_LAYER:
        assert any(CR.pad_of(E.network(CR.BY_NAME[name]).base[0])), name
    for c in CR.CASES:
        assert any(any(CR.pad_of(l)) for l in E.network(c).base), c.name


def test_recurrent_case_seed_keeps_the_margin(mods):
    assert FR.rec_trajectory_ok(mods[0], CR.REC)


def test_padded_output_of_the_reference_is_the_pad0_conv_on_the_extended_map():
    """the definition itself, on the NumPy leg: stride 2 drops part of the trailing padding"""
    rng = np.random.default_rng(0); l = CR.PConv(3, 2, 4, CR.TANH, stride=2, pad=1)
    x = rng.standard_normal((3, 2, 7, 8)); W = rng.standard_normal((4, 2, 3, 3)); b = rng.standard_normal(4)
    y = FR._fwd([l], [W, b], x)[0]
    assert y.shape == (3, 4, 4, 4) == (3,) + l.out_shape((2, 7, 8))
    np.testing.assert_array_equal(y, O.layer_forward(O.Conv(3, 2, 4, CR.TANH, 2), np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1))), W, b)[0])


# ------------------------------------------------------------------ the Python mirror
def test_lowering_of_int_tuple_4tuple_and_samepad(mods):
    nn, abi, _ = mods
    def desc(**kw):
        k = kw.pop("k", 3)
        return nn.lower(nn.Chain(nn.Conv(k, 2, 4, nn.relu, **kw), nn.Dense(4, 4)))[0][0]
    d = desc(pad=1)
    assert (d.kind, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw) == (abi.LAYER_CONV, 1, 1, 2, 4, 3, 3, 1, 1)
    d = desc(k=(3, 5), pad=(1, 2), stride=(2, 1))
    assert (d.n_in, d.n_out, d.kh, d.kw, d.sh, d.sw) == (1, 2, 3, 5, 2, 1)
    d = desc(k=(3, 5), pad=(2, 2, 1, 1))      # Flux's 4-tuple: the first pair belongs to the W axis
    assert (d.n_in, d.n_out) == (1, 2)
    d = desc(k=(3, 5), pad=nn.SamePad())
    assert (d.n_in, d.n_out) == (1, 2)
    d = desc(k=1, pad=nn.SamePad())
    assert (d.n_in, d.n_out) == (0, 0)
    d = desc()      # pad 0: the descriptor every earlier caller built
    assert (d.n_in, d.n_out) == (0, 0)
    assert "pad=(1, 2)" in repr(nn.Conv((3, 5), 2, 4, pad=(1, 2)))


def test_python_side_refusals_carry_their_messages(mods):
    nn, abi, _ = mods
    with pytest.raises(abi.DQNError, match=r"SamePad\(\) on an even kernel is an asymmetric pad"):
        nn.Conv(4, 1, 4, pad=nn.SamePad())
    with pytest.raises(abi.DQNError, match=r"SamePad\(\) on an even kernel is an asymmetric pad"):
        nn.Conv((3, 2), 1, 4, pad=nn.SamePad())
    with pytest.raises(abi.DQNError, match=r"Conv\(\(3, 3\).*asymmetric pad \(lo != hi"):
        nn.Conv(3, 1, 4, pad=(1, 2, 1, 1))
    with pytest.raises(abi.DQNError, match=r"pad \(-1, 0\) must not be negative"):
        nn.Conv(3, 1, 4, pad=(-1, 0))
    with pytest.raises(abi.DQNError, match=r"pad \(3, 1\) is larger than kernel - 1 = \(2, 2\)"):
        nn.Conv(3, 1, 4, pad=(3, 1))
    with pytest.raises(abi.DQNError, match=r"pad must be an int, a 2-tuple, a symmetric 4-tuple or SamePad\(\)"):
        nn.Conv(3, 1, 4, pad=(1, 1, 1))
    with pytest.raises(abi.DQNError, match=r"MaxPool with pad=0 only"):      # padded pooling stays refused
        nn.MaxPool(2, pad=1)


def test_pad_is_no_parameter(mods, pkg):
    nn, abi, bson = mods
    a = nn.Chain(nn.Conv(3, 2, 4, nn.relu, pad=1), nn.Dense(4 * 6 * 6, 4)); b = nn.Chain(nn.Conv(3, 2, 4, nn.relu), nn.Dense(4 * 4 * 4, 4))
    assert bson.julia_param_shapes(a)[:2] == bson.julia_param_shapes(b)[:2] == [((3, 3, 2, 4), 72), ((4,), 4)]
    np.testing.assert_array_equal(nn.glorot_params(a, seed=2)[:76], nn.glorot_params(b, seed=2)[:76])


# ------------------------------------------------------------------ the shim and the header (static)
def test_julia_shim_lowers_the_pad():
    src = open(os.path.join(ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    conv = src[src.index("elseif l isa Conv"):src.index("elseif l isa Flux.MaxPool")]
    assert "pad=0 only" not in conv and not re.search(r"all\(==\(0\), l\.pad\)", conv)      # no blanket pad refusal for Conv
    assert re.search(r"\(p\[1\] == p\[2\] && p\[3\] == p\[4\]\) \|\| throw\(\"DeepQLearningError: [^\"]*symmetric pad[^\"]*asymmetric[^\"]*\"\)", conv)      # lo != hi is refused by name
    assert re.search(r"p = length\(l\.pad\) == 4 \? l\.pad :", conv)
    # (pad_h, pad_w) in the n_in, n_out slots: the first pair of l.pad belongs to the W axis, as l.stride[1] does
    assert re.search(r"return LayerDesc\(1, ACT\[l\.σ\], stream, p\[3\], p\[1\], cin, cout, kh, kw, l\.stride\[2\], l\.stride\[1\]\)", conv)
    for name in ("MaxPool", "MeanPool"):      # padded pooling stays refused
        assert re.search(r"any\(!=\(0\), l\.pad\) && throw\(\"DeepQLearningError: [^\"]*%s with pad=0 only" % name, src)


def test_header_documents_the_pad_slots():
    hdr = open(os.path.join(ROOT, "include", "dqn_mi355x.h")).read()
    assert re.search(r"for DQN_LAYER_CONV the slots n_in / n_out carry pad_h / pad_w", hdr)
    assert re.search(r"0 <= pad_h <= kh - 1", hdr) and re.search(r"#define DQN_PLAN_VERSION 3\b", hdr)


# ------------------------------------------------------------------ the library's host-only entries: geometry, plan, parameter count, refusals
def _hp(pkg, obs, B=32, nA=4, **kw):
    return pkg.default_hparams(batch_size=B, n_actions=nA, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], dueling=0, buffer_size=64, **kw)


def _L(abi, kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, k=(0, 0), s=(0, 0)):
    d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, k[0], k[1], s[0], s[1]
    return d


@pytest.mark.parametrize("B", [8, 32, 128, 512])
@pytest.mark.parametrize("geo", [((4, 20, 20), (3, 3), (1, 1), (1, 1), 32), ((4, 84, 84), (8, 8), (4, 4), (2, 2), 32), ((2, 9, 12), (3, 5), (2, 1), (1, 2), 16), ((16, 10, 10), (3, 3), (1, 1), (1, 0), 64)],
                         ids=["same3", "nature8_pad2", "rect", "one_axis"])
def test_plan_default_of_a_padded_layer_is_the_pad0_plan_on_the_extended_observation(pkg, mods, geo, B):
    nn, abi, _ = mods
    (c, h, w), k, s, (ph, pw), cout = geo
    oh, ow = (h + 2 * ph - k[0]) // s[0] + 1, (w + 2 * pw - k[1]) // s[1] + 1
    tail = lambda: [_L(abi, abi.LAYER_CONV, act=1, cin=cout, cout=cout, k=(1, 1), s=(1, 1)), _L(abi, abi.LAYER_DENSE, n_in=cout * oh * ow, n_out=4)]      # the padded layer has a consumer conv too
    padded = [_L(abi, abi.LAYER_CONV, act=1, n_in=ph, n_out=pw, cin=c, cout=cout, k=k, s=s)] + tail()
    plain = [_L(abi, abi.LAYER_CONV, act=1, cin=c, cout=cout, k=k, s=s)] + tail()
    pa = pkg.default_plan(padded, _hp(pkg, (c, h, w), B)); pb = pkg.default_plan(plain, _hp(pkg, (c, h + 2 * ph, w + 2 * pw), B))
    assert pa == pb, (pa, pb)
    # ... and behind another layer (the layer has a dX): the same rule
    front = lambda: _L(abi, abi.LAYER_CONV, act=1, cin=c, cout=c, k=(1, 1), s=(1, 1))
    mid_p = [front(), _L(abi, abi.LAYER_CONV, act=1, n_in=ph, n_out=pw, cin=c, cout=cout, k=k, s=s), _L(abi, abi.LAYER_DENSE, n_in=cout * oh * ow, n_out=4)]
    mid_0 = [front(), _L(abi, abi.LAYER_CONV, act=1, cin=c, cout=cout, k=k, s=s), _L(abi, abi.LAYER_DENSE, n_in=cout * oh * ow, n_out=4)]
    assert pkg.default_plan(mid_p, _hp(pkg, (c, h, w), B))[1:] == pkg.default_plan(mid_0, _hp(pkg, (c, h + 2 * ph, w + 2 * pw), B))[1:]


def test_refusals_of_build_layers(pkg, mods):
    nn, abi, _ = mods
    conv = lambda ph, pw, k=(3, 3), s=(1, 1), stream=0: _L(abi, abi.LAYER_CONV, stream=stream, n_in=ph, n_out=pw, cin=1, cout=2, k=k, s=s)
    plan = lambda layers, obs=(1, 6, 6), **kw: pkg.default_plan(layers, pkg.default_hparams(batch_size=8, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], buffer_size=64, **({"dueling": 0} | kw)))
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv pad \(3, 1\) is larger than kernel - 1 = \(2, 2\)"):
        plan([conv(3, 1), _L(abi, abi.LAYER_DENSE, n_in=2 * 10 * 6, n_out=4)])
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv pad \(1, 5\) is larger than kernel - 1 = \(2, 4\)"):
        plan([conv(1, 5, k=(3, 5)), _L(abi, abi.LAYER_DENSE, n_in=8, n_out=4)])
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv pad \(-1, 0\) must not be negative"):
        plan([conv(-1, 0), _L(abi, abi.LAYER_DENSE, n_in=8, n_out=4)])
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv kernel \(5, 5\) / stride \(1, 1\) does not fit the 2x2 input map extended by pad \(1, 1\)"):
        plan([conv(1, 1, k=(5, 5)), _L(abi, abi.LAYER_DENSE, n_in=8, n_out=4)], obs=(1, 2, 2))
    with pytest.raises(abi.DQNError, match=r"layer 2: Conv with pad \(1, 1\) is supported in the base chain only"):
        plan([_L(abi, abi.LAYER_CONV, cin=1, cout=1, k=(1, 1), s=(1, 1)), _L(abi, abi.LAYER_DENSE, 1, n_in=36, n_out=1), conv(1, 1, stream=2), _L(abi, abi.LAYER_DENSE, 2, n_in=72, n_out=4)], dueling=1)
    with pytest.raises(abi.DQNError, match=r"conv kernel/stride does not fit the 2x2 input"):      # pad 0: the message it always had
        plan([conv(0, 0), _L(abi, abi.LAYER_DENSE, n_in=8, n_out=4)], obs=(1, 2, 2))
    # accepted: the largest pad, and a kernel that fits only the extended map
    assert len(plan([conv(2, 2), _L(abi, abi.LAYER_DENSE, n_in=2 * 8 * 8, n_out=4)])) == 2
    assert len(plan([conv(1, 1), _L(abi, abi.LAYER_DENSE, n_in=2 * 2 * 2, n_out=4)], obs=(1, 2, 2))) == 2
    with pytest.raises(abi.DQNError, match=r"dense n_in 9 != incoming features 8"):      # the padded geometry reaches the next layer: (2 + 2 - 3) + 1 = 2
        plan([conv(1, 1), _L(abi, abi.LAYER_DENSE, n_in=9, n_out=4)], obs=(1, 2, 2))
