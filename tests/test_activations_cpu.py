"""CPU: the seven further activations (leakyrelu, elu, selu, softplus, softsign, relu6, hardtanh) in the fp64 reference the GPU tests (test_activations_gpu.py) stand on --
known values, its two legs against each other along three steps of every case, the margin and occupancy rules of the table's seeds, and the proof that the tests can
tell five wrong engines from the law --, then in the Python mirror, the ABI header and the library's host-side validation (no GPU: dqn_plan_default), and the Julia shim."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import activation_reference as AR

ROOT = ge.ROOT
IDS = lambda cs: [c.name for c in cs]


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "_abi"))


# ------------------------------------------------------------------ the fp64 reference
KNOWN = [(AR.SELU, 1.0, 1.0507009873554805), (AR.SELU, -1.0, -1.1113307378125625), (AR.ELU, -1.0, -0.6321205588285577), (AR.SOFTPLUS, 0.0, math.log(2.0)),
         (AR.SOFTSIGN, 3.0, 0.75), (AR.LEAKYRELU, -2.0, -0.02), (AR.RELU6, 7.0, 6.0), (AR.HARDTANH, -3.0, -1.0)]


@pytest.mark.parametrize("a,x,want", KNOWN, ids=[f"{AR.NAMES[a]}({x:g})" for a, x, _ in KNOWN])
def test_known_values(a, x, want):
    """both legs, to 1e-15"""
    assert abs(float(AR.act_np(np.array([x]), a)[0]) - want) <= 1e-15
    assert abs(float(AR.act_torch(torch.tensor([x], dtype=torch.float64), a)[0]) - want) <= 1e-15


def test_derivative_from_the_output_is_the_derivative():
    """dact_np -- a function of y alone -- against torch float64 autograd of torch.nn.functional's functions on a grid that straddles every kink (off the kinks themselves)"""
    x = np.concatenate([np.linspace(-9.0, 9.0, 721) + 1e-3, [-30.0, 30.0]])
    for a in range(11):
        t = torch.tensor(x, requires_grad=True)
        y = AR.act_torch(t, a); y.sum().backward()
        got = AR.dact_np(np.ones_like(x), AR.act_np(x, a), a)
        assert np.abs(got - t.grad.numpy()).max() <= 1e-14, AR.NAMES[a]
        assert np.abs(AR.act_np(x, a) - y.detach().numpy()).max() <= 1e-14, AR.NAMES[a]
    assert AR.LAMBDA_ALPHA == AR.LAMBDA * AR.ALPHA


@pytest.mark.parametrize("c", AR.ALL, ids=IDS(AR.ALL))
def test_legs_agree_and_the_seed_keeps_the_rules(c):
    """torch autograd over torch.nn.functional and the NumPy closed forms with the derivative-from-y column: 1e-10 relative on every quantity along the three steps of the
    case; along the same steps the fixed seed keeps every pre-activation on s RELU_MARGIN off the kinks of its activation, one twentieth of the layer's units in every piece
    of every piecewise activation, the LayerNorm's sigma and the argmax gap; no gradient block is dead on the first step"""
    D = AR.data(c)
    worst = [np.inf, 1.0, np.inf, np.inf]
    for k, p, batch, o in AR.trajectory(c, D):
        AR.legs_agree(o, AR.step(c, D, p, batch, k, leg="numpy"))
        m, occ, sg = AR.rules(D.net, p, batch[0], AR.masks_of(D.net, k, c.B, c.T), batch[5] if c.T else None)
        qsel = o["q_on_sp"] if c.dq else o["q_tg_sp"]
        worst = [min(worst[0], m), min(worst[1], occ), min(worst[2], sg), min(worst[3], AR.LR._gap(np.concatenate(qsel) if c.T else qsel))]
        if k == 0:
            AR.check_grads(D.net, o["grads"], o["grads"], live=True)
    assert worst[0] > AR.RELU_MARGIN and worst[1] >= AR.OCCUPANCY and worst[2] >= AR.LR.SIGMA_MIN and worst[3] > AR.GAP, (c.name, worst)
    acts = {l.act for l in AR.nn.all_layers(D.net) if l.kind in ("dense", "conv", "layernorm")}
    assert c.act in acts


def test_the_table_covers_every_activation_in_every_family():
    assert {(c.family, c.act) for c in AR.ALL} == {(f, a) for f in AR.FAMILIES for a in AR.NEW}
    assert set(AR.KINKS) == {AR.RELU, AR.LEAKYRELU, AR.SELU, AR.RELU6, AR.HARDTANH} and AR.KINKS[AR.RELU6] == (0.0, 6.0) and AR.KINKS[AR.HARDTANH] == (-1.0, 1.0)
    assert set(AR.PIECES) == {AR.LEAKYRELU, AR.ELU, AR.SELU, AR.RELU6, AR.HARDTANH}


TELL_CASES = [(w, c) for w, a in AR.WRONG.items() for c in AR.ALL if c.act == a]


@pytest.mark.parametrize("wrong,c", TELL_CASES, ids=[f"{w}-{c.name}" for w, c in TELL_CASES])
def test_the_tests_can_tell(wrong, c):
    """leakyrelu with slope 0.1, elu differentiated as relu, selu without lambda, softplus differentiated as y (1 - y), relu6 without its upper kink: each is off by more
    than 100 tolerances of some compared quantity on every case that uses the activation"""
    d = AR.tell_distance(c, wrong)
    assert d > AR.TELL, (wrong, c.name, d)


# ------------------------------------------------------------------ the mirror, the header, the host-side validation
def test_header_and_abi_agree_on_the_eleven_codes(mods):
    nn, abi = mods
    hdr = open(os.path.join(ROOT, "include", "dqn_mi355x.h")).read()
    for code, name in enumerate(AR.NAMES):
        assert int(re.search(r"DQN_ACT_%s\s*=\s*(\d+)" % name.upper(), hdr).group(1)) == code == getattr(abi, "ACT_" + name.upper()) == getattr(nn, name)
    assert int(re.search(r"#define DQN_PLAN_VERSION\s+(\d+)", hdr).group(1)) == 3      # no summation order changed


def test_lowering_emits_codes_4_to_10(mods):
    nn, abi = mods
    new = [nn.leakyrelu, nn.elu, nn.selu, nn.softplus, nn.softsign, nn.relu6, nn.hardtanh]
    assert new == [4, 5, 6, 7, 8, 9, 10] == list(AR.NEW)
    layers, _ = nn.lower(nn.Chain(*[nn.Dense(6, 6, a) for a in new], nn.Dense(6, 4)))
    assert [l.act for l in layers] == new + [0]
    layers, _ = nn.lower(nn.Chain(nn.Conv(3, 1, 4, nn.elu, pad=1), nn.MeanPool(2), nn.flattenbatch, nn.Dense(36, 16, nn.selu), nn.LayerNorm(16, nn.hardtanh), nn.Dense(16, 4)))
    assert [l.act for l in layers] == [5, 0, 6, 10, 0]
    d = nn.lower(nn.create_dueling_network(nn.Chain(nn.Dense(6, 8, nn.relu6), nn.Dense(8, 4, nn.softsign))))[0]
    assert [(l.stream, l.act) for l in d] == [(1, 9), (1, 0), (2, 9), (2, 8)]      # the value head is a fresh Dense(8, 1)


def test_the_mirror_refuses_by_name(mods):
    nn, abi = mods
    for bad in (nn.gelu, nn.swish, nn.mish, nn.hardswish):
        with pytest.raises(abi.DQNError, match=r"DeepQLearningError: unsupported activation %s on Dense\(6, 8, act=%s\): %s is not monotone, so its derivative needs the "
                                               r"pre-activation, and the MI355X engine keeps only each layer's output y" % (bad.name, bad.name, bad.name)) as ei:
            nn.lower(nn.Chain(nn.Dense(6, 8, bad), nn.Dense(8, 4)))
        assert "supported: identity / relu / tanh / sigmoid / leakyrelu / elu / selu / softplus / softsign / relu6 / hardtanh" in str(ei.value)
    with pytest.raises(abi.DQNError, match=r"unsupported activation gelu on LayerNorm\(8"):
        nn.lower(nn.Chain(nn.Dense(6, 8), nn.LayerNorm(8, nn.gelu), nn.Dense(8, 4)))
    with pytest.raises(abi.DQNError, match=r"unsupported activation mish on Conv\("):
        nn.lower(nn.Chain(nn.Conv(3, 1, 4, nn.mish), nn.flattenbatch, nn.Dense(64, 4)))
    for bad in (11, -1, 2.0, "elu", None, (lambda x: x)):
        with pytest.raises(abi.DQNError, match=r"DeepQLearningError: unsupported activation .* \(supported: identity / relu / .* / hardtanh, with NNlib's default parameters only\)"):
            nn.lower(nn.Chain(nn.Dense(6, 8, bad), nn.Dense(8, 4)))


def _L(abi, kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, k=0, s=0):
    d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, k, k, s, s
    return d


def test_host_side_validation_without_a_gpu(pkg, mods):
    """dqn_plan_default runs build_layers on the host: Dense, Conv and LayerNorm take the codes 0..10 and refuse every other by layer index and code; the RNN cell keeps
    its four"""
    nn, abi = mods
    D, CV, LN, RNN = abi.LAYER_DENSE, abi.LAYER_CONV, abi.LAYER_LAYERNORM, abi.LAYER_RNN
    plan = lambda layers, obs=(6, 1, 1), **kw: pkg.default_plan(layers, pkg.default_hparams(batch_size=8, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], buffer_size=64, **({"dueling": 0} | kw)))
    head = _L(abi, D, n_in=16, n_out=4)
    for a in range(11):
        plan([_L(abi, D, act=a, n_in=6, n_out=16), _L(abi, D, act=a, n_in=16, n_out=4)])
        plan([_L(abi, CV, act=a, cin=1, cout=4, k=3, s=1), _L(abi, D, n_in=64, n_out=4)], obs=(1, 6, 6))
        plan([_L(abi, D, n_in=6, n_out=16), _L(abi, LN, act=a, n_in=16, n_out=16), head])
    with pytest.raises(abi.DQNError, match=r"layer 0: Dense activation 11 is not one of DQN_ACT_\* \(0\.\.10\)"):
        plan([_L(abi, D, act=11, n_in=6, n_out=16), head])
    with pytest.raises(abi.DQNError, match=r"layer 1: Dense activation -3 is not one of DQN_ACT_\*"):
        plan([_L(abi, D, n_in=6, n_out=16), _L(abi, D, act=-3, n_in=16, n_out=4)])
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv activation -1 is not one of DQN_ACT_\* \(0\.\.10\)"):
        plan([_L(abi, CV, act=-1, cin=1, cout=4, k=3, s=1), _L(abi, D, n_in=64, n_out=4)], obs=(1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"layer 2: Dense activation 12 is not one of DQN_ACT_\*"):      # in a stream of a dueling network too
        plan([_L(abi, D, n_in=6, n_out=16), _L(abi, D, stream=1, n_in=16, n_out=1), _L(abi, D, stream=2, act=12, n_in=16, n_out=4)], dueling=1)
    with pytest.raises(abi.DQNError, match=r"layer 1: LayerNorm activation 11 is not one of DQN_ACT_\*"):
        plan([_L(abi, D, n_in=6, n_out=16), _L(abi, LN, act=11, n_in=16, n_out=16), head])
    rnn = lambda a: [_L(abi, RNN, act=a, n_in=6, n_out=16), head]
    for a in range(4):
        plan(rnn(a), recurrence=1, trace_length=3)
    for a in (5, 10):
        with pytest.raises(abi.DQNError, match=r"layer 0: RNN activation %d is not one of DQN_ACT_\*" % a):
            plan(rnn(a), recurrence=1, trace_length=3)
    with pytest.raises(abi.DQNError, match=r"layer 0: RNN activation 5"):      # ... through the mirror as well: the cell's sigma is lowered like any code
        layers, _ = nn.lower(nn.Chain(nn.RNN(6, 16, nn.elu), nn.Dense(16, 4)))
        plan(layers, recurrence=1, trace_length=3)


def test_julia_shim_knows_the_eleven_names_and_explains_every_refusal():
    src = open(os.path.join(ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    m = re.search(r"const ACT = Dict\(([^)]*)\)", src)
    assert m and {k.strip(): int(v) for k, v in (kv.split("=>") for kv in m.group(1).split(","))} == {n: i for i, n in enumerate(AR.NAMES)}
    assert re.search(r"const ACT_NEEDS_X = \(gelu, swish, mish, hardswish\)", src)
    assert re.search(r"function lower_layer\(l, stream\)::LayerDesc\n\s*check_act\(l\)\n", src)      # before any ACT[...] lookup
    body = src[src.index("function check_act(l)"):src.index("function lower_layer")]
    assert len(re.findall(r'throw\("DeepQLearningError: unsupported activation', body)) == 2
    assert "not monotone" in body and "needs the pre-activation" in body and "default parameters only" in body and "x -> leakyrelu(x, 0.2f0)" in body
    assert body.count("$(ACT_SUPPORTED)") == 2 and " / ".join(AR.NAMES) in src
    assert not re.search(r"ACT\[", re.sub(r"#.*", "", src[:src.index("function lower_layer")]))      # no lookup in front of the check
