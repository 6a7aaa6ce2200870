"""CPU: Flux LayerNorm layers in the Python mirror, the ABI header, the library's host-side validation (no GPU: dqn_plan_default), BSON and the Julia shim, and the fp64
reference the GPU tests (test_layernorm_gpu.py) stand on: its two legs against each other on every case, the hand-written gradient against central differences, the
case that tells Flux's law from torch's, and the margin seeds of the table."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import layernorm_reference as LR

ROOT = ge.ROOT
ALL = LR.CASES + LR.REC_CASES
IDS = lambda cs: [c.name for c in cs]


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "_abi", "bson"))


def _bits(eps):
    return int(np.float32(eps).view(np.int32))


def test_enum_value_matches_the_header(mods):
    nn, abi, _ = mods
    hdr = open(os.path.join(ROOT, "include", "dqn_mi355x.h")).read()
    assert int(re.search(r"DQN_LAYER_LAYERNORM\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_LAYERNORM == 7


def test_lowering(mods):
    nn, abi, _ = mods
    net = nn.Chain(nn.Dense(6, 16, nn.relu), nn.LayerNorm(16), nn.Dense(16, 8, nn.tanh), nn.LayerNorm(8, nn.sigmoid, eps=0.5), nn.Dense(8, 4))
    layers, dueling = nn.lower(net)
    assert not dueling and [l.kind for l in layers] == [abi.LAYER_DENSE, abi.LAYER_LAYERNORM, abi.LAYER_DENSE, abi.LAYER_LAYERNORM, abi.LAYER_DENSE]
    a, b = layers[1], layers[3]
    assert abi.LAYER_LAYERNORM == 7
    assert (a.n_in, a.n_out, a.act, a.stream, a.cin) == (16, 16, abi.ACT_IDENTITY, abi.STREAM_BASE, _bits(1e-5)) and a.cin == 0x3727C5AC
    assert (b.n_in, b.n_out, b.act, b.stream, b.cin) == (8, 8, abi.ACT_SIGMOID, abi.STREAM_BASE, 0x3F000000)
    for l in (a, b):
        assert (l.cout, l.kh, l.kw, l.sh, l.sw) == (0, 0, 0, 0, 0)      # every other slot is 0


def test_shapes_initialisation_and_bson_round_trip(mods, tmp_path):
    nn, abi, bson = mods
    net = nn.Chain(nn.Dense(6, 5, nn.relu), nn.LayerNorm(5), nn.Dense(5, 4))
    assert net.layers[1].shapes() == [(5,), (5,)]
    p = nn.glorot_params(net, seed=3)
    assert p.size == 6 * 5 + 5 + 5 + 5 + 5 * 4 + 4
    np.testing.assert_array_equal(p[35:40], np.ones(5, np.float32)); np.testing.assert_array_equal(p[40:45], np.zeros(5, np.float32))      # Flux Scale(n): ones, then zeros
    shapes = bson.julia_param_shapes(net)
    assert shapes == [((5, 6), 30), ((5,), 5), ((5,), 5), ((5,), 5), ((4, 5), 20), ((4,), 4)]      # Flux.params order: W, b, scale, bias, W, b
    p = (p + np.arange(p.size, dtype=np.float32)).astype(np.float32)
    path = str(tmp_path / "qnetwork.bson")
    bson.save_qnetwork(path, p, shapes)
    flat, sizes = bson.load_qnetwork(path)
    np.testing.assert_array_equal(flat, p)
    assert [tuple(s) for s in sizes] == [s for s, _ in shapes]


def test_dueling_split_leaves_the_layer_in_the_base_chain(mods):
    nn, abi, _ = mods
    d = nn.create_dueling_network(nn.Chain(nn.Dense(6, 16, nn.relu), nn.LayerNorm(16), nn.Dense(16, 8, nn.relu), nn.Dense(8, 4)))
    assert [l.kind for l in d.base] == ["dense", "layernorm"] and [l.kind for l in d.val] == ["dense", "dense"] and [l.kind for l in d.adv] == ["dense", "dense"]
    layers, dueling = nn.lower(d)
    assert dueling and [(l.kind, l.stream) for l in layers] == [(0, 0), (7, 0), (0, 1), (0, 1), (0, 2), (0, 2)]
    d2 = nn.create_dueling_network(nn.Chain(nn.Dense(6, 16, nn.relu), nn.LayerNorm(16), nn.Dense(16, 4)))      # the trailing Dense run stops at the layer: the join sits on it
    assert [l.kind for l in d2.base] == ["dense", "layernorm"] and d2.val.layers[0].n_out == 1


def test_the_mirror_refuses_by_name(mods):
    nn, abi, _ = mods
    with pytest.raises(abi.DQNError, match=r"LayerNorm\(16; affine=false\) is not supported"):
        nn.LayerNorm(16, affine=False)
    with pytest.raises(abi.DQNError, match=r"LayerNorm\(size=\(4, 4\)\): a tuple size"):
        nn.LayerNorm((4, 4))
    with pytest.raises(abi.DQNError, match=r"LayerNorm\(1\): n must be >= 2"):
        nn.LayerNorm(1)
    for bad in (0.0, -1e-5, float("inf"), float("nan"), 1e39):
        with pytest.raises(abi.DQNError, match=r"LayerNorm\(8; eps=.*\): eps must be finite and > 0"):
            nn.LayerNorm(8, eps=bad)
    with pytest.raises(abi.DQNError, match=r"unsupported layer .*MaxPool.*RNN / LayerNorm"):
        nn.lower(nn.Chain(object()))
    # two in a row: the engine refuses it by index (build_layers), the mirror by name -- across the edge of a skip block too
    with pytest.raises(abi.DQNError, match=r"LayerNorm\(16.* cannot directly follow LayerNorm\(16.*: two LayerNorm layers in a row are not supported"):
        nn.lower(nn.Chain(nn.Dense(6, 16), nn.LayerNorm(16), nn.LayerNorm(16), nn.Dense(16, 4)))
    with pytest.raises(abi.DQNError, match=r"two LayerNorm layers in a row are not supported, as the first inner layer of a SkipConnection neither"):
        nn.lower(nn.Chain(nn.Dense(6, 16), nn.LayerNorm(16), nn.SkipConnection(nn.Chain(nn.LayerNorm(16), nn.Dense(16, 16)), "+"), nn.Dense(16, 4)))
    assert len(nn.lower(nn.Chain(nn.Dense(6, 16), nn.LayerNorm(16), nn.Dropout(0.5), nn.LayerNorm(16), nn.Dense(16, 4)))[0]) == 5      # a Dropout between them: accepted, as before


def _L(abi, kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, k=0, s=0):
    d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, k, k, s, s
    return d


def test_host_side_validation_accepts_and_refuses_without_a_gpu(pkg, mods):
    """dqn_plan_default runs build_layers on the host: the supported placements get a plan (the layer's entry all zero), every refusal names the layer index and the value"""
    nn, abi, _ = mods
    D, LN = abi.LAYER_DENSE, abi.LAYER_LAYERNORM
    plan = lambda layers, obs=(6, 1, 1), **kw: pkg.default_plan(layers, pkg.default_hparams(batch_size=8, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], buffer_size=64, **({"dueling": 0} | kw)))
    ln = lambda n=16, **kw: _L(abi, LN, n_in=n, n_out=n, **kw)
    ok = plan([_L(abi, D, act=1, n_in=6, n_out=16), ln(), _L(abi, D, n_in=16, n_out=4)])
    assert tuple(ok[1]) == (0, 0, 0)
    assert tuple(plan([_L(abi, D, act=1, n_in=6, n_out=2048), ln(2048), _L(abi, D, n_in=2048, n_out=4)])[1]) == (0, 0, 0)      # no chunk rule of a GEMM layer applies, at any width
    plan([_L(abi, D, n_in=6, n_out=16), ln(cin=_bits(0.5), act=3), _L(abi, D, stream=1, n_in=16, n_out=1), _L(abi, D, stream=2, n_in=16, n_out=4)], dueling=1)      # the join sits on the layer
    plan([_L(abi, abi.LAYER_LSTM, n_in=6, n_out=8), ln(8), _L(abi, D, n_in=8, n_out=4)], recurrence=1, trace_length=3)      # behind a recurrent layer
    with pytest.raises(abi.DQNError, match=r"layer 0: LayerNorm cannot be the first layer"):
        plan([ln(6), _L(abi, D, n_in=6, n_out=4)])
    with pytest.raises(abi.DQNError, match=r"layer 1: LayerNorm must directly follow a Dense or recurrent layer \(layer 0 is a Conv / MaxPool / MeanPool layer, whose output is a \(2, 4, 4\) map\)"):
        plan([_L(abi, abi.LAYER_CONV, cin=1, cout=2, k=3, s=1), ln(32), _L(abi, D, n_in=32, n_out=4)], obs=(1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"layer 2: LayerNorm must directly follow a Dense or recurrent layer \(layer 1 is a Conv / MaxPool / MeanPool layer"):
        plan([_L(abi, abi.LAYER_CONV, cin=1, cout=2, k=3, s=1), _L(abi, abi.LAYER_MAXPOOL, k=2, s=2), ln(8), _L(abi, D, n_in=8, n_out=4)], obs=(1, 6, 6))
    for stream in (1, 2):
        with pytest.raises(abi.DQNError, match=r"layer 2: LayerNorm layers are supported in the base chain only \(not in a value / advantage stream; stream = %d\)" % stream):
            plan([_L(abi, D, n_in=6, n_out=16), _L(abi, D, stream=stream, n_in=16, n_out=16), ln(stream=stream), _L(abi, D, stream=3 - stream, n_in=16, n_out=4)], dueling=1)
    with pytest.raises(abi.DQNError, match=r"layer 1: a LayerNorm layer cannot be the network's output layer"):
        plan([_L(abi, D, n_in=6, n_out=4), ln(4)])
    with pytest.raises(abi.DQNError, match=r"layer 1: LayerNorm size n = 12 != incoming features 16"):
        plan([_L(abi, D, n_in=6, n_out=16), ln(12), _L(abi, D, n_in=12, n_out=4)])
    with pytest.raises(abi.DQNError, match=r"layer 1: LayerNorm size n = 1 must be >= 2"):
        plan([_L(abi, D, n_in=6, n_out=1), ln(1), _L(abi, D, n_in=1, n_out=4)])
    for bad, shown in ((0.0, None), (-1.0, "-1"), (float("inf"), "inf"), (float("nan"), "nan")):
        bits = int(np.float32(bad).view(np.int32)) if bad != 0.0 else int(np.float32(-0.0).view(np.int32))      # +0 bits mean "the default": -0 is the zero that can be asked for
        with pytest.raises(abi.DQNError, match=r"layer 1: LayerNorm eps = .* \(bit pattern 0x[0-9a-f]{8}\) must be finite and > 0") as ei:
            plan([_L(abi, D, n_in=6, n_out=16), ln(cin=bits), _L(abi, D, n_in=16, n_out=4)])
        assert shown is None or shown in str(ei.value)
    with pytest.raises(abi.DQNError, match=r"layer 1: LayerNorm uses n_in, n_out, act and cin .* cout / kh / kw / sh / sw = 0 / 3 / 3 / 0 / 0 must be 0"):
        plan([_L(abi, D, n_in=6, n_out=16), ln(k=3), _L(abi, D, n_in=16, n_out=4)])
    with pytest.raises(abi.DQNError, match=r"layer 2: LayerNorm must directly follow a Dense or recurrent layer \(layer 1 is a LayerNorm layer\)"):
        plan([_L(abi, D, n_in=6, n_out=16), ln(), ln(), _L(abi, D, n_in=16, n_out=4)])


def test_julia_shim_maps_the_layer_and_keeps_the_unsupported_throw():
    src = open(os.path.join(ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    assert re.search(r"elseif l isa Flux\.LayerNorm\b", src)
    assert re.search(r"length\(l\.size\) == 1 \|\| throw\(\"DeepQLearningError: [^\"]*LayerNorm\(n\) with an integer n only", src)      # a tuple size: refused by name
    assert re.search(r"\(l\.affine && l\.diag isa Flux\.Scale\) \|\| throw\(\"DeepQLearningError: [^\"]*LayerNorm with affine=true only\"\)", src)
    assert re.search(r"return LayerDesc\(7, ACT\[l\.λ\], stream, l\.size\[1\], l\.size\[1\], reinterpret\(Int32, Float32\(l\.ϵ\)\), 0, 0, 0, 0, 0\)", src)
    assert 'throw("DeepQLearningError: unsupported layer' in src and "RNN / LayerNorm / flattenbatch only" in src
    for a, b in (("(", ")"), ("[", "]")):
        assert src.count(a) == src.count(b)
    assert len(re.findall(r"\bend\b", src)) >= len(re.findall(r"^\s*(?:function|if|for|begin|struct|mutable struct|module|let|while|try)\b", src, re.M))


def _first_step(c, leg):
    gamma = float(np.float32(c.gamma))
    if c.T:
        D = LR.rec_data(c); idx, start = D.draws[0]
        return LR.rec_step(D.net, D.p_on, D.p_tg, LR.R.sample_batch(D.ring, idx, start, c.T, c.obs), gamma, bool(c.dq), leg)
    D = LR.ff_data(c)
    return LR.ff_step(D.net, D.p_on, D.p_tg, LR.ff_batch(c, D, D.idx[0]), gamma, bool(c.dq), leg)


@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_reference_legs_agree_and_the_seed_keeps_the_margins(c):
    """torch autograd through the law written out and the hand-written NumPy layer: 1e-10 relative on every quantity.  The case's fixed seed keeps
    sigma_min >= SIGMA_MIN, the relu margin and the argmax gap -- asserted, never redrawn, never skipped"""
    sg, rm, gap = LR.case_margins(c)
    assert sg >= LR.SIGMA_MIN and rm > LR.RELU_MARGIN and gap > LR.GAP, (c.name, sg, rm, gap)
    a, b = _first_step(c, "law"), _first_step(c, "numpy")
    LR.legs_agree(a, b)
    D = LR.rec_data(c) if c.T else LR.ff_data(c)
    assert not LR.dead_blocks(D.net, a["grads"], c.dead), c.name      # every block, ln<i>.scale / ln<i>.bias included, is live (n = 2: those behind the layer, see the table)
    names = [nm for nm, _ in LR.blocks(D.net)]
    assert any(re.fullmatch(r"ln\d+\.scale", nm) for nm in names) and any(re.fullmatch(r"ln\d+\.bias", nm) for nm in names)


@pytest.mark.parametrize("eps", [1e-5, 0.5])
def test_gradient_of_the_law_against_central_differences(eps):
    """the hand-written backward, the path through sigma included, against central differences of the hand-written forward in fp64"""
    rng = np.random.default_rng(3); B, n = 3, 7
    x, scale, bias, dy = rng.standard_normal((B, n)), 1 + 0.3 * rng.standard_normal(n), 0.2 * rng.standard_normal(n), rng.standard_normal((B, n))
    loss = lambda x, s, b: float((LR.ln_forward_np(x, s, b, eps)[0] * dy).sum())
    dx, ds, db = LR.ln_backward_np(LR.ln_forward_np(x, scale, bias, eps)[1], dy)
    h = 1e-6
    def num(arr, f):
        g = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            up, dn = arr.copy(), arr.copy(); up[i] += h; dn[i] -= h
            g[i] = (f(up) - f(dn)) / (2 * h)
        return g
    np.testing.assert_allclose(dx, num(x, lambda v: loss(v, scale, bias)), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(ds, num(scale, lambda v: loss(x, v, bias)), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(db, num(bias, lambda v: loss(x, scale, v)), rtol=1e-6, atol=1e-8)
    # ... and autograd through the law agrees with it
    xt, st, bt = (torch.tensor(v, requires_grad=True) for v in (x, scale, bias))
    (LR.ln_law(xt, st, bt, eps)[0] * torch.tensor(dy)).sum().backward()
    for got, want in ((xt.grad, dx), (st.grad, ds), (bt.grad, db)):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-10, atol=1e-12)
    # without the sigma path (sigma held constant) the input gradient is a different one: the check above can tell
    xh, sigma, r, sc = LR.ln_forward_np(x, scale, bias, eps)[1]; g = dy * sc
    assert np.abs(r * (g - g.mean(axis=1, keepdims=True)) - dx).max() > 1e-2


def test_over_two_features_the_input_gradient_is_of_order_eps():
    """n = 2: x_hat = (+a, -a), a = sigma / (sigma + eps), and dx_1 = -dx_2 = (g_1 - g_2) / 2 * eps / (sigma + eps)^2 -- why case n2_b5 cannot ask the blocks in front
    of the layer to be live"""
    rng = np.random.default_rng(5); eps = 1e-5
    x, dy, scale = rng.standard_normal((4, 2)), rng.standard_normal((4, 2)), np.array([1.3, 0.7])
    y, cache = LR.ln_forward_np(x, scale, np.zeros(2), eps); sigma = cache[1]
    np.testing.assert_allclose(np.abs(cache[0]), np.broadcast_to(sigma / (sigma + eps), (4, 2)), rtol=1e-12)
    g = dy * scale
    want = (g[:, :1] - g[:, 1:]) / 2 * eps / (sigma + eps) ** 2
    np.testing.assert_allclose(LR.ln_backward_np(cache, dy)[0], np.concatenate([want, -want], axis=1), rtol=1e-6, atol=1e-12)


def test_the_tests_can_tell_fluxs_law_from_torchs():
    """eps = 0.5: the reference's Q differs from the Q under sqrt(var + eps) by more than 100 x TOL_Q -- an engine on torch's law fails the eps_half case"""
    c = LR.BY_NAME["eps_half"]; D = LR.ff_data(c); s = LR.ff_batch(c, D, D.idx[0])[0]
    q, qt = LR.q_values(D.net, D.p_on, s), LR.q_values(D.net, D.p_on, s, leg="torchs_law")
    tol = LR.TOL_Q["atol"] + LR.TOL_Q["rtol"] * np.abs(q)
    assert (np.abs(q - qt) / tol).max() > 100 and (np.abs(q - qt) > tol).all(), (float((np.abs(q - qt) / tol).max()), float((np.abs(q - qt) / tol).min()))      # every Q of the batch is off, the worst by thousands of tolerances
    c0 = LR.BY_NAME["single_q"]; D0 = LR.ff_data(c0); s0 = LR.ff_batch(c0, D0, D0.idx[0])[0]      # at the default eps the two laws are close: the case above is the one that bites
    assert np.abs(LR.q_values(D0.net, D0.p_on, s0) - LR.q_values(D0.net, D0.p_on, s0, leg="torchs_law")).max() < 1e-2


def test_sigma_rule_sees_a_constant_column():
    nn = LR.nn
    net = nn.Chain(nn.Dense(2, 4), nn.LayerNorm(4), nn.Dense(4, 2))
    p = nn.glorot_params(net, seed=1); p[:8] = 0.0; p[8:12] = 0.25      # zero weights, equal biases: every column is constant
    assert LR.sigma_min(net, p, np.ones((3, 2))) == 0.0
    assert np.isfinite(LR.q_values(net, p, np.ones((3, 2)))).all()      # x_hat = 0: the forward stays finite
