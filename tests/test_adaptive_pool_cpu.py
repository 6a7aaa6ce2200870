"""CPU: Flux GlobalMaxPool / GlobalMeanPool / AdaptiveMaxPool / AdaptiveMeanPool layers in the Python mirror, the ABI header, the library's host-side validation (no GPU:
dqn_plan_default runs build_layers), BSON and the Julia shim; Flux's window rule against hand-listed windows and against torch's adaptive pooling (equal where in % out == 0,
DIFFERENT at 5 -> 3 and 8 -> 3); and the fp64 reference the GPU tests (test_adaptive_pool_gpu.py) stand on: its two legs against each other on every case of the table, and
the margin seeds of that table."""
import importlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as ge
import adaptive_pool_reference as AR
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


def test_enum_values_match_the_header(mods):
    _, abi, _ = mods
    hdr = open(os.path.join(ROOT, "include", "dqn_mi355x.h")).read()
    assert int(re.search(r"DQN_LAYER_ADAPTIVEMAXPOOL\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_ADAPTIVEMAXPOOL == 12
    assert int(re.search(r"DQN_LAYER_ADAPTIVEMEANPOOL\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_ADAPTIVEMEANPOOL == 13
    assert int(re.search(r"#define DQN_PLAN_VERSION\s+(\d+)", hdr).group(1)) == 3      # no struct changed


def test_lowering_of_the_four_classes(mods):
    nn, abi, _ = mods
    net = nn.Chain(nn.Conv(3, 1, 16, nn.relu), nn.AdaptiveMaxPool((3, 2)), nn.Conv(1, 16, 8, nn.relu), nn.AdaptiveMeanPool(2), nn.GlobalMaxPool(), nn.GlobalMeanPool(), nn.flattenbatch, nn.Dense(8, 4))
    layers, dueling = nn.lower(net)
    AMAX, AMEAN = abi.LAYER_ADAPTIVEMAXPOOL, abi.LAYER_ADAPTIVEMEANPOOL
    assert not dueling and [l.kind for l in layers] == [abi.LAYER_CONV, AMAX, abi.LAYER_CONV, AMEAN, AMAX, AMEAN, abi.LAYER_DENSE]
    slots = lambda d: (d.cin, d.cout, d.kh, d.kw, d.sh, d.sw, d.n_in, d.n_out, d.act, d.stream)
    assert slots(layers[1]) == (16, 16, 3, 2, 0, 0, 0, 0, abi.ACT_IDENTITY, abi.STREAM_BASE)      # kh, kw = the OUTPUT size (oh, ow)
    assert slots(layers[3]) == (8, 8, 2, 2, 0, 0, 0, 0, abi.ACT_IDENTITY, abi.STREAM_BASE)        # an integer: both axes
    assert slots(layers[4]) == slots(layers[5]) == (8, 8, 1, 1, 0, 0, 0, 0, abi.ACT_IDENTITY, abi.STREAM_BASE)      # the global layers: output (1, 1)
    assert [repr(l) for l in net.layers[1:6:2] + net.layers[4:5]] == ["AdaptiveMaxPool((2, 3))", "AdaptiveMeanPool((2, 2))", "GlobalMeanPool()", "GlobalMaxPool()"]      # Flux's reprs: (W, H)
    first = nn.lower(nn.Chain(nn.GlobalMeanPool(), nn.Dense(2, 4)))[0][0]
    assert (first.kind, first.cin, first.cout, first.kh, first.kw) == (AMEAN, 0, 0, 1, 1)      # in front of the first Conv: the engine takes the observation's channels
    d = nn.create_dueling_network(nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.GlobalMaxPool(), nn.flattenbatch, nn.Dense(4, 16, nn.relu), nn.Dense(16, 4)))
    assert [l.kind for l in d.base] == ["conv", "adaptivemaxpool"]
    layers, dueling = nn.lower(d)
    assert dueling and [(l.kind, l.stream) for l in layers] == [(1, 0), (12, 0), (0, 1), (0, 1), (0, 2), (0, 2)]
    # the entry of a convolutional skip block, and a GroupNorm behind the layer: placed as a pool is
    blk = nn.SkipConnection(nn.Chain(nn.Conv(3, 4, 4, nn.relu, pad=1), nn.Conv(3, 4, 4, pad=1)), "+")
    layers, _ = nn.lower(nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.AdaptiveMaxPool(3), blk, nn.GroupNorm(4, 2, nn.relu), nn.flattenbatch, nn.Dense(36, 4)))
    assert [l.kind for l in layers] == [1, 12, 1, 1, abi.LAYER_SKIPADD_MAP, abi.LAYER_GROUPNORM, 0]


def test_the_mirror_refuses_by_name(mods):
    nn, abi, _ = mods
    for cls in (nn.AdaptiveMaxPool, nn.AdaptiveMeanPool):
        with pytest.raises(abi.DQNError, match=r"%s\(\(0, 2\)\): the output size must be at least \(1, 1\)" % cls.__name__):
            cls((0, 2))
        with pytest.raises(abi.DQNError, match=r"%s\(\(1, 2, 3\)\): the output size must be an integer or a pair" % cls.__name__):
            cls((1, 2, 3))
    with pytest.raises(abi.DQNError, match=r"GlobalMaxPool\(\) is supported in the base chain only"):
        nn.lower(nn.DuelingNetwork(nn.Chain(nn.Conv(3, 1, 4)), nn.Chain(nn.GlobalMaxPool(), nn.Dense(4, 1)), nn.Chain(nn.Dense(64, 4))))
    with pytest.raises(abi.DQNError, match=r"GlobalMeanPool\(\) cannot be the network's output layer"):
        nn.lower(nn.Chain(nn.Conv(3, 1, 4), nn.GlobalMeanPool()))
    with pytest.raises(abi.DQNError, match=r"a MaxPool / MeanPool layer inside a convolutional SkipConnection is not supported"):      # an inner layer: refused as a pool is
        nn.lower(nn.Chain(nn.Conv(3, 1, 4), nn.SkipConnection(nn.Chain(nn.Conv(3, 4, 4, pad=1), nn.AdaptiveMaxPool(4)), "+"), nn.Dense(64, 4)))
    with pytest.raises(abi.DQNError, match=r"a Conv / MaxPool / MeanPool layer inside a SkipConnection is not supported"):
        nn.lower(nn.Chain(nn.Dense(6, 8), nn.SkipConnection(nn.Chain(nn.GlobalMeanPool()), "+"), nn.Dense(8, 4)))
    with pytest.raises(abi.DQNError, match=r"cannot follow a Conv / MaxPool / MeanPool layer: a skip block stands on a feature vector"):      # a Dense block directly behind the pool
        nn.lower(nn.Chain(nn.Conv(3, 1, 4), nn.GlobalMaxPool(), nn.SkipConnection(nn.Chain(nn.Dense(4, 4)), "+"), nn.Dense(4, 4)))
    with pytest.raises(abi.DQNError, match=r"MaxPool with pad=0 only"):      # padded pooling stays refused
        nn.MaxPool(2, pad=1)


def test_the_unsupported_layer_vocabulary_gains_the_four_names_in_front_and_keeps_every_existing_regex(mods):
    nn, abi, _ = mods
    with pytest.raises(abi.DQNError) as ei:
        nn.lower(nn.Chain(object()))
    msg = str(ei.value)
    assert "GlobalMaxPool / GlobalMeanPool / AdaptiveMaxPool / AdaptiveMeanPool, and (SkipConnection(+) / Conv / MaxPool / MeanPool / GroupNorm / Dense / Dropout / LSTM / GRU / RNN / LayerNorm / flattenbatch only)" in msg
    for rx in (r"unsupported layer .*MaxPool.*RNN", r"unsupported layer .*Dense / Dropout / LSTM.*RNN / LayerNorm / flattenbatch only", r"unsupported layer .*MaxPool.*RNN / LayerNorm",
               r"unsupported layer .*SkipConnection\(\+\) / Conv / MaxPool", r"unsupported layer .*RNN", "unsupported layer"):
        assert re.search(rx, msg), rx


def test_glorot_params_param_shapes_and_bson_round_trip_hold_no_array_for_the_layers(mods, tmp_path):
    nn, abi, bson = mods
    with_pools = nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.AdaptiveMaxPool(2), nn.AdaptiveMeanPool((1, 2)), nn.GlobalMaxPool(), nn.GlobalMeanPool(), nn.flattenbatch, nn.Dense(4, 4))
    without = nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.Dense(4, 4))
    assert all(l.shapes() == [] for l in with_pools.layers[1:5])
    p = nn.glorot_params(with_pools, seed=3)
    np.testing.assert_array_equal(p, nn.glorot_params(without, seed=3))
    shapes = bson.julia_param_shapes(with_pools)
    assert shapes == bson.julia_param_shapes(without) == [((3, 3, 1, 4), 36), ((4,), 4), ((4, 4), 16), ((4,), 4)]
    path = str(tmp_path / "qnetwork.bson")
    bson.save_qnetwork(path, p, shapes)
    flat, sizes = bson.load_qnetwork(path)
    np.testing.assert_array_equal(flat, p)
    assert [tuple(s) for s in sizes] == [s for s, _ in shapes]      # exactly the Conv and Dense arrays


def test_julia_shim_maps_the_four_layers():
    src = open(os.path.join(ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    assert re.search(r"elseif l isa Flux\.GlobalMaxPool \|\| l isa Flux\.GlobalMeanPool\b[^\n]*\n\s*return LayerDesc\(l isa Flux\.GlobalMaxPool \? 12 : 13, 0, stream, 0, 0, 0, 0, 1, 1, 0, 0\)", src)
    m = re.search(r"elseif l isa Flux\.AdaptiveMaxPool \|\| l isa Flux\.AdaptiveMeanPool\b[^\n]*\n(?:\s*#[^\n]*\n)*\s*return LayerDesc\(l isa Flux\.AdaptiveMaxPool \? 12 : 13, 0, stream, 0, 0, 0, 0, l\.out\[2\], l\.out\[1\], 0, 0\)", src)
    assert m      # Julia's first dimension is the ABI's w, as for a pool's window: (oh, ow) = (out[2], out[1])
    assert re.search(r"is_map_desc\(d\) = d\.kind == 1 \|\| d\.kind == 5 \|\| d\.kind == 6 \|\| d\.kind == 10 \|\| d\.kind == 11 \|\| d\.kind == 12 \|\| d\.kind == 13", src)      # appended
    assert re.search(r"is_map_layer\(x\) = x isa Conv \|\| x isa Flux\.MaxPool \|\| x isa Flux\.MeanPool \|\| x isa Flux\.AdaptiveMaxPool \|\| x isa Flux\.AdaptiveMeanPool \|\| x isa Flux\.GlobalMaxPool \|\| x isa Flux\.GlobalMeanPool", src)
    assert 'unsupported layer $(typeof(l)) (supported: GlobalMaxPool / GlobalMeanPool / AdaptiveMaxPool / AdaptiveMeanPool, and (SkipConnection(+) / Conv / MaxPool / MeanPool / GroupNorm / Dense' in src
    for a, b in (("(", ")"), ("[", "]")):
        assert src.count(a) == src.count(b)


# ------------------------------------------------------------------ the window rule
HAND = {(5, 3): [(0, 2), (1, 3), (2, 4)], (8, 3): [(0, 3), (2, 5), (4, 7)], (7, 2): [(0, 3), (3, 6)], (8, 2): [(0, 3), (4, 7)], (7, 7): [(i, i) for i in range(7)], (7, 1): [(0, 6)],
        (8, 8): [(i, i) for i in range(8)], (17, 1): [(0, 16)], (7, 3): [(0, 2), (2, 4), (4, 6)]}


def _torch_windows(n_in, n_out):
    """torch's adaptive pooling: window i is [floor(i * in / out), ceil((i + 1) * in / out)), as inclusive pairs"""
    return [((i * n_in) // n_out, -((-(i + 1) * n_in) // n_out) - 1) for i in range(n_out)]


def test_flux_windows_against_hand_listed_ones():
    for (n_in, n_out), want in HAND.items():
        assert AR.windows(n_in, n_out) == want, (n_in, n_out)
    # rectangular (7, 8) -> (2, 3): the axes resolve independently
    assert (AR.resolve(7, 2), AR.resolve(8, 3)) == ((4, 3), (4, 2))
    p = AR.APool("maxpool", (7, 8), (2, 3))
    assert (p.kh, p.kw, p.sh, p.sw) == (4, 4, 3, 2) and p.out_shape((5, 7, 8)) == (5, 2, 3)


def test_flux_rule_equals_torch_adaptive_pooling_where_divisible_and_differs_at_5to3_and_8to3():
    rng = np.random.default_rng(0)
    for n_in, n_out in ((8, 2), (8, 4), (6, 3), (9, 3), (7, 7), (7, 1), (10, 5)):
        assert n_in % n_out == 0 and AR.windows(n_in, n_out) == _torch_windows(n_in, n_out)
    for n_in, n_out in ((5, 3), (8, 3)):
        assert AR.windows(n_in, n_out) != _torch_windows(n_in, n_out)
    assert _torch_windows(5, 3) == [(0, 1), (1, 3), (3, 4)]      # torch: [0,2) [1,4) [3,5)
    # on data, through the reference's own pooling (F.max_pool2d / F.avg_pool2d on the resolved geometry) against F.adaptive_*_pool2d
    for (h, w), out, same in (((8, 6), (4, 3), True), ((9, 10), (3, 5), True), ((5, 5), (3, 3), False), ((8, 8), (3, 3), False), ((7, 8), (7, 1), True)):
        x = torch.tensor(rng.standard_normal((3, 2, h, w)))
        for kind, adaptive in (("maxpool", F.adaptive_max_pool2d), ("meanpool", F.adaptive_avg_pool2d)):
            got, want = FR._layer_t(AR.APool(kind, (h, w), out), x), adaptive(x, out)
            assert got.shape == want.shape
            assert bool(torch.allclose(got, want, rtol=1e-13, atol=0)) == same, (h, w, out, kind)
            np.testing.assert_allclose(FR.pool_forward(AR.APool(kind, (h, w), out), x.numpy())[0], got.numpy(), rtol=1e-13)      # the NumPy leg, same geometry


def test_the_table_states_the_geometry_it_was_written_for():
    rows = lambda name: int(np.prod(AR.pools(E.network(AR.BY_NAME[name]))[0][1].hw))
    assert [rows(n) for n in ("g88_max", "g57_max_c3", "g117_max", "g44_max_c16", "g11_max")] == [64, 35, 17, 16, 1]
    for c in AR.CASES:
        net = E.network(c); ps = AR.pools(net)
        assert ps, c.name
        shp = net.obs_shape
        for i, l in enumerate(net.base):      # every APool stands on the map it was resolved for
            if isinstance(l, AR.APool):
                assert shp[1:] == l.hw, (c.name, i, shp)
            shp = l.out_shape(shp) if l.kind != "dense" else (l.n_out, 1, 1)
        assert all(l.is_global for _, l in ps) == (c in AR.GLOBAL and c.name != "first_amean_u8"), c.name      # (the placement section's adaptive first layer)
        d = AR.descs(net)
        for i, l in ps:
            assert (d[i].kind, d[i].kh, d[i].kw, d[i].sh, d[i].sw, d[i].n_in, d[i].n_out) == (12 if l.kind == "maxpool" else 13, l.out[0], l.out[1], 0, 0, 0, 0)
    assert not AR.exact(E.network(AR.BY_NAME["g88_mean"])) and AR.exact(E.network(AR.BY_NAME["g44_mean_c16"])) and AR.exact(E.network(AR.BY_NAME["g88_max"]))
    assert all(AR.exact(E.network(c)) for c in AR.ADAPTIVE)


@pytest.mark.parametrize("c", AR.CASES, ids=IDS(AR.CASES))
def test_reference_legs_agree_and_the_seed_keeps_the_margins(c):
    """NumPy (hand-written backward) and torch autograd (F.max_pool2d / F.avg_pool2d) share no pooling code: 1e-10 relative on every quantity, along the
    fp64 trajectory of the case's three steps.  prepare() asserts the case's fixed seed against the argmax, relu and MaxPool margins."""
    E.check_legs_along_trajectory(c)


def test_tie_case_ties_everywhere_and_both_legs_take_row_0():
    """case `ties`: all 64 rows of every channel of the online net are equal (fp64 and, by construction, fp32), and the NumPy leg's argmax is tap 0 = row 0"""
    c = AR.BY_NAME["g88_ties"]; net, D = E.prepare(c)
    x = D["s"][D["idx"][0]].astype(np.float64); ps = net.unflatten(D["p_on"].astype(np.float64))
    y, _ = O.layer_forward(net.base[0], x, ps[0], ps[1])
    t = FR._taps(net.base[1], y)[0]
    assert t.shape[0] == 64 and (t == t[0]).all() and (FR.pool_forward(net.base[1], y)[1] == 0).all()


def test_recurrent_case_seed_keeps_the_margins(mods):
    nn = mods[0]
    assert FR.rec_trajectory_ok(nn, AR.REC)
    a, b = nn.lower(AR.rec_net(nn))[0], AR.rec_nn(nn).lower(AR.rec_net(nn))[0]      # the reference's chain and the engine's differ in the pool's descriptor alone
    assert [d.kind for d in a] == [1, 6, 2, 0] and [d.kind for d in b] == [1, 13, 2, 0] and (b[1].kh, b[1].kw, b[1].sh, b[1].sw) == (1, 1, 0, 0)
    np.testing.assert_array_equal(nn.glorot_params(AR.rec_net(nn), seed=3), nn.glorot_params(AR.rec_engine_net(nn), seed=3))


def test_host_side_validation_accepts_and_refuses_without_a_gpu(pkg, mods):
    """dqn_plan_default runs build_layers on the host: the supported placements get a plan (the layer's entry all zero), every refusal names the layer index and the value"""
    _, abi, _ = mods
    plan = lambda layers, obs=(1, 6, 6), **kw: pkg.default_plan(layers, pkg.default_hparams(batch_size=8, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], buffer_size=64, **({"dueling": 0} | kw)))
    AR.engine_accepts_and_refuses(plan, lambda rx: pytest.raises(abi.DQNError, match=rx))
    p = plan([AR.L(abi.LAYER_CONV, act=1, cin=1, cout=2, kh=3, kw=3, sh=1, sw=1), AR.L(abi.LAYER_ADAPTIVEMEANPOOL, kh=1, kw=1), AR.L(abi.LAYER_DENSE, n_in=2, n_out=4)])
    assert tuple(p[1]) == (0, 0, 0)
