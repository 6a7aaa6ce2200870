"""CPU: Flux MaxPool / MeanPool layers in the Python mirror, the ABI header, BSON and the Julia shim, and the fp64 reference the GPU tests
(test_pool_gpu.py) stand on: its two legs against each other on the whole case table, and the margin seeds of that table."""
import importlib
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_reference as FR
import pool_reference as PR

ROOT = ge.ROOT

IDS = lambda cs: [c.name for c in cs]


@pytest.fixture(scope="module")
def mods():
    p = ge.load_package()
    return tuple(importlib.import_module(p.__name__ + "." + m) for m in ("nn", "_abi", "bson"))


def test_enum_values_match_the_header(mods):
    nn, abi, _ = mods
    hdr = open(os.path.join(ROOT, "include", "dqn_mi355x.h")).read()
    assert int(re.search(r"DQN_LAYER_MAXPOOL\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_MAXPOOL == 5
    assert int(re.search(r"DQN_LAYER_MEANPOOL\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_MEANPOOL == 6
    assert re.search(r"#define DQN_PLAN_VERSION 3\b", hdr)


def test_lowering(mods):
    nn, abi, _ = mods
    net = nn.Chain(nn.Conv(3, 1, 16, nn.relu), nn.MaxPool(2), nn.Conv(3, 16, 8, nn.relu), nn.MeanPool((2, 3), stride=(1, 2)), nn.flattenbatch, nn.Dense(32, 4))
    layers, dueling = nn.lower(net)
    assert not dueling and [l.kind for l in layers] == [abi.LAYER_CONV, abi.LAYER_MAXPOOL, abi.LAYER_CONV, abi.LAYER_MEANPOOL, abi.LAYER_DENSE]
    mp, ap = layers[1], layers[3]
    assert (mp.cin, mp.cout, mp.kh, mp.kw, mp.sh, mp.sw, mp.act) == (16, 16, 2, 2, 2, 2, abi.ACT_IDENTITY)      # stride defaults to the window
    assert (ap.cin, ap.cout, ap.kh, ap.kw, ap.sh, ap.sw, ap.act) == (8, 8, 2, 3, 1, 2, abi.ACT_IDENTITY)
    first = nn.lower(nn.Chain(nn.MaxPool(2), nn.Conv(3, 2, 4), nn.Dense(16, 4)))[0][0]
    assert (first.kind, first.cin, first.cout) == (abi.LAYER_MAXPOOL, 0, 0)      # in front of the first Conv: the engine takes the observation's channels
    d = nn.create_dueling_network(nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.MaxPool(2), nn.Dense(64, 16, nn.relu), nn.Dense(16, 4)))
    layers, dueling = nn.lower(d)
    assert dueling and [(l.kind, l.stream) for l in layers] == [(abi.LAYER_CONV, 0), (abi.LAYER_MAXPOOL, 0), (abi.LAYER_DENSE, 1), (abi.LAYER_DENSE, 1), (abi.LAYER_DENSE, 2), (abi.LAYER_DENSE, 2)]


def test_pad_is_refused_by_the_mirror_with_the_layers_name(mods):
    nn, abi, _ = mods
    with pytest.raises(abi.DQNError, match=r"MaxPool with pad=0 only"):
        nn.MaxPool(2, pad=1)
    with pytest.raises(abi.DQNError, match=r"MeanPool with pad=0 only"):
        nn.MeanPool(2, pad=(0, 1))
    with pytest.raises(abi.DQNError, match=r"unsupported layer .*MaxPool.*RNN"):      # the refusal of an unknown layer names the vocabulary, pools included
        nn.lower(nn.Chain(object()))


def test_glorot_params_param_shapes_and_bson_round_trip_skip_pools(mods, tmp_path):
    nn, abi, bson = mods
    with_pool = nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.MaxPool(2), nn.MeanPool(1), nn.Dense(64, 4))
    without = nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.Dense(64, 4))
    p = nn.glorot_params(with_pool, seed=3)
    np.testing.assert_array_equal(p, nn.glorot_params(without, seed=3))
    shapes = bson.julia_param_shapes(with_pool)
    assert shapes == bson.julia_param_shapes(without) == [((3, 3, 1, 4), 36), ((4,), 4), ((4, 64), 256), ((4,), 4)]
    path = str(tmp_path / "qnetwork.bson")
    bson.save_qnetwork(path, p, shapes)
    flat, sizes = bson.load_qnetwork(path)
    np.testing.assert_array_equal(flat, p)
    assert [tuple(s) for s in sizes] == [s for s, _ in shapes]      # exactly the Conv and Dense arrays


def test_julia_shim_maps_the_two_pools():
    src = open(os.path.join(ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    for name, kind in (("MaxPool", 5), ("MeanPool", 6)):
        m = re.search(r"elseif l isa Flux\.%s\b[^\n]*\n\s*any\(!=\(0\), l\.pad\) && throw\(\"DeepQLearningError: [^\"]*%s[^\"]*\"\)\n\s*"
                      r"return LayerDesc\((\d+), 0, stream, 0, 0, 0, 0, l\.k\[2\], l\.k\[1\], l\.stride\[2\], l\.stride\[1\]\)" % (name, name), src)
        assert m and int(m.group(1)) == kind, name
    # window and stride dimensions are mapped exactly as the Conv branch maps its kernel and stride: Julia's first dimension is the ABI's w
    assert re.search(r"kw, kh, cin, cout = size\(l\.weight\)", src) and re.search(r"cin, cout, kh, kw, l\.stride\[2\], l\.stride\[1\]\)", src)
    assert "GRUv3Cell" not in src.replace("(GRUv3Cell / RNNCell: unsupported)", "")
    assert 'throw("DeepQLearningError: unsupported layer' in src


@pytest.mark.parametrize("c", PR.CASES, ids=IDS(PR.CASES))
def test_reference_legs_agree_and_the_seed_keeps_the_margins(c):
    """NumPy (hand-written backward) and torch autograd (F.max_pool2d / F.avg_pool2d) share no pooling code: 1e-10 relative on every quantity, along the
    fp64 trajectory of the case's three steps.  prepare() asserts the case's fixed seed against the argmax, relu and MaxPool margins."""
    E.check_legs_along_trajectory(c)


def test_tie_case_ties_everywhere_and_both_legs_take_the_first_tap():
    """case `ties`: every MaxPool window of the online net holds four equal taps (fp64 and, by construction, fp32), and the NumPy leg's argmax is tap 0"""
    c = PR.BY_NAME["ties"]; net, D = E.prepare(c)
    x = D["s"][D["idx"][0]].astype(np.float64); ps = net.unflatten(D["p_on"].astype(np.float64))
    y, _ = O.layer_forward(net.base[0], x, ps[0], ps[1])
    t = FR._taps(net.base[1], y)[0]
    assert (t == t[0]).all() and (FR.pool_forward(net.base[1], y)[1] == 0).all()


def test_margin_rule_sees_a_near_tie():
    """the rule itself: a window whose top two taps are 1e-6 apart is below RELU_MARGIN; a window of relu zeros is exempt"""
    net = O.Network((1, 2, 2), [PR.MaxPool(2), O.Dense(1, 2)])
    p = np.array([1.0, 1.0, 0.0, 0.0])
    s = np.array([[[[0.5, 0.5 + 1e-6], [0.1, 0.2]]]])
    assert FR.margins(net, p, s)[1] < E.RELU_MARGIN
    net2 = O.Network((1, 3, 3), [O.Conv(2, 1, 1, O.ACT_RELU), PR.MaxPool(2), O.Dense(1, 2)])
    p2 = np.array([1.0, 1.0, 1.0, 1.0, -100.0, 1.0, 1.0, 0.0, 0.0])      # every pre-activation far below 0: the map is all relu zeros
    assert FR.margins(net2, p2, np.ones((1, 1, 3, 3)))[1] == np.inf


def test_recurrent_case_seed_keeps_the_margins(mods):
    nn, _, _ = mods
    assert FR.rec_trajectory_ok(nn, PR.REC)
