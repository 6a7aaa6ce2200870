"""CPU: Flux RNN layers (Recur(RNNCell), h' = σ.(Wi*x .+ Wh*h .+ b)) in the Python mirror, the ABI, BSON and the Julia shim, and the fp64
reference the GPU tests (tests/test_rnn_gpu.py) check the engine against.  No compute call is made on the engine."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from rnn_reference import rnn_cell


@pytest.fixture(scope="module")
def pkg():
    return ge.build()


@pytest.fixture(scope="module")
def mods():
    p = ge.load_package()
    return p, importlib.import_module(p.__name__ + ".nn"), importlib.import_module(p.__name__ + ".bson"), importlib.import_module(p.__name__ + "._abi")


@pytest.mark.parametrize("nonlinearity,act", [("tanh", 2), ("relu", 1)])
def test_reference_cell_equals_torch_rnncell(nonlinearity, act):
    """the in-test RNN cell is torch.nn.RNNCell with weight_ih = Wi, weight_hh = Wh, bias_ih = b, bias_hh = 0"""
    rng = np.random.default_rng(0)
    n_in, H, B = 7, 5, 4
    Wi, Wh, b = rng.standard_normal((H, n_in)), rng.standard_normal((H, H)), rng.standard_normal(H)
    cell = torch.nn.RNNCell(n_in, H, nonlinearity=nonlinearity).double()
    with torch.no_grad():
        cell.weight_ih.copy_(torch.tensor(Wi)); cell.weight_hh.copy_(torch.tensor(Wh)); cell.bias_ih.copy_(torch.tensor(b)); cell.bias_hh.zero_()
    h_ref = h = torch.tensor(rng.standard_normal((B, H)))
    for _ in range(6):
        x = torch.tensor(rng.standard_normal((B, n_in)))
        with torch.no_grad():
            h_ref = cell(x, h_ref)
            h = rnn_cell(x, h, torch.tensor(Wi.T.copy()), torch.tensor(Wh.T.copy()), torch.tensor(b), act)
        np.testing.assert_allclose(h.numpy(), h_ref.numpy(), rtol=1e-13, atol=1e-13)


def test_rnn_lowering_param_count_and_order(mods):
    p, nn, bson, abi = mods
    net = nn.Chain(nn.flattenbatch, nn.RNN(25, 32), nn.Dense(32, 4))
    layers, dueling = nn.lower(net)
    assert not dueling and [l.kind for l in layers] == [abi.LAYER_RNN, abi.LAYER_DENSE]
    assert (layers[0].n_in, layers[0].n_out, layers[0].act) == (25, 32, abi.ACT_TANH)      # Flux's default σ = tanh, carried in act
    assert [l.act for l in nn.lower(nn.Chain(nn.RNN(4, 3, nn.relu), nn.RNN(3, 2, nn.sigmoid), nn.RNN(2, 2, nn.identity)))[0]] == [abi.ACT_RELU, abi.ACT_SIGMOID, abi.ACT_IDENTITY]
    flat = nn.glorot_params(net, seed=3)
    assert flat.size == 800 + 1024 + 32 + 32 + 132 and flat.dtype == np.float32
    # Flux.params order Wi (H, in), Wh (H, H), b, state0: glorot weights, zero bias, zero state0
    Wi, Wh, b, h0 = flat[:800], flat[800:1824], flat[1824:1856], flat[1856:1888]
    lim_i, lim_h = np.sqrt(6.0 / (25 + 32)), np.sqrt(6.0 / (32 + 32))
    assert np.abs(Wi).max() <= lim_i * (1 + 1e-6) and np.abs(Wi).max() > 0.5 * lim_i
    assert np.abs(Wh).max() <= lim_h * (1 + 1e-6) and np.abs(Wh).max() > 0.5 * lim_h
    assert not b.any() and not h0.any()
    assert nn.RNN(25, 32).shapes() == [(25, 32), (32, 32), (32,), (32,)]
    with pytest.raises(abi.DQNError, match=r"unsupported layer .*RNN"):
        nn.lower(nn.Chain(object()))


def test_rnn_is_recurrent_and_stays_in_the_base_chain(mods):
    p, nn, bson, abi = mods
    m = nn.Chain(nn.flattenbatch, nn.RNN(25, 32), nn.Dense(32, 4))
    assert nn.isrecurrent(m) and not nn.isrecurrent(nn.Chain(nn.Dense(4, 2)))
    d = nn.create_dueling_network(m)
    assert [l.kind for l in d.base] == ["rnn"] and [(l.n_in, l.n_out) for l in d.val] == [(32, 1)] and [(l.n_in, l.n_out) for l in d.adv] == [(32, 4)]
    layers, dueling = nn.lower(d)
    assert dueling and [(l.kind, l.stream) for l in layers] == [(abi.LAYER_RNN, abi.STREAM_BASE), (abi.LAYER_DENSE, abi.STREAM_VAL), (abi.LAYER_DENSE, abi.STREAM_ADV)]


def test_bson_round_trip_with_rnn_shapes(mods, tmp_path):
    p, nn, bson, abi = mods
    net = nn.Chain(nn.RNN(6, 8, nn.relu), nn.Dense(8, 3))
    shapes = bson.julia_param_shapes(net)
    assert [s for s, _ in shapes] == [(8, 6), (8, 8), (8,), (8, 1), (3, 8), (3,)]
    assert sum(n for _, n in shapes) == nn.glorot_params(net).size
    flat = np.random.default_rng(1).standard_normal(sum(n for _, n in shapes)).astype(np.float32)
    path = tmp_path / "qnetwork.bson"
    bson.save_qnetwork(str(path), flat, shapes)
    w, sizes = bson.load_qnetwork(str(path))
    np.testing.assert_array_equal(w, flat)
    assert sizes == [s for s, _ in shapes]


def test_abi_enum_matches_the_header(mods):
    p, nn, bson, abi = mods
    hdr = open(os.path.join(ge.ROOT, "include", "dqn_mi355x.h")).read()
    assert int(re.search(r"DQN_LAYER_RNN\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_RNN == 4
    assert "An RNN layer writes h only" in hdr


def test_julia_shim_maps_rnncell_to_kind_4_with_its_activation():
    src = open(os.path.join(ge.ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    m = re.search(r"elseif l isa Flux\.Recur && l\.cell isa Flux\.RNNCell[^\n]*\n\s*return LayerDesc\((\d+), ACT\[l\.cell\.σ\], stream, size\(l\.cell\.Wi, 2\), size\(l\.cell\.Wh, 2\)", src)
    assert m and int(m.group(1)) == 4
    assert "GRUv3Cell" not in src      # GRUv3 stays unmapped
    assert 'throw("DeepQLearningError: unsupported layer' in src


def test_default_plan_of_an_rnn_network_has_no_column_groups(pkg):
    nn = importlib.import_module(pkg.__name__ + ".nn")
    for net, B, T, dueling in ((nn.Chain(nn.RNN(25, 32), nn.Dense(32, 4)), 32, 8, 0), (nn.create_dueling_network(nn.Chain(nn.RNN(16, 32, nn.relu), nn.Dense(32, 4))), 16, 10, 1)):
        layers, _ = nn.lower(net)
        hp = pkg.default_hparams(batch_size=B, n_actions=4, obs_c=layers[0].n_in, dueling=dueling, recurrence=1, trace_length=T, prioritized_replay=0)
        plan = pkg.default_plan(layers, hp)
        assert all(p[2] >= 0 for p in plan), plan


def test_rnn_refusals_from_the_plan_and_the_solver(pkg):
    nn = importlib.import_module(pkg.__name__ + ".nn")
    S = importlib.import_module(pkg.__name__ + ".solver")
    layers, _ = nn.lower(nn.Chain(nn.RNN(6, 8), nn.Dense(8, 3)))
    hp = pkg.default_hparams(batch_size=4, n_actions=3, obs_c=6, dueling=0, recurrence=0)
    with pytest.raises(pkg.DQNError, match="recurrent model but recurrence is set to false"):
        pkg.default_plan(layers, hp)
    # an RNN in the advantage stream
    layers, _ = nn.lower(nn.DuelingNetwork(nn.Chain(nn.Dense(6, 8)), nn.Chain(nn.Dense(8, 1)), nn.Chain(nn.RNN(8, 3))))
    hp = pkg.default_hparams(batch_size=4, n_actions=3, obs_c=6, dueling=1, recurrence=1, trace_length=3, prioritized_replay=0)
    with pytest.raises(pkg.DQNError, match="base chain only"):
        pkg.default_plan(layers, hp)
    # an activation code outside DQN_ACT_*
    layers, _ = nn.lower(nn.Chain(nn.RNN(6, 8, 7), nn.Dense(8, 3)))
    hp = pkg.default_hparams(batch_size=4, n_actions=3, obs_c=6, dueling=0, recurrence=1, trace_length=3, prioritized_replay=0)
    with pytest.raises(pkg.DQNError, match="RNN activation 7"):
        pkg.default_plan(layers, hp)
    envs = importlib.import_module(pkg.__name__ + ".envs")
    env = envs.TestMDP((5, 5), 1, 6, n=1, seed=7)
    solver = S.DeepQLearningSolver(qnetwork=nn.Chain(nn.flattenbatch, nn.RNN(25, 8), nn.Dense(8, 4)), max_steps=10, recurrence=False, verbose=False, logdir=None)
    with pytest.raises(pkg.DQNError, match="recurrent model but recurrence is set to false"):
        S.solve(solver, env)
