"""CPU: Flux GRU layers (Recur(GRUCell)) in the Python mirror, the ABI, BSON and the Julia shim, and the fp64 reference the GPU tests
(tests/test_gru_gpu.py) check the engine against.  No compute call is made on the engine."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from gru_reference import gru_cell


@pytest.fixture(scope="module")
def pkg():
    return ge.build()


@pytest.fixture(scope="module")
def mods():
    p = ge.load_package()
    return p, importlib.import_module(p.__name__ + ".nn"), importlib.import_module(p.__name__ + ".bson"), importlib.import_module(p.__name__ + "._abi")


def test_reference_cell_equals_torch_grucell():
    """the in-test GRU (gates r, z, n; r multiplies Wh_n*h) is torch.nn.GRUCell with weight_ih = Wi, weight_hh = Wh, bias_ih = b, bias_hh = 0"""
    rng = np.random.default_rng(0)
    n_in, H, B = 7, 5, 4
    Wi, Wh, b = rng.standard_normal((3 * H, n_in)), rng.standard_normal((3 * H, H)), rng.standard_normal(3 * H)
    cell = torch.nn.GRUCell(n_in, H).double()
    with torch.no_grad():
        cell.weight_ih.copy_(torch.tensor(Wi)); cell.weight_hh.copy_(torch.tensor(Wh)); cell.bias_ih.copy_(torch.tensor(b)); cell.bias_hh.zero_()
    h_ref = h = torch.tensor(rng.standard_normal((B, H)))
    for _ in range(6):
        x = torch.tensor(rng.standard_normal((B, n_in)))
        with torch.no_grad():
            h_ref = cell(x, h_ref)
            h = gru_cell(x, h, torch.tensor(Wi.T.copy()), torch.tensor(Wh.T.copy()), torch.tensor(b))
        np.testing.assert_allclose(h.numpy(), h_ref.numpy(), rtol=1e-13, atol=1e-13)


def test_gru_lowering_param_count_and_order(mods):
    p, nn, bson, abi = mods
    net = nn.Chain(nn.flattenbatch, nn.GRU(25, 32), nn.Dense(32, 4))
    layers, dueling = nn.lower(net)
    assert not dueling and [l.kind for l in layers] == [abi.LAYER_GRU, abi.LAYER_DENSE]
    assert (layers[0].n_in, layers[0].n_out) == (25, 32)
    flat = nn.glorot_params(net, seed=3)
    assert flat.size == 5600 + 132 and flat.dtype == np.float32
    # Flux.params order Wi (3H, in), Wh (3H, H), b, state0: glorot weights, zero bias (no forget-gate bias), zero state0
    Wi, Wh, b, h0 = flat[:2400], flat[2400:2400 + 3072], flat[5472:5568], flat[5568:5600]
    lim_i, lim_h = np.sqrt(6.0 / (25 + 96)), np.sqrt(6.0 / (32 + 96))
    assert np.abs(Wi).max() <= lim_i * (1 + 1e-6) and np.abs(Wi).max() > 0.5 * lim_i
    assert np.abs(Wh).max() <= lim_h * (1 + 1e-6) and np.abs(Wh).max() > 0.5 * lim_h
    assert not b.any() and not h0.any()
    with pytest.raises(abi.DQNError, match="unsupported layer"):
        nn.lower(nn.Chain(object()))


def test_gru_is_recurrent_and_stays_in_the_base_chain(mods):
    p, nn, bson, abi = mods
    m = nn.Chain(nn.flattenbatch, nn.GRU(25, 32), nn.Dense(32, 4))
    assert nn.isrecurrent(m) and not nn.isrecurrent(nn.Chain(nn.Dense(4, 2)))
    d = nn.create_dueling_network(m)
    assert [l.kind for l in d.base] == ["gru"] and [(l.n_in, l.n_out) for l in d.val] == [(32, 1)] and [(l.n_in, l.n_out) for l in d.adv] == [(32, 4)]
    layers, dueling = nn.lower(d)
    assert dueling and [(l.kind, l.stream) for l in layers] == [(abi.LAYER_GRU, abi.STREAM_BASE), (abi.LAYER_DENSE, abi.STREAM_VAL), (abi.LAYER_DENSE, abi.STREAM_ADV)]


def test_bson_round_trip_with_gru_shapes(mods, tmp_path):
    p, nn, bson, abi = mods
    net = nn.Chain(nn.GRU(6, 8), nn.Dense(8, 3))
    shapes = bson.julia_param_shapes(net)
    assert [s for s, _ in shapes] == [(24, 6), (24, 8), (24,), (8, 1), (3, 8), (3,)]
    flat = np.random.default_rng(1).standard_normal(sum(n for _, n in shapes)).astype(np.float32)
    path = tmp_path / "qnetwork.bson"
    bson.save_qnetwork(str(path), flat, shapes)
    w, sizes = bson.load_qnetwork(str(path))
    np.testing.assert_array_equal(w, flat)
    assert sizes == [s for s, _ in shapes]


def test_abi_enum_matches_the_header(mods):
    p, nn, bson, abi = mods
    hdr = open(os.path.join(ge.ROOT, "include", "dqn_mi355x.h")).read()
    assert int(re.search(r"DQN_LAYER_GRU\s*=\s*(\d+)", hdr).group(1)) == abi.LAYER_GRU == 3
    assert "a GRU layer writes h" in hdr


def test_julia_shim_maps_grucell_to_kind_3():
    src = open(os.path.join(ge.ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")).read()
    m = re.search(r"elseif l isa Flux\.Recur && l\.cell isa Flux\.GRUCell[^\n]*\n\s*return LayerDesc\((\d+), 0, stream, size\(l\.cell\.Wi, 2\), size\(l\.cell\.Wh, 2\)", src)
    assert m and int(m.group(1)) == 3
    assert "GRUv3Cell" not in src.replace("(GRUv3Cell / RNNCell: unsupported)", "")      # no other cell is mapped
    assert 'throw("DeepQLearningError: unsupported layer' in src


def test_default_plan_of_a_gru_network_has_no_column_groups(pkg):
    nn = importlib.import_module(pkg.__name__ + ".nn")
    for net, B, T, dueling in ((nn.Chain(nn.GRU(25, 32), nn.Dense(32, 4)), 32, 8, 0), (nn.create_dueling_network(nn.Chain(nn.GRU(16, 32), nn.Dense(32, 4))), 16, 10, 1)):
        layers, _ = nn.lower(net)
        hp = pkg.default_hparams(batch_size=B, n_actions=4, obs_c=layers[0].n_in, dueling=dueling, recurrence=1, trace_length=T, prioritized_replay=0)
        plan = pkg.default_plan(layers, hp)
        assert all(p[2] >= 0 for p in plan), plan
    # the same shape with an LSTM takes the fused step's column groups: the GRU's plan is the multi-launch program by choice, not by accident
    layers, _ = nn.lower(nn.Chain(nn.LSTM(25, 32), nn.Dense(32, 4)))
    hp = pkg.default_hparams(batch_size=32, n_actions=4, obs_c=25, dueling=0, recurrence=1, trace_length=8, prioritized_replay=0)
    assert all(p[2] < 0 for p in pkg.default_plan(layers, hp))


def test_gru_without_recurrence_is_refused_by_the_plan_and_the_solver(pkg):
    nn = importlib.import_module(pkg.__name__ + ".nn")
    S = importlib.import_module(pkg.__name__ + ".solver")
    layers, _ = nn.lower(nn.Chain(nn.GRU(6, 8), nn.Dense(8, 3)))
    hp = pkg.default_hparams(batch_size=4, n_actions=3, obs_c=6, dueling=0, recurrence=0)
    with pytest.raises(pkg.DQNError, match="recurrent model but recurrence is set to false"):
        pkg.default_plan(layers, hp)
    envs = importlib.import_module(pkg.__name__ + ".envs")
    env = envs.TestMDP((5, 5), 1, 6, n=1, seed=7)
    solver = S.DeepQLearningSolver(qnetwork=nn.Chain(nn.flattenbatch, nn.GRU(25, 8), nn.Dense(8, 4)), max_steps=10, recurrence=False, verbose=False, logdir=None)
    with pytest.raises(pkg.DQNError, match="recurrent model but recurrence is set to false"):
        S.solve(solver, env)
