"""GPU: train steps, policy forward and refusals of networks with Flux MaxPool / MeanPool layers (csrc/pool.hip) against the two-legged fp64 reference of
feedforward_reference.py.  Every case of pool_reference.CASES runs three train steps on given indices under the shared per-step checks of the feed-forward edge
tests (Q, greedy indices exactly, y, td, loss, per-block gradients, grad_norm, parameters after fp64 Adam, priorities; tolerances unchanged), and
use_graph 0 and 1 must give identical bits.  Window 1x1 / stride 1 must equal the network WITHOUT the layer bit for bit -- the one exact check there is.
Case `ties` pins the tie rule: every window ties and the conv's dW / db must match the fp64 legs, which route to the first tap.

One MI355X, one run: 33 tests in 3.5 s (the file prints 1 s for its own cases).  Worst error / tolerance per quantity (1.0 = at the bound): q_on_s 0.032, q_on_sp 0.028,
q_tg_sp 0.029, policy_q 0.017, y 0.015, td 0.017, loss 0.020, grad_norm 0.011, is_weights 0.055, beta powers 0.0002; worst gradient error / max |g| per block kind: conv.W 5.4e-07, conv.b 4.3e-07,
dense.W 5.4e-07, dense.b 3.9e-07 (GRAD_C = 2e-5).

Beyond the train step: the recurrent Conv -> MaxPool -> LSTM chain (case 11), the policy forward, the device environment loop against the fp64 argmax, dqn_evaluate,
the solver round trip (qnetwork.bson, restore_best_model) and the refusals, replicas included."""
import importlib
import time

import pytest

import __graft_entry__ as ge
import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_gpu_common as G
import feedforward_reference as FR
import pool_reference as PR

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


@pytest.mark.parametrize("c", PR.CASES, ids=IDS(PR.CASES))
def test_case_vs_fp64_reference_and_graph_vs_eager(pkg, c):
    h, rec = E.run_checked(pkg.Engine, c)
    E.same_bits(rec, E.replay_steps(pkg.Engine, c, graph=1 - c.graph), f"{c.name}: use_graph {c.graph} vs {1 - c.graph}")
    net = E.network(c)
    if PR.is_pool(net.base[0]):
        assert h.batch_arena_elem_bytes() == 4, c.name      # a pool as the first layer reads floats: no byte arena, u8 replay or not
    assert all(p == (0, 0, 0) for p, l in zip(h.plan(), FR.layer_descs(net)) if l.kind in (PR.abi.LAYER_MAXPOOL, PR.abi.LAYER_MEANPOOL))
    names = [n for n, _ in h.profile_step()]
    for i, l in enumerate(net.base):
        if PR.is_pool(l):
            assert names.count(f"fwd_on_pool{i}") == 1 and names.count(f"fwd_tg_pool{i}") == 1, names      # one launch per pass
            assert names.count(f"bwd_pool{i}") == (1 if i > 0 else 0), names                              # on the observation: no input gradient
    h.close()


@pytest.mark.parametrize("name", ["one_max", "one_mean"])
def test_one_by_one_window_equals_the_network_without_the_layer_bit_for_bit(pkg, name):
    c = PR.BY_NAME[name]; net, D = E.prepare(c)
    with_pool = E.replay_steps(pkg.Engine, c)
    E.same_bits(with_pool, E.replay_steps(pkg.Engine, c, net_D=(PR.without_pool(c), D)), f"{name}: with and without the 1x1 pool")


@pytest.mark.parametrize("name", ["max_c16", "between", "dueling_max", "first_mean_u8"])
def test_policy_forward_and_greedy_action(pkg, name):
    G.policy_forward_and_greedy_action(pkg, PR.BY_NAME[name])


def test_refusals(pkg):
    abi = PR.abi
    def create(layers, obs, nA=4, dueling=False):
        net = type("N", (), dict(obs_shape=obs, n_actions=nA, dueling=dueling))
        return pkg.Engine(layers, E.ref.hparams_for(net, batch_size=8, buffer_size=32))
    def L(kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, k=0, s=0):
        d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, k, k, s, s
        return d
    conv = lambda: L(abi.LAYER_CONV, cin=1, cout=2, k=3, s=1)      # 1x6x6 -> 2x4x4
    with pytest.raises(abi.DQNError, match=r"MaxPool layers are supported in the base chain only"):
        create([conv(), L(abi.LAYER_DENSE, 1, n_in=32, n_out=1), L(abi.LAYER_MAXPOOL, 2, k=2, s=2), L(abi.LAYER_DENSE, 2, n_in=32, n_out=4)], (1, 6, 6), dueling=True)
    with pytest.raises(abi.DQNError, match=r"MeanPool must be the first layer or follow a Conv / MaxPool / MeanPool"):
        create([L(abi.LAYER_DENSE, n_in=36, n_out=16), L(abi.LAYER_MEANPOOL, k=2, s=2), L(abi.LAYER_DENSE, n_in=4, n_out=4)], (1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"MaxPool window \(5, 5\) does not fit the 4x4 input map"):
        create([conv(), L(abi.LAYER_MAXPOOL, k=5, s=1), L(abi.LAYER_DENSE, n_in=2, n_out=4)], (1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"MaxPool stride \(0, 0\) must be positive"):
        create([conv(), L(abi.LAYER_MAXPOOL, k=2, s=0), L(abi.LAYER_DENSE, n_in=8, n_out=4)], (1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"MeanPool has no activation"):
        create([conv(), L(abi.LAYER_MEANPOOL, act=abi.ACT_RELU, k=2, s=2), L(abi.LAYER_DENSE, n_in=8, n_out=4)], (1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"cin 3 / cout 3 != incoming channels 2"):
        create([conv(), L(abi.LAYER_MAXPOOL, cin=3, cout=3, k=2, s=2), L(abi.LAYER_DENSE, n_in=8, n_out=4)], (1, 6, 6))
    create([conv(), L(abi.LAYER_MAXPOOL, k=2, s=2), L(abi.LAYER_DENSE, n_in=8, n_out=4)], (1, 6, 6)).close()      # cin = cout = 0: taken from the map


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "envs", "solver", "bson"))


def test_recurrent_conv_maxpool_lstm_chain(pkg, mods):
    """case 11: Conv(2, 1=>8, relu) -> MaxPool(2) -> LSTM(32, 8) -> Dense(8, 4), T = 3, B = 4 -- the pool runs once over the T*B columns (Conv -> LSTM chains train on
    the parent commit: the multi-launch recurrent program)"""
    G.recurrent_chain(pkg, mods[0], PR.REC, {"fwd_on_pool1": 1, "fwd_tg_pool1": 1, "bwd_pool1": 1})


def test_device_env_loop_acts_on_the_fp64_argmax_and_evaluates(pkg, mods):
    """the acting program with a pool level: a pool network takes the general four-launch tail, not the fused acting head"""
    nn = mods[0]
    G.device_env_loop(pkg, mods, nn.Chain(nn.Conv(2, 4, 8, nn.relu), nn.MaxPool(2), nn.flattenbatch, nn.Dense(32, 4)),
                      [O.Conv(2, 4, 8, O.ACT_RELU), PR.MaxPool(2), O.Dense(32, 4)], fused_head=False)


def test_solver_round_trip_with_a_pool_network(pkg, mods, tmp_path, monkeypatch):
    nn = mods[0]
    G.solver_round_trip(pkg, mods, tmp_path, monkeypatch, nn.Chain(nn.Conv(2, 4, 8, nn.relu), nn.MaxPool(2), nn.flattenbatch, nn.Dense(32, 4)),
                        [(2, 2, 4, 8), (8,), (4, 32), (4,)])      # exactly the Conv and Dense arrays: the pool holds none


def test_replicas_of_a_pool_network_are_refused(pkg, monkeypatch):
    """a pool contributes nothing to the exchange, but the exchange paths have no pool network under test: dqn_comm_init and DQN_SIM_WORLD refuse, with the reason"""
    c = PR.BY_NAME["b16_max"]; net, D = E.prepare(c)
    h, _ = E.make_handle(pkg.Engine, c, net, D)
    with pytest.raises(PR.abi.DQNError, match=r"dqn_comm_init: layer 1 is a MaxPool / MeanPool layer; data-parallel replicas .* not supported"):
        h.comm_init(bytes(128), 0, 1)
    h.train_step(D["idx"][0])      # the engine is left as it was
    h.close()
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    with pytest.raises(PR.abi.DQNError, match=r"DQN_SIM_WORLD: layer 1 is a MaxPool / MeanPool layer"):
        E.make_handle(pkg.Engine, c, net, D)


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (the module docstring records them)"""
    print("\nworst error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("worst gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(FR.WORST.items()) if k.startswith(("conv", "dense"))})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
