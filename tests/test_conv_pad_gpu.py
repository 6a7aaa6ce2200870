"""GPU: train steps, policy forward, device loop and refusals of networks with a PADDED convolution (csrc/conv_own.hip) against the two-legged fp64 reference of
feedforward_reference.py.  Every case of conv_pad_reference.CASES runs three train steps on given indices under the shared per-step checks of the feed-forward edge
tests (Q, greedy indices exactly, y, td, loss, per-block gradients, grad_norm, parameters after fp64 Adam, priorities; tolerances unchanged); use_graph 0 and 1 and
use_mfma 0 and 1 must give identical bits.

The exact check: every case whose padded conv is the first layer also runs as the SAME network with pad = 0 on observations zero-extended by (ph, pw) (a 0 byte
border for u8), same parameters, same explicit plan -- a network the existing suite holds bit-exact to the CPU twin -- and everything recorded for three steps must
be equal bit for bit: the padded path's canonical-order leg ("Padded convolutions").

Beyond the train step: the recurrent Conv(pad=1) -> LSTM chain over T*B columns, the policy forward and greedy action, the device environment loop against the fp64
argmax, dqn_evaluate, the solver round trip (qnetwork.bson, restore_best_model), dqn_n_params, and the refusals through the C ABI, replicas included.

One MI355X, one run: 40 tests in 3 s.  Worst error / tolerance per quantity (1.0 = at the bound): q_on_s 0.040, q_on_sp 0.045, q_tg_sp 0.050, policy_q 0.033, y 0.016,
td 0.024, loss 0.043, grad_norm 0.003, is_weights 0.056, beta powers 0.0002; worst gradient error / max |g| per block kind: conv.W 6.3e-07, conv.b 7.3e-07, dense.W 4.7e-07, dense.b 2.8e-07
(GRAD_C = 2e-5)."""
import importlib
import time

import pytest

import __graft_entry__ as ge
import conv_pad_reference as CR
import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_gpu_common as G
import feedforward_reference as FR

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "envs", "solver", "bson"))


@pytest.mark.parametrize("c", CR.CASES, ids=IDS(CR.CASES))
def test_case_vs_fp64_reference_graph_vs_eager_and_mfma_vs_valu(pkg, c):
    h, rec = E.run_checked(pkg.Engine, c)
    E.same_bits(rec, E.replay_steps(pkg.Engine, c, graph=1 - c.graph), f"{c.name}: use_graph {c.graph} vs {1 - c.graph}")
    E.same_bits(rec, E.replay_steps(pkg.Engine, c, mfma=1 - c.mfma), f"{c.name}: use_mfma {c.mfma} vs {1 - c.mfma}")
    names = [n for n, _ in h.profile_step()]
    net = E.network(c)
    for i, l in enumerate(net.base):
        if any(CR.pad_of(l)):
            assert names.count(f"fwd_on_conv{i}") == 1 and names.count(f"fwd_tg_conv{i}") == 1, names      # one forward launch per pass
            assert names.count(f"dw_conv{i}") == 1, names
            reads_obs = all(CR.is_pool(p) for p in net.base[:i])
            assert names.count(f"bwd_conv{i}") == (0 if reads_obs else 1), names                           # on the observation: no input gradient
    if c.u8 and any(CR.pad_of(net.base[0])):
        assert h.batch_arena_elem_bytes() == 1, c.name      # a first-layer padded conv reads the byte arena
    h.close()


@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("name", CR.FIRST_LAYER)
def test_exact_padded_equals_pad0_on_the_zero_extended_observation(pkg, name, mfma):
    c = CR.BY_NAME[name]; net, D = E.prepare(c)
    ha, _ = E.make_handle(pkg.Engine, c, net, D, mfma=mfma); plan = ha.plan(); ha.close()
    a = E.replay_steps(pkg.Engine, c, mfma=mfma, plan=plan)
    layers, view, s, sp = CR.extended(c, net, D)
    b = E.replay_steps(pkg.Engine, c, mfma=mfma, plan=plan, layers=layers, hp_net=view, s=s, sp=sp)
    E.same_bits(a, b, f"{name} (use_mfma {mfma}): pad vs pad 0 on the extended map")


@pytest.mark.parametrize("name", ["same3", "stride2", "interior", "pool_before", "dueling_u8"])
def test_policy_forward_and_greedy_action(pkg, name):
    G.policy_forward_and_greedy_action(pkg, CR.BY_NAME[name])


def test_n_params_is_unchanged_by_pad(pkg):
    c = CR.BY_NAME["rect"]; net, D = E.prepare(c)
    h, _ = E.make_handle(pkg.Engine, c, net, D)
    assert h.P == net.n_params() == D["p_on"].size
    h.close()


def test_recurrent_padded_conv_lstm_chain(pkg, mods):
    """Conv(3, 1=>8, relu; pad=1) -> LSTM(200, 8) -> Dense(8, 4), T = 3, B = 4: the padded layer runs once over the T*B columns"""
    G.recurrent_chain(pkg, mods[0], CR.REC, {"fwd_on_conv0": 1, "fwd_tg_conv0": 1, "dw_conv0": 1, "bwd_conv0": 0})


def test_device_env_loop_acts_on_the_fp64_argmax_and_evaluates(pkg, mods):
    """the acting program with a first-layer pad = 1 trunk: a network with a padded conv takes the general acting tail, not the fused acting head"""
    nn = mods[0]
    G.device_env_loop(pkg, mods, nn.Chain(nn.Conv(3, 4, 8, nn.relu, pad=1), nn.flattenbatch, nn.Dense(200, 4)),
                      [CR.PConv(3, 4, 8, O.ACT_RELU, pad=1), O.Dense(200, 4)], fused_head=False)


def test_solver_round_trip_with_a_padded_conv_network(pkg, mods, tmp_path, monkeypatch):
    nn = mods[0]
    G.solver_round_trip(pkg, mods, tmp_path, monkeypatch, nn.Chain(nn.Conv(3, 4, 8, nn.relu, pad=nn.SamePad()), nn.flattenbatch, nn.Dense(200, 4)),
                        [(3, 3, 4, 8), (8,), (4, 200), (4,)])      # the Conv and Dense arrays: the pad is no parameter


def test_refusals_through_the_c_abi(pkg, monkeypatch):
    abi = CR.abi
    def create(layers, obs, nA=4):
        net = type("N", (), dict(obs_shape=obs, n_actions=nA, dueling=False))
        return pkg.Engine(layers, E.ref.hparams_for(net, batch_size=8, buffer_size=32))
    def L(kind, n_in=0, n_out=0, cin=0, cout=0, k=0, s=0):
        d = abi.LayerDesc(); d.kind, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, n_in, n_out, cin, cout, k, k, s, s
        return d
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv pad \(3, 3\) is larger than kernel - 1 = \(2, 2\)"):
        create([L(abi.LAYER_CONV, 3, 3, cin=1, cout=2, k=3, s=1), L(abi.LAYER_DENSE, n_in=200, n_out=4)], (1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv pad \(0, -2\) must not be negative"):
        create([L(abi.LAYER_CONV, 0, -2, cin=1, cout=2, k=3, s=1), L(abi.LAYER_DENSE, n_in=8, n_out=4)], (1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv kernel \(5, 5\) / stride \(1, 1\) does not fit the 2x2 input map extended by pad \(1, 1\)"):
        create([L(abi.LAYER_CONV, 1, 1, cin=1, cout=2, k=5, s=1), L(abi.LAYER_DENSE, n_in=8, n_out=4)], (1, 2, 2))
    c = CR.BY_NAME["one_axis"]; net, D = E.prepare(c)
    h, _ = E.make_handle(pkg.Engine, c, net, D)
    with pytest.raises(abi.DQNError, match=r"dqn_comm_init: layer 0 is a Conv with pad \(1, 0\); data-parallel replicas .* not supported"):
        h.comm_init(bytes(128), 0, 1)
    h.train_step(D["idx"][0])      # the engine is left as it was
    h.close()
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    with pytest.raises(abi.DQNError, match=r"DQN_SIM_WORLD: layer 0 is a Conv with pad \(1, 0\)"):
        E.make_handle(pkg.Engine, c, net, D)


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file"""
    print("\nworst error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("worst gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(FR.WORST.items()) if k.startswith(("conv", "dense"))})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
