"""GPU: train steps, policy forward, device loop, solver round trip and refusals of networks with Flux GlobalMaxPool / GlobalMeanPool / AdaptiveMaxPool / AdaptiveMeanPool
layers (layer kinds 12 / 13; csrc/pool_global.hip where the resolved window is the whole map, csrc/pool.hip on the resolved geometry otherwise) against the two-legged fp64
reference of feedforward_reference.py, which holds the resolved MaxPool / MeanPool.  Every case of adaptive_pool_reference.CASES runs three train steps on given indices
under the shared per-step checks of the feed-forward edge tests (Q, greedy indices exactly, y, td, loss, per-block gradients, grad_norm, parameters after fp64 Adam,
priorities; the project's existing tolerances, none added); use_graph 0 against 1 and a second identical run must give identical bits.

Exact companions, engine against engine: the kinds 5 / 6 network with the resolved window (pool.hip) gives the same bits for every MaxPool, every adaptive output and a
GlobalMeanPool over n <= 16 rows; on a 1x1 map the layer gives the bits of the network without it; the same equalities hold directly behind a GroupNorm(..., relu) and with
an adaptive pool as the entry of a convolutional skip block -- both compositions are thereby held without a new reference.  Case `ties` pins the tie rule under
GlobalMaxPool: all 64 rows tie, row 0 takes dY, and the conv's dW / db match both fp64 legs.

No learning test: a global pool discards the position that TestMDP's and GridWorld's rewards depend on, so no reference threshold applies to a network that ends in one;
the solver round trip asserts finite losses and the saved arrays only.

Without the feature every test here fails: nn.GlobalMeanPool does not exist, abi.LAYER_ADAPTIVEMAXPOOL does not exist, and the engine answers "unknown kind 12".

One MI355X, one run: docs/history/global_pool.md records the worst error / tolerance per quantity and per gradient block kind."""
import importlib
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import adaptive_pool_reference as AR
import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_gpu_common as G
import feedforward_reference as FR

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()
abi = AR.abi


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "envs", "solver", "bson"))


@pytest.mark.parametrize("c", AR.CASES, ids=IDS(AR.CASES))
def test_case_vs_fp64_reference_graph_vs_eager_rerun_and_the_resolved_pool(pkg, c):
    net = E.network(c); layers = AR.descs(net)
    h, rec = E.run_checked(pkg.Engine, c, layers=layers)
    E.same_bits(rec, E.replay_steps(pkg.Engine, c, graph=1 - c.graph, layers=layers), f"{c.name}: use_graph {c.graph} vs {1 - c.graph}")
    E.same_bits(rec, E.replay_steps(pkg.Engine, c, layers=layers), f"{c.name}: two identical runs")
    if AR.exact(net):      # kinds 5 / 6 with the resolved window: pool.hip
        E.same_bits(rec, E.replay_steps(pkg.Engine, c), f"{c.name}: kinds 12 / 13 vs MaxPool / MeanPool(k, stride) with the resolved geometry")
    if FR.is_pool(net.base[0]):
        assert h.batch_arena_elem_bytes() == 4, c.name      # a pool as the first layer reads floats: no byte arena, u8 replay or not
    assert all(p == (0, 0, 0) for p, l in zip(h.plan(), layers) if l.kind in (abi.LAYER_ADAPTIVEMAXPOOL, abi.LAYER_ADAPTIVEMEANPOOL))      # the plan entry is all zeros and ignored
    names = [n for n, _ in h.profile_step()]
    for i, _ in AR.pools(net):
        assert names.count(f"fwd_on_pool{i}") == 1 and names.count(f"fwd_tg_pool{i}") == 1, names      # one launch per pass
        assert names.count(f"bwd_pool{i}") == (1 if i > 0 else 0), names                              # on the observation: no input gradient has a reader
    h.close()


def test_global_meanpool_above_16_rows_has_an_order_of_its_own(pkg):
    """64 rows: four per slot, summed per slot and then across the slots -- not pool.hip's one chain over the 64 taps.  The two agree within the fp32 tolerances (both pass the
    fp64 checks) and are NOT the same bits on this case's data: were they, the whole-map window would not have taken pool_global.hip"""
    c = AR.BY_NAME["g88_mean"]; net = E.network(c)
    a, b = E.replay_steps(pkg.Engine, c, layers=AR.descs(net)), E.replay_steps(pkg.Engine, c)
    for ra, rb in zip(a, b):
        np.testing.assert_allclose(ra["q"]["q_on_s"], rb["q"]["q_on_s"], **E.TOL_Q)
    assert any((ra["q"]["q_on_s"] != rb["q"]["q_on_s"]).any() or (ra["g"] != rb["g"]).any() for ra, rb in zip(a, b))


@pytest.mark.parametrize("name", ["g11_max", "g11_mean"])
def test_on_a_1x1_map_the_layer_equals_the_network_without_it_bit_for_bit(pkg, name):
    c = AR.BY_NAME[name]; net, D = E.prepare(c)
    with_pool = E.replay_steps(pkg.Engine, c, layers=AR.descs(net))
    E.same_bits(with_pool, E.replay_steps(pkg.Engine, c, net_D=(AR.without_pool(c), D)), f"{name}: with and without the pool on the 1x1 map")


# ------------------------------------------------------------------ engine against engine on package nn chains: compositions the fp64 reference does not describe
def nn_record(pkg, nn, net, obs, B=32, nA=4, steps=3, graph=1):
    layers, dueling = nn.lower(net)
    hp = pkg.default_hparams(batch_size=B, n_actions=nA, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], dueling=int(dueling), buffer_size=B + 24, learning_rate=1e-3, gamma=0.95,
                             double_q=1, prioritized_replay=1, use_graph=graph, seed=5)
    rng = np.random.default_rng(11); n = B + 24
    s, sp = (rng.random((n,) + tuple(obs), dtype=np.float32) for _ in range(2))
    a = rng.integers(0, nA, n).astype(np.int32); r = (2 * rng.standard_normal(n)).astype(np.float32); d = (rng.random(n) < 0.2).astype(np.uint8)
    p = nn.glorot_params(net, seed=3)
    p_on = (p + 0.05 * rng.standard_normal(p.size)).astype(np.float32); p_tg = (p_on + 0.05 * rng.standard_normal(p.size)).astype(np.float32)
    h = pkg.Engine(layers, hp); h.replay_add(s, a, r, sp, d); h.set_params(p_on, 0); h.set_params(p_tg, 1)
    rec = []
    for k in range(steps):
        loss, gn, td = h.train_step(rng.choice(n, B, replace=False).astype(np.int64))
        rec.append(dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities()))
    names = [nm for nm, _ in h.profile_step(max_entries=512)]
    h.close()
    assert all(np.isfinite(x["g"]).all() and np.abs(x["g"]).max() > 0 for x in rec)
    return rec, names


@pytest.mark.parametrize("kind,hw", [("max", (8, 8)), ("max", (5, 7)), ("mean", (4, 4)), ("max", (1, 1)), ("mean", (1, 1))])
def test_behind_a_groupnorm_the_layer_equals_the_resolved_pool_bit_for_bit(pkg, mods, kind, hw):
    """Conv(3, 1 => 4) -> GroupNorm(4, 2, relu) -> pool -> Dense -> Dense: the pool's backward applies the GroupNorm's activation derivative (its producer) and hands
    dpre to the GroupNorm's backward launches.  On the 1x1 map the third network is the one without the layer"""
    nn = mods[0]; obs = (1, hw[0] + 2, hw[1] + 2)
    trunk = lambda: [nn.Conv(3, 1, 4), nn.GroupNorm(4, 2, nn.relu)]
    head = lambda: [nn.flattenbatch, nn.Dense(4, 16, nn.relu), nn.Dense(16, 4)]
    glob, pool = (nn.GlobalMaxPool, nn.MaxPool) if kind == "max" else (nn.GlobalMeanPool, nn.MeanPool)
    a, names = nn_record(pkg, nn, nn.Chain(*trunk(), glob(), *head()), obs)
    assert names.count("fwd_on_pool2") == 1 and names.count("fwd_tg_pool2") == 1 and names.count("bwd_pool2") == 1 and names.count("bwd_gn1") == 1, names
    E.same_bits(a, nn_record(pkg, nn, nn.Chain(*trunk(), pool(hw), *head()), obs)[0], f"GroupNorm -> Global{kind} vs {kind}pool({hw})")
    E.same_bits(a, nn_record(pkg, nn, nn.Chain(*trunk(), glob(), *head()), obs, graph=0)[0], "use_graph 1 vs 0")
    if hw == (1, 1):
        E.same_bits(a, nn_record(pkg, nn, nn.Chain(*trunk(), *head()), obs)[0], "with and without the pool on the 1x1 map")


@pytest.mark.parametrize("kind", ["max", "mean"])
def test_as_the_entry_of_a_convolutional_skip_block_the_layer_equals_the_resolved_pool_bit_for_bit(pkg, mods, kind):
    """Conv(3, 1 => 4, relu) -> AdaptivePool((3, 3)) on the 8x8 map (window 4, stride 2) -> SkipConnection(Conv(pad 1, relu), Conv(pad 1); +) -> Dense: the pool's output has
    two consumers and its dY is the block's entry sum.  And the global layer in front of a block on the (4, 1, 1) map"""
    nn = mods[0]; obs = (1, 10, 10)
    blk = lambda: nn.SkipConnection(nn.Chain(nn.Conv(3, 4, 4, nn.relu, pad=1), nn.Conv(3, 4, 4, pad=1)), "+")
    ada, glob, pool = (nn.AdaptiveMaxPool, nn.GlobalMaxPool, nn.MaxPool) if kind == "max" else (nn.AdaptiveMeanPool, nn.GlobalMeanPool, nn.MeanPool)
    net = lambda p, feat: nn.Chain(nn.Conv(3, 1, 4, nn.relu), p, blk(), nn.flattenbatch, nn.Dense(feat, 4))
    a, names = nn_record(pkg, nn, net(ada((3, 3)), 36), obs)
    assert names.count("fwd_on_pool1") == 1 and names.count("bwd_pool1") == 1, names
    E.same_bits(a, nn_record(pkg, nn, net(pool(4, stride=2), 36), obs)[0], f"Adaptive{kind}((3, 3)) vs {kind}pool(4, stride 2) as a block's entry")
    if kind == "max":      # (a GlobalMeanPool over 64 rows has an order of its own)
        E.same_bits(nn_record(pkg, nn, net(glob(), 4), obs)[0], nn_record(pkg, nn, net(pool(8), 4), obs)[0], "GlobalMaxPool vs MaxPool(8) as a block's entry")


# ------------------------------------------------------------------ beyond the step
@pytest.mark.parametrize("name", ["g88_max", "g88_mean", "g57_mean_c3", "g117_max", "g57_b5_mean", "g57_b128_max", "a5to3_mean", "first_gmax_f32"])
def test_forward_at_1_and_7_columns(pkg, name):
    """dqn_forward on 1 and 7 observations (one column a piece): within TOL_Q of fp64, and the bits the train step's Q has on the same rows -- the reduction has one order,
    whatever the column count, the column's position or the aligned / unaligned path"""
    c = AR.BY_NAME[name]; net, D = E.prepare(c)
    h, _ = E.make_handle(pkg.Engine, c, net, D, layers=AR.descs(net)); idx = D["idx"][0]
    f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
    ps = net.unflatten(D["p_on"].astype(np.float64))
    fw = {n: h.forward(f(D["s"][idx[:n]])) for n in (1, 7) if n <= c.B}
    for n, q in fw.items():
        E._close("policy_q", q, FR.q_numpy(net, ps, f(D["s"][idx[:n]]).astype(np.float64))[0], msg=f"{name} n={n}", **E.TOL_Q)
    h.train_step(idx)
    q_on_s = h.last_q()["q_on_s"]
    for n, q in fw.items():
        np.testing.assert_array_equal(q, q_on_s[:n], err_msg=f"{name} n={n}")
    h.close()


def test_recurrent_conv_globalmeanpool_lstm_chain(pkg, mods):
    """Conv(2, 1=>8, relu) -> GlobalMeanPool() -> flattenbatch -> LSTM(8, 8) -> Dense(8, 4), T = 3, B = 4: the pool runs once over the T*B columns in front of the cell.  The
    reference reads the chain with MeanPool((4, 4)); the engine is handed the GlobalMeanPool chain (adaptive_pool_reference.rec_nn)"""
    G.recurrent_chain(pkg, AR.rec_nn(mods[0]), AR.REC, {"fwd_on_pool1": 1, "fwd_tg_pool1": 1, "bwd_pool1": 1})


def test_device_env_loop_acts_on_the_fp64_argmax_and_evaluates(pkg, mods):
    """the acting program with a global pool level: as a pool network it takes the general four-launch tail, not the fused acting head"""
    nn = mods[0]
    G.device_env_loop(pkg, mods, nn.Chain(nn.Conv(2, 4, 8, nn.relu), nn.GlobalMeanPool(), nn.flattenbatch, nn.Dense(8, 4)),
                      [O.Conv(2, 4, 8, O.ACT_RELU), AR.APool("meanpool", (4, 4)), O.Dense(8, 4)], fused_head=False)


def test_solver_round_trip_with_a_global_pool_network(pkg, mods, tmp_path, monkeypatch):
    nn = mods[0]
    G.solver_round_trip(pkg, mods, tmp_path, monkeypatch, nn.Chain(nn.Conv(2, 4, 8, nn.relu), nn.GlobalMaxPool(), nn.flattenbatch, nn.Dense(8, 4)),
                        [(2, 2, 4, 8), (8,), (4, 8), (4,)])      # exactly the Conv and Dense arrays: the pool holds none


def test_replicas_are_refused(pkg, monkeypatch):
    """the new kinds take the pool row of the traits table: dqn_comm_init and DQN_SIM_WORLD refuse, with the pool's reason"""
    c = AR.BY_NAME["g57_b16_max"]; net, D = E.prepare(c)
    h, _ = E.make_handle(pkg.Engine, c, net, D, layers=AR.descs(net))
    with pytest.raises(abi.DQNError, match=r"dqn_comm_init: layer 1 is a MaxPool / MeanPool layer; data-parallel replicas of a network with pool layers are not supported \(single GPU only\)"):
        h.comm_init(bytes(128), 0, 1)
    h.train_step(D["idx"][0])      # the engine is left as it was
    h.close()
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    with pytest.raises(abi.DQNError, match=r"DQN_SIM_WORLD: layer 1 is a MaxPool / MeanPool layer"):
        E.make_handle(pkg.Engine, c, net, D, layers=AR.descs(net))


def test_engine_refusals_by_raw_descriptors(pkg):
    def create(layers, obs=(1, 6, 6), **kw):
        hp = pkg.default_hparams(batch_size=8, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], buffer_size=64, **({"dueling": 0} | kw))
        pkg.Engine(layers, hp).close()
    AR.engine_accepts_and_refuses(create, lambda rx: pytest.raises(abi.DQNError, match=rx))


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (docs/history/global_pool.md records them)"""
    print("\nworst error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("worst gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(FR.WORST.items()) if k.startswith(("conv", "dense"))})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
