"""GPU: train steps, policy forward and refusals of networks with Flux MaxPool / MeanPool layers (csrc/pool.hip) against the two-legged fp64 reference of
pool_reference.py.  Every case of pool_reference.CASES runs three train steps on given indices under the shared per-step checks of the feed-forward edge
tests (Q, greedy indices exactly, y, td, loss, per-block gradients, grad_norm, parameters after fp64 Adam, priorities; tolerances unchanged), and
use_graph 0 and 1 must give identical bits.  Window 1x1 / stride 1 must equal the network WITHOUT the layer bit for bit -- the one exact check there is.
Case `ties` pins the tie rule: every window ties and the conv's dW / db must match the fp64 legs, which route to the first tap.

One MI355X, one run: 33 tests in 3.5 s (the file prints 1 s for its own cases).  Worst error / tolerance per quantity (1.0 = at the bound): q_on_s 0.032, q_on_sp 0.028,
q_tg_sp 0.029, policy_q 0.017, y 0.015, td 0.017, loss 0.020, grad_norm 0.011, is_weights 0.055; worst gradient error / max |g| per block kind: conv.W 5.4e-07, conv.b 4.3e-07,
dense.W 5.4e-07, dense.b 3.9e-07 (GRAD_C = 2e-5).

Beyond the train step: the recurrent Conv -> MaxPool -> LSTM chain (case 11), the policy forward, the device environment loop against the fp64 argmax, dqn_evaluate,
the solver round trip (qnetwork.bson, restore_best_model) and the refusals, replicas included."""
import importlib
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import feedforward_edges_common as E
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
    h, rec = PR.run_checked(pkg.Engine, c)
    E.same_bits(rec, PR.replay_steps(pkg.Engine, c, graph=1 - c.graph), f"{c.name}: use_graph {c.graph} vs {1 - c.graph}")
    if PR.is_pool(PR.network(c).base[0]):
        assert h.batch_arena_elem_bytes() == 4, c.name      # a pool as the first layer reads floats: no byte arena, u8 replay or not
    assert all(p == (0, 0, 0) for p, l in zip(h.plan(), PR.layer_descs(PR.network(c))) if l.kind in (PR.abi.LAYER_MAXPOOL, PR.abi.LAYER_MEANPOOL))
    names = [n for n, _ in h.profile_step()]
    net = PR.network(c)
    for i, l in enumerate(net.base):
        if PR.is_pool(l):
            assert names.count(f"fwd_on_pool{i}") == 1 and names.count(f"fwd_tg_pool{i}") == 1, names      # one launch per pass
            assert names.count(f"bwd_pool{i}") == (1 if i > 0 else 0), names                              # on the observation: no input gradient
    h.close()


@pytest.mark.parametrize("name", ["one_max", "one_mean"])
def test_one_by_one_window_equals_the_network_without_the_layer_bit_for_bit(pkg, name):
    c = PR.BY_NAME[name]; net, D = PR.prepare(c)
    with_pool = PR.replay_steps(pkg.Engine, c)
    E.same_bits(with_pool, PR.replay_steps(pkg.Engine, c, net_D=(PR.without_pool(c), D)), f"{name}: with and without the 1x1 pool")


@pytest.mark.parametrize("name", ["max_c16", "between", "dueling_max", "first_mean_u8"])
def test_policy_forward_and_greedy_action(pkg, name):
    c = PR.BY_NAME[name]; net, D = PR.prepare(c)
    h, _ = PR.make_handle(pkg.Engine, c, net, D)
    f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
    ps = net.unflatten(D["p_on"].astype(np.float64))
    for n in (1, 3):
        obs = f(D["s"][:n])
        q64 = PR._q_np(net, ps, obs.astype(np.float64))[0]
        E._close("policy_q", h.forward(obs), q64, msg=f"{name} n={n}", **E.TOL_Q)
        a = h.greedy_action(obs); t = np.sort(q64, axis=1)
        clear = t[:, -1] - t[:, -2] >= E.GAP
        np.testing.assert_array_equal(np.asarray(a)[clear], q64.argmax(1)[clear])
    h.close()


def test_refusals(pkg):
    abi = PR.abi
    def create(layers, obs, nA=4, dueling=False):
        net = type("N", (), dict(obs_shape=obs, n_actions=nA, dueling=dueling))
        return pkg.Engine(layers, PR.ref.hparams_for(net, batch_size=8, buffer_size=32))
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
    the parent commit: the multi-launch recurrent program).  The checker of test_recurrent_edges_gpu.run_checked with pool_reference's chain; use_graph 0 equals 1 bit for bit."""
    import recurrent_reference as R
    from drqn_common import feed
    nn = mods[0]; c = PR.REC
    net, cap, eps, ring, p_on, p_tg, dr = PR.rec_data(nn)
    layers, _ = nn.lower(net)

    def engine(graph):
        hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=c.obs[0], obs_h=c.obs[1], obs_w=c.obs[2], dueling=0, buffer_size=cap, recurrence=1, trace_length=c.T,
                                 learning_rate=1e-3, prioritized_replay=0, use_graph=graph, seed=5, gamma=c.gamma, double_q=c.double_q)
        h = pkg.Engine(layers, hp); feed(h, eps); h.set_params(p_on, 0); h.set_params(p_tg, 1)
        return h
    h, h0 = engine(1), engine(0)
    adam = R.Adam(p_on.size); blks = PR.rec_blocks(net, nn)
    for k, (idx, start) in enumerate(dr):
        p_prev = h.get_params(0)
        batch = h.episode_get_batch(idx, start)
        for got, want in zip(batch, R.sample_batch(ring, idx, start, c.T, c.obs)):
            np.testing.assert_array_equal(np.asarray(got).reshape(want.shape), want)
        batch = tuple(np.asarray(x).reshape((c.T, c.B) + (c.obs if i in (0, 3) else ())) for i, x in enumerate(batch))
        rm, pm = PR.rec_margins(net, nn, p_prev, batch[0], batch[5])
        assert rm > E.RELU_MARGIN and pm > E.RELU_MARGIN, (k, rm, pm)
        o = PR.rec_train_grads(net, nn, p_prev, p_tg, batch, float(np.float32(c.gamma)), True)
        loss, gn = h.train_step_drqn(idx, start)
        g = h.get_grads()
        np.testing.assert_allclose(loss, o["loss"], rtol=2e-5, atol=1e-7, err_msg=f"step {k}: loss")
        R.check_grads(net, nn, g, o["grads"], live=k == 0, blks=blks)
        np.testing.assert_allclose(gn, o["grad_norm"], rtol=1e-4, err_msg=f"step {k}: grad_norm")
        R.check_params(h.get_params(0), adam.step(p_prev, g))
        assert h0.train_step_drqn(idx, start) == (loss, gn)
        np.testing.assert_array_equal(h0.get_grads(), g); np.testing.assert_array_equal(h0.get_params(0), h.get_params(0))
    names = [n for n, _ in h.profile_step(max_entries=512)]
    assert names.count("fwd_on_pool1") == 1 and names.count("fwd_tg_pool1") == 1 and names.count("bwd_pool1") == 1, names
    h.close(); h0.close()


ENV_SEED = 1      # parameter seed of the env-loop network (glorot + 0.1 N(0, 1)): its fp64 top-two gaps on the observations TestMDP (5, 5) shows stay above GAP


def _env_engine(pkg, mods, B=8, cap=64):
    nn, envs = mods[0], mods[1]
    net = nn.Chain(nn.Conv(2, 4, 8, nn.relu), nn.MaxPool(2), nn.flattenbatch, nn.Dense(32, 4))
    layers, _ = nn.lower(net)
    hp = pkg.default_hparams(batch_size=B, n_actions=4, obs_c=4, obs_h=5, obs_w=5, dueling=0, buffer_size=cap, learning_rate=1e-3, gamma=0.95, seed=5)
    h = pkg.Engine(layers, hp)
    rng = np.random.default_rng(ENV_SEED)
    p = nn.glorot_params(net, seed=ENV_SEED); p = (p + 0.1 * rng.standard_normal(p.size)).astype(np.float32)
    h.set_params(p, 0); h.sync_target()
    return h, p, envs.TestMDP((5, 5), 4, 6, n=8, seed=3)


def test_device_env_loop_acts_on_the_fp64_argmax_and_evaluates(pkg, mods):
    """the acting program of the device loop (general tail) with a pool level: 20 single-step dqn_rollout calls, eps 0, no training; at each the peeked actions equal the
    fp64 argmax on the observations peeked before the step, except where the fp64 gap is below GAP (at most 10 % of the (step, copy) pairs).  dqn_evaluate: finite averages."""
    import dqn_oracle as O
    h, p, spec = _env_engine(pkg, mods)
    onet = O.Network((4, 5, 5), [O.Conv(2, 4, 8, O.ACT_RELU), PR.MaxPool(2), O.Dense(32, 4)])
    ps = onet.unflatten(p.astype(np.float64))
    h.envs_create(spec, max_episode_length=100, seed=17)
    skipped = total = 0
    for t in range(20):
        obs = h.envs_peek()[0].copy()
        h.rollout(1, t0=t + 1, train_freq=0, target_update_freq=0, eps=(0.0, 0.0, 1.0))
        a = h.envs_peek()[1]
        q = PR._q_np(onet, ps, obs.astype(np.float64))[0]; top = np.sort(q, axis=1)
        clear = top[:, -1] - top[:, -2] >= E.GAP
        np.testing.assert_array_equal(a[clear], q.argmax(1)[clear], err_msg=f"step {t}")
        skipped += int((~clear).sum()); total += clear.size
    assert skipped <= 0.1 * total, (skipped, total)
    assert h.envs_info()[1] is False      # a pool network takes the general four-launch tail, not the fused acting head
    r, st = h.evaluate(8, 50, seed=5)
    assert np.isfinite(r) and np.isfinite(st) and st > 0
    h.close()


def test_solver_round_trip_with_a_pool_network(pkg, mods, tmp_path, monkeypatch):
    """S.solve for 300 steps with device_envs and a logdir: finite losses, qnetwork.bson holds exactly the Conv and Dense arrays, restore_best_model puts them back bit for bit
    (no learning threshold is asserted)"""
    nn, envs, S, bson = mods
    env = envs.TestMDP((5, 5), 4, 6, n=8, seed=7)
    model = nn.Chain(nn.Conv(2, 4, 8, nn.relu), nn.MaxPool(2), nn.flattenbatch, nn.Dense(32, env.n_actions))
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.05, steps=200), rng=np.random.default_rng(1))
    solver = S.DeepQLearningSolver(qnetwork=model, max_steps=300, learning_rate=0.005, exploration_policy=expl, eval_freq=100, save_freq=100, num_ep_eval=10, log_freq=100,
                                   double_q=True, dueling=False, prioritized_replay=True, train_start=64, verbose=False, logdir=str(tmp_path / "log"), device_envs=True)
    losses, saved = [], []
    real_rollout = pkg.Engine.rollout

    def rollout(self, *a, **kw):      # the device loop's train steps report their last loss and grad_norm in the rollout statistics
        st = real_rollout(self, *a, **kw)
        if st["train_steps"] > 0:
            losses.append((st["loss"], st["grad_norm"]))
        return st
    monkeypatch.setattr(pkg.Engine, "rollout", rollout)
    real_save = bson.save_qnetwork
    monkeypatch.setattr(bson, "save_qnetwork", lambda path, flat, shapes: (saved.append(np.array(flat, np.float32, copy=True)), real_save(path, flat, shapes))[1])
    policy = S.solve(solver, env)
    assert losses and np.isfinite(np.array(losses)).all(), losses
    assert np.isfinite(policy.engine.get_params(pkg.NET_ONLINE)).all()
    path = tmp_path / "log" / "qnetwork.bson"
    assert path.exists() and saved, "no model was saved"
    w, sizes = bson.load_qnetwork(path)
    np.testing.assert_array_equal(w, saved[-1])
    assert [tuple(x) for x in sizes] == [(2, 2, 4, 8), (8,), (4, 32), (4,)]      # exactly the Conv and Dense arrays: the pool holds none
    policy.engine.set_params(w * np.float32(0.5), pkg.NET_ONLINE)
    S.restore_best_model(solver, policy)
    np.testing.assert_array_equal(policy.engine.get_params(pkg.NET_ONLINE), w)
    policy.engine.close()


def test_replicas_of_a_pool_network_are_refused(pkg, monkeypatch):
    """a pool contributes nothing to the exchange, but the exchange paths have no pool network under test: dqn_comm_init and DQN_SIM_WORLD refuse, with the reason"""
    c = PR.BY_NAME["b16_max"]; net, D = PR.prepare(c)
    h, _ = PR.make_handle(pkg.Engine, c, net, D)
    with pytest.raises(PR.abi.DQNError, match=r"dqn_comm_init: layer 1 is a MaxPool / MeanPool layer; data-parallel replicas .* not supported"):
        h.comm_init(bytes(128), 0, 1)
    h.train_step(D["idx"][0])      # the engine is left as it was
    h.close()
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    with pytest.raises(PR.abi.DQNError, match=r"DQN_SIM_WORLD: layer 1 is a MaxPool / MeanPool layer"):
        PR.make_handle(pkg.Engine, c, net, D)


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (the module docstring records them)"""
    print("\nworst error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("worst gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(FR.WORST.items()) if k.startswith(("conv", "dense"))})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
