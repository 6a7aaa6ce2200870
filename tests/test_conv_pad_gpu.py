"""GPU: train steps, policy forward, device loop and refusals of networks with a PADDED convolution (csrc/conv_pad.hip) against the two-legged fp64 reference of
conv_pad_reference.py.  Every case of conv_pad_reference.CASES runs three train steps on given indices under the shared per-step checks of the feed-forward edge
tests (Q, greedy indices exactly, y, td, loss, per-block gradients, grad_norm, parameters after fp64 Adam, priorities; tolerances unchanged); use_graph 0 and 1 and
use_mfma 0 and 1 must give identical bits.

The exact check: every case whose padded conv is the first layer also runs as the SAME network with pad = 0 on observations zero-extended by (ph, pw) (a 0 byte
border for u8), same parameters, same explicit plan -- a network the existing suite holds bit-exact to the CPU twin -- and everything recorded for three steps must
be equal bit for bit: the padded path's canonical-order leg ("Padded convolutions").

Beyond the train step: the recurrent Conv(pad=1) -> LSTM chain over T*B columns, the policy forward and greedy action, the device environment loop against the fp64
argmax, dqn_evaluate, the solver round trip (qnetwork.bson, restore_best_model), dqn_n_params, and the refusals through the C ABI, replicas included.

One MI355X, one run: 40 tests in 3 s.  Worst error / tolerance per quantity (1.0 = at the bound): q_on_s 0.040, q_on_sp 0.045, q_tg_sp 0.050, policy_q 0.033, y 0.016,
td 0.024, loss 0.043, grad_norm 0.003, is_weights 0.056; worst gradient error / max |g| per block kind: conv.W 6.3e-07, conv.b 7.3e-07, dense.W 3.7e-07, dense.b 2.8e-07
(GRAD_C = 2e-5)."""
import importlib
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import conv_pad_reference as CR
import feedforward_edges_common as E
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
    h, rec = CR.run_checked(pkg.Engine, c)
    E.same_bits(rec, CR.replay_steps(pkg.Engine, c, graph=1 - c.graph), f"{c.name}: use_graph {c.graph} vs {1 - c.graph}")
    E.same_bits(rec, CR.replay_steps(pkg.Engine, c, mfma=1 - c.mfma), f"{c.name}: use_mfma {c.mfma} vs {1 - c.mfma}")
    names = [n for n, _ in h.profile_step()]
    net = CR.network(c)
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
    c = CR.BY_NAME[name]; net, D = CR.prepare(c)
    ha, _ = CR.make_handle(pkg.Engine, c, net, D, mfma=mfma); plan = ha.plan(); ha.close()
    a = CR.replay_steps(pkg.Engine, c, mfma=mfma, plan=plan)
    layers, view, s, sp = CR.extended(c, net, D)
    b = CR.replay_steps(pkg.Engine, c, mfma=mfma, plan=plan, layers=layers, hp_net=view, s=s, sp=sp)
    E.same_bits(a, b, f"{name} (use_mfma {mfma}): pad vs pad 0 on the extended map")


@pytest.mark.parametrize("name", ["same3", "stride2", "interior", "pool_before", "dueling_u8"])
def test_policy_forward_and_greedy_action(pkg, name):
    c = CR.BY_NAME[name]; net, D = CR.prepare(c)
    h, _ = CR.make_handle(pkg.Engine, c, net, D)
    f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
    ps = net.unflatten(D["p_on"].astype(np.float64))
    for n in (1, 3):
        obs = f(D["s"][:n])
        q64 = CR._q_np(net, ps, obs.astype(np.float64))[0]
        E._close("policy_q", h.forward(obs), q64, msg=f"{name} n={n}", **E.TOL_Q)
        a = h.greedy_action(obs); t = np.sort(q64, axis=1)
        clear = t[:, -1] - t[:, -2] >= E.GAP
        np.testing.assert_array_equal(np.asarray(a)[clear], q64.argmax(1)[clear])
    h.close()


def test_n_params_is_unchanged_by_pad(pkg):
    c = CR.BY_NAME["rect"]; net, D = CR.prepare(c)
    h, _ = CR.make_handle(pkg.Engine, c, net, D)
    assert h.P == net.n_params() == D["p_on"].size
    h.close()


def test_recurrent_padded_conv_lstm_chain(pkg, mods):
    """Conv(3, 1=>8, relu; pad=1) -> LSTM(200, 8) -> Dense(8, 4), T = 3, B = 4: the padded layer runs once over the T*B columns.  The checker of
    test_pool_gpu's recurrent case with this module's chain; use_graph 0 equals 1 bit for bit."""
    import pool_reference as PR
    import recurrent_reference as R
    from drqn_common import feed
    nn = mods[0]; c = CR.REC
    net, cap, eps, ring, p_on, p_tg, dr = CR.rec_data(nn)
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
        batch = tuple(np.asarray(x).reshape((c.T, c.B) + (c.obs if i in (0, 3) else ())) for i, x in enumerate(batch))
        assert CR.rec_margin(net, nn, p_prev, batch[0], batch[5]) > E.RELU_MARGIN, k
        o = CR.rec_train_grads(net, nn, p_prev, p_tg, batch, float(np.float32(c.gamma)), True)
        loss, gn = h.train_step_drqn(idx, start)
        g = h.get_grads()
        np.testing.assert_allclose(loss, o["loss"], rtol=2e-5, atol=1e-7, err_msg=f"step {k}: loss")
        R.check_grads(net, nn, g, o["grads"], live=k == 0, blks=blks)
        np.testing.assert_allclose(gn, o["grad_norm"], rtol=1e-4, err_msg=f"step {k}: grad_norm")
        R.check_params(h.get_params(0), adam.step(p_prev, g))
        assert h0.train_step_drqn(idx, start) == (loss, gn)
        np.testing.assert_array_equal(h0.get_grads(), g); np.testing.assert_array_equal(h0.get_params(0), h.get_params(0))
    names = [n for n, _ in h.profile_step(max_entries=512)]
    assert names.count("fwd_on_conv0") == 1 and names.count("fwd_tg_conv0") == 1 and names.count("dw_conv0") == 1 and names.count("bwd_conv0") == 0, names
    h.close(); h0.close()


ENV_SEED = 1      # parameter seed of the env-loop network (glorot + 0.1 N(0, 1))


def _env_engine(pkg, mods, B=8, cap=64):
    nn, envs = mods[0], mods[1]
    net = nn.Chain(nn.Conv(3, 4, 8, nn.relu, pad=1), nn.flattenbatch, nn.Dense(200, 4))
    layers, _ = nn.lower(net)
    hp = pkg.default_hparams(batch_size=B, n_actions=4, obs_c=4, obs_h=5, obs_w=5, dueling=0, buffer_size=cap, learning_rate=1e-3, gamma=0.95, seed=5)
    h = pkg.Engine(layers, hp)
    rng = np.random.default_rng(ENV_SEED)
    p = nn.glorot_params(net, seed=ENV_SEED); p = (p + 0.1 * rng.standard_normal(p.size)).astype(np.float32)
    h.set_params(p, 0); h.sync_target()
    return h, p, envs.TestMDP((5, 5), 4, 6, n=8, seed=3)


def test_device_env_loop_acts_on_the_fp64_argmax_and_evaluates(pkg, mods):
    """the acting program of the device loop with a first-layer pad = 1 trunk: 20 single-step dqn_rollout calls, eps 0, no training; at each the peeked actions equal the
    fp64 argmax on the observations peeked before the step, except where the fp64 gap is below GAP (at most 10 % of the (step, copy) pairs).  dqn_evaluate: finite averages."""
    import dqn_oracle as O
    h, p, spec = _env_engine(pkg, mods)
    onet = O.Network((4, 5, 5), [CR.PConv(3, 4, 8, O.ACT_RELU, pad=1), O.Dense(200, 4)])
    ps = onet.unflatten(p.astype(np.float64))
    h.envs_create(spec, max_episode_length=100, seed=17)
    skipped = total = 0
    for t in range(20):
        obs = h.envs_peek()[0].copy()
        h.rollout(1, t0=t + 1, train_freq=0, target_update_freq=0, eps=(0.0, 0.0, 1.0))
        a = h.envs_peek()[1]
        q = CR._q_np(onet, ps, obs.astype(np.float64))[0]; top = np.sort(q, axis=1)
        clear = top[:, -1] - top[:, -2] >= E.GAP
        np.testing.assert_array_equal(a[clear], q.argmax(1)[clear], err_msg=f"step {t}")
        skipped += int((~clear).sum()); total += clear.size
    assert skipped <= 0.1 * total, (skipped, total)
    assert h.envs_info()[1] is False      # a network with a padded conv takes the general acting tail, not the fused acting head
    r, st = h.evaluate(8, 50, seed=5)
    assert np.isfinite(r) and np.isfinite(st) and st > 0
    h.close()


def test_solver_round_trip_with_a_padded_conv_network(pkg, mods, tmp_path, monkeypatch):
    """S.solve for 300 steps with device_envs and a logdir: finite losses, qnetwork.bson holds the Conv and Dense arrays (the pad is no parameter), restore_best_model
    puts them back bit for bit (no learning threshold is asserted)"""
    nn, envs, S, bson = mods
    env = envs.TestMDP((5, 5), 4, 6, n=8, seed=7)
    model = nn.Chain(nn.Conv(3, 4, 8, nn.relu, pad=nn.SamePad()), nn.flattenbatch, nn.Dense(200, env.n_actions))
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.05, steps=200), rng=np.random.default_rng(1))
    solver = S.DeepQLearningSolver(qnetwork=model, max_steps=300, learning_rate=0.005, exploration_policy=expl, eval_freq=100, save_freq=100, num_ep_eval=10, log_freq=100,
                                   double_q=True, dueling=False, prioritized_replay=True, train_start=64, verbose=False, logdir=str(tmp_path / "log"), device_envs=True)
    losses, saved = [], []
    real_rollout = pkg.Engine.rollout

    def rollout(self, *a, **kw):
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
    assert [tuple(x) for x in sizes] == [(3, 3, 4, 8), (8,), (4, 200), (4,)]
    policy.engine.set_params(w * np.float32(0.5), pkg.NET_ONLINE)
    S.restore_best_model(solver, policy)
    np.testing.assert_array_equal(policy.engine.get_params(pkg.NET_ONLINE), w)
    policy.engine.close()


def test_refusals_through_the_c_abi(pkg, monkeypatch):
    abi = CR.abi
    def create(layers, obs, nA=4):
        net = type("N", (), dict(obs_shape=obs, n_actions=nA, dueling=False))
        return pkg.Engine(layers, CR.ref.hparams_for(net, batch_size=8, buffer_size=32))
    def L(kind, n_in=0, n_out=0, cin=0, cout=0, k=0, s=0):
        d = abi.LayerDesc(); d.kind, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, n_in, n_out, cin, cout, k, k, s, s
        return d
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv pad \(3, 3\) is larger than kernel - 1 = \(2, 2\)"):
        create([L(abi.LAYER_CONV, 3, 3, cin=1, cout=2, k=3, s=1), L(abi.LAYER_DENSE, n_in=200, n_out=4)], (1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv pad \(0, -2\) must not be negative"):
        create([L(abi.LAYER_CONV, 0, -2, cin=1, cout=2, k=3, s=1), L(abi.LAYER_DENSE, n_in=8, n_out=4)], (1, 6, 6))
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv kernel \(5, 5\) / stride \(1, 1\) does not fit the 2x2 input map extended by pad \(1, 1\)"):
        create([L(abi.LAYER_CONV, 1, 1, cin=1, cout=2, k=5, s=1), L(abi.LAYER_DENSE, n_in=8, n_out=4)], (1, 2, 2))
    c = CR.BY_NAME["one_axis"]; net, D = CR.prepare(c)
    h, _ = CR.make_handle(pkg.Engine, c, net, D)
    with pytest.raises(abi.DQNError, match=r"dqn_comm_init: layer 0 is a Conv with pad \(1, 0\); data-parallel replicas .* not supported"):
        h.comm_init(bytes(128), 0, 1)
    h.train_step(D["idx"][0])      # the engine is left as it was
    h.close()
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    with pytest.raises(abi.DQNError, match=r"DQN_SIM_WORLD: layer 0 is a Conv with pad \(1, 0\)"):
        CR.make_handle(pkg.Engine, c, net, D)


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file"""
    print("\nworst error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("worst gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(FR.WORST.items()) if k.startswith(("conv", "dense"))})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
