"""GPU: train steps, policy forward, device loop, solver round trip and refusals of networks with Flux GroupNorm layers (csrc/groupnorm.hip), all through the C ABI, against
the two-legged fp64 reference of groupnorm_reference.py.  Every case of its tables runs one train step under the per-step checks of the feed-forward edge tests (Q on s
and s', target Q, greedy indices exactly, y, td, loss, per-block gradients, grad_norm, parameters after fp64 Adam; tolerances are the project's existing constants,
unchanged), then use_graph 0 against 1 and a second identical run, bit for bit.  The C twin does not know the layer: parity rests on the fp64 reference plus these
bit-for-bit companions (the LayerNorm / RNN precedent).

Without the layer every test here fails at engine creation ("unknown kind 11"); on LayerNorm's law (sigma + eps) case eps_half fails by thousands of tolerances
(test_groupnorm_cpu.test_the_tests_can_tell_the_two_eps_laws_apart).

One MI355X, one run: see docs/history/groupnorm.md for the worst error / tolerance per quantity and per gradient block kind."""
import importlib
import json
import os
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import feedforward_edges_common as E
import feedforward_gpu_common as G
import groupnorm_reference as GR
import groupnorm_traits_cases as KT
import recurrent_reference as R
from drqn_common import feed

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()
nn = GR.nn
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "groupnorm_traits_gpu.json")))
FUSED = ("tiny_step", "red_head", "head_cols4", "drqn_cols")      # the whole-step and head fusions that decline a network with the layer


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "envs", "solver", "bson"))


def ff_engine(pkg, c, D, graph=1):
    layers, dueling = nn.lower(D.net); o = c.obs
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=o[0], obs_h=o[1], obs_w=o[2], dueling=int(dueling), buffer_size=c.B + 24, learning_rate=GR.LRATE, gamma=c.gamma,
                             double_q=c.dq, prioritized_replay=c.prio, obs_dtype=c.u8, use_mfma=c.mfma, use_graph=graph, seed=5)
    h = pkg.Engine(layers, hp)
    h.replay_add(D.s, D.a, D.r, D.sp, D.d); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def ff_record(h, idx):
    loss, gn, td = h.train_step(idx)
    return dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities())


def gn_launches(net, dx=True):
    """{launch name: 1} of every GroupNorm layer: two forward launches per network pass (chunk statistics, normalise), four backward launches (chunk sums, dX, row sums, dgamma / dbeta)"""
    out = {}
    for i, d in enumerate(nn.lower(net)[0]):
        if d.kind == nn._abi.LAYER_GROUPNORM:
            out.update({f"fwd_on_gn{i}_stat": 1, f"fwd_on_gn{i}": 1, f"fwd_tg_gn{i}_stat": 1, f"fwd_tg_gn{i}": 1, f"bwd_gn{i}_sums": 1, f"bwd_gn{i}": 1, f"bwd_gn{i}_rows": 1, f"bwd_gn{i}_par": 1})
    return out


def assert_launches(h, net):
    names = [n for n, _ in h.profile_step(max_entries=512)]
    tokens = [t for n in names for t in n.split("+")]
    want = gn_launches(net)
    assert want and all(tokens.count(n) == k for n, k in want.items()), (want, names)
    assert not set(FUSED) & set(tokens), names
    return names


def data_rule(c, net, p_on, p_tg, s, sp, mask=None):
    on_s = GR.probe_of(net, p_on, s, mask)
    sg = min(on_s["sigma"], GR.probe_of(net, p_on, sp, mask)["sigma"], GR.probe_of(net, p_tg, sp, mask)["sigma"])
    assert sg >= GR.SIGMA_MIN and on_s["relu"] > GR.RELU_MARGIN and on_s["pool"] > GR.RELU_MARGIN, (c.name, sg, on_s)
    assert (on_s["dead"] > 0) == bool(c.dead), (c.name, on_s)


@pytest.mark.parametrize("c", GR.CASES, ids=IDS(GR.CASES))
def test_step_vs_fp64_reference_graph_vs_eager_and_rerun(pkg, c):
    D = GR.ff_data(c); net = D.net; idx = D.idx[0]; msg = c.name
    h = ff_engine(pkg, c, D, graph=1)
    p_prev = h.get_params(0); np.testing.assert_array_equal(p_prev, D.p_on)
    batch = h.get_batch(idx)
    want_batch = GR.ff_batch(c, D, idx)
    for k, (a, b) in enumerate(zip(batch, want_batch)):      # the batch the engine trains on is the drawn rows; IS weights to 2e-6 of the fp64 law
        if k < 5:
            np.testing.assert_array_equal(np.asarray(a, np.float64).reshape(np.shape(b)), np.asarray(b, np.float64), err_msg=f"{msg}: batch[{k}]")
    E._close("is_weights", batch[5], want_batch[5], rtol=2e-6, msg=msg)
    batch = tuple(np.asarray(x).reshape(np.shape(w)) for x, w in zip(batch, want_batch))
    o = GR.ff_step(net, p_prev, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq))
    data_rule(c, net, p_prev, D.p_tg, batch[0], batch[3])
    rec = ff_record(h, idx); q = rec["q"]
    print(f"\n{msg}: loss {rec['loss']!r} (fp64 {o['loss']!r}), grad_norm {rec['gn']!r} (fp64 {o['grad_norm']!r}), max |q - q64| {np.abs(q['q_on_s'] - o['q_on_s']).max():.3g}")
    E._close("q_on_s", q["q_on_s"], o["q_on_s"], msg=msg, **GR.TOL_Q)
    E._close("q_tg_sp", q["q_tg_sp"], o["q_tg_sp"], msg=msg, **GR.TOL_Q)
    if c.dq:
        E._close("q_on_sp", q["q_on_sp"], o["q_on_sp"], msg=msg, **GR.TOL_Q)
    assert GR._gap(o["q_on_sp"] if c.dq else o["q_tg_sp"]) > GR.GAP, msg
    np.testing.assert_array_equal(q["best_a"], o["best_a"], err_msg=msg)
    E._close("y", q["y"], o["y"], msg=msg, **GR.TOL_TD)
    E._close("td", rec["td"], o["td"], msg=msg, **GR.TOL_TD)
    E._close("loss", rec["loss"], o["loss"], msg=msg, **GR.TOL_LOSS)
    assert np.isfinite(rec["g"]).all(), msg
    GR.check_grads(net, rec["g"], o["grads"], live=True)
    E._close("grad_norm", rec["gn"], o["grad_norm"], msg=msg, **GR.TOL_GN)
    GR.check_params(rec["p"], GR.Adam(D.p_on.size, lr=GR.LRATE).step(p_prev, rec["g"]))
    # eager against graph, and a second identical run: one summation order, whatever the launch mode or timing
    for graph, what in ((0, "use_graph 0 vs 1"), (1, "two identical runs")):
        h2 = ff_engine(pkg, c, D, graph=graph)
        E.same_bits([rec], [ff_record(h2, idx)], f"{msg}: {what}")
        h2.close()
    assert all(p == (0, 0, 0) for p, l in zip(h.plan(), nn.lower(net)[0]) if l.kind == nn._abi.LAYER_GROUPNORM)      # the layer's plan entry is ignored
    names = assert_launches(h, net)
    assert ("head_td" in names) or ("td_huber" in names), names
    h.close()


def test_dead_group_output_is_act_of_beta_exactly(pkg):
    """group 0 of case dead_group is identically 0 (kernel 0, bias -1, relu): x_hat = 0 * r = 0 and y = leakyrelu(fma(gamma, 0, beta)) = leakyrelu(beta_ch) EXACTLY,
    whatever the column and the row.  Read out through a Dense head that selects one feature per action (weight 1, bias 0; sums of exact zeros): features of channels
    0 and 1 (the dead group) at two positions each"""
    c = GR.BY_NAME["dead_group"]; D = GR.ff_data(c); net = D.net
    blks = dict(GR.blocks(net)); p = D.p_on.copy()
    feats = [0 * 16 + 0, 0 * 16 + 13, 1 * 16 + 5, 1 * 16 + 15]      # [c][y][x] on the (4, 4, 4) map
    W = np.zeros((64, 4), np.float32)
    for k, f in enumerate(feats):
        W[f, k] = 1.0
    p[blks["dense2.W"]] = W.reshape(-1); p[blks["dense2.b"]] = 0.0
    beta = p[blks["gn1.beta"]]
    assert (beta[:2] > 0).any() or (beta[:2] < 0).any()
    want = np.where(beta > 0, beta, np.float32(0.01) * beta).astype(np.float32)      # DQN_ACT_LEAKYRELU in fp32
    h = ff_engine(pkg, c, D); h.set_params(p, 0)
    for n in (1, 7, 8):
        q = h.forward(D.s[:n])
        np.testing.assert_array_equal(q, np.tile(want[[0, 0, 1, 1]], (n, 1)), err_msg=f"n = {n}")
    h.close()


def rec_engine(pkg, c, D, graph=1):
    layers, dueling = nn.lower(D.net)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=c.obs[0], obs_h=c.obs[1], obs_w=c.obs[2], dueling=int(dueling), buffer_size=D.cap, recurrence=1, trace_length=c.T,
                             learning_rate=GR.LRATE, prioritized_replay=0, use_mfma=c.mfma, use_graph=graph, seed=5, gamma=c.gamma, double_q=c.dq)
    h = pkg.Engine(layers, hp)
    feed(h, D.eps); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def rec_record(h, idx, start):
    loss, gn = h.train_step_drqn(idx, start)
    return dict(loss=loss, gn=gn, g=h.get_grads(), p=h.get_params(0))


@pytest.mark.parametrize("c", GR.REC_CASES, ids=IDS(GR.REC_CASES))
def test_recurrent_step_vs_fp64_reference(pkg, c):
    """Conv -> GroupNorm -> flattenbatch -> LSTM -> Dense, T = 3: the layer runs once over the T * B columns in front of the cell"""
    D = GR.rec_data(c); net = D.net; idx, start = D.draws[0]
    h = rec_engine(pkg, c, D, graph=1)
    p_prev = h.get_params(0)
    batch = h.episode_get_batch(idx, start)
    want = R.sample_batch(D.ring, idx, start, c.T, c.obs)
    for got, w in zip(batch, want):
        np.testing.assert_array_equal(np.asarray(got).reshape(w.shape), w)
    batch = tuple(np.asarray(x).reshape(w.shape) for x, w in zip(batch, want))
    data_rule(c, net, p_prev, D.p_tg, batch[0], batch[3], batch[5])
    o = GR.rec_step(net, p_prev, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq))
    rec = rec_record(h, idx, start)
    np.testing.assert_allclose(rec["loss"], o["loss"], rtol=2e-5, atol=1e-7, err_msg=f"{c.name}: loss")      # the recurrent tables' loss tolerance (test_recurrent_edges_gpu.run_checked)
    GR.check_grads(net, rec["g"], o["grads"], live=True)
    E._close("grad_norm", rec["gn"], o["grad_norm"], msg=c.name, **GR.TOL_GN)
    GR.check_params(rec["p"], GR.Adam(D.p_on.size, lr=GR.LRATE).step(p_prev, rec["g"]))
    for graph, what in ((0, "use_graph 0 vs 1"), (1, "two identical runs")):
        h2 = rec_engine(pkg, c, D, graph=graph); r2 = rec_record(h2, idx, start); h2.close()
        assert (rec["loss"], rec["gn"]) == (r2["loss"], r2["gn"]), what
        np.testing.assert_array_equal(rec["g"], r2["g"], err_msg=what); np.testing.assert_array_equal(rec["p"], r2["p"], err_msg=what)
    assert_launches(h, net)
    h.close()


@pytest.mark.parametrize("name", ["g2_b5", "chunks_b8", "hw_odd", "gn_gn"])
def test_forward_at_1_and_7_columns(pkg, name):
    """dqn_forward on 1 and 7 observations (the one-column path): within TOL_Q of fp64, and the bits the train step's Q has on the same rows -- the layer's sums have one
    order, whatever the column count, the column's position or the work split"""
    c = GR.BY_NAME[name]; D = GR.ff_data(c); h = ff_engine(pkg, c, D); idx = D.idx[0]
    f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
    fw = {n: h.forward(f(D.s[idx[:n]])) for n in (1, 7) if n <= c.B}
    for n, q in fw.items():
        E._close("policy_q", q, GR.q_values(D.net, D.p_on, f(D.s[idx[:n]])), msg=f"{name} n={n}", **GR.TOL_Q)
    h.train_step(idx)
    q_on_s = h.last_q()["q_on_s"]
    for n, q in fw.items():
        np.testing.assert_array_equal(q, q_on_s[:n], err_msg=f"{name} n={n}")
    h.close()


def test_train_steps_5_equals_five_train_step_calls(pkg):
    """dqn_train_steps(5) -- the pipelined gather and the grouped middle-step graphs -- against five dqn_train_step calls on sampled batches, bit for bit"""
    c = GR.BY_NAME["dueling"]; D = GR.ff_data(c)
    a, b = ff_engine(pkg, c, D), ff_engine(pkg, c, D)
    la = a.train_steps(5)
    for _ in range(5):
        lb = b.train_step(want_td=False)
    assert la == lb
    np.testing.assert_array_equal(a.get_params(0), b.get_params(0)); np.testing.assert_array_equal(a.get_grads(), b.get_grads())
    np.testing.assert_array_equal(a.replay_priorities(), b.replay_priorities())
    assert np.isfinite(a.get_params(0)).all() and np.abs(a.get_params(0) - D.p_on).max() > 0
    a.close(); b.close()


def _env_net():
    return nn.Chain(nn.Conv(3, 4, 8, nn.relu), nn.GroupNorm(8, 2, nn.relu), nn.flattenbatch, nn.Dense(72, 16, nn.relu), nn.Dense(16, 4))


def test_device_loop_acts_on_the_fp64_argmax_and_evaluate_leaves_the_parameters(pkg, mods):
    """TestMDP((5, 5), 4, 6), 8 copies: 12 vector steps at eps = 0; every action is the fp64 argmax where the gap is at least GAP; the acting program takes the general
    tail (fused_tail = 0)"""
    net = _env_net()
    h, p, spec = G._env_engine(pkg, mods, net)
    h.envs_create(spec, max_episode_length=100, seed=17)
    checked = 0
    for t in range(12):
        obs = h.envs_peek()[0].copy()
        h.rollout(1, t0=t + 1, train_freq=0, target_update_freq=0, eps=(0.0, 0.0, 1.0))
        a = h.envs_peek()[1]
        q = GR.q_values(net, p, obs.reshape(-1, 4, 5, 5)); top = np.sort(q, axis=1)
        clear = top[:, -1] - top[:, -2] >= GR.GAP
        np.testing.assert_array_equal(a[clear], q.argmax(1)[clear], err_msg=f"step {t}")
        checked += int(clear.sum())
    assert checked >= 0.9 * 12 * 8, checked
    assert h.envs_info() == (8, False)
    before = h.get_params(0)
    r, st = h.evaluate(8, 50, seed=5)
    assert np.isfinite(r) and np.isfinite(st) and st > 0
    np.testing.assert_array_equal(h.get_params(0), before); np.testing.assert_array_equal(h.get_params(1), before)
    h.close()


def test_solve_on_testmdp_with_device_envs_learns(pkg, mods):
    """The reference's TestMDP end-to-end test (test/runtests.jl:45-57: return >= 1.5 of the optimal 2.1) through solve with device_envs = True, with a GroupNorm in the
    trunk -- test_solve_gpu.test_testmdp_device_envs with a convolutional trunk.  The threshold is the reference's.  The budget is 3000 steps, not that test's 1000: it is
    what the SAME trunk needs WITHOUT the layer (Conv(3, 4 => 8, relu) -> Dense(72, 8, tanh) -> Dense(8, 4): return 1.1 / 1.0 / 1.1 after 1000 steps and the optimum
    2.1 after 3000 on env seeds 7 / 8 / 9; with the layer 1.1 / 1.1 / 2.1 and 2.1 / 2.1 / 2.1 -- docs/history/groupnorm.md).  The acting program takes the general tail"""
    _, envs, S, _ = mods
    env = envs.TestMDP((5, 5), 4, 6, n=16, seed=7)
    model = nn.Chain(nn.Conv(3, 4, 8, nn.relu), nn.GroupNorm(8, 2, nn.relu), nn.flattenbatch, nn.Dense(72, 8, nn.tanh), nn.Dense(8, env.n_actions))
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.01, steps=3000 / 2))
    solver = S.DeepQLearningSolver(qnetwork=model, max_steps=3000, learning_rate=0.005, exploration_policy=expl, eval_freq=1500, num_ep_eval=16, train_freq=1,
                                   log_freq=1500, double_q=False, dueling=False, prioritized_replay=True, verbose=False, logdir=None, device_envs=True,
                                   buffer_size=4096, train_start=64)
    policy = S.solve(solver, env)
    assert policy.engine.envs_info()[1] is False
    r, st = policy.engine.evaluate(32, 100, seed=99)
    print(f"\nsolve(TestMDP, device_envs) with a GroupNorm trunk: evaluate -> return {r}, steps {st}")
    assert r >= 1.5, (r, st)
    policy.engine.close()


def test_solver_round_trip(pkg, mods, tmp_path, monkeypatch):
    """solve with a logdir (save_model at save_freq), then restore_best_model: bit-identical parameters; qnetwork.bson holds [W, b, beta, gamma, W, b, W, b]"""
    G.solver_round_trip(pkg, mods, tmp_path, monkeypatch, _env_net(), [(3, 3, 4, 8), (8,), (8,), (8,), (16, 72), (16,), (4, 16), (4,)])


def test_replicas_are_refused(pkg, monkeypatch):
    c = GR.BY_NAME["g1"]; D = GR.ff_data(c)
    h = ff_engine(pkg, c, D)
    with pytest.raises(nn._abi.DQNError, match=r"dqn_comm_init: layer 1 is a GroupNorm layer; data-parallel replicas of a network with GroupNorm layers are not supported \(single GPU only\)"):
        h.comm_init(bytes(128), 0, 1)
    h.train_step(D.idx[0])      # the engine is left as it was
    h.close()
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    with pytest.raises(nn._abi.DQNError, match=r"DQN_SIM_WORLD: layer 1 is a GroupNorm layer; .*\(single GPU only\)"):
        ff_engine(pkg, c, D)


def test_the_fixture_holds_the_paths_it_was_recorded_for():
    assert set(GOLD) == set(KT.CASES)
    for k in ("gn", "gn_prio_u8", "gn_all_maps", "gn_dueling_b128", "gn_lstm"):
        toks = [t for n in GOLD[k]["step"] for t in n.split("+")]
        assert not set(FUSED) & set(toks), k
        assert {"fwd_on_gn1_stat", "fwd_on_gn1", "fwd_tg_gn1_stat", "fwd_tg_gn1", "bwd_gn1_sums", "bwd_gn1", "bwd_gn1_rows", "bwd_gn1_par"} <= set(toks), k
    assert GOLD["act_gn"]["fused_tail"] is False
    assert GOLD["refuse_gn"]["comm_init"].startswith("dqn_comm_init: layer 1 is a GroupNorm layer") and GOLD["refuse_gn"]["sim_world"].startswith("DQN_SIM_WORLD: layer 1 is a GroupNorm layer")
    assert GOLD["refuse_gn1_pool3"]["comm_init"].startswith("dqn_comm_init: layer 3 is a MaxPool / MeanPool layer")      # the existing kinds keep their place in the order


@pytest.mark.parametrize("name", sorted(KT.CASES))
def test_the_program_is_the_recorded_program(name):
    assert KT.observe(name) == GOLD[name]


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (docs/history/groupnorm.md records them)"""
    print("\nWORST error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("WORST gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(R.WORST.items())})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
