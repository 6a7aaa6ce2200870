"""GPU: train steps, policy forward, device loops, solver round trip and refusals of networks with Flux LayerNorm layers (csrc/layernorm.hip), all through the C ABI,
against the two-legged fp64 reference of layernorm_reference.py.  Every case of its tables runs one train step under the per-step checks of the feed-forward edge tests
(Q on s and s', target Q, greedy indices exactly, y, td, loss, per-block gradients -- live --, grad_norm, parameters after fp64 Adam; tolerances are the project's existing
constants, unchanged), then use_graph 0 against 1 and a second identical run, bit for bit.  The C twin does not know the layer: parity rests on the fp64 reference plus
these bit-for-bit companions (the RNN precedent).

Without the layer every test here fails at engine creation ("unknown kind 7"); on torch's law (sqrt(var + eps)) case eps_half fails by thousands of tolerances
(test_layernorm_cpu.test_the_tests_can_tell_fluxs_law_from_torchs).

One MI355X, one run: see docs/history/layernorm.md for the worst error / tolerance per quantity and per gradient block kind."""
import importlib
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import feedforward_edges_common as E
import feedforward_gpu_common as G
import layernorm_reference as LR
import recurrent_reference as R
from drqn_common import feed

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()
nn = LR.nn


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "envs", "solver", "bson"))


def _obs3(obs):
    return tuple(obs) + (1,) * (3 - len(obs))


def ff_engine(pkg, c, D, graph=1, prio=None):
    layers, dueling = nn.lower(D.net); o = _obs3(c.obs)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=o[0], obs_h=o[1], obs_w=o[2], dueling=int(dueling), buffer_size=c.B + 24, learning_rate=LR.LR, gamma=c.gamma,
                             double_q=c.dq, prioritized_replay=c.prio if prio is None else prio, obs_dtype=c.u8, use_mfma=c.mfma, use_graph=graph, seed=5)
    h = pkg.Engine(layers, hp)
    h.replay_add(D.s, D.a, D.r, D.sp, D.d); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def ff_record(h, idx):
    loss, gn, td = h.train_step(idx)
    return dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities())


def ln_launches(net):
    """{launch name: 1} of every LayerNorm layer: one forward launch per network pass, one backward entry"""
    out = {}
    for i, l in enumerate(nn.all_layers(net)):
        if l.kind == "layernorm":
            out.update({f"fwd_on_ln{i}": 1, f"fwd_tg_ln{i}": 1, f"bwd_ln{i}": 1})
    return out


FUSED = ("tiny_step", "red_head", "head_cols4", "drqn_cols")      # the whole-step and head fusions that decline a network with the layer


def assert_launches(h, net):
    names = [n for n, _ in h.profile_step(max_entries=512)]
    tokens = [t for n in names for t in n.split("+")]
    want = ln_launches(net)
    assert want and all(tokens.count(n) == k for n, k in want.items()), (want, names)
    assert not set(FUSED) & set(tokens), names
    return names


@pytest.mark.parametrize("c", LR.CASES, ids=IDS(LR.CASES))
def test_step_vs_fp64_reference_graph_vs_eager_and_rerun(pkg, c):
    D = LR.ff_data(c); net = D.net; idx = D.idx[0]; msg = c.name
    h = ff_engine(pkg, c, D, graph=1)
    p_prev = h.get_params(0); np.testing.assert_array_equal(p_prev, D.p_on)
    batch = h.get_batch(idx)
    o = LR.ff_step(net, p_prev, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq))
    for k, (a, b) in enumerate(zip(batch, LR.ff_batch(c, D, idx))):      # the batch the engine trains on is the drawn rows; IS weights: unequal, to 2e-6 of the fp64 law
        if k < 5:
            np.testing.assert_array_equal(np.asarray(a, np.float64).reshape(np.shape(b)), np.asarray(b, np.float64), err_msg=f"{msg}: batch[{k}]")
    E._close("is_weights", batch[5], LR.ff_batch(c, D, idx)[5], rtol=2e-6, msg=msg)
    assert np.ptp(batch[5]) > 1e-3, "the IS weights of the batch are trivial"
    sg = min(LR.sigma_min(net, p_prev, batch[0]), LR.sigma_min(net, p_prev, batch[3]), LR.sigma_min(net, D.p_tg, batch[3]))
    assert sg >= LR.SIGMA_MIN and LR.relu_margin(net, p_prev, batch[0]) > LR.RELU_MARGIN, (msg, sg)
    rec = ff_record(h, idx); q = rec["q"]
    E._close("q_on_s", q["q_on_s"], o["q_on_s"], msg=msg, **LR.TOL_Q)
    E._close("q_tg_sp", q["q_tg_sp"], o["q_tg_sp"], msg=msg, **LR.TOL_Q)
    if c.dq:
        E._close("q_on_sp", q["q_on_sp"], o["q_on_sp"], msg=msg, **LR.TOL_Q)
    assert LR._gap(o["q_on_sp"] if c.dq else o["q_tg_sp"]) > LR.GAP, msg
    np.testing.assert_array_equal(q["best_a"], o["best_a"], err_msg=msg)
    E._close("y", q["y"], o["y"], msg=msg, **LR.TOL_TD)
    E._close("td", rec["td"], o["td"], msg=msg, **LR.TOL_TD)
    E._close("loss", rec["loss"], o["loss"], msg=msg, **LR.TOL_LOSS)
    LR.check_grads(net, rec["g"], o["grads"], live=True, exempt=c.dead)
    E._close("grad_norm", rec["gn"], o["grad_norm"], msg=msg, **LR.TOL_GN)
    LR.check_params(rec["p"], LR.Adam(D.p_on.size, lr=LR.LR).step(p_prev, rec["g"]))
    # eager against graph, and a second identical run: one summation order, whatever the launch mode or timing
    for graph, what in ((0, "use_graph 0 vs 1"), (1, "two identical runs")):
        h2 = ff_engine(pkg, c, D, graph=graph)
        E.same_bits([rec], [ff_record(h2, idx)], f"{msg}: {what}")
        h2.close()
    assert all(p == (0, 0, 0) for p, l in zip(h.plan(), nn.lower(net)[0]) if l.kind == LR.nn._abi.LAYER_LAYERNORM)      # the layer's plan entry is ignored
    names = assert_launches(h, net)
    assert ("head_td" in names) or ("td_huber" in names), names
    h.close()


def rec_engine(pkg, c, D, graph=1, env=None, monkeypatch=None):
    layers, dueling = nn.lower(D.net)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=c.obs[0], dueling=int(dueling), buffer_size=D.cap, recurrence=1, trace_length=c.T, learning_rate=LR.LR,
                             prioritized_replay=0, use_mfma=c.mfma, use_graph=graph, seed=5, gamma=c.gamma, double_q=c.dq)
    if env:
        monkeypatch.setenv(env, "1")
    try:
        h = pkg.Engine(layers, hp)
    finally:
        if env:
            monkeypatch.delenv(env, raising=False)
    feed(h, D.eps); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def rec_record(h, idx, start):
    loss, gn = h.train_step_drqn(idx, start)
    return dict(loss=loss, gn=gn, g=h.get_grads(), p=h.get_params(0))


def rec_same(a, b, what):
    assert (a["loss"], a["gn"]) == (b["loss"], b["gn"]), what
    np.testing.assert_array_equal(a["g"], b["g"], err_msg=what); np.testing.assert_array_equal(a["p"], b["p"], err_msg=what)


@pytest.mark.parametrize("c", LR.REC_CASES, ids=IDS(LR.REC_CASES))
def test_recurrent_step_vs_fp64_reference_on_both_recurrence_schedules(pkg, c, monkeypatch):
    """LSTM(6, 8) -> LN(8) -> Dense(8, 3) and GRU(6, 8) -> LN(8, tanh) -> dueling heads, T = 3: the layer runs once over the T * B columns and hands its dX to the cell's dH.
    B = 4 takes the per-step recurrence launches (H * B = 32), B = 8 the whole-sequence kernels; the GRU at B = 8 also runs under DQN_GRU_STEPWISE, bit for bit"""
    D = LR.rec_data(c); net = D.net; idx, start = D.draws[0]; kind = nn.all_layers(net)[0].kind
    h = rec_engine(pkg, c, D, graph=1)
    p_prev = h.get_params(0)
    batch = h.episode_get_batch(idx, start)
    for got, want in zip(batch, R.sample_batch(D.ring, idx, start, c.T, c.obs)):
        np.testing.assert_array_equal(np.asarray(got).reshape(want.shape), want)
    sg = min(LR.sigma_min(net, p_prev, batch[0]), LR.sigma_min(net, p_prev, batch[3]), LR.sigma_min(net, D.p_tg, batch[3]))
    assert sg >= LR.SIGMA_MIN, (c.name, sg)
    o = LR.rec_step(net, p_prev, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq))
    rec = rec_record(h, idx, start)
    np.testing.assert_allclose(rec["loss"], o["loss"], rtol=2e-5, atol=1e-7, err_msg=f"{c.name}: loss")      # the recurrent tables' loss tolerance (test_recurrent_edges_gpu.run_checked)
    LR.check_grads(net, rec["g"], o["grads"], live=True)
    E._close("grad_norm", rec["gn"], o["grad_norm"], msg=c.name, **LR.TOL_GN)
    LR.check_params(rec["p"], LR.Adam(D.p_on.size, lr=LR.LR).step(p_prev, rec["g"]))
    for graph, what in ((0, "use_graph 0 vs 1"), (1, "two identical runs")):
        h2 = rec_engine(pkg, c, D, graph=graph); rec_same(rec, rec_record(h2, idx, start), f"{c.name}: {what}"); h2.close()
    names = assert_launches(h, net)
    seq = c.B == 8
    assert (f"{kind}_seq_dense0" in names) == seq and (f"{kind}_step_dense0" in names) == (not seq), names
    if kind == "gru" and seq:
        h3 = rec_engine(pkg, c, D, env="DQN_GRU_STEPWISE", monkeypatch=monkeypatch)
        rec_same(rec, rec_record(h3, idx, start), f"{c.name}: per-step schedule")
        assert "gru_step_dense0" in [n for n, _ in h3.profile_step(max_entries=512)]
        h3.close()
    h.close()


@pytest.mark.parametrize("name", ["n5_b32", "n512_b32"])
def test_train_steps_5_equals_five_train_step_calls(pkg, name):
    """dqn_train_steps(5) -- the pipelined gather and the grouped middle-step graphs -- against five dqn_train_step calls on sampled batches, bit for bit"""
    c = LR.BY_NAME[name]; D = LR.ff_data(c)
    a, b = ff_engine(pkg, c, D, prio=1), ff_engine(pkg, c, D, prio=1)
    la = a.train_steps(5)
    for _ in range(5):
        lb = b.train_step(want_td=False)
    assert la == lb
    np.testing.assert_array_equal(a.get_params(0), b.get_params(0)); np.testing.assert_array_equal(a.get_grads(), b.get_grads())
    np.testing.assert_array_equal(a.replay_priorities(), b.replay_priorities())
    for x, y in zip(a.get_adam_state(), b.get_adam_state()):
        np.testing.assert_array_equal(x, y)
    assert np.abs(a.get_params(0) - D.p_on).max() > 0
    a.close(); b.close()


@pytest.mark.parametrize("name", ["n65_b32", "two_layers", "dueling_prio"])
def test_three_steps_of_fp64_adam(pkg, name):
    """an fp64 Adam carried over three steps on the engine's own gradients: every parameter, the scale / bias blocks included, within check_params"""
    c = LR.BY_NAME[name]; D = LR.ff_data(c); h = ff_engine(pkg, c, D)
    adam = LR.Adam(D.p_on.size, lr=LR.LR); blks = dict(LR.blocks(D.net))
    for k in range(3):
        p_prev = h.get_params(0)
        h.train_step(D.idx[k])
        g, p = h.get_grads(), h.get_params(0)
        LR.check_params(p, adam.step(p_prev, g))
        for nm, sl in blks.items():
            if nm.startswith("ln"):
                assert np.abs(g[sl]).max() > 0 and np.abs(p[sl] - p_prev[sl]).max() > 0, (k, nm)
    E._close("beta_powers", h.get_adam_state()[2], [0.9 ** 4, 0.999 ** 4], rtol=1e-12, msg=name)
    h.close()


@pytest.mark.parametrize("name", ["n5_b32", "n65_b32", "n512_b32"])
def test_forward_at_1_and_7_columns(pkg, name):
    """dqn_forward on 1 and 7 observations (odd column counts: the scalar column path): within TOL_Q of fp64, and the bits the train step's Q has on the same rows --
    the layer's sums over the features have one order, whatever the column count or the work split"""
    c = LR.BY_NAME[name]; D = LR.ff_data(c); h = ff_engine(pkg, c, D); idx = D.idx[0]
    fw = {n: h.forward(D.s[idx[:n]]) for n in (1, 7)}
    for n, q in fw.items():
        E._close("policy_q", q, LR.q_values(D.net, D.p_on, D.s[idx[:n]]), msg=f"{name} n={n}", **LR.TOL_Q)
    h.train_step(idx)
    q_on_s = h.last_q()["q_on_s"]
    for n, q in fw.items():
        np.testing.assert_array_equal(q, q_on_s[:n], err_msg=f"{name} n={n}")
    h.close()


def _env_net():
    return nn.Chain(nn.Dense(100, 16, nn.relu), nn.LayerNorm(16), nn.Dense(16, 4))


def test_device_loop_acts_on_the_fp64_argmax_and_evaluate_leaves_the_parameters(pkg, mods):
    """TestMDP((5, 5), 4, 6), 8 copies, Dense(100, 16, relu) -> LN(16) -> Dense(16, 4): 12 vector steps at eps = 0; every action is the fp64 argmax where the gap is at
    least GAP; the acting program takes the general tail (fused_tail = 0)"""
    net = _env_net()
    h, p, spec = G._env_engine(pkg, mods, net)
    h.envs_create(spec, max_episode_length=100, seed=17)
    checked = 0
    for t in range(12):
        obs = h.envs_peek()[0].copy()
        h.rollout(1, t0=t + 1, train_freq=0, target_update_freq=0, eps=(0.0, 0.0, 1.0))
        a = h.envs_peek()[1]
        q = LR.q_values(net, p, obs); top = np.sort(q, axis=1)
        clear = top[:, -1] - top[:, -2] >= LR.GAP
        np.testing.assert_array_equal(a[clear], q.argmax(1)[clear], err_msg=f"step {t}")
        checked += int(clear.sum())
    assert checked >= 0.9 * 12 * 8, checked
    assert h.envs_info() == (8, False)
    before = h.get_params(0)
    r, st = h.evaluate(8, 50, seed=5)
    assert np.isfinite(r) and np.isfinite(st) and st > 0
    np.testing.assert_array_equal(h.get_params(0), before); np.testing.assert_array_equal(h.get_params(1), before)
    h.close()


@pytest.mark.parametrize("explore", [None, ("softmax", 0.5)])
def test_device_loop_trains_under_both_exploration_modes(pkg, mods, explore):
    """the env-cadence graphs (acting step + pipelined train steps) with the layer in both programs: finite losses, parameters move"""
    net = _env_net()
    h, p, spec = G._env_engine(pkg, mods, net)
    h.envs_create(spec, max_episode_length=100, seed=17)
    st = h.rollout(24, t0=1, train_freq=2, target_update_freq=8, eps=(1.0, 0.1, 20.0), explore=explore)
    assert st["train_steps"] > 0 and np.isfinite(st["loss"]) and np.isfinite(st["grad_norm"]), st
    pn = h.get_params(0)
    assert np.isfinite(pn).all() and np.abs(pn - p).max() > 0
    h.close()


def test_recurrent_device_loop_commits_episodes_and_trains(pkg, mods):
    """the network of case 11 at SimpleGridWorld's shapes (2 features, 4 actions): the recurrent acting program runs the layer between the cell and the head,
    episodes are committed on the device, one recurrent train step on them is finite and moves every block (a smoke run)"""
    envs = mods[1]
    net = nn.Chain(nn.LSTM(2, 8), nn.LayerNorm(8), nn.Dense(8, 4))
    layers, _ = nn.lower(net)
    hp = pkg.default_hparams(batch_size=4, n_actions=4, obs_c=2, dueling=0, buffer_size=16, recurrence=1, trace_length=3, learning_rate=LR.LR, prioritized_replay=0, seed=5, gamma=0.95)
    h = pkg.Engine(layers, hp)
    p = nn.glorot_params(net, seed=2); p = (p + 0.05 * np.random.default_rng(2).standard_normal(p.size)).astype(np.float32)
    h.set_params(p, 0); h.sync_target()
    h.envs_create(envs.SimpleGridWorld(n=8, seed=3), n_envs=8, max_episode_length=20, seed=11)
    h.rollout(200, t0=1, train_freq=0, target_update_freq=0, eps=(1.0, 1.0, 1.0))      # an episode is committed when it reaches a terminal cell (truncation leaves it open)
    assert h.episode_count()[0] >= 4 and h.envs_info() == (8, False), h.episode_count()
    loss, gn = h.train_step_drqn()
    assert np.isfinite(loss) and np.isfinite(gn) and gn > 0
    g = h.get_grads()
    for nm, sl in LR.blocks(net):
        assert np.isfinite(g[sl]).all() and (not nm.startswith("ln") or np.abs(g[sl]).max() > 0), nm
    assert np.abs(h.get_params(0) - p).max() > 0
    h.close()


def test_solver_round_trip(pkg, mods, tmp_path, monkeypatch):
    """solve with a logdir (save_model at save_freq), then restore_best_model: bit-identical parameters; qnetwork.bson holds [W, b, scale, bias, W, b]"""
    G.solver_round_trip(pkg, mods, tmp_path, monkeypatch, _env_net(), [(16, 100), (16,), (16,), (16,), (4, 16), (4,)])


def test_replicas_are_refused(pkg, monkeypatch):
    c = LR.BY_NAME["n5_b32"]; D = LR.ff_data(c)
    h = ff_engine(pkg, c, D)
    with pytest.raises(nn._abi.DQNError, match=r"dqn_comm_init: layer 1 is a LayerNorm layer; data-parallel replicas .* not supported \(single GPU only\)"):
        h.comm_init(bytes(128), 0, 1)
    h.train_step(D.idx[0])      # the engine is left as it was
    h.close()
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    with pytest.raises(nn._abi.DQNError, match=r"DQN_SIM_WORLD: layer 1 is a LayerNorm layer; .*\(single GPU only\)"):
        ff_engine(pkg, c, D)


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (docs/history/layernorm.md records them)"""
    print("\nWORST error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("WORST gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(R.WORST.items())})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
