"""GPU: train steps, every forward pass, device loops, resume, solver round trip and refusals of networks with Flux SkipConnection(layers, +) blocks (csrc/skip.hip), all
through the C ABI.  The join is read out EXACTLY through identity weights (Q = 3x in every pass); every case of skip_reference.py's tables then runs three train steps,
each against the two-legged fp64 reference at the engine's own previous parameters and batch, with the per-step checks of the LayerNorm / Dropout tests (Q on s and s',
target Q, greedy indices exactly under GAP, y, td, loss, per-block gradients -- live on the first step --, grad_norm, parameters after fp64 Adam, priorities; tolerances are
the project's existing constants, unchanged), then use_graph 0 against 1, use_mfma 0 against 1 and a second identical run, bit for bit.  The C twin does not know the
layer: parity rests on the fp64 reference plus these bit-for-bit companions (the RNN / LayerNorm / Dropout precedent).

Without the layer every test here fails: nn.SkipConnection is missing, and the engine answers "unknown kind 9".  Each wrong engine -- the entry gradient without + dY,
the entry's derivative before the sum or twice, the last inner layer's derivative omitted, its pre-activation added, the skip read from the first inner layer -- is off
by thousands of tolerances on every case it applies to (test_skip_cpu.test_the_tests_can_tell).

One MI355X, one run: docs/history/skip.md records the worst error / tolerance per quantity and per gradient block kind."""
import importlib
import os
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_gpu_common as G
import layernorm_reference as LR
import recurrent_reference as R
import skip_reference as SR
from drqn_common import feed

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()
nn = SR.nn
FUSED = ("tiny_step", "red_head", "head_cols4", "drqn_cols")      # the whole-step and head fusions that decline a network with the layer


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "envs", "solver", "bson"))


def tokens(h):
    return [t for nm, _ in h.profile_step(max_entries=512) for t in nm.split("+")]


# ------------------------------------------------------------------ 1: the join, read out exactly
READOUT = [(n, B) for n in (5, 8, 33, 64) for B in (4, 5, 6, 32)] + [(64, 128)]


@pytest.mark.parametrize("n,B", READOUT, ids=[f"n{n}_b{B}" for n, B in READOUT])
def test_exact_readout_q_is_3x_in_every_pass(pkg, n, B):
    """Dense(n, n), W = I -> block around Dense(n, n), W = 2I -> Dense(n, n), W = I on small-integer observations: Q = 3x exactly -- online on s and s', target,
    dqn_forward on 1 and 7 columns, dqn_greedy_action -- under use_graph 1 and 0"""
    net = nn.Chain(nn.Dense(n, n), nn.SkipConnection(nn.Dense(n, n), "+"), nn.Dense(n, n))
    I = np.eye(n, dtype=np.float32).ravel(); z = np.zeros(n, np.float32); flat = np.concatenate([I, z, 2 * I, z, I, z])
    rng = np.random.default_rng(n * 1000 + B); m = B + 8
    s, sp = (rng.integers(-8, 9, (m, n)).astype(np.float32) for _ in range(2))
    idx = rng.permutation(m)[:B].astype(np.int64)
    for graph in (1, 0):
        hp = pkg.default_hparams(batch_size=B, n_actions=n, obs_c=n, dueling=0, buffer_size=m, learning_rate=0.0, gamma=0.95, prioritized_replay=0, use_graph=graph, seed=SR.ENGINE_SEED)
        h = pkg.Engine(nn.lower(net)[0], hp)
        h.replay_add(s, rng.integers(0, n, m).astype(np.int32), rng.standard_normal(m).astype(np.float32), sp, (rng.random(m) < 0.2).astype(np.uint8))
        h.set_params(flat, 0); h.set_params(flat, 1)
        h.train_step(idx); q = h.last_q()
        np.testing.assert_array_equal(q["q_on_s"], 3 * s[idx]); np.testing.assert_array_equal(q["q_on_sp"], 3 * sp[idx]); np.testing.assert_array_equal(q["q_tg_sp"], 3 * sp[idx])
        rows = np.concatenate([idx, idx])[:7]
        for k in (1, 7):
            np.testing.assert_array_equal(h.forward(s[rows[:k]]), 3 * s[rows[:k]])
            np.testing.assert_array_equal(h.forward(sp[rows[:k]], which=pkg.NET_TARGET), 3 * sp[rows[:k]])
        np.testing.assert_array_equal(h.greedy_action(s[rows]), (3 * s[rows]).argmax(1))
        names = tokens(h)
        assert names.count("fwd_on_skip2") == 1 and names.count("fwd_tg_skip2") == 1 and names.count("bwd_entry_skip2") == 1 and "bwd_join_skip2" not in names, names      # the join's backward is an alias
        assert not set(FUSED) & set(names), names
        h.close()


# ------------------------------------------------------------------ 2: three train steps against the fp64 reference
def _obs3(obs):
    return tuple(obs) + (1,) * (3 - len(obs))


def ff_engine(pkg, c, D, graph=1, prio=None, mfma=None):
    layers, dueling = nn.lower(D.net); o = _obs3(c.obs)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=o[0], obs_h=o[1], obs_w=o[2], dueling=int(dueling), buffer_size=c.B + 24, learning_rate=LR.LR, gamma=c.gamma,
                             double_q=c.dq, prioritized_replay=c.prio if prio is None else prio, obs_dtype=c.u8, use_mfma=c.mfma if mfma is None else mfma, use_graph=graph, seed=SR.ENGINE_SEED)
    h = pkg.Engine(layers, hp)
    h.replay_add(D.s, D.a, D.r, D.sp, D.d); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def ff_record(h, idx):
    loss, gn, td = h.train_step(idx)
    return dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities())


def assert_launches(h, net):
    """one forward launch per join and pass, one entry launch per block, a join launch exactly where the last inner layer has an activation; none of the fused launches"""
    names = tokens(h); prog = SR.program(net)
    for j, e in enumerate(prog):
        if e.kind != "join":
            continue
        K = prog[e.src]; alias = K.kind == "join" or K.l.act == nn.identity
        assert names.count(f"fwd_on_skip{j}") == 1 and names.count(f"fwd_tg_skip{j}") == 1 and names.count(f"bwd_entry_skip{j}") == 1, (j, names)
        assert names.count(f"bwd_join_skip{j}") == (0 if alias else 1), (j, names)
    assert not set(FUSED) & set(names), names
    return names


@pytest.mark.parametrize("c", SR.CASES, ids=IDS(SR.CASES))
def test_three_steps_vs_fp64_reference_graph_eager_mfma_and_rerun(pkg, c):
    D = SR.ff_data(c); net = D.net; msg = c.name
    h = ff_engine(pkg, c, D, graph=1); recs = []
    adam = LR.Adam(D.p_on.size, lr=LR.LR)
    sg, rm, gap = SR.case_margins(c)
    assert sg >= LR.SIGMA_MIN and rm > LR.RELU_MARGIN and gap > LR.GAP, (msg, sg, rm, gap)
    for k in range(3):
        idx = D.idx[k]; msgk = f"{msg} step {k}"
        p_prev = h.get_params(0)
        batch = h.get_batch(idx)
        for i, (a, b) in enumerate(zip(batch, SR.ff_batch(c, D, idx))):
            if i < 5:
                np.testing.assert_array_equal(np.asarray(a, np.float64).reshape(np.shape(b)), np.asarray(b, np.float64), err_msg=f"{msgk}: batch[{i}]")
        want_w = SR.ff_batch(c, D, idx)[5]
        if k == 0 or not c.prio:      # (later steps of a prioritized case: the engine's own new priorities weigh the batch)
            E._close("is_weights", batch[5], want_w, rtol=2e-6, msg=msgk)
        assert h.get_counters()["train_steps"] == k
        masks = SR.masks_for(net, k, c.B)
        o = SR.ff_step(net, p_prev, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq), masks)
        rec = ff_record(h, idx); recs.append(rec); q = rec["q"]
        E._close("q_on_s", q["q_on_s"], o["q_on_s"], msg=msgk, **LR.TOL_Q)
        E._close("q_tg_sp", q["q_tg_sp"], o["q_tg_sp"], msg=msgk, **LR.TOL_Q)
        if c.dq:
            E._close("q_on_sp", q["q_on_sp"], o["q_on_sp"], msg=msgk, **LR.TOL_Q)
        qsel = np.sort(o["q_on_sp"] if c.dq else o["q_tg_sp"], axis=1); clear = qsel[:, -1] - qsel[:, -2] >= LR.GAP
        assert clear.all() or k > 0, msgk      # the seed keeps the first step's gap
        np.testing.assert_array_equal(q["best_a"][clear], o["best_a"][clear], err_msg=msgk)
        if clear.all():
            E._close("y", q["y"], o["y"], msg=msgk, **LR.TOL_TD)
            E._close("td", rec["td"], o["td"], msg=msgk, **LR.TOL_TD)
            E._close("loss", rec["loss"], o["loss"], msg=msgk, **LR.TOL_LOSS)
            SR.check_grads(net, rec["g"], o["grads"], live=k == 0)
            E._close("grad_norm", rec["gn"], o["grad_norm"], msg=msgk, **LR.TOL_GN)
        LR.check_params(rec["p"], adam.step(p_prev, rec["g"]))
        if c.prio and clear.all():
            eps, alpha = 1e-3, 0.6; t = np.abs(o["td"])
            want = O.priority_from_td(t, np.float32(eps), np.float32(alpha)).astype(np.float64)
            bound = 2 * alpha * (t + eps) ** (alpha - 1) * (LR.TOL_TD["atol"] + LR.TOL_TD["rtol"] * t) + 1e-6 * want
            assert (np.abs(rec["pr"][idx] - want) <= bound).all(), (msgk, np.abs(rec["pr"][idx] - want).max())
    for kw, what in ((dict(graph=0), "use_graph 0 vs 1"), (dict(graph=1), "two identical runs"), (dict(mfma=1 - c.mfma), f"use_mfma {1 - c.mfma} vs {c.mfma}")):
        h2 = ff_engine(pkg, c, D, **kw)
        E.same_bits(recs, [ff_record(h2, D.idx[k]) for k in range(3)], f"{msg}: {what}")
        h2.close()
    assert all(tuple(p) == (0, 0, 0) for p, l in zip(h.plan(), nn.lower(net)[0]) if l.kind == nn._abi.LAYER_SKIPADD)      # the join's plan entry is all zeros
    names = assert_launches(h, net)
    assert ("head_td" in names) or ("td_huber" in names), names
    h.close()


# ------------------------------------------------------------------ 3: the other forward passes
@pytest.mark.parametrize("name", ["two_dense_n64_b32", "pre_norm_n33_b32", "do_last_n8_b5", "p_dropout_n64_b32", "two_blocks_n33_b32", "dueling_prio"])
def test_forward_and_greedy_action_vs_fp64_and_the_bits_of_the_steps_s_prime_pass(pkg, name):
    """dqn_forward on 1 and 7 rows of s': within TOL_Q of the fp64 network (Dropout inactive) and the bits of the step's q_on_sp"""
    c = SR.BY_NAME[name]; D = SR.ff_data(c); h = ff_engine(pkg, c, D); idx = D.idx[0]
    rows = np.concatenate([idx, idx])[:7]
    fw = {n: h.forward(D.sp[rows[:n]]) for n in (1, 7)}
    for n, q in fw.items():
        E._close("policy_q", q, SR.q_values(D.net, D.p_on, D.sp[rows[:n]]), msg=f"{name} n={n}", **LR.TOL_Q)
    a = h.greedy_action(D.sp[rows]); q64 = SR.q_values(D.net, D.p_on, D.sp[rows]); t = np.sort(q64, axis=1)
    clear = t[:, -1] - t[:, -2] >= LR.GAP
    assert clear.sum() >= 5
    np.testing.assert_array_equal(np.asarray(a)[clear], q64.argmax(1)[clear])
    h.train_step(idx)
    q_on_sp = h.last_q()["q_on_sp"]; q_sp7 = np.concatenate([q_on_sp, q_on_sp])[:7]
    for n, q in fw.items():
        np.testing.assert_array_equal(q, q_sp7[:n], err_msg=f"{name} n={n}")
    h.close()


# ------------------------------------------------------------------ 4: recurrent
def rec_engine(pkg, c, D, graph=1, mfma=None):
    layers, dueling = nn.lower(D.net)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=c.obs[0], dueling=int(dueling), buffer_size=D.cap, recurrence=1, trace_length=c.T, learning_rate=LR.LR,
                             prioritized_replay=0, use_mfma=c.mfma if mfma is None else mfma, use_graph=graph, seed=SR.ENGINE_SEED, gamma=c.gamma, double_q=c.dq)
    h = pkg.Engine(layers, hp)
    feed(h, D.eps); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def rec_record(h, idx, start):
    loss, gn = h.train_step_drqn(idx, start)
    return dict(loss=loss, gn=gn, g=h.get_grads(), p=h.get_params(0))


@pytest.mark.parametrize("c", SR.REC_CASES, ids=IDS(SR.REC_CASES))
def test_recurrent_steps_vs_fp64_reference(pkg, c):
    """T = 3, B = 4: the block runs over the T * B columns like every feed-forward layer of the recurrent program; three steps compare what a recurrent step reports
    (loss, gradients per block, grad_norm, parameters after fp64 Adam); use_graph 0 against 1, use_mfma 0 against 1 and a rerun, bit for bit"""
    D = SR.rec_data(c); net = D.net
    h = rec_engine(pkg, c, D, graph=1); recs = []
    adam = LR.Adam(D.p_on.size, lr=LR.LR)
    for k in range(3):
        idx, start = D.draws[k]
        p_prev = h.get_params(0)
        batch = h.episode_get_batch(idx, start)
        for got, want in zip(batch, R.sample_batch(D.ring, idx, start, c.T, c.obs)):
            np.testing.assert_array_equal(np.asarray(got).reshape(want.shape), want)
        batch = R.sample_batch(D.ring, idx, start, c.T, c.obs)
        o = SR.rec_step(net, p_prev, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq), SR.masks_for(net, k, c.B, c.T))
        rec = rec_record(h, idx, start); recs.append(rec)
        np.testing.assert_allclose(rec["loss"], o["loss"], rtol=2e-5, atol=1e-7, err_msg=f"{c.name} step {k}: loss")      # the recurrent tables' loss tolerance
        SR.check_grads(net, rec["g"], o["grads"], live=k == 0)
        E._close("grad_norm", rec["gn"], o["grad_norm"], msg=c.name, **LR.TOL_GN)
        LR.check_params(rec["p"], adam.step(p_prev, rec["g"]))
    for kw, what in ((dict(graph=0), "use_graph 0 vs 1"), (dict(graph=1), "two identical runs"), (dict(mfma=0), "use_mfma 0 vs 1")):
        h2 = rec_engine(pkg, c, D, **kw)
        for k in range(3):
            r2 = rec_record(h2, *D.draws[k])
            assert (r2["loss"], r2["gn"]) == (recs[k]["loss"], recs[k]["gn"]), what
            np.testing.assert_array_equal(r2["g"], recs[k]["g"], err_msg=what); np.testing.assert_array_equal(r2["p"], recs[k]["p"], err_msg=what)
        h2.close()
    assert_launches(h, net)
    h.close()


# ------------------------------------------------------------------ 5: device loops
def _env_net(obs=100):
    return nn.Chain(nn.Dense(obs, 16, nn.relu), nn.SkipConnection(nn.Chain(nn.LayerNorm(16), nn.Dense(16, 32, nn.relu), nn.Dense(32, 16)), "+"), nn.Dense(16, 4))


def test_device_loop_acts_on_the_fp64_argmax_and_reports_the_general_tail(pkg, mods):
    """TestMDP((5, 5), 4, 6), 8 copies: 12 vector steps at eps = 0; every action is the fp64 argmax where the gap is at least GAP; envs_info reports fused tail false"""
    net = _env_net()
    h, p, spec = G._env_engine(pkg, mods, net)
    h.envs_create(spec, max_episode_length=100, seed=17)
    checked = 0
    for t in range(12):
        obs = h.envs_peek()[0].copy()
        h.rollout(1, t0=t + 1, train_freq=0, target_update_freq=0, eps=(0.0, 0.0, 1.0))
        a = h.envs_peek()[1]
        q = SR.q_values(net, p, obs.reshape(obs.shape[0], -1)); top = np.sort(q, axis=1)
        clear = top[:, -1] - top[:, -2] >= LR.GAP
        np.testing.assert_array_equal(a[clear], q.argmax(1)[clear], err_msg=f"step {t}")
        checked += int(clear.sum())
    assert checked >= 0.9 * 12 * 8, checked
    assert h.envs_info() == (8, False)
    r, st = h.evaluate(8, 50, seed=5)
    assert np.isfinite(r) and np.isfinite(st) and st > 0
    h.close()


def _rollout_engine(pkg, envs, net, p, env=None):
    layers, _ = nn.lower(net)
    hp = pkg.default_hparams(batch_size=8, n_actions=4, obs_c=1, obs_h=5, obs_w=5, dueling=0, buffer_size=256, learning_rate=1e-3, gamma=0.95, seed=5)
    if env:
        os.environ[env] = "1"
    try:
        h = pkg.Engine(layers, hp)
    finally:
        if env:
            os.environ.pop(env, None)
    h.set_params(p, 0); h.sync_target()
    h.envs_create(envs.TestMDP((5, 5), 1, 6, n=32, seed=3), max_episode_length=100, seed=17)
    return h


def test_device_rollout_walks_the_four_launch_tails_trajectory(pkg, mods):
    """32 copies of TestMDP((5, 5), 1, 6) with a block in the net: 16 vector steps that explore, act greedily and train.  A network with a block takes the general
    four-launch acting tail by itself; under DQN_NO_ACT_HEAD (that tail forced) and under use_graph 0 it walks the same trajectory -- observations, actions, rewards,
    terminals after every step and the parameters at the end, bit for bit"""
    envs = mods[1]; net = _env_net(25)
    p = nn.glorot_params(net, seed=2); p = (p + 0.1 * np.random.default_rng(2).standard_normal(p.size)).astype(np.float32)
    g, t = _rollout_engine(pkg, envs, net, p), _rollout_engine(pkg, envs, net, p, env="DQN_NO_ACT_HEAD")
    assert g.envs_info() == (32, False) and t.envs_info() == (32, False)
    acted = set()
    for k in range(16):
        for h in (g, t):
            h.rollout(1, t0=k + 1, train_freq=2, target_update_freq=8, eps=(0.5, 0.1, 16.0))
        for x, y, what in zip(g.envs_peek(), t.envs_peek(), ("observations", "actions", "rewards", "terminals")):
            np.testing.assert_array_equal(x, y, err_msg=f"step {k}: {what}")
        acted |= set(np.asarray(g.envs_peek()[1]).tolist())
    assert len(acted) > 1
    np.testing.assert_array_equal(g.get_params(0), t.get_params(0))
    assert np.abs(g.get_params(0) - p).max() > 0 and g.get_counters()["train_steps"] > 0
    g.close(); t.close()


# ------------------------------------------------------------------ 6: checkpoint / resume and the solver's save / restore
@pytest.mark.parametrize("name", ["pre_norm_n33_b32", "do_last_n8_b5", "dueling_prio"])
def test_checkpoint_resume_gives_the_same_bits(pkg, name):
    """four sampled steps straight against two, a checkpoint restored into a FRESH engine, and two more: the same step outputs, parameters, Adam state, priorities and
    dqn_forward bits"""
    c = SR.BY_NAME[name]; D = SR.ff_data(c)
    a = ff_engine(pkg, c, D, prio=1)
    for _ in range(4):
        la = a.train_step(want_td=False)
    b = ff_engine(pkg, c, D, prio=1)
    for _ in range(2):
        b.train_step(want_td=False)
    ck = b.checkpoint(); b.close()
    b2 = ff_engine(pkg, c, D, prio=1); b2.restore(ck)
    assert b2.get_counters()["train_steps"] == 2
    for _ in range(2):
        lb = b2.train_step(want_td=False)
    assert la == lb
    np.testing.assert_array_equal(a.last_indices(), b2.last_indices())
    for k in ("q_on_s", "q_on_sp", "q_tg_sp", "y"):
        np.testing.assert_array_equal(a.last_q()[k], b2.last_q()[k], err_msg=k)
    np.testing.assert_array_equal(a.get_params(0), b2.get_params(0)); np.testing.assert_array_equal(a.get_grads(), b2.get_grads())
    np.testing.assert_array_equal(a.replay_priorities(), b2.replay_priorities())
    for x, y in zip(a.get_adam_state(), b2.get_adam_state()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a.forward(D.s[:7]), b2.forward(D.s[:7]))
    assert np.abs(a.get_params(0) - D.p_on).max() > 0
    a.close(); b2.close()


def test_train_steps_5_equals_five_train_step_calls(pkg):
    c = SR.BY_NAME["pre_norm_n33_b32"]; D = SR.ff_data(c)
    a, b = ff_engine(pkg, c, D, prio=1), ff_engine(pkg, c, D, prio=1)
    la = a.train_steps(5)
    for _ in range(5):
        lb = b.train_step(want_td=False)
    assert la == lb
    np.testing.assert_array_equal(a.get_params(0), b.get_params(0)); np.testing.assert_array_equal(a.get_grads(), b.get_grads())
    np.testing.assert_array_equal(a.replay_priorities(), b.replay_priorities())
    assert a.get_counters() == b.get_counters() and a.get_counters()["train_steps"] == 5
    a.close(); b.close()


SOLVE_SIZES = [(16, 100), (16,), (16,), (16,), (32, 16), (32,), (16, 32), (16,), (4, 16), (4,)]


def test_short_solve_reaches_the_optimal_evaluation_return_and_the_saved_model_gives_the_same_forward_bits(pkg, mods, tmp_path):
    """TestMDP((5, 5), 4, 6), device_envs, Dense(100, 16, relu) -> SkipConnection(Chain(LayerNorm(16), Dense(16, 32, relu), Dense(32, 16)), +) -> Dense(16, 4), the solver
    settings of test_solve_gpu's TestMDP test: the evaluation reaches the MDP's optimal return 2.1 in its five steps (ONE run, one seed); qnetwork.bson holds the inner
    layers' arrays in Flux.params order, and restore_best_model puts back parameters whose dqn_forward bits are the saved model's"""
    nn_, envs, S, bson = mods
    env = envs.TestMDP((5, 5), 4, 6, n=16, seed=7)
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.01, steps=1000 / 2), rng=np.random.default_rng(1))
    solver = S.DeepQLearningSolver(qnetwork=_env_net(), max_steps=1000, learning_rate=0.005, exploration_policy=expl, eval_freq=500, save_freq=500, num_ep_eval=16, train_freq=1,
                                   log_freq=500, double_q=False, dueling=False, prioritized_replay=True, verbose=False, logdir=str(tmp_path / "log"), device_envs=True,
                                   buffer_size=4096, train_start=64)
    policy = S.solve(solver, env); h = policy.engine
    r, st = h.evaluate(16, 50, seed=5)
    print(f"\nshort solve with a pre-norm block: evaluation return {r:.4f} over {st:.1f} steps (one run, one seed)")
    assert abs(r - 2.1) <= 1e-5 and st == 5.0, (r, st)
    path = tmp_path / "log" / "qnetwork.bson"
    assert path.exists(), "no model was saved"
    w, sizes = bson.load_qnetwork(path)
    assert [tuple(x) for x in sizes] == SOLVE_SIZES
    obs = np.random.default_rng(3).random((7, 4, 5, 5), dtype=np.float32)
    h.set_params(w, pkg.NET_ONLINE); q_saved = h.forward(obs)
    h.set_params(w * np.float32(0.5), pkg.NET_ONLINE)
    assert np.abs(h.forward(obs) - q_saved).max() > 0
    S.restore_best_model(solver, policy)
    np.testing.assert_array_equal(h.forward(obs), q_saved)
    np.testing.assert_array_equal(h.get_params(pkg.NET_ONLINE), w)
    h.close()


# ------------------------------------------------------------------ 7: refusals
def test_replicas_are_refused(pkg, monkeypatch):
    c = SR.BY_NAME["one_dense_n5_b4"]; D = SR.ff_data(c)
    h = ff_engine(pkg, c, D)
    with pytest.raises(nn._abi.DQNError, match=r"dqn_comm_init: layer 2 is a skip block; data-parallel replicas .* not supported \(single GPU only\)"):
        h.comm_init(bytes(128), 0, 1)
    h.train_step(D.idx[0])      # the engine is left as it was
    h.close()
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    with pytest.raises(nn._abi.DQNError, match=r"DQN_SIM_WORLD: layer 2 is a skip block; .*\(single GPU only\)"):
        ff_engine(pkg, c, D)


def test_engine_creation_refuses_by_layer_index(pkg):
    abi = nn._abi

    def L(kind, **kw):
        d = abi.LayerDesc(); d.kind = kind
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    hp = pkg.default_hparams(batch_size=8, n_actions=4, obs_c=6, dueling=0, buffer_size=64)
    first, mid, head = L(0, n_in=6, n_out=16, act=1), L(0, n_in=16, n_out=16), L(0, n_in=16, n_out=4)
    for layers, msg in (([first, mid, L(9, cin=0), head], r"layer 2: a skip block holds at least one inner layer \(cin = m = 0 must be >= 1\)"),
                        ([first, mid, L(9, cin=3), head], r"layer 2: the skip block's 3 inner layers would start before the first layer"),
                        ([first, mid, L(9, cin=1), mid, L(9, cin=3), head], r"layer 4: .*reach across the join of another skip block \(layer 2\)"),
                        ([L(0, n_in=6, n_out=6), L(9, cin=1), L(0, n_in=6, n_out=4)], r"layer 1: the skip block's first inner layer \(layer 0\) reads the observation"),
                        ([first, L(0, n_in=16, n_out=12), L(9, cin=1), L(0, n_in=12, n_out=4)], r"layer 2: the skip block maps 16 features to 12"),
                        ([first, mid, L(9, cin=1, act=1), head], r"layer 2: a skip block's join has no activation"),
                        ([L(0, n_in=6, n_out=4), L(0, n_in=4, n_out=4), L(9, cin=1)], r"layer 2: a skip block cannot be the network's output layer")):
        with pytest.raises(abi.DQNError, match=msg):
            pkg.Engine(layers, hp)
    hpd = pkg.default_hparams(batch_size=8, n_actions=4, obs_c=6, dueling=1, buffer_size=64)
    with pytest.raises(abi.DQNError, match=r"layer 2: a skip block is supported in the base chain only"):
        pkg.Engine([first, L(0, stream=1, n_in=16, n_out=16), L(9, stream=1, cin=1), L(0, stream=1, n_in=16, n_out=1), L(0, stream=2, n_in=16, n_out=4)], hpd)
    hpr = pkg.default_hparams(batch_size=4, n_actions=4, obs_c=6, dueling=0, buffer_size=16, recurrence=1, trace_length=3, prioritized_replay=0)
    with pytest.raises(abi.DQNError, match=r"layer 2: the skip block holds a recurrent layer \(layer 1\)"):
        pkg.Engine([L(0, n_in=6, n_out=8), L(3, n_in=8, n_out=8), L(9, cin=1), L(0, n_in=8, n_out=4)], hpr)
    hpc = pkg.default_hparams(batch_size=8, n_actions=4, obs_c=1, obs_h=6, obs_w=6, dueling=0, buffer_size=64)
    with pytest.raises(abi.DQNError, match=r"layer 2: the skip block holds a Conv / MaxPool / MeanPool layer \(layer 1\)"):
        pkg.Engine([L(1, cin=1, cout=2, kh=3, kw=3, sh=1, sw=1), L(1, cin=2, cout=2, kh=1, kw=1, sh=1, sw=1), L(9, cin=1), L(0, n_in=32, n_out=4)], hpc)


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (docs/history/skip.md records them)"""
    print("\nWORST error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("WORST gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(R.WORST.items())})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
