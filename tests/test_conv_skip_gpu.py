"""GPU: train steps, every forward pass, device loops, resume, solver round trip and refusals of networks with CONVOLUTIONAL Flux SkipConnection(layers, +) blocks --
x + Conv(Conv(x)) on a (c, h, w) map, descriptor kind 10, the residual epilogues of csrc/conv_own.hip --, all through the C ABI.  The join is read out EXACTLY through
centre-tap identity kernels (Q = 2^blocks * x in every pass) and through a zero branch (the network without the block, bit for bit); every case of
conv_skip_reference.py's tables then runs three train steps, each against the two-legged fp64 reference at the engine's own previous parameters and batch (Q on s and
s', target Q, greedy indices exactly under GAP, y, td, loss, per-block gradients -- live on the first step --, grad_norm, parameters after fp64 Adam, priorities;
tolerances are the project's existing constants, unchanged), then use_graph 0 against 1, use_mfma 0 against 1, DQN_NO_SKIP_FUSE 1 against 0 and a second identical run,
bit for bit.  The C twin does not know the layer: parity rests on the fp64 reference plus these bit-for-bit companions (the kind-9 precedent).

Without the layer every test here fails: nn.lower refuses the block ("convolutional residual blocks are not supported") and the engine answers "unknown kind 10".  Each
wrong engine -- the entry gradient without + dY, the entry's derivative before the sum or twice, the last inner layer's derivative omitted, the skip read from the first
inner layer -- is off by thousands of tolerances on every case it applies to (test_conv_skip_cpu.test_the_tests_can_tell).

One MI355X, one run: docs/history/conv_skip.md records the worst error / tolerance per quantity and per gradient block kind."""
import importlib
import os
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import conv_skip_reference as CR
import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_gpu_common as G
import recurrent_reference as R
from drqn_common import feed

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()
nn = CR.nn
LR = CR.LR
FUSED = ("tiny_step", "red_head", "head_cols4", "drqn_cols")      # the whole-step and head fusions that decline a network with the layer


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "envs", "solver", "bson"))


def names_of(h):
    return [nm for nm, _ in h.profile_step(max_entries=512)]


def engine(pkg, layers, hp, unfused=False):
    """DQN_NO_SKIP_FUSE is read once, at engine creation"""
    if unfused:
        os.environ["DQN_NO_SKIP_FUSE"] = "1"
    try:
        return pkg.Engine(layers, hp)
    finally:
        os.environ.pop("DQN_NO_SKIP_FUSE", None)


def assert_launches(h, net, unfused):
    """fused (the default): where the block's last inner layer K has no activation, K's forward launch of each pass is named <pass>_conv<K>+skip<join> and the join emits
    none; the first inner layer's input-gradient launch is bwd_conv<F>+skip<join> and no bwd_entry launch exists.  Where K has an activation the join keeps its forward
    launches and its bwd_join launch.  Unfused (DQN_NO_SKIP_FUSE): the plain conv launches plus fwd_*_skip<j>, bwd_entry_skip<j> and -- where K has an activation --
    bwd_join_skip<j> (where it has none the join's backward is the alias, as for kind 9)"""
    names = names_of(h); prog = CR.program(net); rec = any(e.kind == "layer" and e.l.kind == "lstm" for e in prog)
    for j, e in enumerate(prog):
        if e.kind != "join":
            continue
        K, F = e.src, CR._first_inner(prog, j); alias = prog[K].l.act == nn.identity
        own = [n for n in names if n in (f"fwd_on_skip{j}", f"fwd_tg_skip{j}")]
        fused_fwd = [n for n in names if n in (f"fwd_on_conv{K}+skip{j}", f"fwd_tg_conv{K}+skip{j}")]
        if unfused or not alias:
            assert sorted(own) == [f"fwd_on_skip{j}", f"fwd_tg_skip{j}"] and not fused_fwd, (j, names)
            assert names.count(f"fwd_on_conv{K}") == 1 and names.count(f"fwd_tg_conv{K}") == 1, (j, names)
        else:
            assert sorted(fused_fwd) == [f"fwd_on_conv{K}+skip{j}", f"fwd_tg_conv{K}+skip{j}"] and not own, (j, names)
            assert f"fwd_on_conv{K}" not in names and f"fwd_tg_conv{K}" not in names, (j, names)
        assert names.count(f"bwd_join_skip{j}") == (0 if alias else 1), (j, names)
        if unfused:
            assert names.count(f"bwd_entry_skip{j}") == 1 and names.count(f"bwd_conv{F}") == 1 and f"bwd_conv{F}+skip{j}" not in names, (j, names)
            assert names.index(f"bwd_conv{F}") < names.index(f"bwd_entry_skip{j}"), (j, names)
        else:
            assert names.count(f"bwd_conv{F}+skip{j}") == 1 and f"bwd_conv{F}" not in names, (j, names)
    if not unfused:
        assert not [n for n in names if n.startswith("bwd_entry")], names
    assert not set(FUSED) & {t for n in names for t in n.split("+")}, names
    assert rec or ("head_td" in names) or ("td_huber" in names), names
    return names


# ------------------------------------------------------------------ 1: the join, read out exactly
READOUT = [(4, (3, 3), 5, 2), (4, (3, 3), 32, 1), (16, (2, 2), 32, 2), (16, (1, 2), 128, 2)]      # c = 4: the VALU forms; c = 16: MFMA tiles; one inner layer: F == K


@pytest.mark.parametrize("c,hw,B,m", READOUT, ids=[f"c{c}_{hw[0]}x{hw[1]}_b{B}_m{m}" for c, hw, B, m in READOUT])
def test_exact_readout_q_is_4x_in_every_pass(pkg, c, hw, B, m):
    """Conv(centre tap I) -> two blocks of m centre-tap identity convs, zero bias -> Dense(W = I) on small-integer observations: each join doubles its input exactly,
    Q = 4x -- online on s and s', target, dqn_forward on 1 and 7 columns, dqn_greedy_action -- under use_graph 1 and 0, fused and unfused"""
    net, flat, n = CR.readout_net(c, hw, blocks=2, m=m)
    rng = np.random.default_rng(n * 1000 + B); cap = B + 8
    s, sp = (rng.integers(-8, 9, (cap, c) + hw).astype(np.float32) for _ in range(2))
    idx = rng.permutation(cap)[:B].astype(np.int64); f2 = lambda x: x.reshape(x.shape[0], -1)
    for graph, unfused in ((1, False), (0, False), (1, True)):
        hp = pkg.default_hparams(batch_size=B, n_actions=n, obs_c=c, obs_h=hw[0], obs_w=hw[1], dueling=0, buffer_size=cap, learning_rate=0.0, gamma=0.95, prioritized_replay=0, use_graph=graph, seed=CR.ENGINE_SEED)
        h = engine(pkg, nn.lower(net)[0], hp, unfused)
        h.replay_add(s, rng.integers(0, n, cap).astype(np.int32), rng.standard_normal(cap).astype(np.float32), sp, (rng.random(cap) < 0.2).astype(np.uint8))
        h.set_params(flat, 0); h.set_params(flat, 1)
        h.train_step(idx); q = h.last_q()
        np.testing.assert_array_equal(q["q_on_s"], 4 * f2(s[idx])); np.testing.assert_array_equal(q["q_on_sp"], 4 * f2(sp[idx])); np.testing.assert_array_equal(q["q_tg_sp"], 4 * f2(sp[idx]))
        rows = np.concatenate([idx, idx])[:7]
        for k in (1, 7):
            np.testing.assert_array_equal(h.forward(s[rows[:k]]), 4 * f2(s[rows[:k]]))
            np.testing.assert_array_equal(h.forward(sp[rows[:k]], which=pkg.NET_TARGET), 4 * f2(sp[rows[:k]]))
        np.testing.assert_array_equal(h.greedy_action(s[rows]), (4 * f2(s[rows])).argmax(1))
        assert_launches(h, net, unfused)
        h.close()


def _zero_branch(c, B, seed):
    """(net with a block whose last inner layer is all zero, the same net without the block, their parameters)"""
    blk = nn.Chain(nn.Conv(3, 2, c, nn.relu, 1, 1), CR.block(c)(), nn.flattenbatch, nn.Dense(c * 36, 4))
    plain = nn.Chain(nn.Conv(3, 2, c, nn.relu, 1, 1), nn.flattenbatch, nn.Dense(c * 36, 4))
    rng = np.random.default_rng(seed)
    pp = nn.glorot_params(plain, seed=3); pp = (pp + 0.05 * rng.standard_normal(pp.size)).astype(np.float32)
    n0 = 18 * c + c; nc = 9 * c * c + c      # the stem's block; one inner conv's
    inner_f = (nn.glorot_params(nn.Chain(nn.Conv(3, c, c, nn.relu, 1, 1)), seed=4) + 0.05 * rng.standard_normal(nc)).astype(np.float32)
    pb = np.concatenate([pp[:n0], inner_f, np.zeros(nc, np.float32), pp[n0:]])
    return blk, plain, pb, pp, n0, nc


@pytest.mark.parametrize("c,B", [(4, 5), (16, 32)], ids=["valu_c4_b5", "mfma_c16_b32"])
def test_a_zero_branch_leaves_the_network_without_the_block_bit_for_bit(pkg, c, B):
    """K's weights and bias zero, P a relu layer: the join hands on y_P and the entry (dF + dY) with dF = 0, so Q, td, loss and every gradient outside the block are those
    of the same network without the block on the same batch, bit for bit; inside the block K's dW is not zero (F's is: nothing flows back through a zero K)"""
    blk, plain, pb, pp, n0, nc = _zero_branch(c, B, seed=c + B)
    rng = np.random.default_rng(7 * c + B); cap = B + 24
    s, sp = ((2 * rng.standard_normal((cap, 2, 6, 6))).astype(np.float32) for _ in range(2))
    a = rng.integers(0, 4, cap).astype(np.int32); r = (2 * rng.standard_normal(cap)).astype(np.float32); d = (rng.random(cap) < 0.2).astype(np.uint8)
    idx = rng.permutation(cap)[:B].astype(np.int64); recs = {}
    for what, net, p, unfused in (("block", blk, pb, False), ("block unfused", blk, pb, True), ("plain", plain, pp, False)):
        hp = pkg.default_hparams(batch_size=B, n_actions=4, obs_c=2, obs_h=6, obs_w=6, dueling=0, buffer_size=cap, learning_rate=LR.LR, gamma=0.95, prioritized_replay=0, seed=CR.ENGINE_SEED)
        h = engine(pkg, nn.lower(net)[0], hp, unfused)
        h.replay_add(s, a, r, sp, d); h.set_params(p, 0); h.set_params(p, 1)
        loss, gn, td = h.train_step(idx)
        recs[what] = dict(loss=loss, td=td, g=h.get_grads(), q=h.last_q()); h.close()
    want = recs["plain"]
    for what in ("block", "block unfused"):
        got = recs[what]
        assert got["loss"] == want["loss"], what
        np.testing.assert_array_equal(got["td"], want["td"], err_msg=what)
        for k in ("q_on_s", "q_on_sp", "q_tg_sp", "best_a", "y"):
            np.testing.assert_array_equal(got["q"][k], want["q"][k], err_msg=f"{what}: {k}")
        np.testing.assert_array_equal(got["g"][:n0], want["g"][:n0], err_msg=f"{what}: the stem's gradient")
        np.testing.assert_array_equal(got["g"][n0 + 2 * nc:], want["g"][n0:], err_msg=f"{what}: the head's gradient")
        gk = got["g"][n0 + nc:n0 + 2 * nc]
        assert np.abs(gk[:9 * c * c]).max() > 0 and np.abs(gk[9 * c * c:]).max() > 0, what      # K's dW and db
        assert not got["g"][n0:n0 + nc].any(), what                                               # F's: exact zeros
    assert np.abs(want["g"]).max() > 0


# ------------------------------------------------------------------ 2: three train steps against the fp64 reference
def ff_engine(pkg, c, D, graph=1, prio=None, mfma=None, unfused=False):
    layers, dueling = nn.lower(D.net); o = c.obs
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=o[0], obs_h=o[1], obs_w=o[2], dueling=int(dueling), buffer_size=c.B + 24, learning_rate=LR.LR, gamma=c.gamma,
                             double_q=c.dq, prioritized_replay=c.prio if prio is None else prio, obs_dtype=c.u8, use_mfma=c.mfma if mfma is None else mfma, use_graph=graph, seed=CR.ENGINE_SEED)
    h = engine(pkg, layers, hp, unfused)
    h.replay_add(D.s, D.a, D.r, D.sp, D.d); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def ff_record(h, idx):
    loss, gn, td = h.train_step(idx)
    return dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities())


@pytest.mark.parametrize("c", CR.CASES, ids=IDS(CR.CASES))
def test_three_steps_vs_fp64_reference_graph_eager_mfma_fusion_and_rerun(pkg, c):
    D = CR.ff_data(c); net = D.net; msg = c.name
    h = ff_engine(pkg, c, D, graph=1); recs = []
    adam = LR.Adam(D.p_on.size, lr=LR.LR)
    rm, pm, gap = CR.case_margins(c)
    assert rm > CR.RELU_MARGIN and pm > CR.RELU_MARGIN and gap > CR.GAP, (msg, rm, pm, gap)
    for k in range(3):
        idx = D.idx[k]; msgk = f"{msg} step {k}"
        p_prev = h.get_params(0)
        batch = h.get_batch(idx)
        for i, (a, b) in enumerate(zip(batch, CR.ff_batch(c, D, idx))):
            if i < 5:
                np.testing.assert_array_equal(np.asarray(a, np.float64).reshape(np.shape(b)), np.asarray(b, np.float64), err_msg=f"{msgk}: batch[{i}]")
        if k == 0 or not c.prio:      # (later steps of a prioritized case: the engine's own new priorities weigh the batch)
            E._close("is_weights", batch[5], CR.ff_batch(c, D, idx)[5], rtol=2e-6, msg=msgk)
        assert h.get_counters()["train_steps"] == k
        batch = tuple(np.asarray(x).reshape(np.shape(y)) if i in (0, 3) else x for i, (x, y) in enumerate(zip(batch, CR.ff_batch(c, D, idx))))
        o = CR.ff_step(net, p_prev, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq))
        rec = ff_record(h, idx); recs.append(rec); q = rec["q"]
        E._close("q_on_s", q["q_on_s"], o["q_on_s"], msg=msgk, **CR.TOL_Q)
        E._close("q_tg_sp", q["q_tg_sp"], o["q_tg_sp"], msg=msgk, **CR.TOL_Q)
        if c.dq:
            E._close("q_on_sp", q["q_on_sp"], o["q_on_sp"], msg=msgk, **CR.TOL_Q)
        qsel = np.sort(o["q_on_sp"] if c.dq else o["q_tg_sp"], axis=1); clear = qsel[:, -1] - qsel[:, -2] >= CR.GAP
        assert clear.all(), msgk      # the seed keeps the gap on all three steps of the trajectory
        np.testing.assert_array_equal(q["best_a"], o["best_a"], err_msg=msgk)
        E._close("y", q["y"], o["y"], msg=msgk, **CR.TOL_TD)
        E._close("td", rec["td"], o["td"], msg=msgk, **CR.TOL_TD)
        E._close("loss", rec["loss"], o["loss"], msg=msgk, **CR.TOL_LOSS)
        CR.check_grads(net, rec["g"], o["grads"], live=k == 0)
        E._close("grad_norm", rec["gn"], o["grad_norm"], msg=msgk, **CR.TOL_GN)
        CR.check_params(rec["p"], adam.step(p_prev, rec["g"]))
        if c.prio:
            eps, alpha = 1e-3, 0.6; t = np.abs(o["td"])
            want = O.priority_from_td(t, np.float32(eps), np.float32(alpha)).astype(np.float64)
            bound = 2 * alpha * (t + eps) ** (alpha - 1) * (CR.TOL_TD["atol"] + CR.TOL_TD["rtol"] * t) + 1e-6 * want
            assert (np.abs(rec["pr"][idx] - want) <= bound).all(), (msgk, np.abs(rec["pr"][idx] - want).max())
    for kw, what in ((dict(graph=0), "use_graph 0 vs 1"), (dict(graph=1), "two identical runs"), (dict(mfma=1 - c.mfma), f"use_mfma {1 - c.mfma} vs {c.mfma}"),
                     (dict(unfused=True), "DQN_NO_SKIP_FUSE 1 vs 0"), (dict(unfused=True, mfma=1 - c.mfma, graph=0), "DQN_NO_SKIP_FUSE 1, the other form, eager")):
        h2 = ff_engine(pkg, c, D, **kw)
        E.same_bits(recs, [ff_record(h2, D.idx[k]) for k in range(3)], f"{msg}: {what}")
        if kw.get("unfused"):
            assert_launches(h2, net, True)
        h2.close()
    assert all(tuple(p) == (0, 0, 0) for p, l in zip(h.plan(), nn.lower(net)[0]) if l.kind == nn._abi.LAYER_SKIPADD_MAP)      # the join's plan entry is all zeros
    assert_launches(h, net, False)
    h.close()


# ------------------------------------------------------------------ 3: the other forward passes
@pytest.mark.parametrize("name", ["valu_c4_5x5_b5", "mfma_c16_6x6_b32", "k_tanh_c16_b32", "p_maxpool_c16_b32", "two_blocks_c16_b32", "dueling_prio_u8"])
def test_forward_and_greedy_action_vs_fp64_and_the_bits_of_the_steps_s_prime_pass(pkg, name):
    """dqn_forward on 1 and 7 rows of s' (the join as a launch of its own there): within TOL_Q of the fp64 network and the bits of the step's fused q_on_sp"""
    c = CR.BY_NAME[name]; D = CR.ff_data(c); h = ff_engine(pkg, c, D); idx = D.idx[0]
    rows = np.concatenate([idx, idx])[:7]
    f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
    fw = {n: h.forward(f(D.sp[rows[:n]])) for n in (1, 7)}
    for n, q in fw.items():
        E._close("policy_q", q, CR.q_values(D.net, D.p_on, f(D.sp[rows[:n]])), msg=f"{name} n={n}", **CR.TOL_Q)
    a = h.greedy_action(f(D.sp[rows])); q64 = CR.q_values(D.net, D.p_on, f(D.sp[rows])); t = np.sort(q64, axis=1)
    clear = t[:, -1] - t[:, -2] >= CR.GAP
    assert clear.sum() >= 5
    np.testing.assert_array_equal(np.asarray(a)[clear], q64.argmax(1)[clear])
    h.train_step(idx)
    q_on_sp = h.last_q()["q_on_sp"]; q_sp7 = np.concatenate([q_on_sp, q_on_sp])[:7]
    for n, q in fw.items():
        np.testing.assert_array_equal(q, q_sp7[:n], err_msg=f"{name} n={n}")
    h.close()


# ------------------------------------------------------------------ 4: recurrent
def rec_engine(pkg, c, D, graph=1, mfma=None, unfused=False):
    layers, dueling = nn.lower(D.net)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=c.obs[0], obs_h=c.obs[1], obs_w=c.obs[2], dueling=int(dueling), buffer_size=D.cap, recurrence=1, trace_length=c.T,
                             learning_rate=LR.LR, prioritized_replay=0, use_mfma=c.mfma if mfma is None else mfma, use_graph=graph, seed=CR.ENGINE_SEED, gamma=c.gamma, double_q=c.dq)
    h = engine(pkg, layers, hp, unfused)
    feed(h, D.eps); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def rec_record(h, idx, start):
    loss, gn = h.train_step_drqn(idx, start)
    return dict(loss=loss, gn=gn, g=h.get_grads(), p=h.get_params(0))


@pytest.mark.parametrize("c", CR.REC_CASES, ids=IDS(CR.REC_CASES))
def test_recurrent_steps_vs_fp64_reference(pkg, c):
    """Conv -> block -> LSTM, T = 3, B = 4: the block runs over the T * B columns like every feed-forward layer of the recurrent program; three steps compare what a
    recurrent step reports (loss, gradients per block, grad_norm, parameters after fp64 Adam); use_graph 0 against 1, use_mfma 0 against 1, unfused and a rerun, bit for bit"""
    D = CR.rec_data(c); net = D.net
    h = rec_engine(pkg, c, D, graph=1); recs = []
    adam = LR.Adam(D.p_on.size, lr=LR.LR)
    for k in range(3):
        idx, start = D.draws[k]
        p_prev = h.get_params(0)
        batch = h.episode_get_batch(idx, start)
        for got, want in zip(batch, R.sample_batch(D.ring, idx, start, c.T, c.obs)):
            np.testing.assert_array_equal(np.asarray(got).reshape(want.shape), want)
        batch = R.sample_batch(D.ring, idx, start, c.T, c.obs)
        o = CR.rec_step(net, p_prev, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq))
        rec = rec_record(h, idx, start); recs.append(rec)
        np.testing.assert_allclose(rec["loss"], o["loss"], rtol=2e-5, atol=1e-7, err_msg=f"{c.name} step {k}: loss")      # the recurrent tables' loss tolerance
        CR.check_grads(net, rec["g"], o["grads"], live=k == 0)
        E._close("grad_norm", rec["gn"], o["grad_norm"], msg=c.name, **CR.TOL_GN)
        CR.check_params(rec["p"], adam.step(p_prev, rec["g"]))
    for kw, what in ((dict(graph=0), "use_graph 0 vs 1"), (dict(graph=1), "two identical runs"), (dict(mfma=0), "use_mfma 0 vs 1"), (dict(unfused=True), "DQN_NO_SKIP_FUSE 1 vs 0")):
        h2 = rec_engine(pkg, c, D, **kw)
        for k in range(3):
            r2 = rec_record(h2, *D.draws[k])
            assert (r2["loss"], r2["gn"]) == (recs[k]["loss"], recs[k]["gn"]), what
            np.testing.assert_array_equal(r2["g"], recs[k]["g"], err_msg=what); np.testing.assert_array_equal(r2["p"], recs[k]["p"], err_msg=what)
        if kw.get("unfused"):
            assert_launches(h2, net, True)
        h2.close()
    assert_launches(h, net, False)
    h.close()


# ------------------------------------------------------------------ 5: device loops
def _env_net(frames=4):
    return nn.Chain(nn.Conv(3, frames, 8, nn.relu, 1, 1), CR.block(8)(), nn.flattenbatch, nn.Dense(200, 16, nn.relu), nn.Dense(16, 4))


def test_device_loop_acts_on_the_fp64_argmax_and_reports_the_general_tail(pkg, mods):
    """TestMDP((5, 5), 4, 6), 8 copies: 12 vector steps at eps = 0; every action is the fp64 argmax where the gap is at least GAP; envs_info reports fused tail false
    (fused_tail = 0: a network with a block takes the general acting tail); dqn_evaluate gives finite averages"""
    net = _env_net()
    h, p, spec = G._env_engine(pkg, mods, net)
    h.envs_create(spec, max_episode_length=100, seed=17)
    checked = 0
    for t in range(12):
        obs = h.envs_peek()[0].copy()
        h.rollout(1, t0=t + 1, train_freq=0, target_update_freq=0, eps=(0.0, 0.0, 1.0))
        a = h.envs_peek()[1]
        q = CR.q_values(net, p, obs.reshape((obs.shape[0], 4, 5, 5))); top = np.sort(q, axis=1)
        clear = top[:, -1] - top[:, -2] >= CR.GAP
        np.testing.assert_array_equal(a[clear], q.argmax(1)[clear], err_msg=f"step {t}")
        checked += int(clear.sum())
    assert checked >= 0.9 * 12 * 8, checked
    assert h.envs_info() == (8, False)
    r, st = h.evaluate(8, 50, seed=5)
    assert np.isfinite(r) and np.isfinite(st) and st > 0
    h.close()


# ------------------------------------------------------------------ 6: checkpoint / resume and the solver's save / restore
@pytest.mark.parametrize("name", ["mfma_c16_6x6_b32", "dueling_prio_u8"])
def test_checkpoint_resume_gives_the_same_bits(pkg, name):
    """four sampled steps straight against two, a checkpoint restored into a FRESH engine, and two more: the same step outputs, parameters, Adam state, priorities and
    dqn_forward bits"""
    c = CR.BY_NAME[name]; D = CR.ff_data(c)
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
    f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
    np.testing.assert_array_equal(a.forward(f(D.s[:7])), b2.forward(f(D.s[:7])))
    assert np.abs(a.get_params(0) - D.p_on).max() > 0
    a.close(); b2.close()


SOLVE_SIZES = [(3, 3, 4, 8), (8,), (3, 3, 8, 8), (8,), (3, 3, 8, 8), (8,), (16, 200), (16,), (4, 16), (4,)]


def test_short_solve_round_trip_through_qnetwork_bson(pkg, mods, tmp_path):
    """TestMDP((5, 5), 4, 6), device_envs, Conv -> block -> Dense -> Dense: a short solve trains, saves qnetwork.bson with the inner convs' arrays in Flux.params order,
    and restore_best_model puts back parameters whose dqn_forward bits are the saved model's"""
    nn_, envs, S, bson = mods
    env = envs.TestMDP((5, 5), 4, 6, n=16, seed=7)
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.01, steps=200 / 2), rng=np.random.default_rng(1))
    solver = S.DeepQLearningSolver(qnetwork=_env_net(), max_steps=200, learning_rate=0.005, exploration_policy=expl, eval_freq=100, save_freq=100, num_ep_eval=16, train_freq=1,
                                   log_freq=100, double_q=False, dueling=False, prioritized_replay=True, verbose=False, logdir=str(tmp_path / "log"), device_envs=True,
                                   buffer_size=1024, train_start=64)
    policy = S.solve(solver, env); h = policy.engine
    assert h.get_counters()["train_steps"] > 0
    path = tmp_path / "log" / "qnetwork.bson"
    assert path.exists(), "no model was saved"
    w, sizes = bson.load_qnetwork(path)
    assert [tuple(x) for x in sizes] == SOLVE_SIZES
    obs = np.random.default_rng(3).random((7, 4, 5, 5), dtype=np.float32)
    h.set_params(w, pkg.NET_ONLINE); q_saved = h.forward(obs)
    E._close("saved_q", q_saved, CR.q_values(_env_net(), w, obs), msg="the saved model", **CR.TOL_Q)
    h.set_params(w * np.float32(0.5), pkg.NET_ONLINE)
    assert np.abs(h.forward(obs) - q_saved).max() > 0
    S.restore_best_model(solver, policy)
    np.testing.assert_array_equal(h.forward(obs), q_saved)
    np.testing.assert_array_equal(h.get_params(pkg.NET_ONLINE), w)
    h.close()


# ------------------------------------------------------------------ 7: refusals
def test_replicas_are_refused(pkg, monkeypatch):
    c = CR.BY_NAME["valu_c4_5x5_b5"]; D = CR.ff_data(c)
    h = ff_engine(pkg, c, D)
    with pytest.raises(nn._abi.DQNError, match=r"dqn_comm_init: layer 0 is a Conv with pad \(1, 1\); data-parallel replicas .* not supported \(single GPU only\)"):
        h.comm_init(bytes(128), 0, 1)      # (the padded stem is named first: the refusals go in the kind table's order)
    h.train_step(D.idx[0])      # the engine is left as it was
    h.close()
    c = CR.BY_NAME["p_pad0_tanh_c16_b32"]; D = CR.ff_data(c)      # no padded Conv and no pool outside the block ... but the inner convs are padded ones
    h = ff_engine(pkg, c, D)
    with pytest.raises(nn._abi.DQNError, match=r"dqn_comm_init: layer 1 is a Conv with pad \(1, 1\); .*\(single GPU only\)"):
        h.comm_init(bytes(128), 0, 1)
    h.close()
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    with pytest.raises(nn._abi.DQNError, match=r"DQN_SIM_WORLD: layer 1 is a Conv with pad \(1, 1\); .*\(single GPU only\)"):
        ff_engine(pkg, c, D)


def test_engine_creation_refuses_by_layer_index(pkg):
    abi = nn._abi

    def L(kind, **kw):
        d = abi.LayerDesc(); d.kind = kind
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    cv = lambda cin=16, cout=16, k=3, pad=1, **kw: L(1, cin=cin, cout=cout, kh=k, kw=k, sh=1, sw=1, n_in=pad, n_out=pad, **kw)
    hp = pkg.default_hparams(batch_size=8, n_actions=4, obs_c=2, obs_h=6, obs_w=6, dueling=0, buffer_size=64)
    stem, head = cv(2, 16, act=1), L(0, n_in=576, n_out=4)
    for layers, msg in (([stem, cv(), L(10, cin=0), head], r"layer 2: a convolutional skip block holds at least one inner layer \(cin = m = 0 must be >= 1\)"),
                        ([stem, cv(), L(10, cin=3), head], r"layer 2: the convolutional skip block's 3 inner layers would start before the first layer"),
                        ([stem, cv(), L(10, cin=1), cv(), L(10, cin=3), head], r"layer 4: .*reach across the join of another skip block \(layer 2\)"),
                        ([cv(2, 2), L(10, cin=1), L(0, n_in=72, n_out=4)], r"layer 1: the convolutional skip block's first inner layer \(layer 0\) reads the observation"),
                        ([stem, cv(k=1, pad=0), L(10, cin=1), head], r"layer 2: the convolutional skip block holds a Conv with pad 0 \(layer 1, kernel \(1, 1\)\)"),
                        ([stem, cv(), L(5, kh=1, kw=1, sh=1, sw=1), L(10, cin=2), head], r"layer 3: the convolutional skip block holds a MaxPool / MeanPool layer \(layer 2\)"),
                        ([stem, cv(16, 8), L(10, cin=1), L(0, n_in=288, n_out=4)], r"layer 2: the convolutional skip block maps a \(16, 6, 6\) map to a \(8, 6, 6\) map"),
                        ([stem, cv(k=5), L(10, cin=1), L(0, n_in=256, n_out=4)], r"layer 2: the convolutional skip block maps a \(16, 6, 6\) map to a \(16, 4, 4\) map"),
                        ([stem, cv(), L(10, cin=1, act=1), head], r"layer 2: a convolutional skip block's join has no activation"),
                        ([stem, cv(), L(9, cin=1), head], r"layer 2: the skip block holds a Conv / MaxPool / MeanPool layer \(layer 1\).*convolutional residual blocks are not supported")):
        with pytest.raises(abi.DQNError, match=msg):
            pkg.Engine(layers, hp)
    hp1 = pkg.default_hparams(batch_size=8, n_actions=4, obs_c=2, obs_h=1, obs_w=1, dueling=0, buffer_size=64)
    with pytest.raises(abi.DQNError, match=r"layer 2: a skip block cannot be the network's output layer"):
        pkg.Engine([cv(2, 4), cv(4, 4), L(10, cin=1)], hp1)
    hpd = pkg.default_hparams(batch_size=8, n_actions=4, obs_c=2, obs_h=6, obs_w=6, dueling=1, buffer_size=64)
    with pytest.raises(abi.DQNError, match=r"layer 2: a convolutional skip block is supported in the base chain only"):
        pkg.Engine([stem, cv(), L(10, stream=1, cin=1), L(0, stream=1, n_in=576, n_out=1), L(0, stream=2, n_in=576, n_out=4)], hpd)


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (docs/history/conv_skip.md records them)"""
    print("\nWORST error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("WORST gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(R.WORST.items())})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
