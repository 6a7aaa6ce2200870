"""GPU: train steps, inactive passes, device loops, resume, solver round trip and refusals of networks with Flux Dropout layers (csrc/dropout.hip), all through the C ABI.
The mask is read out EXACTLY through an identity network and compared with the NumPy statement of the mask law, element for element; every case of
dropout_reference.py's tables then runs one train step against the two-legged fp64 reference under that law's masks, with the per-step checks of the LayerNorm tests
(Q on s and s', target Q, greedy indices exactly, y, td, loss, per-block gradients -- live --, grad_norm, parameters after fp64 Adam, priorities; tolerances are the
project's existing constants, unchanged), then use_graph 0 against 1 and a second identical run, bit for bit.  The C twin does not know the layer: parity rests on the
fp64 reference plus these bit-for-bit companions (the RNN and LayerNorm precedent).

Without the layer every test here fails at engine creation ("unknown kind 8").  A mask wrong in one element, or the layer active on s' / in the target pass, is off by
hundreds of tolerances on every case (test_dropout_cpu.test_the_tests_can_tell).

One MI355X, one run: docs/history/dropout.md records the worst error / tolerance per quantity and per gradient block kind."""
import importlib
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import dqn_oracle as O
import dropout_reference as DR
import feedforward_edges_common as E
import feedforward_gpu_common as G
import layernorm_reference as LR
import recurrent_reference as R
from drqn_common import feed

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()
nn = DR.nn
FUSED = ("tiny_step", "red_head", "head_cols4", "drqn_cols")      # the whole-step and head fusions that decline a network with the layer


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "envs", "solver", "bson"))


# ------------------------------------------------------------------ 1: the mask, read out exactly
def readout_net(n, ps):
    """Dense(n, n) -> Dropout(p) [-> Dense(n, n) -> Dropout(p2)] -> Dense(n, n) with W = I, first bias 1, the others 0: on zero observations Q[b, f] is exactly the product of
    (keep ? scale : 0) over the Dropout layers in the active pass and exactly 1 in every other pass"""
    layers, flat = [nn.Dense(n, n)], [np.eye(n, dtype=np.float32).ravel(), np.ones(n, np.float32)]
    for p in ps:
        layers += [nn.Dropout(p), nn.Dense(n, n)]; flat += [np.eye(n, dtype=np.float32).ravel(), np.zeros(n, np.float32)]
    return nn.Chain(*layers), np.concatenate(flat)


def readout_engine(pkg, net, flat, n, B, graph=1):
    hp = pkg.default_hparams(batch_size=B, n_actions=n, obs_c=n, dueling=0, buffer_size=B + 8, learning_rate=0.0, gamma=0.95, prioritized_replay=0, use_graph=graph, seed=DR.ENGINE_SEED)
    h = pkg.Engine(nn.lower(net)[0], hp)
    rng = np.random.default_rng(n * 100 + B); m = B + 8
    z = np.zeros((m, n), np.float32)
    h.replay_add(z, rng.integers(0, n, m).astype(np.int32), rng.standard_normal(m).astype(np.float32), z, (rng.random(m) < 0.2).astype(np.uint8))
    h.set_params(flat, 0); h.set_params(flat, 1)
    return h


def expected_q(net, k, B):
    q = 1.0
    for l, m in DR.masks_for(net, k, B).items():
        q = q * np.where(m, np.float32(DR.do_scale(nn.all_layers(net)[l].p)), np.float32(0))
    return q.astype(np.float32)


READOUT_P = (0.25, 0.5, 0.9)
READOUT = [(n, B, READOUT_P[(i + j) % 3]) for i, n in enumerate((7, 16, 33, 64)) for j, B in enumerate((4, 5, 6, 32, 70))]


@pytest.mark.parametrize("n,B,p", READOUT, ids=[f"n{n}_b{B}_p{p}" for n, B, p in READOUT])
def test_mask_readout_is_the_numpy_law_element_for_element(pkg, n, B, p):
    """three consecutive steps (parameters set back between them; the learning rate is 0): step k shows counter k; q_on_sp and q_tg_sp are exactly 1; use_graph 0 gives the
    same bits; dqn_train_steps(3) ends on the mask of counter 2"""
    net, flat = readout_net(n, [p]); idx = np.arange(B, dtype=np.int64)
    shown = {}
    for graph in (1, 0):
        h = readout_engine(pkg, net, flat, n, B, graph)
        for k in range(3):
            assert h.get_counters()["train_steps"] == k
            h.train_step(idx); q = h.last_q()
            np.testing.assert_array_equal(q["q_on_s"], expected_q(net, k, B), err_msg=f"graph {graph} step {k}")
            np.testing.assert_array_equal(q["q_on_sp"], np.ones((B, n), np.float32)); np.testing.assert_array_equal(q["q_tg_sp"], np.ones((B, n), np.float32))
            np.testing.assert_array_equal(h.get_params(0), flat)
            shown[(graph, k)] = (q["q_on_s"].copy(), h.get_grads())
            h.set_params(flat, 0)
        names = [t for nm, _ in h.profile_step(max_entries=512) for t in nm.split("+")]
        assert names.count("fwd_on_do1") == 1 and names.count("bwd_do1") == 1 and "fwd_tg_do1" not in names and not set(FUSED) & set(names), names
        h.close()
    for k in range(3):
        np.testing.assert_array_equal(shown[(1, k)][0], shown[(0, k)][0]); np.testing.assert_array_equal(shown[(1, k)][1], shown[(0, k)][1])
    assert not np.array_equal(shown[(1, 0)][0], shown[(1, 1)][0])
    h = readout_engine(pkg, net, flat, n, B)
    h.train_steps(3)
    assert h.get_counters()["train_steps"] == 3
    got = h.last_q()["q_on_s"]; rows = h.last_indices()      # the sampled rows are all zero observations: any batch shows the mask of its columns
    assert rows.shape == (B,)
    np.testing.assert_array_equal(got, expected_q(net, 2, B))
    h.close()


@pytest.mark.parametrize("ps", [(0.0, 0.5), (0.5, 0.0), (0.5, 0.25)], ids=["second_alone", "first_alone", "both"])
def test_a_second_dropout_layer_shows_its_own_layer_tag(pkg, ps):
    n, B = 16, 6
    net, flat = readout_net(n, list(ps)); h = readout_engine(pkg, net, flat, n, B)
    h.train_step(np.arange(B, dtype=np.int64))
    m = DR.masks_for(net, 0, B)
    assert sorted(m) == [1, 3] and not np.array_equal(DR.keep_mask(DR.ENGINE_SEED, 0, 1, n, B, 0.5), DR.keep_mask(DR.ENGINE_SEED, 0, 3, n, B, 0.5))
    np.testing.assert_array_equal(h.last_q()["q_on_s"], expected_q(net, 0, B))
    names = [t for nm, _ in h.profile_step(max_entries=512) for t in nm.split("+")]
    assert all(names.count(x) == 1 for x in ("fwd_on_do1", "fwd_on_do3", "bwd_do1", "bwd_do3")) and not [x for x in names if x.startswith("fwd_tg_do")], names
    h.close()


# ------------------------------------------------------------------ 2, 4: one train step against the fp64 reference
def _obs3(obs):
    return tuple(obs) + (1,) * (3 - len(obs))


def ff_engine(pkg, c, D, graph=1, prio=None):
    layers, dueling = nn.lower(D.net); o = _obs3(c.obs)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=o[0], obs_h=o[1], obs_w=o[2], dueling=int(dueling), buffer_size=c.B + 24, learning_rate=LR.LR, gamma=c.gamma,
                             double_q=c.dq, prioritized_replay=c.prio if prio is None else prio, obs_dtype=c.u8, use_mfma=c.mfma, use_graph=graph, seed=DR.ENGINE_SEED)
    h = pkg.Engine(layers, hp)
    h.replay_add(D.s, D.a, D.r, D.sp, D.d); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def ff_record(h, idx):
    loss, gn, td = h.train_step(idx)
    return dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities())


def do_launches(net):
    return [i for i, l in enumerate(nn.all_layers(net)) if l.kind == "dropout"]


def assert_launches(h, net):
    """exactly one fwd_on_do<i> and one bwd_do<i> per Dropout layer, no fwd_tg_do<i>, none of the fused launches"""
    names = [n for n, _ in h.profile_step(max_entries=512)]
    tokens = [t for n in names for t in n.split("+")]
    layers = do_launches(net)
    assert layers and all(tokens.count(f"fwd_on_do{i}") == 1 and tokens.count(f"bwd_do{i}") == 1 and f"fwd_tg_do{i}" not in tokens for i in layers), names
    assert not [t for t in tokens if t.startswith(("fwd_tg_do", "act_fwd_do"))], names      # (bwd_valu_do<i> is the level's VALU task table: the tail tasks of the layers above)
    assert not set(FUSED) & set(tokens), names
    return names


@pytest.mark.parametrize("c", DR.CASES, ids=IDS(DR.CASES))
def test_step_vs_fp64_reference_graph_vs_eager_and_rerun(pkg, c):
    D = DR.ff_data(c); net = D.net; idx = D.idx[0]; msg = c.name
    h = ff_engine(pkg, c, D, graph=1)
    p_prev = h.get_params(0); np.testing.assert_array_equal(p_prev, D.p_on)
    batch = h.get_batch(idx)
    for k, (a, b) in enumerate(zip(batch, DR.ff_batch(c, D, idx))):
        if k < 5:
            np.testing.assert_array_equal(np.asarray(a, np.float64).reshape(np.shape(b)), np.asarray(b, np.float64), err_msg=f"{msg}: batch[{k}]")
    E._close("is_weights", batch[5], DR.ff_batch(c, D, idx)[5], rtol=2e-6, msg=msg)
    masks = DR.masks_for(net, 0, c.B)
    sg, rm, gap = DR.case_margins(c)
    assert sg >= LR.SIGMA_MIN and rm > LR.RELU_MARGIN and gap > LR.GAP, (msg, sg, rm, gap)
    o = DR.ff_step(net, p_prev, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq), masks)
    rec = ff_record(h, idx); q = rec["q"]
    E._close("q_on_s", q["q_on_s"], o["q_on_s"], msg=msg, **LR.TOL_Q)
    E._close("q_tg_sp", q["q_tg_sp"], o["q_tg_sp"], msg=msg, **LR.TOL_Q)
    if c.dq:
        E._close("q_on_sp", q["q_on_sp"], o["q_on_sp"], msg=msg, **LR.TOL_Q)
    np.testing.assert_array_equal(q["best_a"], o["best_a"], err_msg=msg)
    E._close("y", q["y"], o["y"], msg=msg, **LR.TOL_TD)
    E._close("td", rec["td"], o["td"], msg=msg, **LR.TOL_TD)
    E._close("loss", rec["loss"], o["loss"], msg=msg, **LR.TOL_LOSS)
    DR.check_grads(net, rec["g"], o["grads"], live=True)
    E._close("grad_norm", rec["gn"], o["grad_norm"], msg=msg, **LR.TOL_GN)
    LR.check_params(rec["p"], LR.Adam(D.p_on.size, lr=LR.LR).step(p_prev, rec["g"]))
    if c.prio:
        # the new priorities (|td| + eps)^alpha come from the MASKED Q's td.  Bound: the td tolerance carried through the derivative alpha (|td| + eps)^(alpha - 1), twice,
        # plus fp32 rounding of the result
        eps, alpha = 1e-3, 0.6; t = np.abs(o["td"])
        want = O.priority_from_td(t, np.float32(eps), np.float32(alpha)).astype(np.float64)
        bound = 2 * alpha * (t + eps) ** (alpha - 1) * (LR.TOL_TD["atol"] + LR.TOL_TD["rtol"] * t) + 1e-6 * want
        assert (np.abs(rec["pr"][idx] - want) <= bound).all(), (msg, np.abs(rec["pr"][idx] - want).max())
    for graph, what in ((0, "use_graph 0 vs 1"), (1, "two identical runs")):
        h2 = ff_engine(pkg, c, D, graph=graph)
        E.same_bits([rec], [ff_record(h2, idx)], f"{msg}: {what}")
        h2.close()
    assert all(p == (0, 0, 0) for p, l in zip(h.plan(), nn.lower(net)[0]) if l.kind == nn._abi.LAYER_DROPOUT)      # the layer's plan entry is all zeros
    names = assert_launches(h, net)
    assert ("head_td" in names) or ("td_huber" in names), names
    h.close()


# ------------------------------------------------------------------ 3: inactive passes
@pytest.mark.parametrize("name", ["n512_b32", "do_ln", "dueling_prio", "two_do"])
def test_forward_is_the_unmasked_network_and_the_bits_of_the_steps_s_prime_pass(pkg, name):
    """dqn_forward on 1 and 7 rows of s': within TOL_Q of the fp64 network WITHOUT masks, and (where the batch has that many columns) the bits of the step's q_on_sp"""
    c = DR.BY_NAME[name]; D = DR.ff_data(c); h = ff_engine(pkg, c, D); idx = D.idx[0]
    rows = np.concatenate([idx, idx])[:7]      # B = 5: seven rows by going round
    fw = {n: h.forward(D.sp[rows[:n]]) for n in (1, 7)}
    for n, q in fw.items():
        E._close("policy_q", q, DR.q_values(D.net, D.p_on, D.sp[rows[:n]]), msg=f"{name} n={n}", **LR.TOL_Q)
    a = h.greedy_action(D.sp[rows]); q64 = DR.q_values(D.net, D.p_on, D.sp[rows]); t = np.sort(q64, axis=1)
    clear = t[:, -1] - t[:, -2] >= LR.GAP
    assert clear.sum() >= 5
    np.testing.assert_array_equal(np.asarray(a)[clear], q64.argmax(1)[clear])
    h.train_step(idx)
    q_on_sp = h.last_q()["q_on_sp"]; q_sp7 = np.concatenate([q_on_sp, q_on_sp])[:7]
    for n, q in fw.items():
        np.testing.assert_array_equal(q, q_sp7[:n], err_msg=f"{name} n={n}")
    h.close()


def test_p0_forward_on_s_is_the_steps_q_on_s_bit_for_bit(pkg):
    c = DR.BY_NAME["p0_n33_b32"]; D = DR.ff_data(c); h = ff_engine(pkg, c, D); idx = D.idx[0]
    fw = {n: h.forward(D.s[idx[:n]]) for n in (1, 7)}
    h.train_step(idx)
    for n, q in fw.items():
        np.testing.assert_array_equal(q, h.last_q()["q_on_s"][:n])
    h.close()


def _env_net():
    return nn.Chain(nn.Dense(100, 16, nn.relu), nn.Dropout(0.1), nn.Dense(16, 4))


def test_device_loop_acts_on_the_fp64_argmax_without_masks_and_evaluate_leaves_the_parameters(pkg, mods):
    """TestMDP((5, 5), 4, 6), 8 copies: 12 vector steps at eps = 0; every action is the fp64 argmax of the UNMASKED network where the gap is at least GAP; the acting
    program emits nothing for the layer and reports the general tail truthfully (fused_tail = 0)"""
    net = _env_net()
    h, p, spec = G._env_engine(pkg, mods, net)
    h.envs_create(spec, max_episode_length=100, seed=17)
    checked = 0
    for t in range(12):
        obs = h.envs_peek()[0].copy()
        h.rollout(1, t0=t + 1, train_freq=0, target_update_freq=0, eps=(0.0, 0.0, 1.0))
        a = h.envs_peek()[1]
        q = DR.q_values(net, p, obs); top = np.sort(q, axis=1)
        clear = top[:, -1] - top[:, -2] >= LR.GAP
        np.testing.assert_array_equal(a[clear], q.argmax(1)[clear], err_msg=f"step {t}")
        checked += int(clear.sum())
    assert checked >= 0.9 * 12 * 8, checked
    assert h.envs_info() == (8, False)
    before = h.get_params(0)
    r, st = h.evaluate(8, 50, seed=5)
    assert np.isfinite(r) and np.isfinite(st) and st > 0
    np.testing.assert_array_equal(h.get_params(0), before); np.testing.assert_array_equal(h.get_params(1), before)
    assert h.get_counters()["train_steps"] == 0      # acting and evaluating leave the mask stream where it was
    h.close()


def test_device_loop_trains(pkg, mods):
    """the env-cadence graphs (acting step + pipelined train steps): finite losses, parameters move, the step counter counts the train steps"""
    net = _env_net()
    h, p, spec = G._env_engine(pkg, mods, net)
    h.envs_create(spec, max_episode_length=100, seed=17)
    st = h.rollout(24, t0=1, train_freq=2, target_update_freq=8, eps=(1.0, 0.1, 20.0))
    assert st["train_steps"] > 0 and np.isfinite(st["loss"]) and np.isfinite(st["grad_norm"]), st
    assert h.get_counters()["train_steps"] == st["train_steps"]
    pn = h.get_params(0)
    assert np.isfinite(pn).all() and np.abs(pn - p).max() > 0
    h.close()


# ------------------------------------------------------------------ 5: recurrent
def rec_engine(pkg, c, D, graph=1):
    layers, dueling = nn.lower(D.net)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=c.obs[0], dueling=int(dueling), buffer_size=D.cap, recurrence=1, trace_length=c.T, learning_rate=LR.LR,
                             prioritized_replay=0, use_mfma=c.mfma, use_graph=graph, seed=DR.ENGINE_SEED, gamma=c.gamma, double_q=c.dq)
    h = pkg.Engine(layers, hp)
    feed(h, D.eps); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def rec_record(h, idx, start):
    loss, gn = h.train_step_drqn(idx, start)
    return dict(loss=loss, gn=gn, g=h.get_grads(), p=h.get_params(0))


@pytest.mark.parametrize("c", DR.REC_CASES, ids=IDS(DR.REC_CASES))
def test_recurrent_steps_vs_fp64_reference(pkg, c):
    """T = 3, B = 4, p = 0.5: the layer runs once over the T * B s columns with a distinct mask per (t, b) column (col = t * B + b); the target loop is unmasked.  Two
    steps: the second one's masks are those of counter 1.  use_graph 0 against 1 and a rerun, bit for bit"""
    D = DR.rec_data(c); net = D.net
    h = rec_engine(pkg, c, D, graph=1); recs = []
    adam = LR.Adam(D.p_on.size, lr=LR.LR)
    for k in range(2):
        idx, start = D.draws[k]
        assert h.get_counters()["train_steps"] == k
        p_prev = h.get_params(0)
        batch = h.episode_get_batch(idx, start)
        for got, want in zip(batch, R.sample_batch(D.ring, idx, start, c.T, c.obs)):
            np.testing.assert_array_equal(np.asarray(got).reshape(want.shape), want)
        batch = R.sample_batch(D.ring, idx, start, c.T, c.obs)
        masks = DR.masks_for(net, k, c.B, c.T)
        if k == 0:      # a distinct mask per (t, b) column (known on the CPU for these seeds: 12 distinct patterns of 8 bits); step 1 draws others
            assert all(len({m[t, b].tobytes() for t in range(c.T) for b in range(c.B)}) == c.T * c.B for m in masks.values())
            assert all(not np.array_equal(m, DR.masks_for(net, 1, c.B, c.T)[l]) for l, m in masks.items())
        o = DR.rec_step(net, p_prev, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq), masks)
        rec = rec_record(h, idx, start); recs.append(rec)
        np.testing.assert_allclose(rec["loss"], o["loss"], rtol=2e-5, atol=1e-7, err_msg=f"{c.name} step {k}: loss")      # the recurrent tables' loss tolerance
        DR.check_grads(net, rec["g"], o["grads"], live=k == 0)
        E._close("grad_norm", rec["gn"], o["grad_norm"], msg=c.name, **LR.TOL_GN)
        LR.check_params(rec["p"], adam.step(p_prev, rec["g"]))
    assert h.get_counters()["train_steps"] == 2
    for graph, what in ((0, "use_graph 0 vs 1"), (1, "two identical runs")):
        h2 = rec_engine(pkg, c, D, graph=graph)
        for k in range(2):
            r2 = rec_record(h2, *D.draws[k])
            assert (r2["loss"], r2["gn"]) == (recs[k]["loss"], recs[k]["gn"]), what
            np.testing.assert_array_equal(r2["g"], recs[k]["g"], err_msg=what); np.testing.assert_array_equal(r2["p"], recs[k]["p"], err_msg=what)
        h2.close()
    assert_launches(h, net)
    h.close()


# ------------------------------------------------------------------ 6, 7: grouped steps and resume
@pytest.mark.parametrize("name", ["relu_n33_b6", "n512_b32", "do_ln"])
def test_train_steps_5_equals_five_train_step_calls(pkg, name):
    c = DR.BY_NAME[name]; D = DR.ff_data(c)
    a, b = ff_engine(pkg, c, D, prio=1), ff_engine(pkg, c, D, prio=1)
    la = a.train_steps(5)
    for _ in range(5):
        lb = b.train_step(want_td=False)
    assert la == lb
    np.testing.assert_array_equal(a.get_params(0), b.get_params(0)); np.testing.assert_array_equal(a.get_grads(), b.get_grads())
    np.testing.assert_array_equal(a.replay_priorities(), b.replay_priorities())
    for k in ("q_on_s", "q_on_sp", "q_tg_sp", "y"):
        np.testing.assert_array_equal(a.last_q()[k], b.last_q()[k])
    for x, y in zip(a.get_adam_state(), b.get_adam_state()):
        np.testing.assert_array_equal(x, y)
    assert a.get_counters() == b.get_counters() and a.get_counters()["train_steps"] == 5
    assert np.abs(a.get_params(0) - D.p_on).max() > 0
    a.close(); b.close()


@pytest.mark.parametrize("name", ["relu_n33_b6", "dueling_prio"])
def test_resume_continues_the_mask_stream(pkg, name):
    """four sampled steps straight against two, a checkpoint (parameters, Adam state, replay, counters) restored into a FRESH engine, and two more: bit-identical,
    masks included (q_on_s of the last step is the masked Q); a resumed engine whose step counter is NOT restored draws other masks"""
    c = DR.BY_NAME[name]; D = DR.ff_data(c)
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
    b3 = ff_engine(pkg, c, D, prio=1); b3.restore(ck)
    cn = b3.get_counters(); b3.set_counters(cn["size"], cn["widx"], cn["sample_ctr"], 0)      # the same batch, another counter: other masks
    b3.set_adam_state(ck["adam_m"], ck["adam_v"], ck["adam_bp"])
    b4 = ff_engine(pkg, c, D, prio=1); b4.restore(ck)
    b3.train_step(want_td=False); b4.train_step(want_td=False)
    np.testing.assert_array_equal(b3.last_indices(), b4.last_indices())
    assert not np.array_equal(b3.last_q()["q_on_s"], b4.last_q()["q_on_s"])
    np.testing.assert_array_equal(b3.last_q()["q_tg_sp"], b4.last_q()["q_tg_sp"])
    for h in (a, b2, b3, b4):
        h.close()


# ------------------------------------------------------------------ 8: solver round trip
def test_solver_round_trip_on_the_device_loop(pkg, mods, tmp_path, monkeypatch):
    """solve with a logdir (save_model at save_freq), then restore_best_model: bit-identical parameters; qnetwork.bson holds exactly [W, b, W, b]"""
    G.solver_round_trip(pkg, mods, tmp_path, monkeypatch, _env_net(), [(16, 100), (16,), (4, 16), (4,)])


def test_solver_round_trip_on_the_host_loop(pkg, mods, tmp_path):
    nn_, envs, S, bson = mods
    env = envs.TestMDP((5, 5), 4, 6, n=8, seed=7)
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.05, steps=200), rng=np.random.default_rng(1))
    solver = S.DeepQLearningSolver(qnetwork=_env_net(), max_steps=300, learning_rate=0.005, exploration_policy=expl, eval_freq=100, save_freq=100, num_ep_eval=10, log_freq=100,
                                   double_q=True, dueling=False, prioritized_replay=True, train_start=64, verbose=False, logdir=str(tmp_path / "log"), device_envs=False)
    policy = S.solve(solver, env)
    p = policy.engine.get_params(pkg.NET_ONLINE)
    assert np.isfinite(p).all() and policy.engine.get_counters()["train_steps"] > 0
    w, sizes = bson.load_qnetwork(tmp_path / "log" / "qnetwork.bson")
    assert [tuple(x) for x in sizes] == [(16, 100), (16,), (4, 16), (4,)] and w.size == 16 * 100 + 16 + 4 * 16 + 4
    policy.engine.set_params(w * np.float32(0.5), pkg.NET_ONLINE)
    S.restore_best_model(solver, policy)
    np.testing.assert_array_equal(policy.engine.get_params(pkg.NET_ONLINE), w)
    policy.engine.close()


# ------------------------------------------------------------------ 9: refusals
def test_replicas_are_refused(pkg, monkeypatch):
    c = DR.BY_NAME["relu_n33_b6"]; D = DR.ff_data(c)
    h = ff_engine(pkg, c, D)
    with pytest.raises(nn._abi.DQNError, match=r"dqn_comm_init: layer 1 is a Dropout layer; data-parallel replicas .* not supported \(single GPU only\)"):
        h.comm_init(bytes(128), 0, 1)
    h.train_step(D.idx[0])      # the engine is left as it was
    h.close()
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    with pytest.raises(nn._abi.DQNError, match=r"DQN_SIM_WORLD: layer 1 is a Dropout layer; .*\(single GPU only\)"):
        ff_engine(pkg, c, D)


def test_engine_creation_refuses_by_layer_index_and_value(pkg):
    abi = nn._abi

    def L(kind, **kw):
        d = abi.LayerDesc(); d.kind = kind
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    hp = pkg.default_hparams(batch_size=8, n_actions=4, obs_c=6, dueling=0, buffer_size=64)
    hi = int(np.uint32(int(np.float64(1.0).view(np.uint64)) >> 32).view(np.int32))
    with pytest.raises(abi.DQNError, match=r"layer 1: Dropout p = 1 .*must be finite with 0 <= p < 1 \(p = 1 drops every feature: Q would be constant\)"):
        pkg.Engine([L(0, n_in=6, n_out=16, act=1), L(8, cout=hi), L(0, n_in=16, n_out=4)], hp)
    with pytest.raises(abi.DQNError, match=r"layer 1: a Dropout layer cannot be the network's output layer"):
        pkg.Engine([L(0, n_in=6, n_out=4), L(8)], hp)
    with pytest.raises(abi.DQNError, match=r"layer 0: Dropout cannot be the first layer"):
        pkg.Engine([L(8), L(0, n_in=6, n_out=4)], hp)


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (docs/history/dropout.md records them)"""
    print("\nWORST error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("WORST gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(R.WORST.items())})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
