"""GPU: train steps, policy forward, device loop, solver round trip and refusals of networks with the standalone activation layer nn.Activation(σ) (layer kind 14,
csrc/act_layer.hip; Julia's Base.Broadcast.BroadcastFunction(σ)), all through the C ABI, against the two-legged fp64 reference of activation_layer_reference.py.  Every
case of its tables runs STEPS train steps on given indices under the per-step checks of the feed-forward edge tests (Q on s and s', target Q, greedy indices exactly, y, td,
loss, per-block gradients, grad_norm, parameters after fp64 Adam, priorities; tolerances are the project's existing constants, unchanged), then use_graph 0 against 1 and a
second identical run, bit for bit.

Exact companions, engine against engine, bit for bit on every recorded field: Dense(6, 16, σ) against Dense(6, 16) -> Activation(σ) and Conv(3, 1 => 4, σ) against
Conv -> Activation(σ) for each of the eleven codes, one padded Conv, Activation(identity) against the network without it (that IS its Dense companion), Activation(tanh) ->
Activation(relu) against Dense(…, tanh) -> Activation(relu), the layer behind a Dropout against Dense(…, relu) -> Dropout, and behind a LayerNorm against LayerNorm(n, σ).  Both engines
get the same per-layer plan entries; the Activation's entry is zeros.  The law makes these identities, not tolerances: a difference is a bug in the new launches or in the
identity-epilogue wiring.

Without the feature every test here fails: nn.Activation does not exist and the engine answers "unknown kind 14".

One MI355X, one run: docs/history/activation_layer.md records the worst error / tolerance per quantity and per gradient block kind."""
import importlib
import json
import os
import time
import types

import numpy as np
import pytest

import __graft_entry__ as ge
import activation_layer_reference as XR
import activation_traits_cases as KT
import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_gpu_common as G
import recurrent_reference as R
from drqn_common import feed

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()
nn = XR.nn
abi = nn._abi
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "activation_traits_gpu.json")))
FUSED = ("tiny_step", "red_head", "head_cols4", "drqn_cols")      # the whole-step and head fusions that decline a network with the layer


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "envs", "solver", "bson"))


def hparams(pkg, c, dueling, graph=1):
    o = c.obs + (1, 1) if len(c.obs) == 1 else c.obs
    return pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=o[0], obs_h=o[1], obs_w=o[2], dueling=int(dueling), buffer_size=c.B + 24, learning_rate=XR.LRATE, gamma=c.gamma,
                               double_q=c.dq, prioritized_replay=c.prio, obs_dtype=c.u8, use_mfma=c.mfma, use_graph=graph, seed=5)


def ff_engine(pkg, c, D, graph=1, net=None, plan=None):
    layers, dueling = nn.lower(net or D.net)
    h = pkg.Engine(layers, hparams(pkg, c, dueling, graph), plan=plan)
    h.replay_add(D.s, D.a, D.r, D.sp, D.d); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def ff_record(h, idx):
    loss, gn, td = h.train_step(idx)
    return dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities())


def replay(pkg, c, D, **kw):
    h = ff_engine(pkg, c, D, **kw)
    rec = [ff_record(h, D.idx[k]) for k in range(XR.STEPS)]
    return h, rec


def assert_launches(h, net, dx=True):
    """one forward launch per network pass and one backward launch per Activation layer; none of the fusions"""
    names = [n for n, _ in h.profile_step(max_entries=512)]
    tokens = [t for n in names for t in n.split("+")]
    acts = XR.activations(net)
    assert acts
    for i, _ in acts:
        assert tokens.count(f"fwd_on_act{i}") == 1 and tokens.count(f"fwd_tg_act{i}") == 1 and tokens.count(f"bwd_act{i}") == (1 if dx else 0), (i, names)
    assert not set(FUSED) & set(tokens), names
    return names


@pytest.mark.parametrize("c", XR.CASES, ids=IDS(XR.CASES))
def test_steps_vs_fp64_reference_graph_vs_eager_and_rerun(pkg, c):
    D = XR.prepare(c); net = D.net; g32 = float(np.float32(c.gamma))
    h = ff_engine(pkg, c, D, graph=1)
    hp = hparams(pkg, c, isinstance(net, nn.DuelingNetwork))
    np.testing.assert_array_equal(h.get_params(0), D.p_on)
    rec = []; adam = XR.Adam(D.p_on.size, lr=XR.LRATE)      # fp64 Adam on the engine's own gradients
    for k in range(XR.STEPS):
        idx = D.idx[k]; msg = f"{c.name} step {k}"
        p_prev = h.get_params(0); pr_before = h.replay_priorities()
        batch = h.get_batch(idx)
        want_batch = XR.ff_batch(c, D, idx)
        if k == 0:      # the batch the engine trains on is the drawn rows (later steps: the priorities have moved, the IS weights are the engine's, checked against the law below)
            for j, (a, b) in enumerate(zip(batch[:5], want_batch[:5])):
                np.testing.assert_array_equal(np.asarray(a, np.float64).reshape(np.shape(b)), np.asarray(b, np.float64), err_msg=f"{msg}: batch[{j}]")
        E._close("is_weights", batch[5], O.is_weights(pr_before[idx], pr_before, hp.prio_beta, np.float64) if c.prio else np.ones(c.B), rtol=2e-6, msg=msg)
        batch = tuple(np.asarray(x).reshape(np.shape(w)) for x, w in zip(batch, want_batch))
        km, pm, gap = XR.margins(c, net, p_prev, D.p_tg, batch)
        assert km > XR.RELU_MARGIN and pm > XR.RELU_MARGIN and gap > XR.GAP, (msg, km, pm, gap)
        o = XR.ff_step(net, p_prev, D.p_tg, batch, g32, bool(c.dq))
        r = ff_record(h, idx); q = r["q"]; rec.append(r)
        print(f"\n{msg}: loss {r['loss']!r} (fp64 {o['loss']!r}), grad_norm {r['gn']!r} (fp64 {o['grad_norm']!r}), max |q - q64| {np.abs(q['q_on_s'] - o['q_on_s']).max():.3g}")
        E._close("q_on_s", q["q_on_s"], o["q_on_s"], msg=msg, **XR.TOL_Q)
        E._close("q_tg_sp", q["q_tg_sp"], o["q_tg_sp"], msg=msg, **XR.TOL_Q)
        if c.dq:
            E._close("q_on_sp", q["q_on_sp"], o["q_on_sp"], msg=msg, **XR.TOL_Q)
        np.testing.assert_array_equal(q["best_a"], o["best_a"], err_msg=msg)
        E._close("y", q["y"], o["y"], msg=msg, **XR.TOL_TD)
        E._close("td", r["td"], o["td"], msg=msg, **XR.TOL_TD)
        E._close("loss", r["loss"], o["loss"], msg=msg, **XR.TOL_LOSS)
        assert np.isfinite(r["g"]).all(), msg
        XR.check_grads(net, r["g"], o["grads"], live=k == 0)
        E._close("grad_norm", r["gn"], o["grad_norm"], msg=msg, **XR.TOL_GN)
        XR.check_params(r["p"], adam.step(p_prev, r["g"]))
        E.check_priorities_after_step(h, hp, idx, pr_before, r["td"], o["td"], batch[5])
    # eager against graph, and a second identical run: element-wise launches, one result whatever the launch mode or timing
    for graph, what in ((0, "use_graph 0 vs 1"), (1, "two identical runs")):
        h2, rec2 = replay(pkg, c, D, graph=graph)
        E.same_bits(rec, rec2, f"{c.name}: {what}"); h2.close()
    assert all(p == (0, 0, 0) for p, l in zip(h.plan(), nn.lower(net)[0]) if l.kind == abi.LAYER_ACTIVATION)      # the layer's plan entry is zeros and ignored
    names = assert_launches(h, net)
    assert ("head_td" in names) or ("td_huber" in names), names
    h.close()


COMPANIONS = [c for c in XR.CASES + XR.EXACT_ONLY if c.plain is not None]


@pytest.mark.parametrize("c", COMPANIONS, ids=IDS(COMPANIONS))
def test_exact_companion_the_fused_activation_bit_for_bit(pkg, c):
    """Dense(6, 16, σ) / Conv(3, 1 => 4, σ) [/ padded] against the same layer with identity -> Activation(σ), on the same data and under the same per-layer plan entries (the
    Activation's is zeros): every recorded field of every step, bit for bit.  σ = identity: the network without the layer"""
    D = XR.prepare(c); plain = c.plain()
    hp_, rec_plain = replay(pkg, c, D, net=plain)
    plan_plain = hp_.plan(); hp_.close()
    plan, it = [], iter(p for p, d in zip(plan_plain, nn.lower(plain)[0]) if d.kind != abi.LAYER_ACTIVATION)
    for d in nn.lower(D.net)[0]:
        plan.append((0, 0, 0) if d.kind == abi.LAYER_ACTIVATION else next(it))
    h, rec = replay(pkg, c, D, plan=plan)
    assert h.plan() == plan
    E.same_bits(rec, rec_plain, f"{c.name}: Activation({XR.NAMES[c.codes[0]]}) behind the layer vs fused into it")
    assert all(np.isfinite(r["g"]).all() and np.abs(r["g"]).max() > 0 for r in rec)
    assert_launches(h, D.net)
    h.close()


def nn_record(pkg, net, obs=(6, 1, 1), B=16, nA=4, steps=3, graph=1):
    """`steps` train steps of a package nn chain on data and parameters drawn here (engine against engine: compositions the fp64 reference of this file does not describe);
    also dqn_forward on 7 rows before the first step -- the passes in which a Dropout layer is the identity"""
    layers, dueling = nn.lower(net)
    hp = pkg.default_hparams(batch_size=B, n_actions=nA, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], dueling=int(dueling), buffer_size=B + 24, learning_rate=1e-3, gamma=0.95,
                             double_q=1, prioritized_replay=1, use_graph=graph, seed=5)
    rng = np.random.default_rng(11); n = B + 24
    s, sp = ((2 * rng.standard_normal((n,) + tuple(obs))).astype(np.float32) for _ in range(2))
    a = rng.integers(0, nA, n).astype(np.int32); r = (2 * rng.standard_normal(n)).astype(np.float32); d = (rng.random(n) < 0.2).astype(np.uint8)
    p = nn.glorot_params(net, seed=3)
    p_on = (2 * p + 0.05 * rng.standard_normal(p.size)).astype(np.float32); p_tg = (p_on + 0.05 * rng.standard_normal(p.size)).astype(np.float32)
    h = pkg.Engine(layers, hp); h.replay_add(s, a, r, sp, d); h.set_params(p_on, 0); h.set_params(p_tg, 1)
    fw = h.forward(s[:7]); rec = []
    for k in range(steps):
        rec.append(ff_record(h, rng.choice(n, B, replace=False).astype(np.int64)))
    names = [t for nm, _ in h.profile_step(max_entries=512) for t in nm.split("+")]
    h.close()
    assert all(np.isfinite(x["g"]).all() and np.abs(x["g"]).max() > 0 for x in rec)
    return rec, fw, names


def test_behind_a_dropout_the_layer_equals_the_fused_relu_bit_for_bit(pkg):
    """Dense(6, 16) -> Dropout(0.5) -> Activation(relu) -> Dense against Dense(6, 16, relu) -> Dropout(0.5) -> Dense, the Dropout at layer 1 in both (the mask law is keyed on
    the layer index).  relu(keep ? x * scale : 0) = keep ? relu(x) * scale : 0 for scale > 0, bit for bit -- a select commutes with one multiply --, and so do the two backwards:
    the layer reads the Dropout's MASKED buffer in the train step's online pass on s and its producer's output (the alias) in every other pass (s', target, dqn_forward).
    Dropout(0): the layer behind it gives the bits of the network without the Dropout"""
    split = lambda p, s: nn.Chain(nn.Dense(6, 16), nn.Dropout(p), XR.A(s), nn.Dense(16, 4))
    a, fa, names = nn_record(pkg, split(0.5, XR.AR.RELU))
    b, fb, _ = nn_record(pkg, nn.Chain(nn.Dense(6, 16, nn.relu), nn.Dropout(0.5), nn.Dense(16, 4)))
    assert names.count("fwd_on_do1") == 1 and names.count("bwd_do1") == 1 and names.count("fwd_on_act2") == 1 and names.count("fwd_tg_act2") == 1 and names.count("bwd_act2") == 1, names
    E.same_bits(a, b, "Dropout -> Activation(relu) vs Dense(relu) -> Dropout"); np.testing.assert_array_equal(fa, fb)
    E.same_bits(a, nn_record(pkg, split(0.5, XR.AR.RELU), graph=0)[0], "use_graph 1 vs 0")
    assert any((x["q"]["q_on_s"] != y["q"]["q_on_s"]).any() for x, y in zip(a, nn_record(pkg, split(0.0, XR.AR.RELU))[0]))      # the mask is live: p = 0.5 is not p = 0
    for s in (XR.GELU, XR.AR.TANH):      # the identity mask: with and without the Dropout layer
        c, fc, _ = nn_record(pkg, split(0.0, s))
        d, fd, _ = nn_record(pkg, nn.Chain(nn.Dense(6, 16), XR.A(s), nn.Dense(16, 4)))
        E.same_bits(c, d, f"Dropout(0) -> Activation({XR.NAMES[s]}) vs Activation alone"); np.testing.assert_array_equal(fc, fd)


@pytest.mark.parametrize("s", [XR.AR.TANH, XR.AR.RELU6], ids=["tanh", "relu6"])
def test_behind_a_layernorm_the_layer_equals_the_fused_activation_bit_for_bit(pkg, s):
    """Dense -> LayerNorm(16) -> Activation(σ) -> Dense against Dense -> LayerNorm(16, σ) -> Dense: the layer's backward hands dpre = dY σ'(y) to the LayerNorm's launches"""
    a, fa, names = nn_record(pkg, nn.Chain(nn.Dense(6, 16, nn.relu), nn.LayerNorm(16), XR.A(s), nn.Dense(16, 4)))
    b, fb, _ = nn_record(pkg, nn.Chain(nn.Dense(6, 16, nn.relu), nn.LayerNorm(16, s), nn.Dense(16, 4)))
    assert names.count("fwd_on_act2") == 1 and names.count("bwd_act2") == 1 and names.count("bwd_ln1") == 1, names
    E.same_bits(a, b, f"LayerNorm -> Activation({XR.NAMES[s]}) vs LayerNorm(σ)"); np.testing.assert_array_equal(fa, fb)


@pytest.mark.parametrize("name", ["vec_gelu", "vec_hardswish_b5_n7", "vec_gelu_b128", "map_mish", "map_gn_swish", "map_gmean_hardswish", "vec_tanh_then_relu", "postadd_map", "dueling_swish"])
def test_forward_at_1_and_7_columns(pkg, name):
    """dqn_forward on 1 and 7 observations (the one-column walk): within TOL_Q of fp64, and the bits the train step's Q has on the same rows"""
    c = XR.BY_NAME[name]; D = XR.prepare(c); h = ff_engine(pkg, c, D); idx = D.idx[0]
    fw = {n: h.forward(D.s[idx[:n]]) for n in (1, 7) if n <= c.B}
    for n, q in fw.items():
        E._close("policy_q", q, XR.q_values(D.net, D.p_on, D.s[idx[:n]]), msg=f"{name} n={n}", **XR.TOL_Q)
    h.train_step(idx)
    q_on_s = h.last_q()["q_on_s"]
    for n, q in fw.items():
        np.testing.assert_array_equal(q, q_on_s[:n], err_msg=f"{name} n={n}")
    h.close()


def rec_engine(pkg, c, D, graph=1):
    layers, dueling = nn.lower(D.net); o = c.obs + (1, 1) if len(c.obs) == 1 else c.obs
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=o[0], obs_h=o[1], obs_w=o[2], dueling=int(dueling), buffer_size=D.cap, recurrence=1, trace_length=c.T,
                             learning_rate=XR.LRATE, prioritized_replay=0, use_mfma=c.mfma, use_graph=graph, seed=5, gamma=c.gamma, double_q=c.dq)
    h = pkg.Engine(layers, hp)
    feed(h, D.eps); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def rec_record(h, idx, start):
    loss, gn = h.train_step_drqn(idx, start)
    return dict(loss=loss, gn=gn, g=h.get_grads(), p=h.get_params(0))


@pytest.mark.parametrize("c", XR.REC_CASES, ids=IDS(XR.REC_CASES))
def test_recurrent_step_vs_fp64_reference(pkg, c):
    """T = 3, B = 4: the layer runs once over the T * B columns, in front of the GRU (on the conv's map) and behind the LSTM"""
    D = XR.prepare(c); net = D.net; idx, start = D.draws[0]
    h = rec_engine(pkg, c, D, graph=1)
    p_prev = h.get_params(0)
    batch = h.episode_get_batch(idx, start)
    want = R.sample_batch(D.ring, idx, start, c.T, c.obs)
    for got, w in zip(batch, want):
        np.testing.assert_array_equal(np.asarray(got).reshape(w.shape), w)
    batch = tuple(np.asarray(x).reshape(w.shape) for x, w in zip(batch, want))
    km, pm, gap = XR.margins(c, net, p_prev, D.p_tg, batch)
    assert km > XR.RELU_MARGIN and pm > XR.RELU_MARGIN and gap > XR.GAP, (c.name, km, pm, gap)
    o = XR.rec_step(net, p_prev, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq))
    rec = rec_record(h, idx, start)
    np.testing.assert_allclose(rec["loss"], o["loss"], rtol=2e-5, atol=1e-7, err_msg=f"{c.name}: loss")      # the recurrent tables' loss tolerance (test_recurrent_edges_gpu.run_checked)
    XR.check_grads(net, rec["g"], o["grads"], live=True)
    E._close("grad_norm", rec["gn"], o["grad_norm"], msg=c.name, **XR.TOL_GN)
    XR.check_params(rec["p"], XR.Adam(D.p_on.size, lr=XR.LRATE).step(p_prev, rec["g"]))
    for graph, what in ((0, "use_graph 0 vs 1"), (1, "two identical runs")):
        h2 = rec_engine(pkg, c, D, graph=graph); r2 = rec_record(h2, idx, start); h2.close()
        assert (rec["loss"], rec["gn"]) == (r2["loss"], r2["gn"]), what
        np.testing.assert_array_equal(rec["g"], r2["g"], err_msg=what); np.testing.assert_array_equal(rec["p"], r2["p"], err_msg=what)
    assert_launches(h, net)
    h.close()


def _env_net():
    return nn.Chain(nn.Conv(3, 4, 8), XR.A(XR.GELU), nn.flattenbatch, nn.Dense(72, 16), XR.A(XR.AR.RELU), nn.Dense(16, 4))


def test_device_loop_acts_on_the_fp64_argmax_and_evaluate_leaves_the_parameters(pkg, mods):
    """TestMDP((5, 5), 4, 6), 8 copies: 12 vector steps at eps = 0; every action is the fp64 argmax where the gap is at least GAP; the acting program takes the general
    tail (fused_tail = 0) and runs the same forward launch"""
    net = _env_net()
    h, p, spec = G._env_engine(pkg, mods, net)
    h.envs_create(spec, max_episode_length=100, seed=17)
    checked = 0
    for t in range(12):
        obs = h.envs_peek()[0].copy()
        h.rollout(1, t0=t + 1, train_freq=0, target_update_freq=0, eps=(0.0, 0.0, 1.0))
        a = h.envs_peek()[1]
        q = XR.q_values(net, p, obs.reshape(-1, 4, 5, 5)); top = np.sort(q, axis=1)
        clear = top[:, -1] - top[:, -2] >= XR.GAP
        np.testing.assert_array_equal(a[clear], q.argmax(1)[clear], err_msg=f"step {t}")
        checked += int(clear.sum())
    assert checked >= 0.9 * 12 * 8, checked
    assert h.envs_info() == (8, False)
    before = h.get_params(0)
    r, st = h.evaluate(8, 50, seed=5)
    assert np.isfinite(r) and np.isfinite(st) and st > 0
    np.testing.assert_array_equal(h.get_params(0), before); np.testing.assert_array_equal(h.get_params(1), before)
    h.close()


def test_solver_round_trip(pkg, mods, tmp_path, monkeypatch):
    """solve with a logdir (save_model at save_freq), then restore_best_model: bit-identical parameters; qnetwork.bson holds exactly the Conv and Dense arrays"""
    G.solver_round_trip(pkg, mods, tmp_path, monkeypatch, _env_net(), [(3, 3, 4, 8), (8,), (16, 72), (16,), (4, 16), (4,)])


def test_replicas_are_refused(pkg, monkeypatch):
    c = XR.BY_NAME["vec_gelu"]; D = XR.prepare(c)
    h = ff_engine(pkg, c, D)
    with pytest.raises(abi.DQNError, match=r"dqn_comm_init: layer 1 is an Activation layer; data-parallel replicas of a network with Activation layers are not supported \(single GPU only\)"):
        h.comm_init(bytes(128), 0, 1)
    h.train_step(D.idx[0])      # the engine is left as it was
    h.close()
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    with pytest.raises(abi.DQNError, match=r"DQN_SIM_WORLD: layer 1 is an Activation layer; .*\(single GPU only\)"):
        ff_engine(pkg, c, D)


def test_the_fixture_holds_the_paths_it_was_recorded_for():
    assert set(GOLD) == set(KT.CASES)
    for k, acts in (("act_vec", (2,)), ("act_map_prio_u8", (1,)), ("act_all_maps", (1, 3, 5, 9)), ("act_dueling_b128", (2,)), ("act_lstm", (1, 3))):
        toks = [t for n in GOLD[k]["step"] for t in n.split("+")]
        assert not set(FUSED) & set(toks), k
        for i in acts:
            assert {f"fwd_on_act{i}", f"fwd_tg_act{i}", f"bwd_act{i}"} <= set(toks), (k, i)
    toks = GOLD["act_behind_first_pool"]["step"]      # nothing computes a gradient nobody reads
    assert "fwd_on_act1" in toks and not [t for t in toks if t in ("bwd_act1", "bwd_pool0")]
    assert GOLD["acting_act"]["fused_tail"] is False
    assert GOLD["refuse_act"]["comm_init"].startswith("dqn_comm_init: layer 1 is an Activation layer") and GOLD["refuse_act"]["sim_world"].startswith("DQN_SIM_WORLD: layer 1 is an Activation layer")
    assert GOLD["refuse_act1_gn3"]["comm_init"].startswith("dqn_comm_init: layer 3 is a GroupNorm layer")      # the existing kinds keep their place in the order


@pytest.mark.parametrize("name", sorted(KT.CASES))
def test_the_program_is_the_recorded_program(name):
    assert KT.observe(name) == GOLD[name]


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (docs/history/activation_layer.md records them)"""
    print("\nWORST error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("WORST gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(R.WORST.items())})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
