"""GPU: train steps, policy forward, device loop, checkpoint, solver round trip and refusals of networks with a dilated, grouped or depthwise convolution (layer kind 15,
csrc/conv_own.hip), all through the C ABI, against the two-legged fp64 reference of conv_dg_reference.py.  Every case of its table runs STEPS train steps on given indices
under the per-step checks of the feed-forward edge tests (Q on s and s', target Q, greedy indices exactly, y, td, loss, per-block gradients, grad_norm, parameters after fp64
Adam, priorities; tolerances are the project's existing constants, unchanged; the margins are asserted on every step), then use_graph 0 against 1, use_mfma 0 against 1 and a
second identical run, bit for bit, and the launch names.

Exact companions, engine against engine, first step, bit for bit: the kind-15 network against the kind-1 network whose conv holds the zero-stuffed, block-diagonal kernel,
both under an unsplit plan entry for that layer -- Q on s / s', target Q, greedy indices, y, td, loss, the gradients of every other layer, the layer's own dW at the live taps
and its db.  And Conv(dilation = 1, groups = 1) forced through kind 15 against the padded and the pad-0 Conv, every step.  The law makes these identities, not tolerances.

Without the feature every test here fails: nn.Conv(..., dilation=2) is a TypeError and the engine answers "unknown kind 15".

One MI355X, one run: docs/history/conv_dilation_groups.md records the worst error / tolerance per quantity and per gradient block kind."""
import importlib
import json
import os
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import conv_dg_reference as XR
import conv_dg_traits_cases as KT
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
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dg_traits_gpu.json")))


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "envs", "solver", "bson"))


def hparams(pkg, c, dueling, graph=1, mfma=None):
    return pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=c.obs[0], obs_h=c.obs[1], obs_w=c.obs[2], dueling=int(dueling), buffer_size=c.B + 24, learning_rate=XR.LRATE,
                               gamma=c.gamma, double_q=c.dq, prioritized_replay=c.prio, obs_dtype=c.u8, use_mfma=c.mfma if mfma is None else mfma, use_graph=graph, seed=5)


def ff_engine(pkg, c, D, graph=1, mfma=None, net=None, layers=None, plan=None, p_on=None, p_tg=None):
    net = net or D.net
    lay, dueling = nn.lower(net)
    h = pkg.Engine(layers or lay, hparams(pkg, c, dueling, graph, mfma), plan=plan)
    h.replay_add(D.s, D.a, D.r, D.sp, D.d); h.set_params(D.p_on if p_on is None else p_on, 0); h.set_params(D.p_tg if p_tg is None else p_tg, 1)
    return h


def ff_record(h, idx):
    loss, gn, td = h.train_step(idx)
    return dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities())


def replay(pkg, c, D, steps=XR.STEPS, **kw):
    h = ff_engine(pkg, c, D, **kw)
    return h, [ff_record(h, D.idx[k]) for k in range(steps)]


def assert_launches(h, net):
    """one forward launch per network pass, one dW launch, and one dX launch unless the layer reads the observation"""
    names = [n for n, _ in h.profile_step(max_entries=512)]
    tokens = [t for n in names for t in n.split("+")]
    gen = XR.general_descs(net)
    assert gen
    for i in gen:
        assert tokens.count(f"fwd_on_cdg{i}") == 1 and tokens.count(f"fwd_tg_cdg{i}") == 1 and tokens.count(f"dw_cdg{i}") == 1 and tokens.count(f"bwd_cdg{i}") == (1 if i > 0 else 0), (i, names)
    return names


@pytest.mark.parametrize("c", XR.CASES, ids=IDS(XR.CASES))
def test_steps_vs_fp64_reference_graph_eager_mfma_valu_and_rerun(pkg, c):
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
        if k == 0:
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
    # eager against graph, the VALU forms against the MFMA forms, and a second identical run: one result whatever the launch mode, the kernel form or the timing
    for kw, what in ((dict(graph=0), "use_graph 0 vs 1"), (dict(mfma=0), "use_mfma 0 vs 1"), (dict(), "two identical runs")):
        h2, rec2 = replay(pkg, c, D, **kw)
        E.same_bits(rec, rec2, f"{c.name}: {what}"); h2.close()
    names = assert_launches(h, net)
    assert ("head_td" in names) or ("td_huber" in names), names
    h.close()


def unsplit_plan(h, net):
    """the engine's plan with an unsplit entry for every kind-15 layer"""
    gen = set(XR.general_descs(net))
    return [(0, 0, 0) if i in gen else p for i, p in enumerate(h.plan())]


@pytest.mark.parametrize("c", XR.CASES, ids=IDS(XR.CASES))
def test_exact_companion_the_zero_stuffed_block_diagonal_kernel_bit_for_bit(pkg, c):
    """kind 15 against kind 1 on the expanded kernel, both under an unsplit plan entry for that layer, first step: a skipped term and a term multiplied by an exact zero give
    the same bits"""
    D = XR.prepare(c); net = D.net; ex = XR.expand(net)
    h0 = ff_engine(pkg, c, D); plan = unsplit_plan(h0, net); h0.close()
    h, (a,) = replay(pkg, c, D, steps=1, plan=plan)
    assert h.plan() == plan
    hx, (b,) = replay(pkg, c, D, steps=1, net=ex, plan=plan, p_on=XR.expand_params(net, D.p_on), p_tg=XR.expand_params(net, D.p_tg))
    assert hx.plan() == plan and all(d.kind != abi.LAYER_CONV_DG for d in nn.lower(ex)[0])
    what = f"{c.name}: kind 15 vs kind 1 on the expanded kernel"
    assert a["loss"] == b["loss"], (what, a["loss"], b["loss"])
    np.testing.assert_array_equal(a["td"], b["td"], err_msg=what)
    for key in ("q_on_s", "q_on_sp", "q_tg_sp", "best_a", "y"):
        np.testing.assert_array_equal(a["q"][key], b["q"][key], err_msg=f"{what}: {key}")
    np.testing.assert_array_equal(a["g"], XR.contract_grads(net, b["g"]), err_msg=f"{what}: gradients (the layer's dW at the live taps, its db, every other layer)")
    assert np.isfinite(a["g"]).all() and all(np.abs(a["g"][sl]).max() > 0 for _, sl in XR.blocks(net))
    assert_launches(h, net)
    assert not [n for n, _ in hx.profile_step(max_entries=512) if "cdg" in n]
    h.close(); hx.close()


FORCED = [XR.case("forced_pad1", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu, pad=1), nn.Dense(144, 4)), 16, (1, 6, 6)),
          XR.case("forced_pad0_b5", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.Dense(64, 4)), 5, (1, 6, 6)),
          XR.case("forced_mfma", lambda: nn.Chain(nn.Conv(3, 1, 16, nn.tanh), nn.Conv(3, 16, 16, nn.relu), nn.Conv(3, 16, 32, nn.tanh, stride=2, pad=1), nn.Dense(128, 4)), 32, (1, 8, 8)),
          XR.case("forced_u8_dueling", lambda: nn.create_dueling_network(nn.Chain(nn.Conv(3, 4, 16, nn.relu, pad=1), nn.Dense(576, 16, nn.relu), nn.Dense(16, 4))), 32, (4, 6, 6), dueling=True, u8=1)]


@pytest.mark.parametrize("c", FORCED, ids=IDS(FORCED))
def test_dilation_1_groups_1_forced_through_kind_15_gives_the_convs_bits(pkg, c):
    """every Conv of the network lowered as kind 15 with dh = dw = g = 1 (a C caller may; the mirror never does) against the padded / pad-0 Conv, same plan, every step"""
    D = XR.ff_data(c)
    hk, rec1 = replay(pkg, c, D)
    plan = hk.plan(); hk.close()
    layers = nn.lower(D.net)[0]
    for d in layers:
        if d.kind == abi.LAYER_CONV:
            d.kind, d.n_in, d.n_out = abi.LAYER_CONV_DG, d.n_in | (d.n_out << 16), 1 | (1 << 8) | (1 << 16)
    h, rec15 = replay(pkg, c, D, layers=layers, plan=plan)
    assert h.plan() == plan and [n for n, _ in h.profile_step(max_entries=512) if "cdg" in n]
    E.same_bits(rec15, rec1, f"{c.name}: Conv(d = 1, g = 1) through kind 15 vs kind 1")
    assert all(np.isfinite(r["g"]).all() and np.abs(r["g"]).max() > 0 for r in rec15)
    h.close()


@pytest.mark.parametrize("name", ["dil2_b5", "rect_aniso", "groups2_4to6", "dw_4to8_pad_b32", "mfma_groups2", "mfma_dil2", "u8_dil2", "separable_gn", "skip_entry", "dueling"])
def test_forward_at_1_and_7_columns(pkg, name):
    """dqn_forward on 1 and 7 observations (the one-column walk): within TOL_Q of fp64, and the bits the train step's Q has on the same rows"""
    c = XR.BY_NAME[name]; D = XR.prepare(c); h = ff_engine(pkg, c, D); idx = D.idx[0]
    f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
    fw = {n: h.forward(f(D.s[idx[:n]])) for n in (1, 7) if n <= c.B}
    for n, q in fw.items():
        E._close("policy_q", q, XR.q_values(D.net, D.p_on, f(D.s[idx[:n]])), msg=f"{name} n={n}", **XR.TOL_Q)
    h.train_step(idx)
    q_on_s = h.last_q()["q_on_s"]
    for n, q in fw.items():
        np.testing.assert_array_equal(q, q_on_s[:n], err_msg=f"{name} n={n}")
    h.close()


def rec_engine(pkg, c, D, graph=1, mfma=1):
    layers, dueling = nn.lower(D.net)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=c.obs[0], obs_h=c.obs[1], obs_w=c.obs[2], dueling=int(dueling), buffer_size=D.cap, recurrence=1, trace_length=c.T,
                             learning_rate=XR.LRATE, prioritized_replay=0, use_mfma=mfma, use_graph=graph, seed=5, gamma=c.gamma, double_q=c.dq)
    h = pkg.Engine(layers, hp)
    feed(h, D.eps); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def rec_record(h, idx, start):
    loss, gn = h.train_step_drqn(idx, start)
    return dict(loss=loss, gn=gn, g=h.get_grads(), p=h.get_params(0))


@pytest.mark.parametrize("c", XR.REC_CASES, ids=IDS(XR.REC_CASES))
def test_recurrent_step_vs_fp64_reference(pkg, c):
    """T = 3, B = 4: the layer runs once over the T * B = 12 columns, in front of the LSTM"""
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
    for kw, what in ((dict(graph=0), "use_graph 0 vs 1"), (dict(mfma=0), "use_mfma 0 vs 1"), (dict(), "two identical runs")):
        h2 = rec_engine(pkg, c, D, **kw); r2 = rec_record(h2, idx, start); h2.close()
        assert (rec["loss"], rec["gn"]) == (r2["loss"], r2["gn"]), what
        np.testing.assert_array_equal(rec["g"], r2["g"], err_msg=what); np.testing.assert_array_equal(rec["p"], r2["p"], err_msg=what)
    tokens = [t for n, _ in h.profile_step(max_entries=512) for t in n.split("+")]
    assert tokens.count("dw_cdg0") == 1 and "bwd_cdg0" not in tokens and [t for t in tokens if t.endswith("_cdg0") and t not in ("dw_cdg0",)], tokens
    h.close()


def _env_net():
    return nn.Chain(nn.DepthwiseConv(3, 4, 8, nn.relu, pad=1), nn.Conv(3, 8, 8, nn.relu, dilation=2, groups=2), nn.flattenbatch, nn.Dense(8, 16, nn.relu), nn.Dense(16, 4))


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
    """solve with a logdir (save_model at save_freq), then restore_best_model: bit-identical parameters; qnetwork.bson holds the arrays in Julia's shapes, (kw, kh, cin ÷ g, cout)"""
    G.solver_round_trip(pkg, mods, tmp_path, monkeypatch, _env_net(), [(3, 3, 1, 8), (8,), (3, 3, 4, 8), (8,), (16, 8), (16,), (4, 16), (4,)])


@pytest.mark.parametrize("name", ["dw_4to8_pad_b32", "mfma_groups2"])
def test_checkpoint_resume_gives_the_same_bits(pkg, name):
    """four sampled steps straight against two, a checkpoint restored into a FRESH engine, and two more"""
    c = XR.BY_NAME[name]; D = XR.prepare(c)
    a = ff_engine(pkg, c, D)
    for _ in range(4):
        la = a.train_step(want_td=False)
    b = ff_engine(pkg, c, D)
    for _ in range(2):
        b.train_step(want_td=False)
    ck = b.checkpoint(); b.close()
    b2 = ff_engine(pkg, c, D); b2.restore(ck)
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
    a.close(); b2.close()


def test_refusals_through_the_engine(pkg, monkeypatch):
    c = XR.BY_NAME["groups2_4to6"]; D = XR.prepare(c)
    h = ff_engine(pkg, c, D)
    assert h.P == D.p_on.size == 6 * 2 * 3 * 3 + 6 + 96 * 4 + 4      # dqn_n_params: (cout, cin/g, kh, kw) + (cout,), then the Dense
    with pytest.raises(abi.DQNError, match=r"dqn_comm_init: layer 0 is a Conv with dilation / groups; data-parallel replicas of a network with dilated / grouped convolutions are not supported \(single GPU only\)"):
        h.comm_init(bytes(128), 0, 1)
    h.train_step(D.idx[0])      # the engine is left as it was
    h.close()
    layers = nn.lower(D.net)[0]; layers[0].n_out = 1 | (1 << 8) | (3 << 16)
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv groups = 3 must be >= 1 and divide cin = 4 and cout = 6"):
        pkg.Engine(layers, hparams(pkg, c, False))
    layers = nn.lower(D.net)[0]; layers[0].n_out = 4 | (4 << 8) | (2 << 16)
    with pytest.raises(abi.DQNError, match=r"layer 0: Conv kernel \(3, 3\) with dilation \(4, 4\) spans \(9, 9\) and does not fit the 6x6 input map"):
        pkg.Engine(layers, hparams(pkg, c, False))
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    with pytest.raises(abi.DQNError, match=r"DQN_SIM_WORLD: layer 0 is a Conv with dilation / groups; .*\(single GPU only\)"):
        ff_engine(pkg, c, D)


def test_the_fixture_holds_the_paths_it_was_recorded_for():
    assert set(GOLD) == set(KT.CASES)
    toks = lambda k, key="step": [t for n in GOLD[k][key] for t in n.split("+")]
    t = toks("cdg_first_u8")
    assert {"fwd_on_cdg0", "fwd_tg_cdg0", "dw_cdg0"} <= set(t) and "bwd_cdg0" not in t
    t = toks("cdg_separable_gn")
    assert {"fwd_on_cdg0", "dw_cdg0", "fwd_on_cdg3", "fwd_tg_cdg3", "dw_cdg3", "bwd_cdg3", "bwd_gn2", "bwd_pool4"} <= set(t) and "bwd_cdg0" not in t
    t = toks("cdg_skip_entry")
    assert {"fwd_on_cdg0", "dw_cdg0"} <= set(t) and any(x.startswith("skip3") or x == "bwd_entry_skip3" for x in t), t
    assert {"fwd_on_cdg1", "fwd_tg_cdg1", "dw_cdg1", "bwd_cdg1"} <= set(toks("cdg_dueling_b128")) and {"dw_cdg1", "bwd_cdg1"} <= set(toks("cdg_dueling_b128", "steady"))
    assert "dw_cdg0" in toks("cdg_lstm") and "drqn_cols" not in toks("cdg_lstm")
    assert GOLD["acting_cdg"]["fused_tail"] is False
    assert GOLD["refuse_cdg"]["comm_init"].startswith("dqn_comm_init: layer 0 is a Conv with dilation / groups") and GOLD["refuse_cdg"]["sim_world"].startswith("DQN_SIM_WORLD: layer 0 is a Conv with dilation / groups")
    assert GOLD["refuse_cdg0_act1"]["comm_init"].startswith("dqn_comm_init: layer 1 is an Activation layer")      # the existing kinds keep their place in the order


@pytest.mark.parametrize("name", sorted(KT.CASES))
def test_the_program_is_the_recorded_program(name):
    assert KT.observe(name) == GOLD[name]


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (docs/history/conv_dilation_groups.md records them)"""
    print("\nWORST error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("WORST gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(R.WORST.items())})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
