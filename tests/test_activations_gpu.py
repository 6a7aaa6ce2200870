"""GPU: train steps, policy forward, the device loop and a short solve of networks that carry leakyrelu, elu, selu, softplus, softsign, relu6 or hardtanh on their Dense, Conv
and LayerNorm layers (csrc/common.h act_slow / dact_slow, csrc/red_head.hip), all through the C ABI, against the two-legged fp64 reference of activation_reference.py.

Every activation runs through every epilogue family of its table at the smallest shape that reaches it (the shapes of feedforward_edges_common.BOUNDARY; the launch class is
asserted with its facts() / launches()): three train steps under the per-step checks of the feed-forward edge tests (Q on s and s', target Q, greedy indices exactly under
GAP, y, td, loss, per-block gradients, grad_norm, parameters after fp64 Adam; the project's constants, unchanged), then use_graph 0 against 1, bit for bit, and use_mfma 0
against 1 where the plan is the same.  The C twin does not know the seven codes: parity rests on the fp64 reference plus these bit-for-bit companions.

Before the feature every engine of this file computed the identity in place of the activation (no kernel knew the codes, nothing refused them): every case fails its first
Q comparison on the parent commit.

One MI355X, one run: docs/history/activations.md has the worst error / tolerance per quantity and per gradient block kind."""
import importlib
import os
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import activation_reference as AR
import feedforward_edges_common as E
import recurrent_reference as R
from drqn_common import feed

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()
nn = AR.nn


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


@pytest.fixture(scope="module")
def mods(pkg):
    return tuple(importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "envs", "solver", "bson"))


def _obs3(obs):
    return tuple(obs) + (1,) * (3 - len(obs))


def ff_engine(pkg, c, D, graph=1, mfma=None, env=None, plan=None):
    layers, dueling = nn.lower(D.net); o = _obs3(c.obs)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=o[0], obs_h=o[1], obs_w=o[2], dueling=int(dueling), buffer_size=c.B + 24, learning_rate=AR.LRATE, gamma=c.gamma,
                             double_q=c.dq, prioritized_replay=c.prio, obs_dtype=c.u8, use_mfma=c.mfma if mfma is None else mfma, use_graph=graph, seed=5)
    if env:
        os.environ[env] = "1"      # the engine reads its switches once, at creation
    try:
        h = pkg.Engine(layers, hp, plan=plan)
    finally:
        if env:
            os.environ.pop(env, None)
    h.replay_add(D.s, D.a, D.r, D.sp, D.d); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def ff_record(h, idx):
    loss, gn, td = h.train_step(idx)
    return dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities())


def run_checked(pkg, c, D):
    """STEPS train steps on the case's indices, each against the reference at the engine's own previous parameters and batch.  -> the open handle, the per-step record"""
    h = ff_engine(pkg, c, D); adam = AR.Adam(D.p_on.size, lr=AR.LRATE); gamma = float(np.float32(c.gamma)); rec = []
    for k in range(AR.STEPS):
        msg = f"{c.name} step {k}"; idx = D.idx[k]
        p_prev = h.get_params(0); batch = h.get_batch(idx)
        masks = AR.masks_of(D.net, k, c.B)
        o = AR.ff_step(D.net, p_prev, D.p_tg, batch, gamma, bool(c.dq), masks)
        m, occ, sg = AR.rules(D.net, p_prev, batch[0], masks)
        assert m > AR.RELU_MARGIN and occ >= AR.OCCUPANCY and sg >= AR.LR.SIGMA_MIN, (msg, m, occ, sg)
        r = ff_record(h, idx); q = r["q"]
        E._close("q_on_s", q["q_on_s"], o["q_on_s"], msg=msg, **AR.TOL_Q)
        E._close("q_tg_sp", q["q_tg_sp"], o["q_tg_sp"], msg=msg, **AR.TOL_Q)
        if c.dq:
            E._close("q_on_sp", q["q_on_sp"], o["q_on_sp"], msg=msg, **AR.TOL_Q)
        assert AR.LR._gap(o["q_on_sp"] if c.dq else o["q_tg_sp"]) > AR.GAP, msg
        np.testing.assert_array_equal(q["best_a"], o["best_a"], err_msg=msg)
        E._close("y", q["y"], o["y"], msg=msg, **AR.TOL_TD)
        E._close("td", r["td"], o["td"], msg=msg, **AR.TOL_TD)
        E._close("loss", r["loss"], o["loss"], msg=msg, **AR.TOL_LOSS)
        AR.check_grads(D.net, r["g"], o["grads"], live=k == 0)
        E._close("grad_norm", r["gn"], o["grad_norm"], msg=msg, **AR.TOL_GN)
        AR.check_params(r["p"], adam.step(p_prev, r["g"]))
        rec.append(r)
    return h, rec


def replay(pkg, c, D, **kw):
    h = ff_engine(pkg, c, D, **kw)
    rec = [ff_record(h, D.idx[k]) for k in range(AR.STEPS)]
    return h, rec


# the families whose networks feedforward_edges_common's vocabulary describes: (layer sizes, output-layer activation is the case's, the facts the family was written for)
MLP = {"lds": ((32, 32, 32, 4), False, {"fwd0": "lds", "dw0": "lds", "fwd1": "lds", "dx1": "lds", "dxmode1": 3, "head": "head_cols4"}),      # dX: one wave per (source, chunk)
       "dx_wide": ((32, 32, 32, 4), False, {"fwd0": "lds", "dx1": "lds", "dxmode1": 2, "dxred1": False}),      # dX: 32 features x 128 samples per workgroup
       "valu": ((33, 32, 32, 4), False, {"fwd0": "valu", "dw0": "valu", "dx1": "valu", "head": "head_td"}),
       "mfma_u8": ((36, 32, 32, 4), False, {"fwd0": "mfma", "arena": False}),
       "split_k": ((1028, 32, 32, 4), False, {"fwd0": "mfma", "fwdS0": 3, "head": "head_cols4"}),
       "red_head": ((1028, 32, 4), False, {"fwd0": "mfma", "fwdS0": 3, "head": "red_head"}),
       "head_cols4": ((64, 128, 4), False, {"fwdS1": 4, "head": "head_cols4", "dxkc0": 32}),
       "head_td": ((64, 127, 4), False, {"fwdS1": 1, "head": "head_td"}),
       "tiny": ((12, 24, 20, 4), False, {"tiny": True}),
       "dueling": ((12, 24, 20, 4), False, {"head": "head_td", "fwd1": "valu", "fwd4": "valu"}),
       "hact": ((64, 128, 4), True, {"head": "head_cols4"}),
       "hact_dueling": ((6, 16, 4), True, {"head": "head_td"})}


def family_facts(c):
    """the launch classes of the case's network by the restated selection rules (feedforward_edges_common.facts on the same sizes, options and default plan)"""
    dims, hact, want = MLP[c.family]
    acts = [AR.TANH if hact else c.act] * (len(dims) - 2) + [c.act if hact else AR.I]
    ec = E.case(c.name, dims[0], E.mlp(*dims, acts=acts), c.B, dueling=c.dueling, u8=c.u8, prio=c.prio, dq=c.dq, gamma=c.gamma)
    f = E.case_facts(ec)
    for k, v in want.items():
        assert f.get(k) == v, f"{c.name}: written for {k} = {v!r}, the rules give {f.get(k)!r}"
    return f


# conv: the padded Conv's own launch, the pool behind it (its backward applies the Conv's derivative), the VALU conv behind the pool; ln_do: the LayerNorm (its lambda) and the
# Dropout behind it (its backward applies the LayerNorm's derivative)
OTHER = {"conv": {"fwd_on_conv0", "fwd_on_pool1", "bwd_pool1", "fwd_valu_conv2", "bwd_valu_conv2", "dw_conv0", "head_td"},
         "ln_do": {"fwd_valu_dense0", "fwd_on_ln1", "fwd_tg_ln1", "bwd_ln1", "fwd_on_do2", "bwd_do2", "head_td"}}


@pytest.mark.parametrize("c", AR.CASES, ids=IDS(AR.CASES))
def test_three_steps_vs_fp64_reference_and_the_schedules_agree(pkg, c):
    D = AR.data(c)
    h, rec = run_checked(pkg, c, D)
    h0, rec0 = replay(pkg, c, D, graph=0)
    E.same_bits(rec, rec0, f"{c.name}: use_graph 0 vs 1"); h0.close()
    tokens = {t for n, _ in h.profile_step(max_entries=512) for t in n.split("+")}
    if c.family in MLP:
        f = family_facts(c)
        must, never = E.launches(f)
        assert must <= tokens and not (never & tokens), (c.name, "missing", sorted(must - tokens), "unexpected", sorted(never & tokens), "launched", sorted(tokens))
        if f["tiny"]:      # the single-launch step against its multi-launch twin schedule
            h2, rec2 = replay(pkg, c, D, env="DQN_NO_TINY")
            assert "tiny_step" not in {t for n, _ in h2.profile_step(max_entries=512) for t in n.split("+")}
            E.same_bits(rec, rec2, f"{c.name}: DQN_NO_TINY"); h2.close()
        elif c.family in ("lds", "dx_wide", "mfma_u8", "split_k", "red_head", "head_cols4", "hact"):      # use_mfma 0: the VALU kernels on the same plan, i.e. the same summation order
            h2, rec2 = replay(pkg, c, D, mfma=0, plan=h.plan())
            E.same_bits(rec, rec2, f"{c.name}: use_mfma 0 vs 1"); h2.close()
    else:      # the layer kinds the restated rules do not describe: the launches that carry the activation, by name
        assert OTHER[c.family] <= tokens and "tiny_step" not in tokens, (c.name, sorted(OTHER[c.family] - tokens), sorted(tokens))
    h.close()


def rec_engine(pkg, c, D, graph=1):
    layers, dueling = nn.lower(D.net)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=c.obs[0], dueling=int(dueling), buffer_size=D.cap, recurrence=1, trace_length=c.T, learning_rate=AR.LRATE,
                             prioritized_replay=0, use_mfma=c.mfma, use_graph=graph, seed=5, gamma=c.gamma, double_q=c.dq)
    h = pkg.Engine(layers, hp)
    feed(h, D.eps); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


@pytest.mark.parametrize("c", AR.REC_CASES, ids=IDS(AR.REC_CASES))
def test_recurrent_three_steps_vs_fp64_reference(pkg, c):
    """LSTM(6, 8) -> Dense(8, 12, act) -> Dense(12, 3), T = 3, B = 4: the Dense layers of a recurrent network.  A recurrent train step reports its loss, grad_norm, gradients
    and parameters only (dqn_get_last_q and the td output describe the feed-forward step), so Q, y and td of the step cannot be compared here; the loss, which sums every
    column's Huber term of td = Q - y, is held to TOL_LOSS.  Q itself is compared on the acting path: dqn_forward over the T observations of the first draw from the reset state"""
    D = AR.data(c); h, h0 = rec_engine(pkg, c, D, 1), rec_engine(pkg, c, D, 0); adam = AR.Adam(D.p_on.size, lr=AR.LRATE)
    idx, start = D.draws[0]; x = R.sample_batch(D.ring, idx, start, c.T, c.obs)[3]
    h.reset_state()
    for t, q64 in enumerate(AR.q_values(D.net, D.p_on, x)):
        E._close("policy_q", h.forward(x[t]), q64, msg=f"{c.name} t={t}", **AR.TOL_Q)
    h.reset_state()
    for k, (idx, start) in enumerate(D.draws[:AR.STEPS]):
        msg = f"{c.name} step {k}"
        p_prev = h.get_params(0)
        batch = h.episode_get_batch(idx, start)
        want = R.sample_batch(D.ring, idx, start, c.T, c.obs)
        for got, w in zip(batch, want):
            np.testing.assert_array_equal(np.asarray(got).reshape(w.shape), w)
        m, occ, _ = AR.rules(D.net, p_prev, want[0], None, want[5])
        assert m > AR.RELU_MARGIN and occ >= AR.OCCUPANCY, (msg, m, occ)
        o = AR.rec_step(D.net, p_prev, D.p_tg, want, float(np.float32(c.gamma)), bool(c.dq))
        loss, gn = h.train_step_drqn(idx, start); g = h.get_grads()
        E._close("loss", loss, o["loss"], msg=msg, **AR.TOL_LOSS)
        AR.check_grads(D.net, g, o["grads"], live=k == 0)
        E._close("grad_norm", gn, o["grad_norm"], msg=msg, **AR.TOL_GN)
        AR.check_params(h.get_params(0), adam.step(p_prev, g))
        assert h0.train_step_drqn(idx, start) == (loss, gn), f"{msg}: use_graph 0 vs 1"
        np.testing.assert_array_equal(h0.get_grads(), g); np.testing.assert_array_equal(h0.get_params(0), h.get_params(0))
    h.close(); h0.close()


@pytest.mark.parametrize("fam", ["lds", "conv"])
@pytest.mark.parametrize("a", AR.NEW, ids=[AR.NAMES[a] for a in AR.NEW])
def test_forward_at_1_and_7_columns(pkg, fam, a):
    """dqn_forward on 1 and 7 observations (the acting program's epilogues at odd column counts): within TOL_Q of fp64"""
    c = AR.BY_NAME[f"{fam}_{AR.NAMES[a]}"]; D = AR.data(c); h = ff_engine(pkg, c, D)
    for n in (1, 7):
        x = D.s[D.idx[0][:n]]
        E._close("policy_q", h.forward(x), AR.q_values(D.net, D.p_on, x), msg=f"{c.name} n={n}", **AR.TOL_Q)
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


@pytest.mark.parametrize("a", AR.NEW, ids=[AR.NAMES[a] for a in AR.NEW])
def test_device_rollout_walks_one_trajectory_on_both_acting_tails(pkg, mods, a):
    """32 copies of TestMDP((5, 5), 1, 6), Dense(25, 32, act) -> Dense(32, 4): 16 vector steps that explore, act greedily and train, under the fused acting tail
    (act_head.hip) and under DQN_NO_ACT_HEAD -- observations, actions, rewards, terminals after every step and the parameters at the end, bit for bit"""
    envs = mods[1]; net = nn.Chain(nn.Dense(25, 32, a), nn.Dense(32, 4))
    p = nn.glorot_params(net, seed=2); p = (3.0 * p + 0.1 * np.random.default_rng(2).standard_normal(p.size)).astype(np.float32)
    g, t = _rollout_engine(pkg, envs, net, p), _rollout_engine(pkg, envs, net, p, env="DQN_NO_ACT_HEAD")
    assert g.envs_info() == (32, True) and t.envs_info() == (32, False), "the schedules under test are not the ones this test names"
    acted = set()
    for k in range(16):
        for h in (g, t):
            h.rollout(1, t0=k + 1, train_freq=2, target_update_freq=8, eps=(0.5, 0.1, 16.0))
        for x, y, what in zip(g.envs_peek(), t.envs_peek(), ("observations", "actions", "rewards", "terminals")):
            np.testing.assert_array_equal(x, y, err_msg=f"step {k}: {what}")
        acted |= set(np.asarray(g.envs_peek()[1]).tolist())
    assert len(acted) > 1
    np.testing.assert_array_equal(g.get_params(0), t.get_params(0))
    assert np.abs(g.get_params(0) - p).max() > 0
    g.close(); t.close()


def test_a_short_solve_finishes_and_the_saved_model_gives_the_same_forward_bits(pkg, mods, tmp_path):
    """Dense(100, 8, elu) -> Dense(8, 4) on TestMDP((5, 5), 4, 6) with device_envs: 300 steps finish with finite parameters; restore_best_model after save_model puts back
    the parameters whose dqn_forward bits are those of the saved model.  The evaluation return is printed (docs/history/activations.md), not asserted"""
    nn_, envs, S, bson = mods
    env = envs.TestMDP((5, 5), 4, 6, n=8, seed=7)
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.05, steps=200), rng=np.random.default_rng(1))
    solver = S.DeepQLearningSolver(qnetwork=nn.Chain(nn.Dense(100, 8, nn.elu), nn.Dense(8, 4)), max_steps=300, learning_rate=0.005, exploration_policy=expl, eval_freq=100,
                                   save_freq=100, num_ep_eval=10, log_freq=100, double_q=True, dueling=False, prioritized_replay=True, train_start=64, verbose=False,
                                   logdir=str(tmp_path / "log"), device_envs=True)
    policy = S.solve(solver, env); h = policy.engine
    assert np.isfinite(h.get_params(pkg.NET_ONLINE)).all()
    path = tmp_path / "log" / "qnetwork.bson"
    assert path.exists(), "no model was saved"
    w, sizes = bson.load_qnetwork(path)
    assert [tuple(x) for x in sizes] == [(8, 100), (8,), (4, 8), (4,)]
    obs = np.random.default_rng(3).random((7, 4, 5, 5), dtype=np.float32)
    h.set_params(w, pkg.NET_ONLINE); q_saved = h.forward(obs)
    h.set_params(w * np.float32(0.5), pkg.NET_ONLINE)
    assert np.abs(h.forward(obs) - q_saved).max() > 0
    S.restore_best_model(solver, policy)
    np.testing.assert_array_equal(h.forward(obs), q_saved)
    np.testing.assert_array_equal(h.get_params(pkg.NET_ONLINE), w)
    r, st = h.evaluate(8, 50, seed=5)
    assert np.isfinite(r) and np.isfinite(st)
    print(f"\nshort solve, Dense(100, 8, elu) -> Dense(8, 4): evaluation return {r:.4f} over {st:.1f} steps")
    h.close()


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (docs/history/activations.md records them)"""
    print("\nWORST error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("WORST gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(R.WORST.items())})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
