"""GPU: seeded random compositions of EVERY layer kind (tests/composition_common.py: 64 feed-forward and 16 recurrent networks drawn from the module's own grammar),
held to the one fp64 step reference -- what test_fuzz_gpu.py does for Dense and unpadded Conv against the C twin, for the kinds the twin does not know.  The per-kind files
check each layer in a hand-chosen setting with at most one neighbour of another kind; here the kernels meet: which stored output a dX kernel differentiates, the map <->
vector layout at the flatten, the dueling join's summed dX arriving at a non-Dense layer, a skip block's entry behind a GroupNorm or an Activation, workspace reuse between
launches of different families, parameter-free plan entries between split sums, the fusions declining with a kind three layers in front.

Every feed-forward case runs STEPS train steps on given indices under the per-step checks of the per-kind files (batch rows exactly, IS weights, Q on s and s', target Q,
greedy indices exactly, y, td, loss, per-block gradients, grad_norm, parameters after fp64 Adam on the engine's own gradients, priorities; the margins of the union probe
asserted on every step, on the engine's own parameters; Dropout under the engine's own mask law), then use_graph 0 against 1, use_mfma 0 against 1 and a second identical
run, bit for bit.  Every recurrent case runs one train_step_drqn.  Tolerances are the project's existing constants, imported and unchanged.  The engine must ACCEPT every
case: the grammar is a restatement of the placement rules, so a refusal is a finding, not a skip.

One MI355X, one run: docs/history/composition_tests.md records the worst error / tolerance per quantity and per gradient block kind, the wall time and the slowest case."""
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import composition_common as C
import dqn_oracle as O
import feedforward_edges_common as E
import recurrent_reference as R
import step_reference as S
from drqn_common import feed

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()
nn = C.nn
SLOWEST = {}


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


def _obs3(obs):
    return tuple(obs) + (1,) * (3 - len(obs))


def hparams(pkg, c, dueling, graph=1, mfma=None):
    o = _obs3(c.obs)
    return pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=o[0], obs_h=o[1], obs_w=o[2], dueling=int(dueling), buffer_size=c.B + 24, learning_rate=C.LRATE, gamma=c.gamma,
                               double_q=c.dq, prioritized_replay=c.prio, obs_dtype=c.u8, use_mfma=c.mfma if mfma is None else mfma, use_graph=graph, seed=C.ENGINE_SEED)


def ff_engine(pkg, c, D, graph=1, mfma=None):
    layers, dueling = nn.lower(D.net)
    h = pkg.Engine(layers, hparams(pkg, c, dueling, graph, mfma))
    h.replay_add(D.s, D.a, D.r, D.sp, D.d); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def ff_record(h, idx):
    loss, gn, td = h.train_step(idx)
    return dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities())


def replay(pkg, c, D, **kw):
    h = ff_engine(pkg, c, D, **kw)
    rec = [ff_record(h, D.idx[k]) for k in range(C.STEPS)]
    h.close()
    return rec


@pytest.mark.parametrize("c", C.FF, ids=IDS(C.FF))
def test_steps_vs_fp64_reference_graph_eager_mfma_valu_and_rerun(pkg, c):
    t0 = time.time()
    D = C.prepare(c); net = D.net
    h = ff_engine(pkg, c, D, graph=1)      # the engine accepts what the grammar admits
    hp = hparams(pkg, c, isinstance(net, nn.DuelingNetwork))
    np.testing.assert_array_equal(h.get_params(0), D.p_on)
    rec = []; adam = C.Adam(D.p_on.size, lr=C.LRATE)      # fp64 Adam on the engine's own gradients
    for k in range(C.STEPS):
        idx = D.idx[k]; msg = f"{c.name} [{' '.join(c.tokens)}] step {k}"
        p_prev = h.get_params(0); pr_before = h.replay_priorities()
        assert h.get_counters()["train_steps"] == k      # the Dropout masks' key
        batch = h.get_batch(idx)
        want_batch = C.ff_batch(c, D, idx)
        for j, (a, b) in enumerate(zip(batch[:5], want_batch[:5])):
            np.testing.assert_array_equal(np.asarray(a, np.float64).reshape(np.shape(b)), np.asarray(b, np.float64), err_msg=f"{msg}: batch[{j}]")
        E._close("is_weights", batch[5], O.is_weights(pr_before[idx], pr_before, hp.prio_beta, np.float64), rtol=2e-6, msg=msg)      # (the buffer weights every batch; prioritized_replay gates update_priorities! only)
        batch = tuple(np.asarray(x).reshape(np.shape(w)) for x, w in zip(batch, want_batch))
        m = C.margins(c, net, p_prev, D.p_tg, batch, k)
        assert C.holds(m), (msg, m)
        o = C.step(c, net, p_prev, D.p_tg, batch, k)
        r = ff_record(h, idx); q = r["q"]; rec.append(r)
        print(f"\n{msg}: loss {r['loss']!r} (fp64 {o['loss']!r}), grad_norm {r['gn']!r} (fp64 {o['grad_norm']!r}), max |q - q64| {np.abs(q['q_on_s'] - o['q_on_s']).max():.3g}")
        E._close("q_on_s", q["q_on_s"], o["q_on_s"], msg=msg, **C.TOL_Q)
        E._close("q_tg_sp", q["q_tg_sp"], o["q_tg_sp"], msg=msg, **C.TOL_Q)
        E._close("q_on_sp", q["q_on_sp"], o["q_on_sp"], msg=msg, **C.TOL_Q)
        np.testing.assert_array_equal(q["best_a"], o["best_a"], err_msg=msg)
        E._close("y", q["y"], o["y"], msg=msg, **C.TOL_TD)
        E._close("td", r["td"], o["td"], msg=msg, **C.TOL_TD)
        E._close("loss", r["loss"], o["loss"], msg=msg, **C.TOL_LOSS)
        assert np.isfinite(r["g"]).all(), msg
        C.check_grads(net, r["g"], o["grads"], live=k == 0)
        E._close("grad_norm", r["gn"], o["grad_norm"], msg=msg, **C.TOL_GN)
        C.check_params(r["p"], adam.step(p_prev, r["g"]))
        E.check_priorities_after_step(h, hp, idx, pr_before, r["td"], o["td"], batch[5])
    h.close()
    # eager against graph, the VALU forms against the MFMA forms, and a second identical run: one result whatever the launch mode, the kernel form or the timing
    for kw, what in ((dict(graph=0), "use_graph 0 vs 1"), (dict(mfma=0), "use_mfma 0 vs 1"), (dict(), "two identical runs")):
        E.same_bits(rec, replay(pkg, c, D, **kw), f"{c.name}: {what}")
    SLOWEST[c.name] = time.time() - t0


@pytest.mark.parametrize("c", C.FF, ids=IDS(C.FF))
def test_policy_forward_at_1_and_7_observations(pkg, c):
    """dqn_forward on 1 and 7 observations (Dropout inactive): within TOL_Q of fp64; without a Dropout layer also the bits the train step's Q on s has on the same rows"""
    D = C.prepare(c); h = ff_engine(pkg, c, D); idx = D.idx[0]
    f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
    rows = np.concatenate([idx, idx])[:7]
    fw = {n: h.forward(f(D.s[rows[:n]])) for n in (1, 7)}
    for n, q in fw.items():
        E._close("policy_q", q, S.q_values(D.net, D.p_on, f(D.s[rows[:n]])), msg=f"{c.name} n={n}", **C.TOL_Q)
    if not C.has_dropout(D.net):
        h.train_step(idx)
        q_on_s = h.last_q()["q_on_s"]; q7 = np.concatenate([q_on_s, q_on_s])[:7]
        for n, q in fw.items():
            np.testing.assert_array_equal(q, q7[:n], err_msg=f"{c.name} n={n}")
    h.close()


def rec_engine(pkg, c, D, graph=1):
    layers, dueling = nn.lower(D.net); o = _obs3(c.obs)
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=o[0], obs_h=o[1], obs_w=o[2], dueling=int(dueling), buffer_size=D.cap, recurrence=1, trace_length=c.T,
                             learning_rate=C.LRATE, prioritized_replay=0, use_mfma=c.mfma, use_graph=graph, seed=C.ENGINE_SEED, gamma=c.gamma, double_q=c.dq)
    h = pkg.Engine(layers, hp)
    feed(h, D.eps); h.set_params(D.p_on, 0); h.set_params(D.p_tg, 1)
    return h


def rec_record(h, idx, start):
    loss, gn = h.train_step_drqn(idx, start)
    return dict(loss=loss, gn=gn, g=h.get_grads(), p=h.get_params(0))


@pytest.mark.parametrize("c", C.REC, ids=IDS(C.REC))
def test_recurrent_step_vs_fp64_reference_graph_eager_and_rerun(pkg, c):
    """one train_step_drqn on the case's draws against rec_step: loss, per-block gradients, grad_norm, parameters after fp64 Adam (the recurrent legs of the per-kind files)"""
    D = C.prepare(c); net = D.net; idx, start = D.draws[0]; msg = f"{c.name} [{' '.join(c.tokens)}]"
    h = rec_engine(pkg, c, D, graph=1)
    p_prev = h.get_params(0)
    batch = h.episode_get_batch(idx, start)
    want = R.sample_batch(D.ring, idx, start, c.T, c.obs)
    for got, w in zip(batch, want):
        np.testing.assert_array_equal(np.asarray(got).reshape(w.shape), w)
    batch = tuple(np.asarray(x).reshape(w.shape) for x, w in zip(batch, want))
    m = C.margins(c, net, p_prev, D.p_tg, batch)
    assert C.holds(m), (msg, m)
    o = C.step(c, net, p_prev, D.p_tg, batch)
    rec = rec_record(h, idx, start)
    np.testing.assert_allclose(rec["loss"], o["loss"], rtol=2e-5, atol=1e-7, err_msg=f"{msg}: loss")      # the recurrent tables' loss tolerance (test_recurrent_edges_gpu.run_checked)
    C.check_grads(net, rec["g"], o["grads"], live=True)
    E._close("grad_norm", rec["gn"], o["grad_norm"], msg=msg, **C.TOL_GN)
    C.check_params(rec["p"], C.Adam(D.p_on.size, lr=C.LRATE).step(p_prev, rec["g"]))
    h.close()
    for kw, what in ((dict(graph=0), "use_graph 0 vs 1"), (dict(), "two identical runs")):
        h2 = rec_engine(pkg, c, D, **kw); r2 = rec_record(h2, idx, start); h2.close()
        assert (rec["loss"], rec["gn"]) == (r2["loss"], r2["gn"]), (msg, what)
        np.testing.assert_array_equal(rec["g"], r2["g"], err_msg=f"{msg}: {what}"); np.testing.assert_array_equal(rec["p"], r2["p"], err_msg=f"{msg}: {what}")


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity, the slowest case and the wall time of this file (docs/history/composition_tests.md records them)"""
    print("\nWORST error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items())})
    print("WORST gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(R.WORST.items())})
    if SLOWEST:
        name = max(SLOWEST, key=SLOWEST.get)
        print(f"slowest feed-forward case: {name} {SLOWEST[name]:.2f} s")
    print(f"wall time of the file: {time.time() - T0:.0f} s")
