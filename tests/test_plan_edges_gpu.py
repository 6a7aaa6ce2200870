"""GPU (-m gpu): the plan table of tests/plan_edges_common.py on the HIP engine through the C ABI -- feed-forward train steps under caller-supplied summation
plans, against the fp64 reference of tests/feedforward_reference.py at the tolerances of feedforward_edges_common.run_checked (none widened).  Per case, three
train steps on given indices; then, the plan being the same and with it the summation order: the engine equals the C twin bit for bit, use_graph 0 equals 1,
use_mfma 0 equals 1; the launch names of profile_step show the kernel family the selection rules (feedforward_edges_common.facts, on the edited plan) give;
plan() returns the plan given; and, for the forward cases -- the acting programs read fwd_kc too -- forward() on 1, 5 and 16 columns stays within TOL_Q of the
fp64 Q values and greedy_action is the fp64 argmax wherever the fp64 top-two gap exceeds GAP.

Also here: the plans engine creation refuses (by message; creation launches nothing).  The checkpoint written under an edited plan is a part of
tests/test_gpu_parity.py::test_checkpoint_resume_is_bit_exact, beside the refusal of a restore into another plan.  Figures and the answers to what the engine does with kc = 1, huge and negative chunk lengths:
docs/history/plan_edges.md."""
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import feedforward_edges_common as C
import feedforward_reference as FR
import plan_edges_common as P
import ref

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()
INT_MIN = -2 ** 31


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


def policy_under_plan(h, c):
    """forward() on 1, 5 and 16 observations against the fp64 Q values; greedy_action is the fp64 argmax wherever the fp64 top-two gap exceeds GAP"""
    net, D = C.prepare(c)
    f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
    ps = net.unflatten(D["p_on"].astype(np.float64))
    for n in (1, 5, 16):
        obs = f(D["s"][:n])
        q64 = FR.q_numpy(net, ps, obs.astype(np.float64))[0]
        C._close("policy_q", h.forward(obs), q64, msg=f"{c.name} n={n}", **C.TOL_Q)
        t = np.sort(q64, axis=1); clear = t[:, -1] - t[:, -2] > C.GAP
        np.testing.assert_array_equal(np.asarray(h.greedy_action(obs))[clear], q64.argmax(1)[clear], err_msg=f"{c.name} n={n}")


@pytest.mark.parametrize("c", P.CASES, ids=IDS(P.CASES))
def test_case_under_its_plan_vs_fp64_reference_twin_schedule_and_kernels(pkg, c):
    f = C.check_want(c)                                   # the case stands on the side of the rule it was written for, on the edited plan
    net = C.network(c); hp = C.hparams(c, net); layers = FR.layer_descs(net)
    plan = C.case_plan(c, layers, hp); p = P.plan_of(c)
    if c.fwd:                                             # before any train step: the parameters are the case's
        h0, _ = C.make_handle(pkg.Engine, c, net, C.prepare(c)[1], plan=p)
        policy_under_plan(h0, c); h0.close()
    h, rec = C.run_checked(pkg.Engine, c, plan=p)         # against the fp64 reference
    assert h.plan() == plan, c.name
    C.same_bits(rec, C.replay_steps(ref.Twin, c, threads=8, plan=p), f"{c.name}: engine vs twin")
    C.same_bits(rec, C.replay_steps(pkg.Engine, c, graph=1 - c.graph, plan=p), f"{c.name}: use_graph {c.graph} vs {1 - c.graph}")
    C.same_bits(rec, C.replay_steps(pkg.Engine, c, mfma=1 - c.mfma, plan=p), f"{c.name}: use_mfma {c.mfma} vs {1 - c.mfma}")
    if not f["tiny"]:
        assert h.batch_arena_elem_bytes() == (1 if f["arena"] else 4), c.name
    C.assert_launches(h, f, c.name)                       # profile_step runs one more (eager) step: last
    h.close()


def _creation(pkg, Engine, plan, B=32, recurrence=0):
    net = C.network(C.case("refusal", 64, C.mlp(64, 32, 4), B, prio=0))
    hp = ref.hparams_for(net, batch_size=B, buffer_size=B + 8, prioritized_replay=0)
    return Engine(FR.layer_descs(net), hp, plan=plan)


@pytest.mark.parametrize("plan, msg", [
    ([(-1, 0, 0), (0, 0, 0)], r"layer 0: fwd_kc = -1, dx_kc = 0: a chunk length must be >= 0"),
    ([(0, 0, 0), (0, -32, 0)], r"layer 1: fwd_kc = 0, dx_kc = -32: a chunk length must be >= 0"),
    ([(INT_MIN, 0, 0), (0, 0, 0)], r"layer 0: fwd_kc = -2147483648"),
    ([(0, 0, INT_MIN), (0, 0, 0)], r"layer 0: dw_kc = -2147483648: a column group \(dw_kc < 0\) holds at most batch_size = 32 columns"),
    ([(0, 0, -33), (0, 0, 0)], r"layer 0: dw_kc = -33: a column group"),
    ([(0, 0, -4), (0, 0, -4)], r"dw_kc < 0 .* needs recurrence = true"),
], ids=["fwd_kc<0", "dx_kc<0", "fwd_kc=INT_MIN", "dw_kc=INT_MIN", "dw_kc<-B", "column-groups-feed-forward"])
def test_plans_refused_at_creation_by_message(pkg, plan, msg):
    """engine creation refuses these before anything is allocated or launched; the twin refuses the first five the same way"""
    with pytest.raises(pkg.DQNError, match=msg):
        _creation(pkg, pkg.Engine, plan)


def test_slab_workspace_bound_is_refused_at_creation(pkg):
    """kc = 1 is S = K slabs: accepted while the slabs of a layer hold at most 2^28 floats (plan_fwd_k96_kc1 runs it), refused by name beyond --
    Dense(8192, 4096) at B = 32 with fwd_kc = 1 would need 8192 x 4096 x 64 floats"""
    net = C.network(C.case("slabs", 8192, C.mlp(8192, 4096, 4), 32, prio=0))
    hp = ref.hparams_for(net, batch_size=32, buffer_size=40, prioritized_replay=0)
    with pytest.raises(pkg.DQNError, match=r"plan: layer 0: \(fwd_kc, dx_kc, dw_kc\) = \(1, 0, 0\) cuts its sums into 8192 / 1 / 1 chunks: the slabs of one layer may hold at most 2\^28 floats"):
        pkg.Engine(FR.layer_descs(net), hp, plan=[(1, 0, 0), (0, 0, 0)])
    # a huge chunk length is no chunk at all: unsplit, whatever its size (conv dw_kc excepted: it must be a multiple of batch_size or of 32 even where it cuts nothing)
    h = _creation(pkg, pkg.Engine, [(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 0, 0)])
    assert h.plan() == [(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 0, 0)]
    h.close()


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (docs/history/plan_edges.md records them)"""
    print("\nworst error / tolerance:", {k: round(v, 4) for k, v in sorted(C.WORST.items())})
    print("worst gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(FR.WORST.items()) if k.startswith(("conv", "dense"))})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
