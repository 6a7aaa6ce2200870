"""GPU (-m gpu): the acting step at its selection edges (acting_edges_common), with the Q column it computed in the comparison (dqn_envs_peek_q).

Per runnable grouped case: a group of one (k_tiny_act), a twin-constructed standalone engine (the multi-launch acting program) and, on a built-in env kind, the CPU
twin, run as calls of (1, 1, 2, 1, 3) vector steps with a train step every 2 and a target sync every 3.  After every call the group's member equals the standalone
engine and the twin in everything group_rollout_common.observables returns -- np.array_equal, the Q columns and greedy actions of the call's last vector step included
-- and q lies within E.TOL_Q of the fp64 forward of the rows that step acted on.  rollout_info() reports the dynamic LDS acting_edges_common.facts predicts.
One heterogeneous group holds every such member at once, between two rollouts of a two-copy group; the two refused cases are refused with the member and the term
facts predicts; the standalone pair runs the unstaged branch of the four-launch tail against the twin.  Nothing here has a tolerance but E.TOL_Q."""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import acting_edges_common as A
import ref

pytestmark = pytest.mark.gpu
CASES = A.cases()
GROUPED = [c["name"] for c in A.runnable_grouped()]


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package()
    p.lib()
    return p


@pytest.fixture(scope="module")
def envs(pkg):
    return importlib.import_module(pkg.__name__ + ".envs")


def close_all(group, *handles):
    if group is not None:
        group.close()
    for h in handles:
        if h is not None:
            h.close()


def group_roll(g, cs, k, t0, eps=None):
    return g.rollout(k, t0=t0, train_freq=A.TRAIN_FREQ, target_update_freq=A.TARGET_FREQ, eps=[c["eps"] if eps is None else eps for c in cs])


@pytest.mark.parametrize("name", GROUPED)
def test_group_of_one_equals_the_standalone_engine_the_twin_and_fp64(pkg, envs, name):
    c = CASES[name]
    m, alone = (A.build(c, pkg.Engine, pkg.default_plan, envs) for _ in range(2))
    twin = A.build(c, ref.Twin, pkg.default_plan, envs, threads=8) if c["twin"] else None
    g = pkg.EngineGroup([m])
    f = A.check_want(c, m.plan())
    assert alone.plan() == m.plan() and (twin is None or twin.plan() == m.plan())
    assert g.rollout_info() == (1, f["lds_bytes"]), (g.rollout_info(), f["lds_bytes"])
    with pytest.raises(pkg.DQNError, match="has not taken a vector step"):
        m.envs_peek_q()
    t0, trained = 1, False
    for j, k in enumerate(A.CALLS):
        p_before = m.get_params(0)
        st = group_roll(g, [c], k, t0)[0]
        sa = A.alone_roll(alone, k, t0, c["eps"])
        trained = trained or st["train_steps"] > 0
        got, want = A.step_record(m, st, trained=trained), A.step_record(alone, sa, trained=trained)
        A.check_record(c, got, want, p_acting=None if A.trains_before_last_step(t0, k) else p_before, what=f"call {j} ({k} steps from {t0}): group vs standalone")
        A.check_record(c, want, what=f"call {j}: standalone")
        if twin is not None:
            stw = A.alone_roll(twin, k, t0, c["eps"])
            A.check_record(c, got, A.step_record(twin, stw, trained=trained, td=False), what=f"call {j} ({k} steps from {t0}): group vs the CPU twin")
        t0 += k
    assert int(got["stats.episodes"]) > 0 and int(got["counters.train_steps"]) == sum(A.CALLS) // A.TRAIN_FREQ
    assert g.rollout_info() == (1, f["lds_bytes"])
    close_all(g, m, alone, twin)
    if isinstance(c["env"], tuple):      # the tabular cases have no twin: a first call under eps = 0 executes the greedy actions
        m2 = A.build(c, pkg.Engine, pkg.default_plan, envs)
        g2 = pkg.EngineGroup([m2])
        p = m2.get_params(0)
        st = group_roll(g2, [c], 1, 1, eps=(0.0, 0.0, 1.0))[0]
        A.check_record(c, A.step_record(m2, st, trained=False), p_acting=p, greedy_only=True, what="eps = 0")
        close_all(g2, m2)


def test_one_heterogeneous_group_of_every_member_between_two_small_groups(pkg, envs):
    """every runnable grouped member in ONE launch per vector step: the member at the LDS bound beside the two-copy one, so each workgroup lays out its own LDS inside
    the launch's maximum.  A two-copy group rolls out before and after: the function's dynamic-LDS request is raised in between and never lowered"""
    cs = [CASES[n] for n in GROUPED]
    small = CASES["ring_two"]
    s_m, s_alone = (A.build(small, pkg.Engine, pkg.default_plan, envs, env_seed=23) for _ in range(2))
    gs = pkg.EngineGroup([s_m])
    st = group_roll(gs, [small], 2, 1)[0]
    A.check_record(small, A.step_record(s_m, st), A.step_record(s_alone, A.alone_roll(s_alone, 2, 1, small["eps"])), what="small group, before")
    members = [A.build(c, pkg.Engine, pkg.default_plan, envs) for c in cs]
    alone = [A.build(c, pkg.Engine, pkg.default_plan, envs) for c in cs]
    g = pkg.EngineGroup(members)
    lds = [A.facts(c)["lds_bytes"] for c in cs]
    assert g.rollout_info() == (1, max(lds)) and max(lds) == 103424 and gs.rollout_info() == (1, A.facts(small)["lds_bytes"]) and A.facts(small)["lds_bytes"] < 1024
    t0, trained = 1, False
    for j, k in enumerate(A.CALLS):
        p_before = [h.get_params(0) for h in members]
        sts = group_roll(g, cs, k, t0)
        trained = trained or sts[0]["train_steps"] > 0
        for i, c in enumerate(cs):
            sa = A.alone_roll(alone[i], k, t0, c["eps"])
            A.check_record(c, A.step_record(members[i], sts[i], trained=trained), A.step_record(alone[i], sa, trained=trained),
                           p_acting=None if A.trains_before_last_step(t0, k) else p_before[i], what=f"member {i} of the heterogeneous group, call {j}")
        t0 += k
    st = group_roll(gs, [small], 3, 3)[0]
    A.check_record(small, A.step_record(s_m, st), A.step_record(s_alone, A.alone_roll(s_alone, 3, 3, small["eps"])), what="small group, after")
    close_all(g, *members, *alone)
    close_all(gs, s_m, s_alone)


def _fingerprint(h):
    return h.get_counters(), h.get_params(0).tobytes(), h.replay_priorities().tobytes(), [x.tobytes() for x in h.envs_peek()]


@pytest.mark.parametrize("name", ["lds_above", "pxn_above"])
def test_refused_cases_name_the_member_and_the_term(pkg, envs, name):
    c, ok = CASES[name], CASES["ring_two"]
    assert A.check_want(c)["refusal"] is not None
    hs = [A.build(ok, pkg.Engine, pkg.default_plan, envs), A.build(c, pkg.Engine, pkg.default_plan, envs)]
    g = pkg.EngineGroup(hs)
    before = [_fingerprint(h) for h in hs]
    why = "member 1 does not take the single-workgroup acting step: "
    with pytest.raises(pkg.DQNError) as ei:
        group_roll(g, [ok, c], 2, 1)
    assert "dqn_rollout_many: " + why in str(ei.value) and A.refusal_text(c) in str(ei.value), str(ei.value)
    with pytest.raises(pkg.DQNError) as ei:
        g.rollout_info()
    assert "dqn_rollout_many_info: " + why in str(ei.value) and A.refusal_text(c) in str(ei.value), str(ei.value)
    assert [_fingerprint(h) for h in hs] == before
    for h in hs:
        with pytest.raises(pkg.DQNError, match="has not taken a vector step"):
            h.envs_peek_q()
    close_all(g, *hs)


def test_accessor_reads_only_and_is_refused_once_another_forward_took_the_workspace(pkg, envs):
    c = CASES["k19_scalar"]
    h = A.build(c, pkg.Engine, pkg.default_plan, envs)
    bare = pkg.Engine(*A.layers_hp(c))
    with pytest.raises(pkg.DQNError, match="no device environments"):
        bare.envs_peek_q()
    st = A.alone_roll(h, 3, 1, c["eps"])
    before = A.step_record(h, st)
    f = pkg.fns()
    assert f["envs_peek_q"](h._h, None, None) == 0      # either pointer may be NULL
    q = np.empty((c["n"], 4), np.float32); a = np.empty(c["n"], np.int32)
    assert f["envs_peek_q"](h._h, q.ctypes.data_as(f["envs_peek_q"].argtypes[1]), None) == 0 and f["envs_peek_q"](h._h, None, a.ctypes.data_as(f["envs_peek_q"].argtypes[2])) == 0
    assert np.array_equal(q, before["peekq.q"]) and np.array_equal(a, before["peekq.greedy"])
    A.assert_same(A.step_record(h, st), before, "the accessor launches nothing and rewrites nothing")
    h.forward(before["peek.obs"])
    with pytest.raises(pkg.DQNError, match="the policy workspace was used since"):
        h.envs_peek_q()
    A.alone_roll(h, 1, 4, c["eps"]); h.envs_peek_q()
    h.evaluate(3, 4, seed=2)
    with pytest.raises(pkg.DQNError, match="the policy workspace was used since"):
        h.envs_peek_q()
    h.envs_create(A.env_of(envs, c), max_episode_length=3, seed=1)
    with pytest.raises(pkg.DQNError, match="has not taken a vector step"):
        h.envs_peek_q()
    close_all(None, h, bare)


@pytest.mark.parametrize("name", ["split_head_at", "split_head_above"])
def test_split_head_pair_on_the_four_launch_tail_equals_the_twin(pkg, envs, monkeypatch, name):
    """16 slabs per head value: 64 floats per copy, 128 copies fill the tail's LDS staging exactly, 129 take the branch that reads the slabs per use.  Created by default
    and under DQN_NO_ACT_HEAD=1: the fused tail wants head chunks of 32 and declines chunks of 4, so both settings run the four-launch tail, which envs_info states"""
    c = CASES[name]
    outs = []
    for no_act_head in (False, True):
        if no_act_head:
            monkeypatch.setenv("DQN_NO_ACT_HEAD", "1")      # read once, at creation
        g = A.build(c, pkg.Engine, pkg.default_plan, envs)
        monkeypatch.delenv("DQN_NO_ACT_HEAD", raising=False)
        t = A.build(c, ref.Twin, pkg.default_plan, envs, threads=8)
        f = A.check_want(c, g.plan())
        assert g.plan() == t.plan() and g.plan()[-1][0] == 4 and f["chunks"][-1] == 16
        assert g.envs_info() == (c["n"], f["fused_tail"]) == (c["n"], False), "the schedule under test is not the one this case names"
        t0, trained = 1, False
        for j, k in enumerate(A.CALLS):
            p_before = g.get_params(0)
            sg, st = A.alone_roll(g, k, t0, c["eps"]), A.alone_roll(t, k, t0, c["eps"])
            trained = trained or sg["train_steps"] > 0
            got = A.step_record(g, sg, trained=trained)
            A.check_record(c, got, A.step_record(t, st, trained=trained, td=False), p_acting=None if A.trains_before_last_step(t0, k) else p_before,
                           what=f"call {j}, DQN_NO_ACT_HEAD={int(no_act_head)}: engine vs the CPU twin")
            t0 += k
        outs.append(got)
        close_all(None, g, t)
    A.assert_same(outs[0], outs[1], "the two settings walk the same trajectory")


def test_zz_report_worst_q_error():
    """not a check: prints the largest |q - fp64| / tolerance this file saw (docs/history/acting_edges.md records it)"""
    import feedforward_edges_common as E
    print("\nworst error / tolerance:", {k: round(v, 4) for k, v in sorted(E.WORST.items()) if k == "acting_q"})
