"""GPU (-m gpu): engine groups through the C ABI (dqn_group_*, include/dqn_mi355x.h).  THE LAW: after dqn_group_train_steps(g, n) every member is bit for bit
what dqn_train_steps(e, n) leaves on a twin-constructed standalone engine -- same layers, hyper-parameters, seed, parameters and replay (engine_group_common).
Every comparison is np.array_equal; nothing here has a tolerance."""
import ctypes
import importlib
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import dqn_oracle as O
import ref
from drqn_common import drqn_nets
from engine_group_common import assert_same, build, member_specs, observables, replay_rows
from nets import small_conv_plain

pytestmark = pytest.mark.gpu
N_STEPS = 5


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package()
    p.lib()
    return p


def close_all(group, *handles):
    if group is not None:
        group.close()
    for h in handles:
        h.close()


@pytest.fixture(scope="module")
def hetero(pkg):
    """computed ONCE, read by several tests: the five members after a group call of N_STEPS steps and their standalone references after train_steps(N_STEPS)"""
    specs = member_specs()
    members = [build(s, pkg.Engine, pkg.default_plan) for s in specs.values()]
    alone = [build(s, pkg.Engine, pkg.default_plan) for s in specs.values()]
    group = pkg.EngineGroup(members)
    info = group.info()
    loss, gn = group.train_steps(N_STEPS)
    got = [observables(h) for h in members]
    scal = [h.train_steps(N_STEPS) for h in alone]
    want = [observables(h) for h in alone]
    close_all(group, *members, *alone)
    return dict(names=list(specs), info=info, loss=loss, gn=gn, got=got, scal=scal, want=want)


def test_heterogeneous_group_equals_standalone_engines(hetero):
    assert hetero["info"]["n_members"] == 5 and hetero["info"]["launches_per_step"] == 1
    assert hetero["info"]["max_lds_bytes"] > 65536                       # member e: the group launch had to raise the function's dynamic-LDS limit
    for k, name in enumerate(hetero["names"]):
        assert_same(hetero["got"][k], hetero["want"][k], "member " + name)
        assert (hetero["loss"][k], hetero["gn"][k]) == tuple(np.float32(x) for x in hetero["scal"][k]), name
        assert int(hetero["want"][k]["counters.train_steps"]) == N_STEPS and int(hetero["want"][k]["counters.sample_ctr"]) == N_STEPS


def test_member_b_equals_the_cpu_twin(pkg, hetero):
    """the chain does not rest on the standalone device path alone: member b against the CPU twin over the same steps"""
    spec = member_specs()["b"]
    twin = build(spec, ref.Twin, pkg.default_plan, threads=8)
    for _ in range(N_STEPS):
        lt, gt = twin.train_step(want_td=False)
    k = hetero["names"].index("b")
    want = observables(twin, td=False)
    got = {key: v for key, v in hetero["got"][k].items() if key in want}
    assert_same(got, want, "member b vs the CPU twin")
    assert (hetero["loss"][k], hetero["gn"][k]) == (np.float32(lt), np.float32(gt))
    twin.close()


def test_group_of_one_equals_the_standalone_engine(pkg):
    spec = member_specs()["c"]
    m, alone = build(spec, pkg.Engine, pkg.default_plan), build(spec, pkg.Engine, pkg.default_plan)
    g = pkg.EngineGroup([m])
    loss, gn = g.train_steps(3)
    assert (loss[0], gn[0]) == tuple(np.float32(x) for x in alone.train_steps(3))
    assert_same(observables(m), observables(alone), "K = 1")
    close_all(g, m, alone)


def test_more_members_than_compute_units(pkg):
    """258 workgroups on 256 compute units: every copy of member a equals every other and one standalone engine"""
    K, spec = 258, member_specs()["a"]
    t0 = time.perf_counter()
    members = [build(spec, pkg.Engine, pkg.default_plan) for _ in range(K)]
    print(f"creating {K} engines: {time.perf_counter() - t0:.2f} s")
    alone = build(spec, pkg.Engine, pkg.default_plan)
    g = pkg.EngineGroup(members)
    loss, gn = g.train_steps(3)
    la, ga = alone.train_steps(3)
    assert np.array_equal(loss, np.full(K, la, np.float32)) and np.array_equal(gn, np.full(K, ga, np.float32))
    want = dict(p_on=alone.get_params(0), m=alone.get_adam_state()[0], pr=alone.replay_priorities(), idx=alone.last_indices(), td=alone.last_td()[0], c=alone.get_counters())
    for k, h in enumerate(members):
        got = dict(p_on=h.get_params(0), m=h.get_adam_state()[0], pr=h.replay_priorities(), idx=h.last_indices(), td=h.last_td()[0], c=h.get_counters())
        assert all(np.array_equal(got[x], want[x]) for x in ("p_on", "m", "pr", "idx", "td")) and got["c"] == want["c"], k
    close_all(g, *members, alone)


def test_member_calls_interleave_with_group_calls_without_host_syncs(pkg):
    specs = member_specs()
    a, b = build(specs["a"], pkg.Engine, pkg.default_plan), build(specs["b"], pkg.Engine, pkg.default_plan)
    a0, b0 = build(specs["a"], pkg.Engine, pkg.default_plan), build(specs["b"], pkg.Engine, pkg.default_plan)
    extra = [replay_rows(specs["b"], n=2, seed=7 + i) for i in range(3)]
    g = pkg.EngineGroup([a, b])
    g.train_steps(2)
    for rows in extra:
        b.replay_add(*rows)
    b.train_step(sync=False)
    a.sync_target()
    loss, gn = g.train_steps(2)
    a0.train_steps(2); b0.train_steps(2)
    for rows in extra:
        b0.replay_add(*rows)
    b0.train_step(sync=False)
    a0.sync_target()
    sa, sb = a0.train_steps(2), b0.train_steps(2)
    assert (loss[0], gn[0]) == tuple(np.float32(x) for x in sa) and (loss[1], gn[1]) == tuple(np.float32(x) for x in sb)
    assert_same(observables(a), observables(a0), "member a")
    assert_same(observables(b), observables(b0), "member b")
    close_all(g, a, b, a0, b0)


def test_getters_right_after_a_group_call_see_its_results(pkg):
    spec = member_specs()["a"]
    m, alone = build(spec, pkg.Engine, pkg.default_plan), build(spec, pkg.Engine, pkg.default_plan)
    g = pkg.EngineGroup([m])
    before = m.get_params(0)
    g.train_steps(2)
    p, c, idx = m.get_params(0), m.get_counters(), m.last_indices()      # no explicit synchronise in between
    alone.train_steps(2)
    assert not np.array_equal(p, before)
    assert np.array_equal(p, alone.get_params(0)) and c == alone.get_counters() and np.array_equal(idx, alone.last_indices())
    close_all(g, m, alone)


def test_a_members_device_assertion_is_reported_with_its_index(pkg):
    """member c's online parameters are NaN: its new priorities fail `> 0` (a CHECKED device assertion, ...replay.jl:78).  The group call names member 2 in the
    standalone call's words; members a and b hold exactly their standalone results"""
    specs = member_specs()
    ms = [build(specs[n], pkg.Engine, pkg.default_plan) for n in "abc"]
    alone = [build(specs[n], pkg.Engine, pkg.default_plan) for n in "ab"]
    ms[2].set_params(np.full(ms[2].P, np.nan, np.float32), 0)
    g = pkg.EngineGroup(ms)
    with pytest.raises(pkg.DQNError, match=r"member 2: AssertionError: all\(new_priorities \.> 0f0\)"):
        g.train_steps(2)
    for h in alone:
        h.train_steps(2)
    assert_same(observables(ms[0]), observables(alone[0]), "member a")
    assert_same(observables(ms[1]), observables(alone[1]), "member b")
    close_all(g, *ms, *alone)


def _engine(pkg, net, B, cap=256, **kw):
    hp = ref.hparams_for(net, batch_size=B, buffer_size=cap, **kw)
    layers = ref.layers_from_network(net)
    return pkg.Engine(layers, hp, plan=pkg.default_plan(layers, hp))


def test_refusals_name_the_member_and_the_reason(pkg, monkeypatch):
    specs = member_specs()
    ok = build(specs["a"], pkg.Engine, pkg.default_plan)
    f = pkg.fns()

    def refused(handles, pattern, n=None):
        arr = (ctypes.c_void_p * len(handles))(*[None if h is None else h._h.value for h in handles])
        out = ctypes.c_void_p()
        assert f["group_create"](arr, len(handles) if n is None else n, ctypes.byref(out)) == -1 and not out.value
        msg = f["last_error"]().decode()
        assert pattern in msg, msg

    refused([ok, None], "member 1 is a null engine handle")
    refused([ok, ok], "member 1 is the same engine as member 0")
    refused([ok], "n_members = 0 is outside 1..4096", n=0)
    refused([ok], "n_members = 4097 is outside 1..4096", n=4097)
    cfg1 = specs["b"]["net"]
    lstm_net, lB, lT, lkw = drqn_nets()["lstm_single_q"]
    monkeypatch.setenv("DQN_NO_TINY", "1")
    no_tiny = _engine(pkg, cfg1, 32)
    monkeypatch.delenv("DQN_NO_TINY")
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    sim = _engine(pkg, cfg1, 32)
    monkeypatch.delenv("DQN_SIM_WORLD")
    others = [
        (_engine(pkg, small_conv_plain(), 16), "member 1 does not take the single-workgroup step: layer 0 is not a Dense layer"),
        (_engine(pkg, lstm_net, lB, cap=16, recurrence=1, trace_length=lT, prioritized_replay=0, **lkw), "member 1 does not take the single-workgroup step: it is recurrent"),
        (_engine(pkg, cfg1, 128), "member 1 does not take the single-workgroup step: B > 64 (batch_size = 128)"),
        (_engine(pkg, cfg1, 32, prioritized_replay=0), "member 1 does not take the single-workgroup step: it has no prioritized replay"),
        (_engine(pkg, O.Network((64,), [O.Dense(64, 300, O.ACT_RELU), O.Dense(300, 4, O.ACT_IDENTITY)]), 8), "member 1 does not take the single-workgroup step: it has too many parameters"),
        (no_tiny, "member 1 does not take the single-workgroup step: it was created under DQN_NO_TINY"),
        (sim, "member 1 does not take the single-workgroup step: it runs as data-parallel replicas (a communicator, or created under DQN_SIM_WORLD)"),
    ]
    for h, pattern in others:
        refused([ok, h], pattern)
    import torch
    if torch.cuda.device_count() > 1:                                    # a member on another device needs a second one
        hp = ref.hparams_for(cfg1, batch_size=32, buffer_size=64)
        far = pkg.Engine(ref.layers_from_network(cfg1), hp, device=1)
        refused([ok, far], "member 1 lives on device 1, member 0 on device 0")
        far.close()
    # train time: too few transitions (the reference's assertion text), n < 1
    hp = ref.hparams_for(cfg1, batch_size=32, buffer_size=64)
    empty = pkg.Engine(ref.layers_from_network(cfg1), hp)
    g = pkg.EngineGroup([ok, empty])
    with pytest.raises(pkg.DQNError, match=r"member 1: AssertionError: r\._curr_size >= r\.batch_size"):
        g.train_steps(1)
    with pytest.raises(pkg.DQNError, match="n = 0"):
        g.train_steps(0)
    # a member of a live group cannot be given a communicator (its step program would be rebuilt under the group): refused before any communicator is made
    with pytest.raises(pkg.DQNError, match="dqn_comm_init: this engine is a member of 1 live group"):
        ok.comm_init(bytes(128), 0, 1)
    # a member of a live group cannot be destroyed; after the group is gone it can
    with pytest.raises(pkg.DQNError, match="member of 1 live group -- destroy the group first"):
        ok.close()
    assert ok.get_counters()["train_steps"] == 0                          # the refused destroy left the engine whole
    g.close()
    close_all(None, ok, empty, *[h for h, _ in others])


def test_solve_many_equals_solve_member_by_member(pkg):
    S, nn, envs = (importlib.import_module(pkg.__name__ + "." + m) for m in ("solver", "nn", "envs"))

    def solver(k):
        env = envs.SimpleGridWorld(n=4, seed=5)
        model = nn.Chain(nn.Dense(2, 16, nn.relu), nn.Dense(16, env.n_actions))
        expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.1, steps=40))
        return S.DeepQLearningSolver(qnetwork=model, exploration_policy=expl, max_steps=48, train_freq=4, target_update_freq=16, train_start=8, batch_size=8,
                                     buffer_size=64, eval_freq=24, num_ep_eval=4, log_freq=24, logdir=None, verbose=False, device_envs=True,
                                     seed=100 + k, learning_rate=1e-3 * (k + 1), rng=np.random.default_rng(9)), env

    many = S.solve_many([solver(k)[0] for k in range(3)], envs.SimpleGridWorld(n=4, seed=5))
    for k, pol in enumerate(many):
        s, env = solver(k)
        one = S.solve(s, env)
        e, e1 = pol.engine, one.engine
        assert e.get_counters() == e1.get_counters() and e.get_counters()["train_steps"] == 12, k
        assert np.array_equal(e.get_params(0), e1.get_params(0)) and np.array_equal(e.get_params(1), e1.get_params(1)), k
        assert np.array_equal(e.replay_priorities(), e1.replay_priorities()), k
        close_all(None, e, e1)
