"""GPU (-m gpu): grouped acting through the C ABI (dqn_rollout_many, include/dqn_mi355x.h; tiny_act.hip).  THE LAW: after dqn_rollout_many(g, n, cfgs, xs, out)
every member is bit for bit what dqn_rollout_explore(member, n, &cfgs[k], xs[k], &out[k]) leaves on a twin-constructed standalone engine -- same layers, plan,
hyper-parameters, parameters, replay prefill and env set (group_rollout_common).  Every comparison is np.array_equal; nothing here has a tolerance."""
import ctypes
import importlib
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import ref
from group_rollout_common import N_STEPS, TARGET_FREQ, TRAIN_FREQ, assert_same, build, member_specs, observables, replay_rows, rollout_alone

pytestmark = pytest.mark.gpu


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
        h.close()


def many(group, specs, n_steps, t0=1, explore=None, train_freq=TRAIN_FREQ, target_update_freq=TARGET_FREQ):
    return group.rollout(n_steps, t0=t0, train_freq=train_freq, target_update_freq=target_update_freq, eps=[s["eps"] for s in specs], explore=explore)


@pytest.fixture(scope="module")
def hetero(pkg, envs):
    """computed ONCE, read by several tests: the six members after one dqn_rollout_many of N_STEPS vector steps, their standalone references after rollout(N_STEPS)"""
    specs = member_specs()
    members = [build(s, pkg.Engine, pkg.default_plan, envs) for s in specs.values()]
    alone = [build(s, pkg.Engine, pkg.default_plan, envs) for s in specs.values()]
    group = pkg.EngineGroup(members)
    info = group.rollout_info()
    st = many(group, list(specs.values()), N_STEPS)
    got = [observables(h, st[k]) for k, h in enumerate(members)]
    want = [observables(h, rollout_alone(h, s, N_STEPS)) for h, s in zip(alone, specs.values())]
    close_all(group, *members, *alone)
    return dict(names=list(specs), info=info, got=got, want=want)


def test_heterogeneous_group_equals_standalone_engines(hetero):
    assert hetero["info"][0] == 1 and hetero["info"][1] > 0
    specs = member_specs()
    for k, name in enumerate(hetero["names"]):
        assert_same(hetero["got"][k], hetero["want"][k], "member " + name)
        w, s = hetero["want"][k], specs[name]
        assert int(w["stats.train_steps"]) == N_STEPS // TRAIN_FREQ == int(w["counters.train_steps"])
        assert int(w["stats.episodes"]) > 0, name      # max_episode_length is small enough that resets occur
        wrapped = s["n_fill"] + N_STEPS * s["n"] > s["cap"]
        assert int(w["replay_size"][0]) == (s["cap"] if wrapped else s["n_fill"] + N_STEPS * s["n"]), name
    # the ring branches of add_exp!'s tree rebuild the run is sized for
    assert specs["grid"]["cap"] % specs["grid"]["n"] != 0 and specs["deep"]["n"] == specs["deep"]["cap"]
    assert all(specs[m]["n_fill"] + N_STEPS * specs[m]["n"] <= specs[m]["cap"] for m in ("plain", "one"))


def test_member_grid_equals_the_cpu_twin(pkg, envs, hetero):
    """the chain does not rest on the standalone device path alone: member `grid` against the CPU twin's rollout -- trajectory, replay rows, priorities, parameters"""
    spec = member_specs()["grid"]
    twin = build(spec, ref.Twin, pkg.default_plan, envs, threads=8)
    st = rollout_alone(twin, spec, N_STEPS)
    k = hetero["names"].index("grid")
    want = observables(twin, st, td=False)
    got = {key: v for key, v in hetero["got"][k].items() if key in want}
    assert_same(got, want, "member grid vs the CPU twin")
    twin.close()


def test_exploration_tables_per_member(pkg, envs):
    """an eps table of n_steps values, a one-value table, a softmax temperature table, a NULL entry -- and explore = NULL as a whole in the second call"""
    base = member_specs()
    names = ["grid", "plain", "tiger", "mdp"]
    specs = [base[n] for n in names]
    tables = [("eps", np.linspace(1.0, 0.0, 7).astype(np.float32)), ("eps", np.float32(0.25)), ("softmax", np.linspace(2.0, 0.05, 7).astype(np.float32)), None]
    members = [build(s, pkg.Engine, pkg.default_plan, envs) for s in specs]
    alone = [build(s, pkg.Engine, pkg.default_plan, envs) for s in specs]
    g = pkg.EngineGroup(members)
    st1 = many(g, specs, 7, explore=tables)
    st2 = many(g, specs, 5, t0=8)
    for k, (h, s) in enumerate(zip(alone, specs)):
        w1 = rollout_alone(h, s, 7, explore=tables[k])
        w2 = rollout_alone(h, s, 5, t0=8)
        assert st1[k] == w1 and st2[k] == w2, (names[k], st1[k], w1, st2[k], w2)
        assert_same(observables(members[k], st2[k]), observables(h, w2), "member " + names[k])
    close_all(g, *members, *alone)


def test_group_of_one_equals_the_standalone_engine(pkg, envs):
    spec = member_specs()["one"]
    m, alone = build(spec, pkg.Engine, pkg.default_plan, envs), build(spec, pkg.Engine, pkg.default_plan, envs)
    g = pkg.EngineGroup([m])
    st = many(g, [spec], 3, train_freq=2)
    assert_same(observables(m, st[0]), observables(alone, rollout_alone(alone, spec, 3, train_freq=2)), "K = 1")
    close_all(g, m, alone)


def test_more_members_than_compute_units(pkg, envs):
    """258 workgroups on 256 compute units: every copy of member `one` equals every other and one standalone engine"""
    K, spec = 258, member_specs()["one"]
    t0 = time.perf_counter()
    members = [build(spec, pkg.Engine, pkg.default_plan, envs) for _ in range(K)]
    print(f"creating {K} engines with env sets: {time.perf_counter() - t0:.2f} s")
    alone = build(spec, pkg.Engine, pkg.default_plan, envs)
    g = pkg.EngineGroup(members)
    st = many(g, [spec] * K, 3, train_freq=2)
    wst = rollout_alone(alone, spec, 3, train_freq=2)
    assert all(s == wst for s in st)

    def light(h):
        return dict(p_on=h.get_params(0), pr=h.replay_priorities(), idx=h.last_indices(), td=h.last_td()[0], c=np.asarray(list(h.get_counters().values())),
                    **{"peek%d" % i: x for i, x in enumerate(h.envs_peek())})

    want = light(alone)
    for k, h in enumerate(members):
        got = light(h)
        assert all(np.array_equal(got[x], want[x]) for x in want), k
    close_all(g, *members, alone)


def test_chunks_interleave_with_member_calls_without_host_syncs(pkg, envs):
    """rollout_many(5), then a member's own rollout, replay_add, a group train step and a getter, then rollout_many(7): the same sequence on standalone engines"""
    base = member_specs()
    names = ["grid", "mdp", "one"]
    specs = [base[n] for n in names]
    members = [build(s, pkg.Engine, pkg.default_plan, envs) for s in specs]
    alone = [build(s, pkg.Engine, pkg.default_plan, envs) for s in specs]
    extra = replay_rows(specs[1], n=3, seed=9)
    g = pkg.EngineGroup(members)
    many(g, specs, 5)
    members[2].rollout(2, t0=6, train_freq=0, target_update_freq=0, eps=specs[2]["eps"], stats=False)      # (its own launches, on its own stream)
    members[1].replay_add(*extra)
    g.train_steps(1)
    p_mid = members[0].get_params(0)
    st = many(g, specs, 7, t0=8)
    for h, s in zip(alone, specs):
        rollout_alone(h, s, 5)
    alone[2].rollout(2, t0=6, train_freq=0, target_update_freq=0, eps=specs[2]["eps"], stats=False)
    alone[1].replay_add(*extra)
    for h in alone:
        h.train_steps(1)
    assert np.array_equal(p_mid, alone[0].get_params(0))
    for k, (h, s) in enumerate(zip(alone, specs)):
        w = rollout_alone(h, s, 7, t0=8)
        assert_same(observables(members[k], st[k]), observables(h, w), "member " + names[k])
    close_all(g, *members, *alone)


def test_a_members_device_assertion_is_reported_with_its_index(pkg, envs):
    """prio_eps = 0 and a zero reward (every SimpleGridWorld step away from a reward cell): add_exp!'s new priority is not positive -- a flag the kernel sets, not a
    fault.  The call names member 1; members 0 and 2 hold exactly their standalone results"""
    base = member_specs()
    bad = dict(base["plain"], hp=dict(base["plain"]["hp"], prio_eps=0.0))
    specs = [base["one"], bad, base["tiger"]]
    members = [build(s, pkg.Engine, pkg.default_plan, envs) for s in specs]
    alone = [build(s, pkg.Engine, pkg.default_plan, envs) for s in (specs[0], specs[2])]
    g = pkg.EngineGroup(members)
    with pytest.raises(pkg.DQNError, match=r"member 1: (device-side error 1|AssertionError: all\(new_priorities \.> 0f0\)) \(?at or before train step \d+\)?; the other members' steps stand"):
        many(g, specs, 4)
    wa, wc = rollout_alone(alone[0], specs[0], 4), rollout_alone(alone[1], specs[2], 4)
    assert_same(observables(members[0]), observables(alone[0]), "member 0")
    assert_same(observables(members[2]), observables(alone[1]), "member 2")
    assert wa["train_steps"] == wc["train_steps"] == 1
    close_all(g, *members, *alone)


def _fingerprint(h):
    return h.get_counters(), h.get_params(0).tobytes(), h.replay_priorities().tobytes(), [x.tobytes() for x in h.envs_peek()]


def test_refusals_name_the_member_and_the_reason(pkg, envs):
    base = member_specs()
    specs = [base["one"], base["plain"]]
    members = [build(s, pkg.Engine, pkg.default_plan, envs) for s in specs]
    g = pkg.EngineGroup(members)
    f = pkg.fns()
    abi = pkg._abi
    before = [_fingerprint(h) for h in members]

    def cfgs(**over):
        out = []
        for k, s in enumerate(specs):
            kw = dict(train_freq=TRAIN_FREQ, target_update_freq=TARGET_FREQ, cadence=0, t0=1)
            kw.update({key: v[k] if isinstance(v, (list, tuple)) else v for key, v in over.items()})
            out.append(abi.RolloutCfg(kw["train_freq"], kw["target_update_freq"], s["eps"][0], s["eps"][1], s["eps"][2], kw["cadence"], kw["t0"]))
        return (abi.RolloutCfg * len(specs))(*out)

    def table(kind, values, n_values=None):
        vals = None if values is None else np.ascontiguousarray(values, np.float32)
        return abi.Exploration(kind, n_values if vals is None else vals.size, None if vals is None else vals.ctypes.data), vals

    def refused(pattern, n_steps=4, c=None, xs=None, group=g):
        arr = None
        if xs is not None:
            arr = (ctypes.POINTER(abi.Exploration) * len(xs))()
            for k, x in enumerate(xs):
                if x is not None:
                    arr[k] = ctypes.pointer(x[0])
        assert f["rollout_many"](group._g, n_steps, cfgs() if c is None else c, arr, None) == -1
        msg = f["last_error"]().decode()
        assert pattern in msg, msg

    assert f["rollout_many"](None, 1, cfgs(), None, None) == -1 and b"null group handle" in f["last_error"]()
    refused("n_steps = 0, at least one vector step is needed", n_steps=0)
    assert f["rollout_many"](g._g, 1, None, None, None) == -1 and b"cfgs is NULL" in f["last_error"]()
    refused("member 1: t0 counts from 1", c=cfgs(t0=[1, 0]))
    refused("t0 differs between members 0 and 1 (1 vs 3)", c=cfgs(t0=[1, 3]))
    refused("train_freq differs between members 0 and 1 (4 vs 2)", c=cfgs(train_freq=[4, 2]))
    refused("target_update_freq differs between members 0 and 1 (8 vs 0)", c=cfgs(target_update_freq=[8, 0]))
    refused("member 0: cadence_env_steps = 1 -- the group runs the vector-step cadence only", c=cfgs(cadence=1))
    refused("member 1: exploration: unknown kind 7", xs=[None, table(7, [0.5])])
    refused("member 1: exploration: n_values = 3 is neither 1 nor n_vector_steps = 4", xs=[None, table(0, [0.5] * 3)])
    refused("member 0: exploration: values is NULL (n_values = 1)", xs=[table(0, None, 1), None])
    refused("member 1: exploration: eps values[2] = 1.5 is outside [0, 1]", xs=[None, table(0, [0.1, 0.2, 1.5, 0.3])])
    refused("member 0: exploration: temperature values[0] = 0 is not a finite positive number", xs=[table(1, [0.0]), None])
    assert [_fingerprint(h) for h in members] == before                      # a refused call leaves the members untouched
    # members that disagree on a due train step: member 1 holds a batch at t = 4, a member with an empty replay of one copy and a batch of 8 does not
    late = dict(base["one"], B=8, n_fill=1)
    hl = build(late, pkg.Engine, pkg.default_plan, envs)
    g2 = pkg.EngineGroup([members[0], hl])
    with pytest.raises(pkg.DQNError, match=r"members 0 and 1 disagree at vector step 4 on whether the train step runs \(member 0 holds 10 of its batch of 4, member 1 holds 5 of 8\)"):
        g2.rollout(4, eps=[specs[0]["eps"], late["eps"]])
    g2.close()
    # a member that does not take the single-workgroup acting step
    noenv = dict(base["one"])
    hn = build(noenv, pkg.Engine, pkg.default_plan, envs)
    hp = ref.hparams_for(noenv["net"], batch_size=4, buffer_size=32)
    bare = pkg.Engine(ref.layers_from_network(noenv["net"]), hp)
    g3 = pkg.EngineGroup([hn, bare])
    with pytest.raises(pkg.DQNError, match="member 1 does not take the single-workgroup acting step: it has no device environments"):
        g3.rollout(2, eps=(1.0, 0.1, 10.0))
    with pytest.raises(pkg.DQNError, match="dqn_rollout_many_info: member 1 does not take the single-workgroup acting step: it has no device environments"):
        g3.rollout_info()
    g3.close()
    # 1024 copies of the deep member: parameters x n_envs above the one-CU budget
    big = dict(base["deep"], n=1024, cap=1024)
    hb = build(big, pkg.Engine, pkg.default_plan, envs)
    g4 = pkg.EngineGroup([hb])
    with pytest.raises(pkg.DQNError, match=r"member 0 does not take the single-workgroup acting step: it has too many parameters for 1024 copies"):
        g4.rollout(2, eps=big["eps"])
    g4.close()
    # ... and 1024 copies of the plain 2-32-4 network: within that budget, but their activations do not fit beside the step's tail
    wide = dict(base["plain"], n=1024, cap=1024)
    hw = build(wide, pkg.Engine, pkg.default_plan, envs)
    g5 = pkg.EngineGroup([hw])
    with pytest.raises(pkg.DQNError, match=r"member 0 does not take the single-workgroup acting step: it needs \d+ bytes of LDS"):
        g5.rollout(2, eps=wide["eps"])
    g5.close()
    assert [_fingerprint(h) for h in members] == before
    close_all(g, *members, hl, hn, bare, hb, hw)


def test_solve_many_equals_solve_member_by_member_with_three_exploration_policies(pkg):
    S, nn, envs = (importlib.import_module(pkg.__name__ + "." + m) for m in ("solver", "nn", "envs"))

    def solver(k):
        env = envs.SimpleGridWorld(n=4, seed=5)
        model = nn.Chain(nn.Dense(2, 16, nn.relu), nn.Dense(16, env.n_actions))
        expl = [S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.1, steps=40)), S.EpsGreedyPolicy(env, 0.3), S.SoftmaxPolicy(env, lambda t: 1.0 / (1.0 + 0.1 * t))][k]
        return S.DeepQLearningSolver(qnetwork=model, exploration_policy=expl, max_steps=48, train_freq=4, target_update_freq=16, train_start=8, batch_size=8,
                                     buffer_size=64, eval_freq=24, num_ep_eval=4, log_freq=24, logdir=None, verbose=False, device_envs=True,
                                     seed=200 + k, learning_rate=1e-3 * (k + 1), rng=np.random.default_rng(9)), env

    calls = []
    orig = pkg._abi.EngineGroup.rollout
    pkg._abi.EngineGroup.rollout = lambda self, *a, **k: (calls.append(a[0]), orig(self, *a, **k))[1]
    try:
        many_pols = S.solve_many([solver(k)[0] for k in range(3)], envs.SimpleGridWorld(n=4, seed=5))
    finally:
        pkg._abi.EngineGroup.rollout = orig
    assert calls == [24, 24]                                                  # one group call per block up to the next eval / log / save mark
    for k, pol in enumerate(many_pols):
        s, env = solver(k)
        one = S.solve(s, env)
        e, e1 = pol.engine, one.engine
        assert e.get_counters() == e1.get_counters() and e.get_counters()["train_steps"] == 12, k
        assert np.array_equal(e.get_params(0), e1.get_params(0)) and np.array_equal(e.get_params(1), e1.get_params(1)), k
        assert np.array_equal(e.replay_priorities(), e1.replay_priorities()), k
        for x, y in zip(e.envs_peek(), e1.envs_peek()):
            assert np.array_equal(x, y), k
        close_all(None, e, e1)
