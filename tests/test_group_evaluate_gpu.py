"""GPU (-m gpu): grouped evaluation through the C ABI (dqn_evaluate_many, include/dqn_mi355x.h; tiny_eval.hip).  THE LAW: avg_reward[k] and avg_steps[k] are bit for
bit the doubles dqn_evaluate(member_k, n_eval, max_episode_length, seeds[k]) returns on a twin-constructed standalone engine, and member k is left as that call
leaves it.  Every comparison is == on the doubles or np.array_equal; nothing here has a tolerance."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import __graft_entry__ as ge
from group_evaluate_common import (LENGTHS, N_EVALS, assert_same, build_member, build_pair, long_mdp_spec, member_specs, one_tile_floats, seeds_for, still,
                                   tiger_spec, warm, wide_spec)
from group_rollout_common import TARGET_FREQ, TRAIN_FREQ, observables, replay_rows

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


def pairs(specs, pkg, envs):
    built = [build_pair(s, pkg, envs) for s in specs]
    return [m for m, _ in built], [a for _, a in built]


def alone_eval(alone, n_eval, length, seeds):
    return [h.evaluate(n_eval, length, seed=sd) for h, sd in zip(alone, seeds)]


@pytest.fixture(scope="module")
def hetero(pkg, envs):
    """built ONCE, read by several tests: group_rollout_common's six members in a group and their standalone references, all WARM_STEPS train steps in"""
    specs = list(member_specs().values())
    members, alone = pairs(specs, pkg, envs)
    group = pkg.EngineGroup(members)
    p0 = [h.get_params(0) for h in members]
    warm(group, alone)
    for h, a, p in zip(members, alone, p0):      # trained, and the references with them
        assert np.array_equal(h.get_params(0), a.get_params(0)) and not np.array_equal(h.get_params(0), p)
    yield dict(names=list(member_specs()), specs=specs, group=group, members=members, alone=alone)
    close_all(group, *members, *alone)


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("n_eval", N_EVALS)
def test_heterogeneous_group_returns_the_standalone_doubles(hetero, n_eval, length):
    seeds = seeds_for(6, n_eval, length)
    got = hetero["group"].evaluate(n_eval, length, seeds)
    want = alone_eval(hetero["alone"], n_eval, length, seeds)
    print("n_eval", n_eval, "L", length, got)
    for k, name in enumerate(hetero["names"]):
        assert got[k] == want[k], (name, got[k], want[k])
    assert len({g for g in got}) > 1      # the members do not all return the same pair: each ran its own network, env and seed


def test_launch_boundaries_with_copies_that_cannot_end_early(pkg, envs, hetero):
    """max_episode_length around the step bound B of one launch, on members whose episodes end at max_episode_length alone: every copy is alive across the boundary"""
    tiger_m, tiger_a = build_pair(tiger_spec(), pkg, envs)
    one = pkg.EngineGroup([tiger_m])
    _, B, _ = one.evaluate_info(5, 1)
    assert B >= 2
    mdp_m, mdp_a = build_pair(long_mdp_spec(2 * B + 8), pkg, envs)
    two = pkg.EngineGroup([tiger_m, mdp_m])
    warm(two, [tiger_a, mdp_a])
    for L in (B - 1, B, B + 1, 2 * B + 3):
        want_launches = math.ceil((L + 1) / B)
        assert one.evaluate_info(5, L)[0] == want_launches == hetero["group"].evaluate_info(5, L)[0], L      # K = 1 and K = 6 alike
        seeds = seeds_for(2, 5, L)
        got = two.evaluate(5, L, seeds)
        want = alone_eval([tiger_a, mdp_a], 5, L, seeds)
        print("L", L, got)
        assert got == want, (L, got, want)
        assert [s for _, s in got] == [float(L + 1)] * 2, (L, got)      # no copy ended before max_episode_length: the boundary was crossed with live copies
        assert one.evaluate(5, L, seeds[:1]) == want[:1], L
    close_all(one); close_all(two, tiger_m, tiger_a, mdp_m, mdp_a)


def test_tiles_a_wide_member_at_1024_copies_and_a_ragged_last_tile(pkg, envs):
    """a member near the parameter limit of a group: its copies do not fit LDS beside its parameters, the forward runs tile by tile"""
    refused = build_member(wide_spec(96), pkg, envs)
    with pytest.raises(pkg.DQNError, match=r"member 0 does not take the single-workgroup step: it needs \d+ bytes of LDS"):
        pkg.EngineGroup([refused])      # (13 156 parameters: three parameter-sized arrays of the TRAIN step exceed its LDS -- group_evaluate_common.wide_spec)
    refused.close()
    m, a = build_pair(wide_spec(80), pkg, envs)
    g = pkg.EngineGroup([m])
    warm(g, [a], 2)
    P = m.P
    assert P == 11028
    _, _, lds = g.evaluate_info(1024, 5)
    per_copy = one_tile_floats(80, 1)
    tile = (lds // 4 - (P + 3) // 4 * 4 - 3 * 1024) // per_copy
    assert 4 <= tile < 1024 and tile % 4 == 0 and lds < 4 * one_tile_floats(80, 1024), (lds, tile)      # more than one tile
    for n_eval in (1024, 3 * tile + 2):      # full tiles; a ragged last tile of width 2
        lds_n = g.evaluate_info(n_eval, 5)[2]
        assert lds_n < 4 * (P + one_tile_floats(80, n_eval)), (n_eval, lds_n)
        got = g.evaluate(n_eval, 5, [77 + n_eval])
        want = alone_eval([a], n_eval, 5, [77 + n_eval])
        print("n_eval", n_eval, "tile", tile, got)
        assert got == want, (n_eval, got, want)
    close_all(g, m, a)


def test_episodes_that_end_at_different_steps(hetero):
    """GridWorld, 100 copies: the episodes end at different steps (a reward cell is terminal, the rest run into max_episode_length), finished copies idle beside live ones"""
    k = hetero["names"].index("grid")
    seeds = seeds_for(6, 100, 30)
    got = hetero["group"].evaluate(100, 30, seeds)[k]
    want = hetero["alone"][k].evaluate(100, 30, seed=seeds[k])
    print(got)
    assert got == want
    assert got[1] != math.floor(got[1]) and 1.0 < got[1] < 31.0, got


def test_nothing_else_moves(pkg, envs):
    specs = list(member_specs().values())
    members, twins = pairs(specs, pkg, envs)
    g, g2 = pkg.EngineGroup(members), pkg.EngineGroup(twins)

    def roll(group, t0):
        return group.rollout(4, t0=t0, train_freq=TRAIN_FREQ, target_update_freq=TARGET_FREQ, eps=[s["eps"] for s in specs])

    for group in (g, g2):
        roll(group, 1); group.train_steps(2)
    before = [still(h) for h in members]
    seeds = seeds_for(6, 37, 7)
    first = g.evaluate(37, 7, seeds)
    for k, h in enumerate(members):
        assert_same(still(h), before[k], "member %d after evaluate_many" % k)
        with pytest.raises(pkg.DQNError, match=r"dqn_envs_peek_q: the env set has not taken a vector step since it was created, or the policy workspace was used"):
            h.envs_peek_q()
    assert g.evaluate(37, 7, seeds) == first      # the same seeds, the same doubles
    # the sequence with an evaluation in the middle ends where the sequence without it ends
    for group in (g, g2):
        st = roll(group, 5); group.train_steps(1)
        if group is g:
            st_g = st
    for k, (h, h2) in enumerate(zip(members, twins)):
        assert_same(observables(h, st_g[k]), observables(h2, st[k]), "member %d: rollout + train around evaluate_many" % k)
    close_all(g, *members); close_all(g2, *twins)


def test_stream_order_needs_no_host_synchronise(pkg, envs):
    """evaluate_many directly behind a group train step and member-side replay_add calls, with no host synchronise, returns what it returns after one"""
    specs = [member_specs()[n] for n in ("grid", "plain")]
    out = []
    for explicit_sync in (False, True):
        members = [build_member(s, pkg, envs) for s in specs]
        g = pkg.EngineGroup(members)
        g.train_steps(1)
        for h, s in zip(members, specs):
            h.replay_add(*replay_rows(s, n=4, seed=1))
        g.train_steps(1)
        if explicit_sync:
            for h in members:
                h.sync()
        out.append(g.evaluate(37, 7, [5, 6]))
        close_all(g, *members)
    print(out)
    assert out[0] == out[1]


def test_refusals_by_message_and_the_group_lives_on(pkg, envs):
    from engine_group_common import build as build_no_env, member_specs as no_env_specs
    spec = member_specs()["plain"]
    m, a = build_pair(spec, pkg, envs)
    g = pkg.EngineGroup([m])
    f = m.f
    K1 = (ctypes.c_uint64 * 1)(3)
    r, s = ctypes.c_double(), ctypes.c_double()

    def refused(rc, pattern):
        assert rc != 0
        msg = f["last_error"]().decode()
        assert pattern in msg, msg

    refused(f["evaluate_many"](None, 4, 5, K1, ctypes.byref(r), ctypes.byref(s)), "null group handle")
    refused(f["evaluate_many_info"](None, 4, 5, None, None, None), "null group handle")
    for bad in (0, 1025, -3):
        refused(f["evaluate_many"](g._g, bad, 5, K1, ctypes.byref(r), ctypes.byref(s)), "dqn_evaluate_many: n_eval = %d is outside 1..1024" % bad)
        refused(f["evaluate_many_info"](g._g, bad, 5, None, None, None), "dqn_evaluate_many_info: n_eval = %d is outside 1..1024" % bad)
    refused(f["evaluate_many"](g._g, 4, 0, K1, ctypes.byref(r), ctypes.byref(s)), "dqn_evaluate_many: max_episode_length = 0, at least 1 is needed")
    refused(f["evaluate_many"](g._g, 4, 5, None, ctypes.byref(r), ctypes.byref(s)), "dqn_evaluate_many: seeds is NULL")
    refused(f["evaluate_many"](g._g, 4, 5, K1, None, None), "dqn_evaluate_many: avg_reward and avg_steps are both NULL")
    with pytest.raises(pkg.DQNError, match="EngineGroup.evaluate: 2 seeds were given for 1 members"):
        g.evaluate(4, 5, [1, 2])
    # a member without device environments, by index
    bare = build_no_env(no_env_specs()["a"], pkg.Engine, pkg.default_plan)
    g2 = pkg.EngineGroup([m, bare])
    for call in (lambda: g2.evaluate(4, 5, [1, 2]), lambda: g2.evaluate_info(4, 5)):
        with pytest.raises(pkg.DQNError, match=r"member 1 does not take the single-workgroup evaluation: it has no device environments"):
            call()
    g2.close(); bare.close()
    # nothing was changed: the group still steps and evaluates as the standalone engine does; one output may be NULL
    warm(g, [a], 1)
    assert g.evaluate(4, 5, [3]) == [a.evaluate(4, 5, seed=3)]
    assert f["evaluate_many"](g._g, 4, 5, K1, ctypes.byref(r), None) == 0 and r.value == a.evaluate(4, 5, seed=3)[0]
    assert np.array_equal(m.get_params(0), a.get_params(0))
    close_all(g, m, a)


def test_solve_many_evaluates_through_the_group(pkg, monkeypatch):
    """solve_many's eval marks: ONE EngineGroup.evaluate per mark for the members that keep basic_evaluation (Engine.evaluate is never called), a member with its own
    evaluation_policy keeps calling it; parameters and every mark's scores equal those of three separate solve calls"""
    S, nn, envs_m = (importlib.import_module(pkg.__name__ + "." + m) for m in ("solver", "nn", "envs"))
    abi = pkg._abi

    def solver(k, **over):
        env = envs_m.SimpleGridWorld(n=4, seed=5)
        model = nn.Chain(nn.Dense(2, 16, nn.relu), nn.Dense(16, env.n_actions))
        expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.1, steps=40))
        kw = dict(qnetwork=model, exploration_policy=expl, max_steps=48, train_freq=4, target_update_freq=16, train_start=8, batch_size=8, buffer_size=64, eval_freq=12,
                  num_ep_eval=10, max_episode_length=20, log_freq=24, logdir=None, verbose=False, device_envs=True, seed=100 + k, learning_rate=1e-3 * (k + 1),
                  rng=np.random.default_rng(9))
        kw.update(over)
        return S.DeepQLearningSolver(**kw), env

    # the references: three separate solve calls, every Engine.evaluate recorded
    alone_scores, real_evaluate = [[] for _ in range(3)], abi.Handle.evaluate
    alone_params = []
    for k in range(3):
        def recording(self, *a, _k=k, **kw):
            out = real_evaluate(self, *a, **kw)
            alone_scores[_k].append(out)
            return out
        monkeypatch.setattr(abi.Handle, "evaluate", recording)
        s, env = solver(k)
        one = S.solve(s, env)
        alone_params.append((one.engine.get_params(0), one.engine.get_params(1), one.engine.get_counters()))
        one.engine.close()
    assert all(len(sc) == 4 for sc in alone_scores)      # marks at 12, 24, 36, 48

    def refuse(self, *a, **kw):
        raise AssertionError("Engine.evaluate was called under solve_many")
    monkeypatch.setattr(abi.Handle, "evaluate", refuse)
    group_calls, real_group_evaluate = [], abi.EngineGroup.evaluate

    def group_recording(self, *a, **kw):
        out = real_group_evaluate(self, *a, **kw)
        group_calls.append(out)
        return out
    monkeypatch.setattr(abi.EngineGroup, "evaluate", group_recording)
    many = S.solve_many([solver(k)[0] for k in range(3)], envs_m.SimpleGridWorld(n=4, seed=5))
    assert len(group_calls) == 4
    for k, pol in enumerate(many):
        e = pol.engine
        assert [c[k] for c in group_calls] == alone_scores[k], k
        assert pol.scores_eval == alone_scores[k][-1][0], k
        assert np.array_equal(e.get_params(0), alone_params[k][0]) and np.array_equal(e.get_params(1), alone_params[k][1]) and e.get_counters() == alone_params[k][2], k
        e.close()
    # a member with its own evaluation policy: that policy is called at every mark, the others are grouped
    own_calls = []

    def own_policy(policy, env, n_eval, max_episode_length, verbose):
        own_calls.append((n_eval, max_episode_length))
        return -1.5, 0, 0
    del group_calls[:]
    solvers = [solver(0)[0], solver(1, evaluation_policy=own_policy, num_ep_eval=3)[0], solver(2)[0]]
    many = S.solve_many(solvers, envs_m.SimpleGridWorld(n=4, seed=5))
    assert own_calls == [(3, 20)] * 4 and len(group_calls) == 4
    assert many[1].scores_eval == -1.5
    for k in (0, 2):
        assert [c[k] for c in group_calls] == alone_scores[k] and np.array_equal(many[k].engine.get_params(0), alone_params[k][0]), k
    assert np.array_equal(many[1].engine.get_params(0), alone_params[1][0])      # evaluation does not touch training
    for pol in many:
        pol.engine.close()
