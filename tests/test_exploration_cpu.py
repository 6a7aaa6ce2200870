"""CPU: exploration by table (dqn_rollout_explore) -- the ABI struct in header, ctypes and shim; the NumPy statement of the softmax law (tests/exploration_common.py)
and the package's own (solver.softmax_pick) against the fp64 softmax; SoftmaxPolicy on the host loop with the CPU twin engine; the lowering dqn_train_device uses;
and, on the twin's Q values, the choices the GPU tests rely on (the interior test's seed, the greedy test's parameter scale)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import exploration_common as XC
import ref
from test_shim_static_cpu import SHIM, julia_struct_layout

pkg = ge.load_package()
nn, envs, S = XC.load(pkg)
TC = XC.TC


def twin_engine(layers, hp, device=0):
    return ref.Twin(layers, hp, plan=None, threads=4)


def test_struct_layout_agrees_between_header_ctypes_and_shim_and_the_symbol_is_exported(tmp_path):
    abi = pkg._abi
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dqn_mi355x.h"\nint main(){printf("%zu %zu %zu %zu %d %d %d %zu %zu %zu\\n", sizeof(dqn_exploration), '
           'offsetof(dqn_exploration, kind), offsetof(dqn_exploration, n_values), offsetof(dqn_exploration, values), DQN_EXPLORE_EPS_GREEDY, DQN_EXPLORE_SOFTMAX, '
           'DQN_ENV_RAND_SOFTMAX, sizeof(dqn_rollout_cfg), sizeof(dqn_env_spec), sizeof(dqn_tabular_env));}')
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ge.ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    X = abi.Exploration
    assert got == [ctypes.sizeof(X), X.kind.offset, X.n_values.offset, X.values.offset, abi.EXPLORE_EPS_GREEDY, abi.EXPLORE_SOFTMAX, abi.ENV_RAND_SOFTMAX,
                   ctypes.sizeof(abi.RolloutCfg), ctypes.sizeof(abi.EnvSpec), ctypes.sizeof(abi.TabularEnv)]
    assert got[:4] == [16, 0, 4, 8] and got[7:] == [32, 152, 80]      # the existing structs keep their size
    assert XC.P_SOFTMAX == abi.ENV_RAND_SOFTMAX == 11
    text = open(SHIM).read()
    size, offsets = julia_struct_layout(text, "Exploration")
    assert size == ctypes.sizeof(X) and list(offsets) == [f[0] for f in X._fields_]
    for f, off in offsets.items():
        assert off == getattr(X, f).offset, f
    pkg.lib()
    assert "rollout_explore" in pkg.fns() and hasattr(pkg.lib(), "dqn_rollout_explore")


def test_shim_lowers_both_policies_to_the_new_entry_point():
    text = open(SHIM).read()
    assert "(:dqn_rollout_explore, LIB)" in text
    assert "exploration_table(p::POMDPTools.SoftmaxPolicy" in text and "p.temperature(t)" in text
    assert "exploration_table(p::POMDPTools.EpsGreedyPolicy" in text and "p.eps(t)" in text and "LinearDecaySchedule && return nothing" in text


LAWS = [("tests", XC.softmax_law32), ("package", S.softmax_pick)]


@pytest.mark.parametrize("which,law", LAWS)
def test_law_frequencies_match_the_fp64_softmax(which, law):
    """chi-square of 20 000 picks against the fp64 softmax probabilities at three temperatures.  Bound: dof + 4 sqrt(2 dof), the normal approximation's 4-sigma point
    (the generator's seed is fixed, so the test is deterministic)"""
    q = np.array([0.3, -0.2, 1.1, 0.5, 0.0], np.float32)
    rng = np.random.default_rng(5)
    for tau in (5.0, 1.0, 0.25):
        u = (rng.integers(0, 1 << 24, 20000).astype(np.float32) * np.float32(2.0 ** -24))      # the grid u01 draws from
        cnt = np.bincount([law(q, tau, x) for x in u], minlength=q.size)
        p = np.diff(XC.softmax_model64(q, tau))
        chi = float((((cnt - 20000 * p) ** 2) / (20000 * p)).sum())
        dof = q.size - 1
        assert chi <= dof + 4.0 * np.sqrt(2.0 * dof), (tau, chi, cnt)


@pytest.mark.parametrize("which,law", LAWS)
def test_law_zero_weights_fallback_and_exact_ends(which, law):
    # a weight that underflowed to zero (exp(-1000) in fp32) is never picked, wherever it sits
    grid = np.linspace(0.0, 1.0, 4097, dtype=np.float32)[:-1]
    for q, never in (([0.0, -1000.0, 0.0, -1000.0], {1, 3}), ([-1000.0, 0.5, 0.25, 0.5], {0}), ([1.0, 1.0, -999.0], {2})):
        got = {law(np.array(q, np.float32), 1.0, u) for u in grid} | {law(np.array(q, np.float32), 1.0, np.float32(1.0 - 2.0 ** -24))}
        assert not (got & never) and got == set(range(len(q))) - never, (q, got)
    # the fallback branch: target = u * c_last is not below c_last only for u = 1, which u01 never returns -- constructed here.  The pick is the last index at which c rose
    seen = {}
    assert XC.softmax_law32(np.array([0.0, 0.0, -1000.0], np.float32), 1.0, 1.0, seen) == 1 and seen.get("fallback")
    assert law(np.array([0.0, 0.0, -1000.0], np.float32), 1.0, 1.0) == 1
    assert law(np.array([-1000.0, 0.0, -1000.0], np.float32), 1.0, 1.0) == 1 and law(np.array([0.0, 0.0, 0.0], np.float32), 1.0, 1.0) == 2
    # tau = 1e30: every weight is exactly 1, c_k = k + 1, target = fp32(u * nA)
    rng = np.random.default_rng(2)
    for _ in range(200):
        q = (rng.standard_normal(4) * 3).astype(np.float32)
        u = np.float32(rng.integers(0, 1 << 24)) * np.float32(2.0 ** -24)
        z = q / np.float32(1e30)
        assert np.all(np.exp((z - z.max()).astype(np.float32)) == np.float32(1))
        want = next(k for k in range(4) if np.float32(u * np.float32(4)) < np.float32(k + 1))
        assert law(q, 1e30, u) == want == int(np.float32(u * np.float32(4)))
    # tau -> 0 with a clear margin: greedy
    assert all(law(np.array([0.1, 0.7, 0.3, -0.2], np.float32), 1e-3, u) == 1 for u in grid)


def test_the_two_statements_of_the_law_agree():
    rng = np.random.default_rng(9)
    for _ in range(2000):
        q = (rng.standard_normal(rng.integers(2, 7)) * 2).astype(np.float32)
        tau = np.float32(10.0 ** rng.uniform(-2, 2))
        u = np.float32(rng.integers(0, 1 << 24)) * np.float32(2.0 ** -24)
        assert XC.softmax_law32(q, tau, u) == S.softmax_pick(q, tau, u)


def host_policy(n=8):
    case = XC.wide_case(nn, n)
    tab = TC.wide_tables("goal")
    env = envs.TabularPOMDP(n=n, seed=0, discount=0.95, **tab.kwargs())
    e = TC.make_engine(pkg, nn, case, engine_cls=twin_engine)
    e.set_params(XC.noisy_params(nn, case["net"]), 0)
    return env, S.NNPolicy(env, e, list(range(4)), 1, qnetwork=case["net"]), e


def test_softmax_policy_on_the_host_loop():
    env, policy, e = host_policy()
    obs = env.observe()
    sched = lambda t: 2.0 * 0.5 ** (t / 10)
    a1 = S.SoftmaxPolicy(env, sched, rng=np.random.default_rng(4)).action(policy, 3, obs)
    a2 = S.SoftmaxPolicy(env, sched, rng=np.random.default_rng(4)).action(policy, 3, obs)
    assert a1.shape == (8,) and a1.min() >= 0 and a1.max() < 4
    np.testing.assert_array_equal(a1, a2)      # deterministic under a seeded rng
    q = policy.actionvalues(obs)
    u = np.random.default_rng(4).random(8, dtype=np.float32)
    np.testing.assert_array_equal(a1, [XC.softmax_law32(q[i], np.float32(sched(3)), u[i]) for i in range(8)])
    sp = S.SoftmaxPolicy(env, 0.5)
    assert sp.loginfo(7) == {"temperature": 0.5} and S.SoftmaxPolicy(env, sched).loginfo(10) == {"temperature": 1.0}
    np.testing.assert_array_equal(S.SoftmaxPolicy(env, 1e-4, rng=np.random.default_rng(0)).action(policy, 1, obs), policy.action(obs))      # cold: greedy
    with pytest.raises(pkg.DQNError, match=r"temperature\(2\) = 0.0 is not a finite positive number"):
        S.SoftmaxPolicy(env, lambda t: 0.0).action(policy, 2, obs)
    # the whole host loop with the twin engine
    solver = S.DeepQLearningSolver(qnetwork=nn.Chain(nn.Dense(8, 16, nn.relu), nn.Dense(16, 4)), max_steps=24, learning_rate=0.002, eval_freq=10 ** 6, train_freq=2, log_freq=8,
                                   exploration_policy=S.SoftmaxPolicy(env, sched, rng=np.random.default_rng(1)), target_update_freq=10, verbose=False, logdir=None,
                                   buffer_size=256, train_start=32, batch_size=8, max_episode_length=20)
    pol = S.solve(solver, env, engine_cls=twin_engine)
    assert pol.engine.get_counters()["train_steps"] == 12 and pol.engine.replay_size()[0] == 32 + 24 * 8


def test_lowering_of_exploration_policies_for_the_device_loop():
    """a LinearDecaySchedule or a number stays on the engine's own law (eps=...); any other callable eps and every SoftmaxPolicy becomes a per-step fp32 table"""
    env = envs.TabularPOMDP(n=2, **TC.wide_tables().kwargs())
    lin = S.exploration_table(S.EpsGreedyPolicy(env, S.LinearDecaySchedule(1.0, 0.1, 50.0)), 5, 4)
    assert lin == dict(eps=(1.0, 0.1, 50.0))
    assert S.exploration_table(S.EpsGreedyPolicy(env, 0.25), 5, 4) == dict(eps=(0.25, 0.25, 1.0))
    f = lambda t: 0.9 ** t
    kind, vals = S.exploration_table(S.EpsGreedyPolicy(env, f), 5, 4)["explore"]
    assert kind == "eps" and vals.dtype == np.float32
    np.testing.assert_array_equal(vals, np.array([f(5), f(6), f(7), f(8)], np.float32))
    kind, vals = S.exploration_table(S.SoftmaxPolicy(env, S.LinearDecaySchedule(2.0, 0.5, 10.0)), 9, 3)["explore"]
    assert kind == "softmax"
    np.testing.assert_array_equal(vals, np.array([0.65, 0.5, 0.5], np.float32))
    kind, vals = S.exploration_table(S.SoftmaxPolicy(env, 0.7), 1, 2)["explore"]
    np.testing.assert_array_equal(vals, np.array([0.7, 0.7], np.float32))


def test_interior_seed_keeps_draws_off_the_boundaries_on_the_twin():
    """the seed of the GPU interior test (XC.INTERIOR_SEED), simulated with the twin's Q values and the NumPy law: at most 1 % of the 512 draws lie within delta of a
    boundary of the fp64 model, every pick of the fp32 law is accepted, and each of the 4 actions is picked at least once per temperature >= 0.3"""
    case = XC.wide_case(nn, XC.INTERIOR_N)
    e = TC.make_engine(pkg, nn, case, engine_cls=twin_engine)
    e.set_params(XC.noisy_params(nn, case["net"]), 0)
    mir = TC.TabMirror(case["tab"], XC.INTERIOR_N, XC.INTERIOR_SEED)
    tally, ep = XC.InteriorTally(), np.zeros(XC.INTERIOR_N, np.int64)
    for t in range(1, XC.INTERIOR_STEPS + 1):
        tau, q = XC.interior_tau(t), e.forward(mir.observe())
        a = np.zeros(XC.INTERIOR_N, np.int32)
        for i in range(XC.INTERIOR_N):
            u = XC.u01(XC.philox(XC.INTERIOR_SEED, t, i, XC.P_SOFTMAX))
            a[i] = XC.softmax_law32(q[i], tau, u)
            assert tally.add(q[i], tau, u, a[i]), (t, i)
        _, d = mir.step(t, a)
        ep += 1
        ended = (d != 0) | (ep >= case["max_len"])
        mir.reset(ended, t); ep[ended] = 0
    assert tally.draws == 512 and tally.max_delta < 1e-4
    tally.check()


def test_greedy_scale_gives_every_state_a_clear_margin_on_the_twin():
    case = XC.wide_case(nn, 8)
    e = TC.make_engine(pkg, nn, case, engine_cls=twin_engine)
    e.set_params((XC.noisy_params(nn, case["net"]) * XC.GREEDY_SCALE).astype(np.float32), 0)
    q = np.sort(e.forward(case["tab"].features), axis=1)
    assert (q[:, -1] - q[:, -2]).min() > 0.2
