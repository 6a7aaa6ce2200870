"""CPU: tabular (PO)MDP environments -- the NumPy model of the sampling law (tests/tabular_envs_common.py) against its own tables, the env seeds the GPU tests use,
the host classes envs.TabularPOMDP / envs.TigerPOMDP, the ABI struct, and the reference's "TigerPOMDP DDRQN" test set (test/runtests.jl:149-163) through the host
loop on the twin engine."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import ref
import tabular_envs_common as TC
from test_shim_static_cpu import SHIM, julia_struct_layout

pkg = ge.load_package()
nn, envs, S = TC.load(pkg)


def twin_engine(layers, hp, device=0):
    return ref.Twin(layers, hp, plan=None, threads=4)


@pytest.mark.parametrize("name", ["tiger", "sparse", "wide_mdp"])
def test_cumulative_rows_are_non_decreasing_and_keep_zero_entries_flat(name):
    tab = TC.cases(nn)[name]["tab"]
    for p, c in ((tab.T, tab.cT), (tab.b0, tab.cb0)) + (((tab.Z, tab.cZ), (tab.Z0, tab.cZ0)) if tab.O else ()):
        assert c.dtype == np.float32 and np.all(np.diff(c, axis=-1) >= 0) and np.all(c[..., 0] == p[..., 0])
        assert np.all((np.diff(c, axis=-1) == 0) == (p[..., 1:] == 0))      # a zero entry never widens its interval, a positive one always does (at these sizes)


def test_sparse_frequencies_match_the_tables():
    """chi-square of the model's draws on `sparse` at a fixed seed (5 copies, 3000 vector steps under eps = 1) against the tables, over every row drawn from at least
    200 times.  The expected probabilities are the table's, with what a row lacks to 1 (the 0.9990 rows) given to its last positive entry, where the fallback puts
    it.  Bound: dof + 4 sqrt(2 dof), the normal approximation's 4-sigma point (chance about 3e-5 for a correct sampler; the seed is fixed, so the test is
    deterministic).  Entries of probability zero are never drawn."""
    c = TC.cases(nn)["sparse"]
    ls, _, _ = TC.simulate("sparse", nn, seed=5, steps=3000)
    tab, cnt = c["tab"], ls.mirror.counts
    chi, dof, rows = 0.0, 0, 0
    for name, p in (("T", tab.T), ("Z", tab.Z), ("Z0", tab.Z0), ("b0", tab.b0[None])):
        k = cnt[name].reshape(-1, p.shape[-1]) if name != "b0" else cnt[name][None]
        p = p.reshape(-1, p.shape[-1]).astype(np.float64)
        assert np.all(k[p == 0] == 0), name
        for row_p, row_k in zip(p, k):
            if row_k.sum() < 200:
                continue
            q = row_p.copy()
            q[np.nonzero(q)[0][-1]] += 1.0 - q.sum()
            pos = q > 0
            chi += float((((row_k[pos] - row_k.sum() * q[pos]) ** 2) / (row_k.sum() * q[pos])).sum())
            dof += int(pos.sum()) - 1
            rows += 1
    assert rows >= 12 and dof >= 12
    assert chi <= dof + 4.0 * np.sqrt(2.0 * dof), (chi, dof)
    assert ls.mirror.seen["fallback"]


@pytest.mark.parametrize("name", ["tiger", "sparse", "wide_mdp"])
def test_env_seeds_reach_every_named_branch(name):
    """the seeds of TC.ENV_SEED under eps = 1 within TC.STEPS: the fallback pick, a zero-probability neighbour on each side of a pick, the first and the last index,
    ring wrap, two finishers in one step, an episode open across a truncation (what applies to the case: TC.WANT)"""
    ls, flags, first_batch = TC.simulate(name, nn)
    for k in TC.WANT[name]:
        assert flags[k], (k, flags)
    if name in TC.WARM:
        assert first_batch == TC.WARM[name]
    if name == "tiger":
        assert ls.model.size == 0      # no terminal state: the training loop never commits an episode


def test_tiger_tables_equal_the_recalled_model():
    env = envs.TigerPOMDP(0.01, -1.0, 0.1, 0.8, 0.95, n=2, seed=3)
    assert (env.n_states, env.n_actions, env.n_obs, env.obs_shape, env.discount) == (2, 3, 2, (1,), 0.95)
    want = TC.tiger_tables(0.01, -1.0, 0.1, 0.8)
    for k in ("T", "Z", "Z0", "R", "terminal", "b0", "features"):
        np.testing.assert_array_equal(getattr(env, k), getattr(want, k), err_msg=k)
    for p in (env.T, env.Z, env.Z0, env.b0[None]):
        np.testing.assert_allclose(p.astype(np.float64).sum(-1), 1.0, atol=1e-6)
    # entry by entry, from the model's words: listening keeps the state and reports the side with p_listen_correctly; opening re-draws both uniformly
    d = envs.TigerPOMDP()
    assert (d.r_listen, d.r_findtiger, d.r_escapetiger, d.p_listen_correctly, d.discount) == (-1.0, -100.0, 10.0, 0.85, 0.95)
    for s in range(2):
        assert d.T[s, 0, s] == 1 and d.T[s, 0, 1 - s] == 0 and d.Z[0, s, s] == np.float32(0.85) and d.Z[0, s, 1 - s] == np.float32(1.0 - 0.85)
        assert np.all(d.T[s, 1:] == 0.5) and np.all(d.Z[1:, s] == 0.5) and np.all(d.R[s, 0] == -1.0)
    assert np.all(d.R[1, 1] == -100.0) and np.all(d.R[0, 1] == 10.0) and np.all(d.R[0, 2] == -100.0) and np.all(d.R[1, 2] == 10.0)      # state 1: the tiger is left
    assert not d.terminal.any() and np.all(d.b0 == 0.5) and np.array_equal(d.Z0, d.Z[0]) and np.array_equal(d.features, [[0.0], [1.0]])


def test_host_class_steps_the_tables():
    """interface of the two existing host classes; an entry of probability zero is never drawn; terminal states end episodes; reset(mask) touches the masked copies only"""
    tab = TC.sparse_tables()
    env = envs.TabularPOMDP(n=64, seed=2, **tab.kwargs())
    assert (env.n_actions, env.obs_shape, env.n) == (3, (6,), 64)
    rng = np.random.default_rng(0)
    for _ in range(200):
        s, a = env.s.copy(), rng.integers(0, 3, 64)
        r = env.act(a)
        assert r.dtype == np.float32 and np.all(tab.T[s, a, env.s] > 0) and np.all(tab.Z[a, env.s, env.o] > 0)
        np.testing.assert_array_equal(r, tab.R[s, a, env.s]); np.testing.assert_array_equal(env.terminated(), tab.terminal[env.s] != 0)
        np.testing.assert_array_equal(env.observe(), tab.features[env.o])
        keep = ~env.terminated()
        before = (env.s.copy(), env.o.copy())
        env.reset(env.terminated().copy())
        assert np.all(env.s[keep] == before[0][keep]) and np.all(env.o[keep] == before[1][keep]) and not env.terminated().any()
        assert np.all(tab.b0[env.s[~keep]] > 0) and np.all(tab.Z0[env.s[~keep], env.o[~keep]] > 0)
    mdp = envs.TabularPOMDP(n=4, **TC.wide_tables().kwargs())
    mdp.act(np.zeros(4, np.int64))
    assert mdp.n_obs == 0 and np.array_equal(mdp.o, mdp.s) and mdp.observe().shape == (4, 8)


def test_python_side_refusals():
    k = TC.sparse_tables().kwargs()
    def bad(match, **chg):
        with pytest.raises(ValueError, match=match):
            envs.TabularPOMDP(**{**k, **chg})
    bad(r"T has shape", T=k["T"][:, :, :4])
    bad(r"R has shape", R=k["R"][:, :2])
    bad(r"Z has shape", Z=k["Z"][:, :4])
    bad(r"Z0 has shape", Z0=k["Z0"][:4])
    bad(r"b0 has shape", b0=k["b0"][:4])
    bad(r"features has shape", features=k["features"][:2])
    bad(r"Z and Z0 come together", Z0=None)
    T = k["T"].copy(); T[0, 0, 0] += 0.1; T[0, 0, 2] -= 0.4
    bad(r"T has a negative", T=T)
    T = k["T"].copy(); T[2, 1, 0] += 0.002
    bad(r"row T\[2\]\[1\] sums to 1\.002", T=T)
    Z = k["Z"].copy(); Z[1, 1, 0] -= 0.002
    bad(r"row Z\[1\]\[1\] sums to 0\.998", Z=Z)
    Z0 = k["Z0"].copy(); Z0[2, 0] -= 0.002
    bad(r"row Z0\[2\] sums to 0\.998", Z0=Z0)
    b0 = k["b0"].copy(); b0[0] += 0.003      # 0.9990 + 0.003
    bad(r"row b0 sums to 1\.002", b0=b0)
    b0 = k["b0"].copy(); b0[0] = np.nan
    bad(r"b0 has a negative or non-finite", b0=b0)
    T = k["T"].copy(); T[4] = 0.0      # a terminal state's rows are exempt
    env = envs.TabularPOMDP(**{**k, "T": T, "b0": np.array([0, 0, 0, 0, 1], np.float32)}, n=6)
    env.act(np.arange(6) % 3)      # an all-zero row picks index 0, as the device law does
    assert np.all(env.s == 0)


def test_struct_sizes_agree_between_ctypes_header_and_shim(tmp_path):
    abi = pkg._abi
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dqn_mi355x.h"\nint main(){printf("%zu %zu %zu %zu %zu %d\\n", sizeof(dqn_tabular_env), '
           'offsetof(dqn_tabular_env, n_states), offsetof(dqn_tabular_env, T), offsetof(dqn_tabular_env, features), sizeof(dqn_env_spec), DQN_ENV_TABULAR);}')
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ge.ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [ctypes.sizeof(abi.TabularEnv), abi.TabularEnv.n_states.offset, abi.TabularEnv.T.offset, abi.TabularEnv.features.offset, ctypes.sizeof(abi.EnvSpec), abi.ENV_TABULAR]
    size, offsets = julia_struct_layout(open(SHIM).read(), "TabularEnv")
    assert size == ctypes.sizeof(abi.TabularEnv) and list(offsets) == [f[0] for f in abi.TabularEnv._fields_]
    for f, off in offsets.items():
        assert off == getattr(abi.TabularEnv, f).offset, f
    assert "(:dqn_envs_create_tabular, LIB)" in open(SHIM).read()


def test_tiger_ddrqn_host_loop_on_the_twin():
    """test/runtests.jl:149-163 with fewer steps: TigerPOMDP(0.01, -1.0, 0.1, 0.8, 0.95), LSTM(1, 4) -> Dense(4, 3), recurrence, trace_length 10, dueling, double-Q,
    max_episode_length 100, target_update_freq 1000; the set's only assertion is the shape of actionvalues"""
    env = envs.TigerPOMDP(0.01, -1.0, 0.1, 0.8, 0.95, n=1, seed=1)
    model = nn.Chain(nn.flattenbatch, nn.LSTM(1, 4), nn.Dense(4, env.n_actions))
    max_steps = 300
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.01, steps=max_steps / 2), rng=np.random.default_rng(1))
    solver = S.DeepQLearningSolver(qnetwork=model, prioritized_replay=False, max_steps=max_steps, learning_rate=0.0001, exploration_policy=expl, log_freq=500,
                                   target_update_freq=1000, recurrence=True, trace_length=10, double_q=True, dueling=True, max_episode_length=100,
                                   train_start=8, buffer_size=16, batch_size=4, eval_freq=10 ** 6, verbose=False, logdir=None)
    policy = S.solve(solver, env, engine_cls=twin_engine)
    assert policy.actionvalues(env.observe()[0]).shape == (env.n_actions,)
    assert policy.engine.episode_count()[0] == 8      # the training loop commits nothing (no terminal state): the prefill is all the replay holds
