"""GPU: every device and pinned block the library allocates is owned by a scope (csrc/devmem.h) that some call releases -- read off the library's own live
counters (dqn_debug_devmem: exact, process-wide, blind to other tenants of the card).  Each case reads the counters, builds, exercises and destroys, and asserts
EXACT equality with the first reading.

Networks.  The smallest that reach each scope: Dense(4, 8, relu) -> Dense(8, 2) with B = 4 and buffer 64 wherever nothing below needs another shape.
  * An engine that gets a SimpleGridWorld has the grid's shape instead -- Dense(2, 8, relu) -> Dense(8, 4): dqn_envs_create refuses a GridWorld on any other
    (2 observation elements, 4 actions).  The recurrent case keeps LSTM(4, 8) -> Dense(8, 2) and steps a tabular MDP with 4 features and 2 actions, which also
    covers the table blocks (env_tab, env_term).
  * dqn_sim_ranks_step needs the gather exchange, i.e. a wide Dense layer and a batch that is a multiple of 32 (engine_program.hip, choose_dp_layers): the
    DQN_SIM_WORLD case uses the conv trunk + Dense(192, 512) dueling network of test_dp_gpu.py at B = 32.  (Under DQN_SIM_WORLD the 4 -> 8 -> 2 network builds a
    step with no exchange at all: no dp_* block would exist to be checked.)"""
import gc

import numpy as np
import pytest

import __graft_entry__ as ge
import dqn_oracle as O
import ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package()
    p.lib()
    return p


@pytest.fixture(scope="module")
def nn(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".nn")


@pytest.fixture(scope="module")
def envs(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".envs")


def devmem(pkg):
    return pkg._abi.debug_devmem(pkg.fns())


def baseline(pkg):
    """the first reading of a case: engines of earlier tests that only the collector can reach are destroyed now, not in the middle of the case"""
    gc.collect()
    return devmem(pkg)


def engine(pkg, nn, net, E, nA, B=4, cap=64, **hp_kw):
    layers, dueling = nn.lower(net)
    kw = dict(batch_size=B, n_actions=nA, obs_c=E, obs_h=1, obs_w=1, dueling=int(dueling), buffer_size=cap, learning_rate=1e-2, gamma=0.95, seed=3)
    kw.update(hp_kw)
    h = pkg.Engine(layers, pkg.default_hparams(**kw))
    p = nn.glorot_params(net, seed=3)
    h.set_params(p, 0); h.set_params(p, 1)
    return h


def fill(h, E, nA, n=64, seed=0):
    rng = np.random.default_rng(seed)
    h.replay_add(rng.random((n, E), dtype=np.float32), rng.integers(0, nA, n).astype(np.int32), rng.standard_normal(n).astype(np.float32),
                 rng.random((n, E), dtype=np.float32), (rng.random(n) < 0.2).astype(np.uint8))


def grid_net(nn):
    return nn.Chain(nn.Dense(2, 8, nn.relu), nn.Dense(8, 4))


def test_feed_forward_engine_returns_every_block(pkg, nn, envs):
    first = baseline(pkg)
    h = engine(pkg, nn, grid_net(nn), 2, 4)
    assert devmem(pkg)[0] > first[0] and devmem(pkg)[1] > first[1]      # the counters see the engine
    fill(h, 2, 4)
    h.train_step(); h.train_steps(3)
    rng = np.random.default_rng(1)
    assert h.forward(rng.random((3, 2), dtype=np.float32)).shape == (3, 4)
    assert h.forward(rng.random((9, 2), dtype=np.float32)).shape == (9, 4)      # regrows policy_ws, drops the acting programs
    h.envs_create(envs.SimpleGridWorld(), n_envs=4, max_episode_length=20, seed=5)
    h.envs_create(envs.SimpleGridWorld(), n_envs=4, max_episode_length=20, seed=6)      # the second call replaces the set
    h.rollout(6)
    h.rollout(6, t0=7, explore=("softmax", np.linspace(1.0, 0.5, 6)))      # builds act_gen (where act has the fused tail) and xtab
    h.evaluate(4, max_episode_length=20, seed=1)
    h.evaluate(8, max_episode_length=20, seed=1)      # reallocates the evaluation set
    h.close()
    assert devmem(pkg) == first


def wide_dense_dueling():
    b, v, a = O.create_dueling_network([O.Conv(4, 3, 8, O.ACT_RELU, 2), O.Conv(3, 8, 16, O.ACT_RELU, 1), O.Dense(16 * 3 * 4, 512, O.ACT_RELU), O.Dense(512, 5, O.ACT_IDENTITY)])
    return O.Network((3, 12, 14), b, v, a)


def test_simulated_ranks_engine_returns_every_block(pkg, monkeypatch):
    first = baseline(pkg)
    net = wide_dense_dueling()
    layers = ref.layers_from_network(net)
    hp = ref.hparams_for(net, batch_size=32, buffer_size=64, learning_rate=1e-3, gamma=0.99)
    monkeypatch.setenv("DQN_SIM_WORLD", "2")
    h = pkg.Engine(layers, hp)
    monkeypatch.delenv("DQN_SIM_WORLD")
    rng = np.random.default_rng(2)
    h.replay_add(rng.random((64,) + net.obs_shape, dtype=np.float32), rng.integers(0, net.n_actions, 64).astype(np.int32), rng.standard_normal(64).astype(np.float32),
                 rng.random((64,) + net.obs_shape, dtype=np.float32), (rng.random(64) < 0.2).astype(np.uint8))
    p = O.Network.flatten(O.init_params(net, seed=5)).astype(np.float32)
    h.set_params(p, 0); h.set_params(p, 1)
    loss, gn, td = h.sim_ranks_step(rng.choice(64, (2, 32), replace=False).astype(np.int64))      # the dp_* and sim_* blocks
    assert loss.shape == (2,) and np.all(np.isfinite(loss)) and td.shape == (2, 32)
    assert h.comm_exchange_bytes() > 0
    h.close()
    assert devmem(pkg) == first


def test_recurrent_engine_returns_every_block(pkg, nn):
    first = baseline(pkg)
    net = nn.Chain(nn.LSTM(4, 8), nn.Dense(8, 2))
    h = engine(pkg, nn, net, 4, 2, recurrence=1, trace_length=4, prioritized_replay=0)
    rng = np.random.default_rng(3)
    for _ in range(4):
        h.episode_add(rng.random((3, 4), dtype=np.float32), rng.integers(0, 2, 3).astype(np.int32), rng.standard_normal(3).astype(np.float32),
                      rng.random((3, 4), dtype=np.float32), np.zeros(3, np.uint8))
        h.episode_commit()
    assert h.episode_count()[0] == 4
    loss, _ = h.train_step_drqn()
    assert np.isfinite(loss)
    h.reset_state()
    assert h.forward(rng.random((1, 4), dtype=np.float32)).shape == (1, 2)
    assert h.forward(rng.random((3, 4), dtype=np.float32)).shape == (3, 2)      # reallocates policy_state
    # a three-state MDP with four features and two actions: state 2 is terminal
    T = np.zeros((3, 2, 3), np.float32); T[0, 0] = [0.5, 0.5, 0.0]; T[0, 1] = [0.0, 0.5, 0.5]; T[1, 0] = [0.5, 0.0, 0.5]; T[1, 1] = [0.0, 0.0, 1.0]
    R = rng.standard_normal((3, 2, 3)).astype(np.float32)
    h.envs_create_tabular(T, R, np.array([0, 0, 1], np.uint8), np.array([0.5, 0.5, 0.0], np.float32), rng.random((3, 4), dtype=np.float32), n_envs=4, max_episode_length=6, seed=4)
    h.rollout(8)
    h.evaluate(4, max_episode_length=6, seed=2)
    h.close()
    assert devmem(pkg) == first


def test_group_returns_every_block_and_guards_its_members(pkg, nn, envs):
    first = baseline(pkg)
    members = [engine(pkg, nn, grid_net(nn), 2, 4, seed=3 + k) for k in range(2)]
    for k, h in enumerate(members):
        fill(h, 2, 4, seed=k)
        h.envs_create(envs.SimpleGridWorld(), n_envs=4, max_episode_length=20, seed=7 + k)
    g = pkg._abi.EngineGroup(members)
    g.train_steps(2)
    g.rollout(4, explore=[("softmax", np.linspace(1.0, 0.5, 4)), None])      # one member on a table
    g.evaluate(4, 20, [1, 2])
    g.evaluate(8, 20, [1, 2])
    live = devmem(pkg)
    with pytest.raises(pkg.DQNError, match="member of 1 live group"):
        members[0].close()      # refused while the group lives ...
    assert devmem(pkg) == live      # ... and nothing moved
    g.close()
    for h in members:
        h.close()
    assert devmem(pkg) == first


@pytest.mark.parametrize("trace_length,u8,msg", [(20000, False, "trace_length 20000 unsupported"),      # T * B = 80000 > 65536
                                                 (4, True, "u8 is not supported with recurrence")])
def test_refused_create_returns_every_block(pkg, nn, trace_length, u8, msg):
    """both are refused inside engine_init, behind its streams and events: dqn_engine_create then runs the destroy path over the half-made engine"""
    first = baseline(pkg)
    with pytest.raises(pkg.DQNError, match=msg):
        engine(pkg, nn, nn.Chain(nn.LSTM(4, 8), nn.Dense(8, 2)), 4, 2, recurrence=1, trace_length=trace_length, prioritized_replay=0,
               obs_dtype=pkg.OBS_U8 if u8 else pkg.OBS_F32)
    assert devmem(pkg) == first
