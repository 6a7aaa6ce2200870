"""CPU: the pieces of the recurrent device-environment loop that need no GPU -- the NumPy ring model (the reference of the GPU tests) against the twin's host path
for one stream, the seeds' coverage on that model, dqn_train's routing by the engine's capability flag, and what the header promises."""
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import recurrent_envs_common as RC
import ref

pkg = ge.load_package()
nn, envs, S = RC.load(pkg)


def twin_cls(layers, hp):
    return ref.Twin(layers, hp, plan=None, threads=2)


def test_ring_model_for_one_stream_equals_the_twins_host_path():
    """the same transitions through Twin.episode_add and through the model with n = 1: an episode longer than T, one shorter, a truncation without `done` (the episode
    stays open across it), and a wrapped ring.  Compared wherever no episode is open on the host side (the host path writes an open episode straight into its slot)."""
    spec, net, n, T, cap, B, max_len = RC.cases(nn, envs)["lstm"]
    twin, _ = RC.make_engine(pkg, nn, (spec, net, 1, T, cap, B, max_len), engine_cls=twin_cls)
    model = RC.RingModel(1, T, cap, spec.obs_shape)
    rng = np.random.default_rng(2)
    lengths = [T + 3, 2, T, 1, T + 1, 3, 2, T + 2]      # 8 episodes into 5 slots
    for k, L in enumerate(lengths):
        for t in range(L):
            s, sp = rng.random((1,) + spec.obs_shape, dtype=np.float32), rng.random((1,) + spec.obs_shape, dtype=np.float32)
            a, r, d = rng.integers(0, 4, 1).astype(np.int32), rng.standard_normal(1).astype(np.float32), np.array([t == L - 1], np.uint8)
            twin.episode_add(s, a, r, sp, d)
            model.add(s, a, r, sp, d)
            if k == 2 and t == 1:
                model.note_truncated(0)      # an env reset by length here changes nothing in either
        model.check(twin, counters=False)
    assert model.seen["wrap"] and model.seen["prefix"] and model.seen["short"] and model.seen["open_across_reset"]
    np.testing.assert_array_equal(twin.episode_export()[5], np.array([3, 2, T + 2, 1, T + 1], np.int32))      # the TRUE lengths, ring order


@pytest.mark.parametrize("name,want", [("lstm", ("wrap", "prefix", "multi")), ("gru_duel", ("wrap", "open_across_reset", "multi")), ("rnn_conv", ("wrap", "short", "multi"))])
def test_chosen_seeds_cover_every_branch_of_the_ring(name, want):
    """the GPU replay test runs these cases under eps = 1 (dynamics and draws do not depend on the network): simulated here on the mirrors, the chosen seeds reach
    ring wrap, prefix truncation, masked rows, a truncated-but-open episode and two copies finishing in one step"""
    spec, net, n, T, cap, B, max_len = RC.cases(nn, envs)[name]
    model = RC.RingModel(n, T, cap, spec.obs_shape)
    ls = RC.LockStep(None, spec, n, max_len, RC.ENV_SEED[name], model, eps=(1.0, 1.0, 1.0))
    for k in range(30):
        ls.step()
        assert (model.size >= B) == (k + 1 >= RC.WARM[name])      # the warm-up of the GPU training tests ends exactly where a batch of episodes is committed
    for k in want:
        assert model.seen[k], (name, k, model.seen)


class StubEngine:
    def __init__(self, B):
        self.calls, self.B, self.eps = [], B, 0

    def sync_target(self):
        self.calls.append("sync_target")

    def envs_create(self, env, n_envs=None, max_episode_length=100, seed=0):
        self.calls.append(("envs_create", n_envs, seed))

    def rollout(self, n_steps, t0=1, train_freq=4, target_update_freq=500, eps=(1.0, 0.01, 5000.0), stats=True, env_step_cadence=False):
        self.calls.append(("rollout", n_steps, t0, train_freq, tuple(eps)))
        self.eps += 1
        return dict(episodes=0, reward_sum=0.0, train_steps=0, loss=0.0, grad_norm=0.0) if stats else None

    def episode_count(self):
        return min(self.eps, self.B), 8

    def evaluate(self, n_eval, max_episode_length=100, seed=0):
        return 0.0, 1.0

    def episode_add(self, *a):
        raise AssertionError("the device route never collects on the host")


def test_dqn_train_routes_by_the_engines_capability_flag():
    env = envs.TestMDP((5, 5), 1, 6, n=4)
    model = nn.Chain(nn.flattenbatch, nn.LSTM(25, 8), nn.Dense(8, 4))
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.1, steps=50))
    solver = S.DeepQLearningSolver(qnetwork=model, exploration_policy=expl, recurrence=True, device_envs=True, verbose=False, logdir=None, max_steps=20, eval_freq=10,
                                   log_freq=10, save_freq=10, batch_size=2, train_start=8, seed=5)
    plain = StubEngine(2)
    with pytest.raises(pkg.DQNError, match=r"device_envs drives the feed-forward path \(recurrence = false\)"):
        S.dqn_train(solver, env, RC.stub_namespace(engine=plain), None)
    assert plain.calls == []
    cap = StubEngine(2)
    cap.recurrent_device_envs = True
    assert isinstance(S.initialize_replay_buffer(solver, env, cap), S.HIPEpisodeReplayBuffer)      # no host prefill (episode_add would raise)
    S.dqn_train(solver, env, RC.stub_namespace(engine=cap, qnetwork=model), None)
    creates = [c for c in cap.calls if c[0] == "envs_create"]
    rolls = [c for c in cap.calls if c[0] == "rollout"]
    assert len(creates) == 2 and creates[0][2] != creates[1][2] and creates[1][2] == 5      # prefill under a derived seed, then the solver's
    assert rolls[0][3] == 0 and rolls[0][4] == (1.0, 1.0, 1.0) and rolls[0][1] == 2            # train_start = 8 env steps of 4 copies
    assert rolls[2][2] == 1 and rolls[2][3] == solver.train_freq                                 # two prefill rollouts (B = 2 episodes), then training counts t from 1
    assert getattr(pkg.Engine, "recurrent_device_envs", False) is True and not hasattr(ref.Twin, "recurrent_device_envs")
    never = StubEngine(2)
    never.recurrent_device_envs = True
    never.episode_count = lambda: (0, 8)
    with pytest.raises(pkg.DQNError, match="device prefill"):
        S.dqn_train(solver, env, RC.stub_namespace(engine=never, qnetwork=model), None)
    assert sum(c[0] == "rollout" for c in never.calls) == 100


def test_header_states_the_commit_order_and_the_truncation_rule():
    text = " ".join(w for w in open(os.path.join(ge.ROOT, "include", "dqn_mi355x.h")).read().split() if w != "*")      # comment continuation stars dropped
    assert "ascending copy index" in text and "(ep_widx + k) % capacity" in text
    assert "does NOT close the open episode" in text
    assert "every vector step advances every copy's state" in text
