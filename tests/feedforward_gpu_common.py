"""Bodies the GPU test files of the layer kinds beyond Dense and plain Conv share (TEST INFRASTRUCTURE): tests/test_pool_gpu.py and tests/test_conv_pad_gpu.py
run the policy forward, a recurrent chain with their layer in its trunk, the device environment loop and the solver round trip the same way; they differ in the
case table, the network, the launch names and the acting tail they expect, which are the arguments here.  The fp64 side is tests/feedforward_reference.py."""
import numpy as np

import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_reference as FR
import recurrent_reference as R
from drqn_common import feed

ENV_SEED = 1      # parameter seed of the env-loop networks (glorot + 0.1 N(0, 1)): their fp64 top-two gaps on the observations TestMDP (5, 5) shows stay above GAP


def policy_forward_and_greedy_action(pkg, c):
    """dqn_forward on 1 and 3 observations against the fp64 Q values; the greedy action is the fp64 argmax wherever the fp64 top-two gap is at least GAP"""
    net, D = E.prepare(c)
    h, _ = E.make_handle(pkg.Engine, c, net, D)
    f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
    ps = net.unflatten(D["p_on"].astype(np.float64))
    for n in (1, 3):
        obs = f(D["s"][:n])
        q64 = FR.q_numpy(net, ps, obs.astype(np.float64))[0]
        E._close("policy_q", h.forward(obs), q64, msg=f"{c.name} n={n}", **E.TOL_Q)
        a = h.greedy_action(obs); t = np.sort(q64, axis=1)
        clear = t[:, -1] - t[:, -2] >= E.GAP
        np.testing.assert_array_equal(np.asarray(a)[clear], q64.argmax(1)[clear])
    h.close()


def recurrent_chain(pkg, nn, spec, launches):
    """spec.net: a Conv / pool trunk -> LSTM -> Dense over T * B columns.  The checker of test_recurrent_edges_gpu.run_checked with feedforward_reference's chain;
    use_graph 0 equals 1 bit for bit.  launches: {launch name: how often one step shows it}"""
    c = spec
    net, cap, eps, ring, p_on, p_tg, dr = FR.rec_data(nn, c)
    layers, _ = nn.lower(net)

    def engine(graph):
        hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=c.obs[0], obs_h=c.obs[1], obs_w=c.obs[2], dueling=0, buffer_size=cap, recurrence=1, trace_length=c.T,
                                 learning_rate=1e-3, prioritized_replay=0, use_graph=graph, seed=5, gamma=c.gamma, double_q=c.double_q)
        h = pkg.Engine(layers, hp); feed(h, eps); h.set_params(p_on, 0); h.set_params(p_tg, 1)
        return h
    h, h0 = engine(1), engine(0)
    adam = R.Adam(p_on.size); blks = FR.rec_blocks(net, nn)
    for k, (idx, start) in enumerate(dr):
        p_prev = h.get_params(0)
        batch = h.episode_get_batch(idx, start)
        for got, want in zip(batch, R.sample_batch(ring, idx, start, c.T, c.obs)):
            np.testing.assert_array_equal(np.asarray(got).reshape(want.shape), want)
        batch = tuple(np.asarray(x).reshape((c.T, c.B) + (c.obs if i in (0, 3) else ())) for i, x in enumerate(batch))
        rm, pm = FR.rec_margins(net, nn, c, p_prev, batch[0], batch[5])
        assert rm > E.RELU_MARGIN and pm > E.RELU_MARGIN, (k, rm, pm)
        o = FR.rec_train_grads(net, nn, p_prev, p_tg, batch, float(np.float32(c.gamma)), True)
        loss, gn = h.train_step_drqn(idx, start)
        g = h.get_grads()
        np.testing.assert_allclose(loss, o["loss"], rtol=2e-5, atol=1e-7, err_msg=f"step {k}: loss")
        R.check_grads(net, nn, g, o["grads"], live=k == 0, blks=blks)
        np.testing.assert_allclose(gn, o["grad_norm"], rtol=1e-4, err_msg=f"step {k}: grad_norm")
        R.check_params(h.get_params(0), adam.step(p_prev, g))
        assert h0.train_step_drqn(idx, start) == (loss, gn)
        np.testing.assert_array_equal(h0.get_grads(), g); np.testing.assert_array_equal(h0.get_params(0), h.get_params(0))
    names = [n for n, _ in h.profile_step(max_entries=512)]
    assert all(names.count(n) == k for n, k in launches.items()), (launches, names)
    h.close(); h0.close()


def _env_engine(pkg, mods, net, B=8, cap=64):
    nn, envs = mods[0], mods[1]
    layers, _ = nn.lower(net)
    hp = pkg.default_hparams(batch_size=B, n_actions=4, obs_c=4, obs_h=5, obs_w=5, dueling=0, buffer_size=cap, learning_rate=1e-3, gamma=0.95, seed=5)
    h = pkg.Engine(layers, hp)
    rng = np.random.default_rng(ENV_SEED)
    p = nn.glorot_params(net, seed=ENV_SEED); p = (p + 0.1 * rng.standard_normal(p.size)).astype(np.float32)
    h.set_params(p, 0); h.sync_target()
    return h, p, envs.TestMDP((5, 5), 4, 6, n=8, seed=3)


def device_env_loop(pkg, mods, net, onet_layers, fused_head):
    """the acting program of the device loop on `net` (a package nn chain on 4x5x5 observations; onet_layers: the same layers in the reference's vocabulary):
    20 single-step dqn_rollout calls, eps 0, no training; at each the peeked actions equal the fp64 argmax on the observations peeked before the step, except where
    the fp64 gap is below GAP (at most 10 % of the (step, copy) pairs).  fused_head: what envs_info reports of the acting tail.  dqn_evaluate: finite averages."""
    h, p, spec = _env_engine(pkg, mods, net)
    onet = O.Network((4, 5, 5), onet_layers)
    ps = onet.unflatten(p.astype(np.float64))
    h.envs_create(spec, max_episode_length=100, seed=17)
    skipped = total = 0
    for t in range(20):
        obs = h.envs_peek()[0].copy()
        h.rollout(1, t0=t + 1, train_freq=0, target_update_freq=0, eps=(0.0, 0.0, 1.0))
        a = h.envs_peek()[1]
        q = FR.q_numpy(onet, ps, obs.astype(np.float64))[0]; top = np.sort(q, axis=1)
        clear = top[:, -1] - top[:, -2] >= E.GAP
        np.testing.assert_array_equal(a[clear], q.argmax(1)[clear], err_msg=f"step {t}")
        skipped += int((~clear).sum()); total += clear.size
    assert skipped <= 0.1 * total, (skipped, total)
    assert h.envs_info()[1] is fused_head
    r, st = h.evaluate(8, 50, seed=5)
    assert np.isfinite(r) and np.isfinite(st) and st > 0
    h.close()


def solver_round_trip(pkg, mods, tmp_path, monkeypatch, model, sizes):
    """S.solve for 300 steps with device_envs and a logdir on TestMDP (5, 5) with `model` (a package nn chain on 4x5x5 observations): finite losses, qnetwork.bson holds
    exactly the arrays of `sizes`, restore_best_model puts them back bit for bit (no learning threshold is asserted)"""
    nn, envs, S, bson = mods
    env = envs.TestMDP((5, 5), 4, 6, n=8, seed=7)
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.05, steps=200), rng=np.random.default_rng(1))
    solver = S.DeepQLearningSolver(qnetwork=model, max_steps=300, learning_rate=0.005, exploration_policy=expl, eval_freq=100, save_freq=100, num_ep_eval=10, log_freq=100,
                                   double_q=True, dueling=False, prioritized_replay=True, train_start=64, verbose=False, logdir=str(tmp_path / "log"), device_envs=True)
    losses, saved = [], []
    real_rollout = pkg.Engine.rollout

    def rollout(self, *a, **kw):      # the device loop's train steps report their last loss and grad_norm in the rollout statistics
        st = real_rollout(self, *a, **kw)
        if st["train_steps"] > 0:
            losses.append((st["loss"], st["grad_norm"]))
        return st
    monkeypatch.setattr(pkg.Engine, "rollout", rollout)
    real_save = bson.save_qnetwork
    monkeypatch.setattr(bson, "save_qnetwork", lambda path, flat, shapes: (saved.append(np.array(flat, np.float32, copy=True)), real_save(path, flat, shapes))[1])
    policy = S.solve(solver, env)
    assert losses and np.isfinite(np.array(losses)).all(), losses
    assert np.isfinite(policy.engine.get_params(pkg.NET_ONLINE)).all()
    path = tmp_path / "log" / "qnetwork.bson"
    assert path.exists() and saved, "no model was saved"
    w, sizes_read = bson.load_qnetwork(path)
    np.testing.assert_array_equal(w, saved[-1])
    assert [tuple(x) for x in sizes_read] == sizes
    policy.engine.set_params(w * np.float32(0.5), pkg.NET_ONLINE)
    S.restore_best_model(solver, policy)
    np.testing.assert_array_equal(policy.engine.get_params(pkg.NET_ONLINE), w)
    policy.engine.close()
