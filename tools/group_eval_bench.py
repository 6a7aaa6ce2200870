"""Grouped evaluation (dqn_evaluate_many): K config-1 engines -- Chain(Dense(2,32), Dense(32,4)) dueling + double-Q + prioritized replay, B = 32, 32 SimpleGridWorld
training copies each -- evaluated with n_eval greedy episodes of at most max_episode_length steps, timed as wall time of

    --mode eval    per K: ONE group.evaluate(n_eval, L, seeds) against K sequential Engine.evaluate(n_eval, L, seed) calls in the same process (dqn_evaluate is the
                   path solve_many took member by member before the grouped evaluation; it is untouched), and their ratio; the results are compared (==) first
    --mode wide    the longest launch: a group of ONE member near the parameter limit of a group, Dense(2,128,relu) -> Dense(128,80,tanh) -> Dense(80,4) (11 028
                   parameters), 1024 copies of an MDP without a terminal state (every copy lives through every step), max_episode_length = steps_per_launch - 1: ONE
                   launch of the full step bound with full tiles
    --mode solve   end to end: solver.solve_many of K solvers, --max-steps vector steps with an evaluation every --eval-freq; total wall time and the share spent in
                   evaluation (the time inside EngineGroup.evaluate / Engine.evaluate).  --per-member routes every mark through the member's own Engine.evaluate,
                   which is what solve_many did before the grouped evaluation (the rest of the loop is the same code)

One JSON line per measurement: median and best wall time over --reps after one warm-up call (the warm-up allocates the evaluation copies, captures the standalone
engines' graphs and raises the LDS attribute).  Kernel times proper come from running this under a kernel trace (tools/README.md); alternate builds / modes on ONE box."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as ge  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("eval", "wide", "solve"), default="eval")
ap.add_argument("--K", default="1,8,64,512")
ap.add_argument("--n-eval", type=int, default=100)
ap.add_argument("--length", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--seq-reps", type=int, default=3, help="repetitions of the K sequential calls (seconds each at K = 512)")
ap.add_argument("--max-steps", type=int, default=2000)
ap.add_argument("--eval-freq", type=int, default=500)
ap.add_argument("--per-member", action="store_true")
args = ap.parse_args()

pkg = ge.load_package()
nn, envs, S = (importlib.import_module(pkg.__name__ + "." + m) for m in ("nn", "envs", "solver"))
build = os.path.basename(os.environ.get("DQN_MI355X_LIB") or "in-tree")
N_ENVS = 32


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); out.append(time.perf_counter() - t0)
    return float(np.median(out)), min(out)


def out(**kw):
    print(json.dumps(dict(mode=args.mode, build=build, **kw)), flush=True)


def engine(net, seed, env):
    layers, _ = nn.lower(net)
    hp = pkg.default_hparams(batch_size=32, n_actions=4, obs_c=2, obs_h=1, obs_w=1, gamma=0.95, buffer_size=10000, seed=seed)
    e = pkg.Engine(layers, hp)
    e.set_params(nn.glorot_params(net, seed=1 + seed), pkg.NET_ONLINE)
    e.sync_target()
    e.envs_create(env, max_episode_length=100, seed=1 + seed)
    e.rollout(4, t0=1, train_freq=0, eps=(1.0, 1.0, 1.0), stats=False)
    return e


if args.mode == "eval":
    net = nn.create_dueling_network(nn.Chain(nn.Dense(2, 32), nn.Dense(32, 4)))
    Ks = [int(x) for x in args.K.split(",")]
    t0 = time.perf_counter()
    pool = [engine(net, k, envs.SimpleGridWorld(n=N_ENVS)) for k in range(max(Ks))]
    out(created=len(pool), seconds=round(time.perf_counter() - t0, 2))
    for K in Ks:
        members, seeds = pool[:K], [1000 + k for k in range(K)]
        group = pkg.EngineGroup(members)
        launches, bound, lds = group.evaluate_info(args.n_eval, args.length)
        many = lambda: group.evaluate(args.n_eval, args.length, seeds)      # noqa: E731
        seq = lambda: [m.evaluate(args.n_eval, args.length, seed=s) for m, s in zip(members, seeds)]      # noqa: E731
        got = many()      # warm-up of both, and THE LAW
        assert args.seq_reps < 1 or got == seq()
        m_med, m_best = timed(many, args.reps)
        s_med, s_best = timed(seq, args.seq_reps) if args.seq_reps > 0 else (float("nan"), float("nan"))      # (--seq-reps 0: the grouped call alone, for a kernel trace)
        steps = max(st for _, st in many())      # the largest avg_steps of a member
        out(K=K, n_eval=args.n_eval, length=args.length, launches=launches, steps_per_launch=bound, lds_bytes=lds, max_avg_steps=steps, many_median_ms=1e3 * m_med,
            many_best_ms=1e3 * m_best, sequential_median_ms=1e3 * s_med, sequential_best_ms=1e3 * s_best, ratio_of_medians=s_med / m_med,
            many_us_per_launch=1e6 * m_med / launches)
        group.close()
    for e in pool:
        e.close()
elif args.mode == "wide":
    net = nn.Chain(nn.Dense(2, 128, nn.relu), nn.Dense(128, 80, nn.tanh), nn.Dense(80, 4))
    T = np.zeros((2, 4, 2), np.float32); T[0, :, 1] = 1.0; T[1, :, 0] = 1.0      # two states, every action flips the state; no terminal state
    feats = np.array([[0.25, 0.5], [0.75, 1.0]], np.float32)
    layers, _ = nn.lower(net)
    hp = pkg.default_hparams(batch_size=2, n_actions=4, obs_c=2, obs_h=1, obs_w=1, gamma=0.95, buffer_size=64, seed=3, dueling=0)
    e = pkg.Engine(layers, hp, plan=[(f, 0, w) for f, _, w in pkg.default_plan(layers, hp)])      # dx_kc = 0: the plan the single-workgroup step takes
    e.set_params(nn.glorot_params(net, seed=4), pkg.NET_ONLINE)
    e.sync_target()
    e.envs_create_tabular(T=T, R=np.ones((2, 4, 2), np.float32), terminal=np.zeros(2, np.uint8), b0=np.array([0.5, 0.5], np.float32), features=feats, n_envs=2,
                          max_episode_length=100, seed=5)
    group = pkg.EngineGroup([e])
    _, bound, lds = group.evaluate_info(1024, 1)
    for L in (bound - 1, 2 * bound - 1):
        launches = group.evaluate_info(1024, L)[0]
        run = lambda: group.evaluate(1024, L, [9])      # noqa: E731
        assert run() == [e.evaluate(1024, L, seed=9)] and run()[0][1] == L + 1
        med, best = timed(run, args.reps)
        out(parameters=e.P, n_eval=1024, length=L, launches=launches, steps_per_launch=bound, lds_bytes=lds, median_ms=1e3 * med, best_ms=1e3 * best,
            median_us_per_vector_step=1e6 * med / (L + 1))
    group.close(); e.close()
else:
    spent = []      # seconds per evaluation call

    def clocked(fn):
        def wrapper(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                spent.append(time.perf_counter() - t0)
        return wrapper
    pkg._abi.EngineGroup.evaluate = clocked(pkg._abi.EngineGroup.evaluate)
    pkg._abi.Handle.evaluate = clocked(pkg._abi.Handle.evaluate)
    if args.per_member:
        S._group_evaluate = lambda group, solvers, nxt: [None] * len(solvers)
    for K in [int(x) for x in args.K.split(",")]:
        def solver(k):
            env = envs.SimpleGridWorld(n=N_ENVS, seed=5)
            model = nn.Chain(nn.Dense(2, 32), nn.Dense(32, env.n_actions))
            expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.05, steps=1000))
            return S.DeepQLearningSolver(qnetwork=model, exploration_policy=expl, max_steps=args.max_steps, train_freq=4, target_update_freq=500, train_start=64, batch_size=32,
                                         buffer_size=10000, eval_freq=args.eval_freq, num_ep_eval=args.n_eval, max_episode_length=args.length, log_freq=args.eval_freq,
                                         logdir=None, verbose=False, device_envs=True, double_q=True, dueling=True, prioritized_replay=True, seed=100 + k)
        solvers = [solver(k) for k in range(K)]
        real_rollout, roll = pkg._abi.EngineGroup.rollout, [0.0]

        def rollout(self, *a, **kw):
            t0 = time.perf_counter()
            try:
                return real_rollout(self, *a, **kw)
            finally:
                roll[0] += time.perf_counter() - t0
        pkg._abi.EngineGroup.rollout = rollout
        del spent[:]
        t0 = time.perf_counter()
        pols = S.solve_many(solvers, envs.SimpleGridWorld(n=N_ENVS, seed=5))
        total = time.perf_counter() - t0
        pkg._abi.EngineGroup.rollout = real_rollout
        out(K=K, evaluation="per member (dqn_evaluate)" if args.per_member else "grouped (dqn_evaluate_many)", max_steps=args.max_steps, eval_freq=args.eval_freq,
            total_s=total, evaluation_s=sum(spent), evaluation_calls=len(spent), rollout_and_train_s=roll[0], evaluation_share=sum(spent) / total,
            evaluation_over_device_loop=sum(spent) / roll[0], first_mark_s=sum(spent[:len(spent) // 4]), later_marks_s=sum(spent[len(spent) // 4:]),
            scores=[float(p.scores_eval) for p in pols[:4]])      # (the first mark allocates every member's evaluation copies, on either path)
        for p in pols:
            p.engine.close()
