"""Grouped acting (dqn_rollout_many): K config-1 engines -- Chain(Dense(2,32), Dense(32,4)) dueling + double-Q + prioritized replay, B = 32 -- with 32 SimpleGridWorld
copies each, `--steps` vector steps of the device loop at train_freq = 4, timed as wall time of

    --mode many    ONE group.rollout(steps, train_freq=4)                       (per vector step one launch of K workgroups; the group train launch inside the call)
    --mode loop    solve_many's inner loop before grouped acting: per block of 4 vector steps every member's own rollout(4, train_freq=0), then ONE group.train_steps(1)
                   (uses nothing newer than the engine groups: run it under the parent commit's build, DQN_MI355X_LIB=deepqlearning.jl_amd/build/base.so,
                   tools/build_variant.sh base)
    --mode alone   K = 1 only: the standalone engine's rollout(steps, train_freq=4), for reference

One JSON line per K: best and median wall time over --reps after one warm-up call, microseconds per vector step, aggregate env steps/s (K x 32 copies x steps / best).
Alternate the modes / builds on ONE box: boxes differ by a few per cent.  --self-check (mode many): before timing, every member is compared with a standalone engine
after the same call (parameters, priorities, counters, env state: bit for bit)."""
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
ap.add_argument("--mode", choices=("many", "loop", "alone"), default="many")
ap.add_argument("--K", default="1,8,64,256")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--self-check", action="store_true")
args = ap.parse_args()

pkg = ge.load_package()
nn = importlib.import_module(pkg.__name__ + ".nn")
envs = importlib.import_module(pkg.__name__ + ".envs")
net = nn.create_dueling_network(nn.Chain(nn.Dense(2, 32), nn.Dense(32, 4)))
layers, _ = nn.lower(net)
build = os.path.basename(os.environ.get("DQN_MI355X_LIB") or "in-tree")
N_ENVS, TRAIN_FREQ, EPS = 32, 4, (1.0, 0.05, 400.0)


def engine(seed):
    hp = pkg.default_hparams(batch_size=32, n_actions=4, obs_c=2, obs_h=1, obs_w=1, gamma=0.95, buffer_size=10000, seed=seed)
    e = pkg.Engine(layers, hp)
    e.set_params(nn.glorot_params(net, seed=1 + seed), pkg.NET_ONLINE)
    e.sync_target()
    e.envs_create(envs.SimpleGridWorld(n=N_ENVS), max_episode_length=100, seed=1 + seed)
    e.rollout(4, t0=1, train_freq=0, eps=(1.0, 1.0, 1.0), stats=False)      # 128 transitions: a batch is there from the first due step
    return e


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); out.append(time.perf_counter() - t0)
    return min(out), float(np.median(out))


def line(K, best, med):
    print(json.dumps(dict(mode=args.mode, build=build, K=K, steps=args.steps, best_ms=1e3 * best, median_ms=1e3 * med, us_per_vector_step=1e6 * best / args.steps,
                          aggregate_env_steps_per_s=K * N_ENVS * args.steps / best)), flush=True)


if args.mode == "alone":
    e = engine(0)
    run = lambda: (e.rollout(args.steps, t0=1, train_freq=TRAIN_FREQ, target_update_freq=500, eps=EPS, stats=False), e.sync())      # noqa: E731
    run()
    line(1, *timed(run, args.reps))
    e.close()
    sys.exit(0)

Ks = [int(x) for x in args.K.split(",")]
t0 = time.perf_counter()
pool = [engine(k) for k in range(max(Ks))]
print(json.dumps(dict(created=len(pool), seconds=round(time.perf_counter() - t0, 2))), flush=True)
if args.mode == "many" and args.self_check:      # the pool is fresh here: every member against a standalone engine built the same way
    group = pkg.EngineGroup(pool)
    group.rollout(9, t0=1, train_freq=TRAIN_FREQ, target_update_freq=8, eps=EPS)
    for k, m in enumerate(pool):
        t = engine(k)
        t.rollout(9, t0=1, train_freq=TRAIN_FREQ, target_update_freq=8, eps=EPS)
        assert np.array_equal(m.get_params(0), t.get_params(0)) and np.array_equal(m.get_params(1), t.get_params(1)) and np.array_equal(m.replay_priorities(), t.replay_priorities()), k
        assert m.get_counters() == t.get_counters() and all(np.array_equal(x, y) for x, y in zip(m.envs_peek(), t.envs_peek())), k
        t.close()
    group.close()
    print(json.dumps(dict(self_check="ok", K=len(pool))), flush=True)
for K in Ks:
    members = pool[:K]
    group = pkg.EngineGroup(members)
    if args.mode == "many":
        run = lambda: group.rollout(args.steps, t0=1, train_freq=TRAIN_FREQ, target_update_freq=500, eps=EPS, stats=False)      # noqa: E731
    else:
        def run():
            for t in range(1, args.steps + 1, TRAIN_FREQ):
                for m in members:
                    m.rollout(TRAIN_FREQ, t0=t, train_freq=0, target_update_freq=0, eps=EPS, stats=False)
                group.train_steps(1)
    run()      # warm-up: graphs captured, LDS attributes set
    line(K, *timed(run, args.reps))
    group.close()
for e in pool:
    e.close()
