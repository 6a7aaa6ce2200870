"""Engine groups (dqn_group_*): K config-1 engines -- Chain(Dense(2,32), Dense(32,4)) dueling + double-Q + prioritized replay, B = 32, replay filled by the device
GridWorld loop, one seed per engine -- trained `--steps` steps each, timed as wall time of

    --mode group   ONE group.train_steps(steps)                      (one launch of K workgroups per step)
    --mode seq     K engines one after the other, train_steps(steps)  (what K seeds cost without a group; run it under the parent commit's build too:
                                                                       DQN_MI355X_LIB=deepqlearning.jl_amd/build/base.so, tools/build_variant.sh base)
    --mode cfg1    config 1 standalone: one engine, train_steps(2000)  (the A/B of the kernel's one-index change: in-tree against base)

One JSON line per K: best and median wall time over --reps, time per (group) step, aggregate train steps/s.  Alternate the modes / builds on ONE box: boxes differ
by a few per cent.  --self-check: before timing, every member of the group is compared with a standalone engine (parameters, priorities, counters: bit for bit)."""
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
ap.add_argument("--mode", choices=("group", "seq", "cfg1"), default="group")
ap.add_argument("--K", default="1,8,64,256,512")
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


def engine(seed):
    hp = pkg.default_hparams(batch_size=32, n_actions=4, obs_c=2, obs_h=1, obs_w=1, gamma=0.95, buffer_size=10000, seed=seed)
    e = pkg.Engine(layers, hp)
    e.set_params(nn.glorot_params(net, seed=1 + seed), pkg.NET_ONLINE)
    e.sync_target()
    e.envs_create(envs.SimpleGridWorld(n=256), max_episode_length=100, seed=1 + seed)
    e.rollout(40, t0=1, train_freq=0, eps=(1.0, 1.0, 1.0), stats=False)      # 10 240 transitions
    return e


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); out.append(time.perf_counter() - t0)
    return min(out), float(np.median(out))


if args.mode == "cfg1":
    e = engine(0)
    e.train_steps(50); e.sync()
    best, med = timed(lambda: (e.train_steps(2000), e.sync()), args.reps)
    print(json.dumps(dict(mode="cfg1", build=build, steps=2000, best_ms=1e3 * best, median_ms=1e3 * med, us_per_step=1e6 * best / 2000, steps_per_s=2000 / best)), flush=True)
    e.close()
    sys.exit(0)

Ks = [int(x) for x in args.K.split(",")]
t0 = time.perf_counter()
pool = [engine(k) for k in range(max(Ks))]
print(json.dumps(dict(created=len(pool), seconds=round(time.perf_counter() - t0, 2))), flush=True)
if args.mode == "group" and args.self_check:      # the pool is fresh here: every member against a standalone engine built the same way
    group = pkg.EngineGroup(pool)
    group.train_steps(3)
    for k, m in enumerate(pool):
        t = engine(k)
        t.train_steps(3)
        assert np.array_equal(m.get_params(0), t.get_params(0)) and np.array_equal(m.replay_priorities(), t.replay_priorities()) and m.get_counters() == t.get_counters(), k
        t.close()
    group.close()
    print(json.dumps(dict(self_check="ok", K=len(pool))), flush=True)
for K in Ks:
    members = pool[:K]
    if args.mode == "group":
        group = pkg.EngineGroup(members)
        run = lambda: group.train_steps(args.steps)      # noqa: E731
    else:
        run = lambda: [m.train_steps(args.steps) for m in members]      # noqa: E731
    run()      # warm-up: graphs captured, LDS attribute set
    best, med = timed(run, args.reps)
    print(json.dumps(dict(mode=args.mode, build=build, K=K, steps=args.steps, best_ms=1e3 * best, median_ms=1e3 * med,
                          us_per_group_step=1e6 * best / args.steps, aggregate_steps_per_s=K * args.steps / best)), flush=True)
    if args.mode == "group":
        group.close()
for e in pool:
    e.close()
