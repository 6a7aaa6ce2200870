"""usage (GPU box, repo root): python tools/do_profile.py [--n 512] [--reps 11] [--solve]
The Dropout launches of one train step (dqn_profile_step) on Dense(64, n, relu) -> Dropout(0.5) -> Dense(n, 4), f32 vector observations, B = 32 and B = 512:
the median us of fwd_on_do1 and bwd_do1 over `reps` profiled steps (after a warm-up of the shapes), their compulsory bytes over that time against the 8 TB/s HBM peak,
and the step time (dqn_train_steps, graphs) beside the same network WITHOUT the layer at the same build.  The yardstick of the forward is LayerNorm's fwd_on_ln1 at the
same (n, columns): run tools/ln_profile.py in the same call.  --solve: the evaluation return of solve on TestMDP((5, 5), 4, 6), max_steps = 10000, with
Dense(100, 16, relu) -> Dropout(0.1) -> Dense(16, 4) beside the same run without the layer.  One box, one call: quote it that way (docs/history/dropout.md)."""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
from ln_profile import HBM_PEAK, engine, step_us


def solve_return(pkg, model):
    envs, S = (importlib.import_module(pkg.__name__ + "." + m) for m in ("envs", "solver"))
    env = envs.TestMDP((5, 5), 4, 6, n=8, seed=7)
    expl = S.EpsGreedyPolicy(env, S.LinearDecaySchedule(start=1.0, stop=0.01, steps=5000), rng=np.random.default_rng(1))
    solver = S.DeepQLearningSolver(qnetwork=model, max_steps=10000, learning_rate=0.005, exploration_policy=expl, eval_freq=2000, num_ep_eval=100, log_freq=500,
                                   double_q=True, dueling=False, prioritized_replay=False, verbose=False, device_envs=True)      # the reference's double-Q solve test (test/runtests.jl)
    policy = S.solve(solver, env)
    r, steps = policy.engine.evaluate(100, 100, seed=3)
    policy.engine.close()
    return r, steps


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--n", type=int, default=512); ap.add_argument("--reps", type=int, default=11); ap.add_argument("--solve", action="store_true")
    a = ap.parse_args(); n = a.n
    pkg = ge.load_package(); pkg.lib()
    nn = importlib.import_module(pkg.__name__ + ".nn")
    for B in (32, 512):
        with_do = nn.Chain(nn.Dense(64, n, nn.relu), nn.Dropout(0.5), nn.Dense(n, 4))
        without = nn.Chain(nn.Dense(64, n, nn.relu), nn.Dense(n, 4))
        h = engine(pkg, nn, with_do, B)
        h.train_steps(20)
        for _ in range(3):
            h.profile_step(max_entries=256)
        runs = [dict(h.profile_step(max_entries=256)) for _ in range(a.reps)]
        med = {k: statistics.median(r[k] for r in runs) * 1e3 for k in runs[0]}
        # compulsory bytes: forward = read X + write Y over the online pass's 2 B columns; backward = read dY and the producer's y, write dX, over B columns
        byt = {"fwd_on_do1": 2 * 4 * n * 2 * B, "bwd_do1": 3 * 4 * n * B}
        print(f"B = {B}, n = {n}: median of {a.reps} profiled steps (eager launches, HIP events); whole profiled step {sum(med.values()):.1f} us in {len(med)} launches")
        for k, b in byt.items():
            print(f"  {k:12s} {med[k]:7.2f} us   {b / 1e6:7.3f} MB compulsory   {b / (med[k] * 1e-6) / 1e12:6.3f} TB/s = {100 * b / (med[k] * 1e-6) / HBM_PEAK:5.1f} % of the 8 TB/s peak")
        print("  all launches:", "  ".join(f"{k} {v:.1f}" for k, v in med.items()))
        t_do = step_us(h); h.close()
        h0 = engine(pkg, nn, without, B); t0 = step_us(h0); h0.close()
        print(f"  step time (dqn_train_steps(400), median of 5): with the layer {t_do:.1f} us, without {t0:.1f} us (+{t_do - t0:.1f} us)")
    if a.solve:
        for name, model in (("with Dropout(0.1)", nn.Chain(nn.Dense(100, 16, nn.relu), nn.Dropout(0.1), nn.Dense(16, 4))), ("without the layer", nn.Chain(nn.Dense(100, 16, nn.relu), nn.Dense(16, 4)))):
            r, steps = solve_return(pkg, model)
            print(f"solve TestMDP((5, 5), 4, 6), max_steps 10000, {name}: evaluation return {r:.3f} over 100 episodes ({steps:.1f} steps each)")


if __name__ == "__main__":
    main()
