"""usage (GPU box, repo root): python tools/ln_profile.py [--n 512] [--reps 11]
The LayerNorm launches of one train step (dqn_profile_step) on Dense(64, n, relu) -> LayerNorm(n) -> Dense(n, 4), f32 vector observations, B = 32 and B = 512:
the median us of each `ln` launch over `reps` profiled steps (after a warm-up of the shapes), its compulsory bytes over that time against the 8 TB/s HBM peak, and
the step time (dqn_train_steps, graphs) beside the same network WITHOUT the layer at the same build.  One box, one call: quote it that way (docs/history/layernorm.md)."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

HBM_PEAK = 8.0e12


def engine(pkg, nn, net, B):
    layers, _ = nn.lower(net)
    hp = pkg.default_hparams(batch_size=B, n_actions=4, obs_c=64, dueling=0, buffer_size=4096, learning_rate=1e-4, seed=1)
    h = pkg.Engine(layers, hp)
    rng = np.random.default_rng(0); n = 4096
    h.replay_add(rng.standard_normal((n, 64)).astype(np.float32), rng.integers(0, 4, n).astype(np.int32), rng.standard_normal(n).astype(np.float32),
                 rng.standard_normal((n, 64)).astype(np.float32), (rng.random(n) < 0.1).astype(np.uint8))
    h.set_params(nn.glorot_params(net, seed=1), 0); h.sync_target()
    return h


def step_us(h, steps=400):
    h.train_steps(50)
    best = []
    for _ in range(5):
        t = time.perf_counter(); h.train_steps(steps); best.append((time.perf_counter() - t) / steps * 1e6)
    return statistics.median(best)


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--n", type=int, default=512); ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args(); n = a.n
    pkg = ge.load_package(); pkg.lib()
    nn = importlib.import_module(pkg.__name__ + ".nn")
    for B in (32, 512):
        with_ln = nn.Chain(nn.Dense(64, n, nn.relu), nn.LayerNorm(n), nn.Dense(n, 4))
        without = nn.Chain(nn.Dense(64, n, nn.relu), nn.Dense(n, 4))
        h = engine(pkg, nn, with_ln, B)
        h.train_steps(20)
        for _ in range(3):
            h.profile_step(max_entries=256)
        runs = [dict(h.profile_step(max_entries=256)) for _ in range(a.reps)]
        med = {k: statistics.median(r[k] for r in runs) * 1e3 for k in runs[0]}
        # compulsory bytes: forward = read X + write Y over the pass's columns; backward = the dX launch reads dpre and X and writes dX, the parameter launch reads dpre and X again
        byt = {"fwd_on_ln1": 2 * 4 * n * 2 * B, "fwd_tg_ln1": 2 * 4 * n * B, "bwd_ln1": 5 * 4 * n * B}
        print(f"B = {B}, n = {n}: median of {a.reps} profiled steps (eager launches, HIP events); whole profiled step {sum(med.values()):.1f} us in {len(med)} launches")
        for k, b in byt.items():
            print(f"  {k:12s} {med[k]:7.2f} us   {b / 1e6:7.3f} MB compulsory   {b / (med[k] * 1e-6) / 1e12:6.3f} TB/s = {100 * b / (med[k] * 1e-6) / HBM_PEAK:5.1f} % of the 8 TB/s peak")
        print("  all launches:", "  ".join(f"{k} {v:.1f}" for k, v in med.items()))
        t_ln = step_us(h); h.close()
        h0 = engine(pkg, nn, without, B); t0 = step_us(h0); h0.close()
        print(f"  step time (dqn_train_steps(400), median of 5): with the layer {t_ln:.1f} us, without {t0:.1f} us (+{t_ln - t0:.1f} us)")


if __name__ == "__main__":
    main()
