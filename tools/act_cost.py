"""usage (GPU box, repo root): [DQN_MI355X_LIB=<another build>] python tools/act_cost.py [--acts tanh,relu,...] [--n 512]
The step time of Dense(64, n, act) -> Dense(n, 4), f32 vector observations, at B = 32 and B = 512 for each named activation: dqn_train_steps(400), median of 5 (after 50
warm-up steps), in us per step.  The yardstick of docs/history/activations.md is `tanh` under the parent commit's library, run twice in the same call to show that
call's noise; the activation codes are passed as integers, so a library that predates a code can still be named (it then runs its own law for that code)."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

NAMES = ("identity", "relu", "tanh", "sigmoid", "leakyrelu", "elu", "selu", "softplus", "softsign", "relu6", "hardtanh")      # index = DQN_ACT_* code


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
    runs = []
    for _ in range(5):
        t = time.perf_counter(); h.train_steps(steps); runs.append((time.perf_counter() - t) / steps * 1e6)
    return statistics.median(runs), min(runs), max(runs)


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--acts", default=",".join(NAMES[1:])); ap.add_argument("--n", type=int, default=512)
    a = ap.parse_args()
    pkg = ge.load_package(); pkg.lib()
    nn = importlib.import_module(pkg.__name__ + ".nn")
    print(f"library: {pkg.LIB_PATH}")
    for name in a.acts.split(","):
        code = NAMES.index(name); out = []
        for B in (32, 512):
            h = engine(pkg, nn, nn.Chain(nn.Dense(64, a.n, code), nn.Dense(a.n, 4)), B)
            med, lo, hi = step_us(h); h.close()
            out.append(f"B = {B}: {med:7.2f} us/step (min {lo:.2f}, max {hi:.2f})")
        print(f"  {name:10s} " + "   ".join(out), flush=True)


if __name__ == "__main__":
    main()
