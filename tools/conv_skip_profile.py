"""usage (GPU box, repo root): python tools/conv_skip_profile.py [--pairs 5] [--mode trunk|padded]
Convolutional skip blocks (DQN_LAYER_SKIPADD_MAP, the residual epilogues of csrc/conv_own.hip), measured in ONE process, alternating:

  --mode trunk   the residual trunk at the workload's shape -- Conv(8, 4 => 32, relu; stride = 4) on 84 x 84 x 4, two blocks of two Conv(3, 32 => 32; pad = 1) (relu
                 between them), Dense(12800, 512, relu), Dense(512, 4); f32 observations -- at B = 32 and B = 512: an engine created with DQN_NO_SKIP_FUSE unset (the
                 fused schedule) and one with it set (the join's own launches), `pairs` times in turn: steps/s of dqn_train_steps (graphs), and once per schedule the
                 launch count and the per-launch averages of dqn_profile_steady_step.
  --mode padded  the step time of a padded network WITHOUT a block -- Conv(3, 4 => 4, tanh; pad = 1) -> Conv(3, 4 => 8, sigmoid; pad = 1) -> Conv(3, 8 => 8, tanh;
                 pad = 1) -> Dense(288, 4) on 4 x 6 x 6 observations at B = 128, the stack_same network of tests/conv_pad_reference.py -- `pairs` times.  Run it under
                 DQN_MI355X_LIB=<another build> and under the in-tree build in turn (one call of a shell loop) to compare two builds of conv_own.hip.
One box, one call: quote it that way (docs/history/conv_skip.md)."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge


def engine(pkg, nn, net, B, obs, unfused=False, n=2048):
    layers, _ = nn.lower(net)
    hp = pkg.default_hparams(batch_size=B, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], dueling=0, buffer_size=n, learning_rate=1e-4, seed=1)
    if unfused:
        os.environ["DQN_NO_SKIP_FUSE"] = "1"
    try:
        h = pkg.Engine(layers, hp)
    finally:
        os.environ.pop("DQN_NO_SKIP_FUSE", None)
    rng = np.random.default_rng(0)
    for o in range(0, n, 256):      # in pieces: 2048 rows of 84 x 84 x 4 floats are 231 MB
        h.replay_add(rng.random((256,) + obs, dtype=np.float32), rng.integers(0, 4, 256).astype(np.int32), rng.standard_normal(256).astype(np.float32),
                     rng.random((256,) + obs, dtype=np.float32), (rng.random(256) < 0.1).astype(np.uint8))
    h.set_params(nn.glorot_params(net, seed=1), 0); h.sync_target()
    return h


def step_us(h, steps):
    t = time.perf_counter(); h.train_steps(steps); return (time.perf_counter() - t) / steps * 1e6


def trunk(nn):
    blk = lambda: nn.SkipConnection(nn.Chain(nn.Conv(3, 32, 32, nn.relu, 1, 1), nn.Conv(3, 32, 32, nn.identity, 1, 1)), "+")
    return nn.Chain(nn.Conv(8, 4, 32, nn.relu, 4), blk(), blk(), nn.flattenbatch, nn.Dense(12800, 512, nn.relu), nn.Dense(512, 4))


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--pairs", type=int, default=5); ap.add_argument("--mode", default="trunk")
    a = ap.parse_args()
    pkg = ge.load_package(); pkg.lib()
    nn = importlib.import_module(pkg.__name__ + ".nn")
    if a.mode == "padded":
        net = nn.Chain(nn.Conv(3, 4, 4, nn.tanh, 1, 1), nn.Conv(3, 4, 8, nn.sigmoid, 1, 1), nn.Conv(3, 8, 8, nn.tanh, 1, 1), nn.flattenbatch, nn.Dense(288, 4))
        h = engine(pkg, nn, net, 128, (4, 6, 6)); h.train_steps(200)
        us = [step_us(h, 2000) for _ in range(a.pairs)]; h.close()
        print(f"padded stack, B = 128, lib = {os.environ.get('DQN_MI355X_LIB') or 'in-tree'}: us/step " + " ".join(f"{u:.2f}" for u in us) + f"   mean {statistics.mean(us):.2f}")
        return
    for B in (32, 512):
        steps = 400 if B == 32 else 100
        hs = {"fused": engine(pkg, nn, trunk(nn), B, (4, 84, 84)), "unfused": engine(pkg, nn, trunk(nn), B, (4, 84, 84), unfused=True)}
        for h in hs.values():
            h.train_steps(50)
        us = {k: [] for k in hs}
        for _ in range(a.pairs):
            for k, h in hs.items():
                us[k].append(step_us(h, steps))
        print(f"B = {B}: {a.pairs} alternating runs of dqn_train_steps({steps})")
        for k in hs:
            m = statistics.mean(us[k])
            print(f"  {k:8s} us/step " + " ".join(f"{u:.1f}" for u in us[k]) + f"   mean {m:.1f} us = {1e6 / m:.0f} steps/s   spread {min(us[k]):.1f} .. {max(us[k]):.1f}")
        for k, h in hs.items():
            for _ in range(2):
                h.profile_step(max_entries=256, steady=True)
            runs = [h.profile_step(max_entries=256, steady=True) for _ in range(5)]
            names = [nm for nm, _ in runs[0]]; med = [statistics.median(r[i][1] for r in runs) * 1e3 for i in range(len(names))]
            print(f"  {k:8s} {len(names)} launches per step, {sum(med):.1f} us of launches: " + "  ".join(f"{nm} {v:.1f}" for nm, v in zip(names, med)))
            h.close()


if __name__ == "__main__":
    main()
