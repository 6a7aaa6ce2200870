"""usage (GPU box, repo root): python tools/gn_profile.py [--reps 11]
The GroupNorm launches of one train step (dqn_profile_step; csrc/groupnorm.hip) on
  * the smallest case of the test table: 6x6x1 observations, Conv(3, 1 => 4, relu) -> GroupNorm(4, 2, relu) -> Dense(64, 4) at B = 5, and
  * Nature-DQN on 84x84x4 observations with GroupNorm(c, 4, relu) behind each of its three convolutions, at B = 32 and B = 512:
the median us of each `gn` launch over `reps` profiled steps (after a warm-up of the shapes), its compulsory bytes, the resulting TB/s against the 8 TB/s HBM peak, and its
workgroup count against the chip's 256 CUs; then the step time (dqn_train_steps, graphs) beside the same network WITHOUT the layers at the same build.  One box, one call:
quote it that way (docs/history/groupnorm.md)."""
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
GN_R = 64      # rows per chunk (common.h)


def engine(pkg, nn, net, B, obs):
    layers, _ = nn.lower(net)
    n = max(1024, 2 * B)
    hp = pkg.default_hparams(batch_size=B, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], dueling=0, buffer_size=n, learning_rate=1e-4, seed=1)
    h = pkg.Engine(layers, hp)
    rng = np.random.default_rng(0)
    for o in range(0, n, 256):
        h.replay_add(rng.random((256,) + obs, dtype=np.float32), rng.integers(0, 4, 256).astype(np.int32), rng.standard_normal(256).astype(np.float32),
                     rng.random((256,) + obs, dtype=np.float32), (rng.random(256) < 0.1).astype(np.uint8))
    h.set_params(nn.glorot_params(net, seed=1), 0); h.sync_target()
    return h


def step_us(h, steps=200):
    h.train_steps(30)
    best = []
    for _ in range(5):
        t = time.perf_counter(); h.train_steps(steps); best.append((time.perf_counter() - t) / steps * 1e6)
    return statistics.median(best)


def gn_maps(nn, net, obs):
    """{layer index: (c, h * w, G)} of the GroupNorm layers of a plain chain"""
    out, shp = {}, obs
    for i, l in enumerate(net.layers):
        if l.kind == "conv":
            shp = (l.cout, (shp[1] + 2 * l.ph - l.kh) // l.sh + 1, (shp[2] + 2 * l.pw - l.kw) // l.sw + 1)
        elif l.kind == "groupnorm":
            out[i] = (shp[0], shp[1] * shp[2], l.G)
    return out


def report(pkg, nn, name, net, without, B, obs, reps):
    h = engine(pkg, nn, net, B, obs)
    h.train_steps(20)
    for _ in range(3):
        h.profile_step(max_entries=256)
    runs = [dict(h.profile_step(max_entries=256)) for _ in range(reps)]
    med = {k: statistics.median(r[k] for r in runs) * 1e3 for k in runs[0]}
    print(f"{name}, B = {B}: median of {reps} profiled steps (eager launches, HIP events); whole profiled step {sum(med.values()):.1f} us in {len(med)} launches")
    tot = 0.0
    for i, (c, hw, G) in gn_maps(nn, net, obs).items():
        n = c * hw; ng = (c // G) * hw; nch = (ng + GN_R - 1) // GN_R
        wg = lambda cols: G * nch * ((cols + 63) // 64 if cols % 4 == 0 else (cols + 15) // 16)
        # compulsory bytes: statistics = read X; normalise = read X, write Y; chunk sums = read dpre and X; dX = read dpre and X, write dX; row sums = read dpre and X; dgamma / dbeta = read the row sums
        rows = [(f"fwd_on_gn{i}_stat", 4 * n * 2 * B, wg(2 * B)), (f"fwd_on_gn{i}", 2 * 4 * n * 2 * B, wg(2 * B)), (f"fwd_tg_gn{i}_stat", 4 * n * B, wg(B)), (f"fwd_tg_gn{i}", 2 * 4 * n * B, wg(B)),
                (f"bwd_gn{i}_sums", 2 * 4 * n * B, wg(B)), (f"bwd_gn{i}", 3 * 4 * n * B, wg(B)), (f"bwd_gn{i}_rows", 2 * 4 * n * B, (n + 3) // 4), (f"bwd_gn{i}_par", 2 * 4 * n, (c + 3) // 4)]
        print(f"  layer {i}: (c, h*w, G) = ({c}, {hw}, {G}), n_g = {ng} rows = {nch} chunks")
        for k, b, w in rows:
            tot += med[k]
            print(f"    {k:18s} {med[k]:7.2f} us   {b / 1e6:8.3f} MB compulsory   {b / (med[k] * 1e-6) / 1e12:6.3f} TB/s = {100 * b / (med[k] * 1e-6) / HBM_PEAK:5.1f} % of the 8 TB/s peak   {w:5d} workgroups")
    print(f"  the gn launches together: {tot:.1f} us")
    print("  all launches:", "  ".join(f"{k} {v:.1f}" for k, v in med.items()))
    t_gn = step_us(h); h.close()
    h0 = engine(pkg, nn, without, B, obs); t0 = step_us(h0); h0.close()
    print(f"  step time (dqn_train_steps(200), median of 5): with the layers {t_gn:.1f} us, without {t0:.1f} us (+{t_gn - t0:.1f} us)")


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    pkg = ge.load_package(); pkg.lib()
    nn = importlib.import_module(pkg.__name__ + ".nn")
    r = nn.relu
    report(pkg, nn, "smallest case", nn.Chain(nn.Conv(3, 1, 4, r), nn.GroupNorm(4, 2, r), nn.flattenbatch, nn.Dense(64, 4)), nn.Chain(nn.Conv(3, 1, 4, r), nn.flattenbatch, nn.Dense(64, 4)), 5, (1, 6, 6), a.reps)
    for B in (32, 512):
        gn = nn.Chain(nn.Conv(8, 4, 32, r, 4), nn.GroupNorm(32, 4, r), nn.Conv(4, 32, 64, r, 2), nn.GroupNorm(64, 4, r), nn.Conv(3, 64, 64, r, 1), nn.GroupNorm(64, 4, r), nn.flattenbatch,
                      nn.Dense(3136, 512, r), nn.Dense(512, 4))
        report(pkg, nn, "Nature-DQN + GroupNorm(c, 4, relu) x 3", gn, nn.nature_dqn(4, 4), B, (4, 84, 84), a.reps)


if __name__ == "__main__":
    main()
