"""usage (GPU box, repo root): python tools/pool_profile.py [--reps 11]
The whole-map pool launches of one train step (dqn_profile_step): csrc/pool_global.hip (GlobalMaxPool / GlobalMeanPool, layer kinds 12 / 13) against csrc/pool.hip on the SAME
geometry (MaxPool / MeanPool((h, w)), kinds 5 / 6), on Conv(3, 4 => c, relu) -> pool -> Dense(c, 64, relu) -> Dense(64, 4) with the pool's input map (c, h, w) = (64, 7, 7) and
(32, 20, 20), at B = 32 and B = 512.  Both engines live in one process and take turns, profiled step by profiled step (after a warm-up of the shapes): the median us of each
`pool` launch over `reps` steps, its compulsory bytes, the resulting TB/s against the 8 TB/s HBM peak, its workgroup count against the chip's 256 CUs, and the launch floor
(the fastest launch of the profiled steps).  One box, one call: quote it that way (docs/history/global_pool.md)."""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

HBM_PEAK = 8.0e12


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


def report(pkg, nn, kind, c, hw, B, reps):
    obs = (4, hw[0] + 2, hw[1] + 2); n = hw[0] * hw[1]
    glob, pool = (nn.GlobalMaxPool, nn.MaxPool) if kind == "max" else (nn.GlobalMeanPool, nn.MeanPool)
    net = lambda p: nn.Chain(nn.Conv(3, 4, c, nn.relu), p, nn.flattenbatch, nn.Dense(c, 64, nn.relu), nn.Dense(64, 4))
    hs = {"pool_global.hip": engine(pkg, nn, net(glob()), B, obs), "pool.hip": engine(pkg, nn, net(pool(hw)), B, obs)}
    for h in hs.values():
        h.train_steps(20)
        for _ in range(3):
            h.profile_step(max_entries=256)
    runs = {k: [] for k in hs}
    for _ in range(reps):      # alternating
        for k, h in hs.items():
            runs[k].append(dict(h.profile_step(max_entries=256)))
    med = {k: {nm: statistics.median(r[nm] for r in rs) * 1e3 for nm in rs[0]} for k, rs in runs.items()}
    floor = min(min(m.values()) for m in med.values())
    tiles = lambda cols: (cols + 63) // 64 if cols % 4 == 0 else (cols + 15) // 16
    quads = lambda cols: (cols + 3) // 4
    # compulsory bytes: forward = read X over the pass's columns, write Y; backward = read X and dY, write dX
    rows = [("fwd_on_pool1", 4 * c * (n + 1) * 2 * B, c * tiles(2 * B), (c * quads(2 * B) + 255) // 256), ("fwd_tg_pool1", 4 * c * (n + 1) * B, c * tiles(B), (c * quads(B) + 255) // 256),
            ("bwd_pool1", 4 * c * (2 * n + 1) * B, c * tiles(B), (c * n * quads(B) + 255) // 256)]
    print(f"{kind}pool over a ({c}, {hw[0]}, {hw[1]}) map, B = {B}: median of {reps} profiled steps, alternating (eager launches, HIP events); launch floor {floor:.1f} us")
    for nm, b, wg_new, wg_old in rows:
        a, o = med["pool_global.hip"][nm], med["pool.hip"][nm]
        tb = lambda us: b / (us * 1e-6) / 1e12
        print(f"  {nm:13s} {b / 1e6:8.3f} MB compulsory   pool_global.hip {a:7.2f} us {tb(a):6.3f} TB/s = {100 * tb(a) * 1e12 / HBM_PEAK:5.1f} % of peak, {wg_new:5d} workgroups   "
              f"pool.hip {o:7.2f} us {tb(o):6.3f} TB/s = {100 * tb(o) * 1e12 / HBM_PEAK:5.1f} %, {wg_old:5d} workgroups   ratio {o / a:5.2f}x")
    for h in hs.values():
        h.close()


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    pkg = ge.load_package(); pkg.lib()
    nn = importlib.import_module(pkg.__name__ + ".nn")
    for c, hw in ((64, (7, 7)), (32, (20, 20))):
        for B in (32, 512):
            for kind in ("max", "mean"):
                report(pkg, nn, kind, c, hw, B, a.reps)


if __name__ == "__main__":
    main()
