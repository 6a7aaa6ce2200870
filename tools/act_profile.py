"""usage (GPU box, repo root): python tools/act_profile.py [--reps 11]
The standalone activation layer's launches of one train step (dqn_profile_step; csrc/act_layer.hip, layer kind 14): `fwd_on_act1` (the online pass on [s; s'], 2B columns),
`fwd_tg_act1` (the target pass, B columns) and `bwd_act1`, for gelu (Float64 transcendentals, derivative from the input) and relu (two selects, derivative from the output),
on a (64, 7, 7) map -- Conv(3, 4 => 64) -> Activation -> Dense(3136, 64, relu) -> Dense(64, 4) -- and on a 512-vector -- Dense(64, 512) -> Activation -> Dense(512, 4) --, at
B = 32 and B = 512.  The median us of each launch over `reps` profiled steps (after a warm-up of the shapes), its compulsory bytes, the resulting TB/s against the 8 TB/s HBM
peak of MI355X_MICROARCH.md (a yardstick, not a bound: at these sizes the operands sit in cache), its workgroup count, and the launch floor (the fastest launch of the
profiled steps).  One box, one call: quote it that way (docs/history/activation_layer.md)."""
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
        h.replay_add(rng.standard_normal((256,) + obs).astype(np.float32), rng.integers(0, 4, 256).astype(np.int32), rng.standard_normal(256).astype(np.float32),
                     rng.standard_normal((256,) + obs).astype(np.float32), (rng.random(256) < 0.1).astype(np.uint8))
    h.set_params(nn.glorot_params(net, seed=1), 0); h.sync_target()
    return h


def report(pkg, nn, shape, sigma, name, B, reps):
    if shape == "map":
        obs, n = (4, 9, 9), 64 * 7 * 7
        net = nn.Chain(nn.Conv(3, 4, 64), nn.Activation(sigma), nn.flattenbatch, nn.Dense(n, 64, nn.relu), nn.Dense(64, 4))
    else:
        obs, n = (64, 1, 1), 512
        net = nn.Chain(nn.Dense(64, 512), nn.Activation(sigma), nn.Dense(512, 4))
    h = engine(pkg, nn, net, B, obs)
    h.train_steps(20)
    for _ in range(3):
        h.profile_step(max_entries=256)
    runs = [dict(h.profile_step(max_entries=256)) for _ in range(reps)]
    med = {nm: statistics.median(r[nm] for r in runs) * 1e3 for nm in runs[0]}
    floor = min(med.values())
    quads = lambda cols: (cols + 3) // 4
    # compulsory bytes: forward = read X over the pass's columns, write Y; backward = read dY and the input (gelu) or the output (relu), write dX
    rows = [("fwd_on_act1", 4 * n * 2 * (2 * B), (n * quads(2 * B) + 255) // 256), ("fwd_tg_act1", 4 * n * 2 * B, (n * quads(B) + 255) // 256), ("bwd_act1", 4 * n * 3 * B, (n * quads(B) + 255) // 256)]
    print(f"Activation({name}) on a {'(64, 7, 7) map' if shape == 'map' else '512-vector'}, B = {B}: median of {reps} profiled steps (eager launches, HIP events); launch floor {floor:.1f} us; "
          f"step {sum(med.values()):.1f} us over {len(med)} launches")
    for nm, b, wg in rows:
        us = med[nm]; tb = b / (us * 1e-6) / 1e12
        print(f"  {nm:12s} {b / 1e6:8.3f} MB compulsory = {b / HBM_PEAK * 1e6:6.3f} us at peak   {us:7.2f} us = {us / floor:4.2f} x floor   {tb:6.3f} TB/s = {100 * tb * 1e12 / HBM_PEAK:5.1f} % of peak   {wg:5d} workgroups")
    h.close()


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    pkg = ge.load_package(); pkg.lib()
    nn = importlib.import_module(pkg.__name__ + ".nn")
    for shape in ("map", "vec"):
        for B in (32, 512):
            for sigma, name in ((nn.gelu, "gelu"), (nn.relu, "relu")):
                report(pkg, nn, shape, sigma, name, B, a.reps)


if __name__ == "__main__":
    main()
