"""usage (GPU box, repo root): python tools/conv_dg_profile.py [--reps 7] [--against deepqlearning.jl_amd/build/<other>.so]
The launches of a dilated / grouped / depthwise Conv (csrc/conv_own.hip, layer kind 15) in a MIDDLE train step (dqn_profile_steady_step), beside the padded Conv's
(the same file's other geometry) on the same map: Conv(1, 4 => 32, relu) -> LAYER -> GlobalMeanPool -> Dense(32, 4) on (4, 20, 20) observations, LAYER one of
    padded     Conv(3, 32 => 32, relu; pad = 1)                 the yardstick: 32 x 9 x 32 x 400 MACs per column
    depthwise  DepthwiseConv(3, 32 => 32, relu; pad = 1)        1 / 32 of the yardstick's MACs
    grouped    Conv(3, 32 => 32, relu; groups = 2, pad = 1)     half of them
    dilated    Conv(3, 32 => 32, relu; dilation = 2, pad = 2)   the same work
at B = 32 and B = 512: the median us of `fwd_on`, `fwd_tg`, `dw` and `bwd` of layer 1 over `reps` profiled steps, the compulsory bytes of each, and the launch floor (the
fastest launch of the profiled steps).  --against: the padded rows are measured a second time in a child process under that library (DQN_MI355X_LIB), e.g. a build of the
parent commit -- the same box, the same call.  One box, one call: quote it that way (docs/history/conv_dilation_groups.md)."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

OBS, C, HW = (4, 20, 20), 32, 400


def layer(nn, which):
    return {"padded": lambda: nn.Conv(3, C, C, nn.relu, pad=1), "depthwise": lambda: nn.DepthwiseConv(3, C, C, nn.relu, pad=1),
            "grouped": lambda: nn.Conv(3, C, C, nn.relu, groups=2, pad=1), "dilated": lambda: nn.Conv(3, C, C, nn.relu, dilation=2, pad=2)}[which]()


def measure(pkg, nn, which, B, reps):
    net = nn.Chain(nn.Conv(1, OBS[0], C, nn.relu), layer(nn, which), nn.GlobalMeanPool(), nn.flattenbatch, nn.Dense(C, 4))
    layers, _ = nn.lower(net); n = max(1024, 2 * B)
    h = pkg.Engine(layers, pkg.default_hparams(batch_size=B, n_actions=4, obs_c=OBS[0], obs_h=OBS[1], obs_w=OBS[2], dueling=0, buffer_size=n, learning_rate=1e-4, seed=1))
    rng = np.random.default_rng(0)
    for _ in range(0, n, 256):
        h.replay_add(rng.standard_normal((256,) + OBS).astype(np.float32), rng.integers(0, 4, 256).astype(np.int32), rng.standard_normal(256).astype(np.float32),
                     rng.standard_normal((256,) + OBS).astype(np.float32), (rng.random(256) < 0.1).astype(np.uint8))
    h.set_params(nn.glorot_params(net, seed=1), 0); h.sync_target()
    h.train_steps(20)
    for _ in range(3):
        h.profile_step(max_entries=256, steady=True)
    runs = [dict(h.profile_step(max_entries=256, steady=True)) for _ in range(reps)]
    plan = h.plan()[1]; h.close()
    med = {nm: statistics.median(r[nm] for r in runs) * 1e3 for nm in runs[0]}
    tag = "conv" if which == "padded" else "cdg"
    pick = lambda op: next(v for k, v in med.items() if f"{op}_{tag}1" in k.split("+"))
    return dict(which=which, B=B, floor=min(med.values()), step=sum(med.values()), plan=plan, spread={op: [min(r[k] for r in runs) * 1e3, max(r[k] for r in runs) * 1e3]
                                                                                                  for op in ("fwd_on", "fwd_tg", "dw", "bwd") for k in runs[0] if f"{op}_{tag}1" in k.split("+")},
                us={op: pick(op) for op in ("fwd_on", "fwd_tg", "dw", "bwd")})


def compulsory(which, B, plan):
    """bytes each launch must move: the map in, the weights, the map out; dW writes one (K + 1) x N block per plan chunk"""
    K = 9 if which == "depthwise" else 9 * C // 2 if which == "grouped" else 9 * C
    m = 4 * C * HW; w = 4 * (K + 1) * C; S = 1 if plan[2] <= 0 else -(-HW * B // plan[2])
    return {"fwd_on": 2 * m * 2 * B + w, "fwd_tg": 2 * m * B + w, "dw": 2 * m * B + S * w, "bwd": 3 * m * B + w}


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--against", default=""); ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    pkg = ge.load_package(); pkg.lib()
    nn = importlib.import_module(pkg.__name__ + ".nn")
    if a.child:      # the padded rows only, as JSON: what a library without kind 15 can run
        print(json.dumps([measure(pkg, nn, "padded", B, a.reps) for B in (32, 512)]))
        return
    rows = [measure(pkg, nn, w, B, a.reps) for B in (32, 512) for w in ("padded", "depthwise", "grouped", "dilated")]
    if a.against:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], env=dict(os.environ, DQN_MI355X_LIB=os.path.abspath(a.against)), check=True,
                             capture_output=True, text=True).stdout
        for r in json.loads(out.strip().splitlines()[-1]):
            rows.append(dict(r, which="padded@" + os.path.basename(a.against)))
    for B in (32, 512):
        print(f"B = {B}: median of {a.reps} middle steps (eager launches, HIP events), us [min .. max of the runs]; compulsory MB")
        for r in (r for r in rows if r["B"] == B):
            cb = compulsory(r["which"].split("@")[0], B, r["plan"])
            print(f"  {r['which']:22s} floor {r['floor']:5.1f}  step {r['step']:7.1f}  plan {tuple(r['plan'])}  " +
                  "  ".join(f"{op} {r['us'][op]:6.1f} [{r['spread'][op][0]:.1f} .. {r['spread'][op][1]:.1f}] {cb[op] / 1e6:.2f} MB" for op in ("fwd_on", "fwd_tg", "dw", "bwd")))


if __name__ == "__main__":
    main()
