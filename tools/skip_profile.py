"""usage (GPU box, repo root): python tools/skip_profile.py [--n 512] [--reps 11]
The skip-block launches of one train step (dqn_profile_step) on Dense(64, n, relu) -> SkipConnection(Chain(Dense(n, n, relu)), +) -> Dense(n, 4), f32 vector
observations, B = 32 and B = 512 (the inner layer carries an activation so that the join's backward is a launch, not an alias): the median us of fwd_on_skip2,
fwd_tg_skip2, bwd_join_skip2 and bwd_entry_skip2 over `reps` profiled steps (after a warm-up of the shapes), their compulsory bytes over that time against the 8 TB/s
HBM peak, and the step time (dqn_train_steps, graphs) beside the same layers WITHOUT the connection at the same build.  The yardsticks are Dropout's fwd_on_do1 and
LayerNorm's fwd_on_ln1 at the same (n, columns): run tools/do_profile.py and tools/ln_profile.py in the same call.  One box, one call: quote it that way
(docs/history/skip.md)."""
import argparse
import importlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge
from ln_profile import HBM_PEAK, engine, step_us


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--n", type=int, default=512); ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args(); n = a.n
    pkg = ge.load_package(); pkg.lib()
    nn = importlib.import_module(pkg.__name__ + ".nn")
    for B in (32, 512):
        with_skip = nn.Chain(nn.Dense(64, n, nn.relu), nn.SkipConnection(nn.Chain(nn.Dense(n, n, nn.relu)), "+"), nn.Dense(n, 4))
        without = nn.Chain(nn.Dense(64, n, nn.relu), nn.Dense(n, n, nn.relu), nn.Dense(n, 4))
        h = engine(pkg, nn, with_skip, B)
        h.train_steps(20)
        for _ in range(3):
            h.profile_step(max_entries=256)
        runs = [dict(h.profile_step(max_entries=256)) for _ in range(a.reps)]
        med = {k: statistics.median(r[k] for r in runs) * 1e3 for k in runs[0]}
        # compulsory bytes: forward = read both operands + write y over the pass's columns; join = read dY and y_K, write dK; entry = read dF, dY and y_P, write dP, over B columns
        byt = {"fwd_on_skip2": 3 * 4 * n * 2 * B, "fwd_tg_skip2": 3 * 4 * n * B, "bwd_join_skip2": 3 * 4 * n * B, "bwd_entry_skip2": 4 * 4 * n * B}
        print(f"B = {B}, n = {n}: median of {a.reps} profiled steps (eager launches, HIP events); whole profiled step {sum(med.values()):.1f} us in {len(med)} launches")
        for k, b in byt.items():
            print(f"  {k:16s} {med[k]:7.2f} us   {b / 1e6:7.3f} MB compulsory   {b / (med[k] * 1e-6) / 1e12:6.3f} TB/s = {100 * b / (med[k] * 1e-6) / HBM_PEAK:5.1f} % of the 8 TB/s peak")
        print("  all launches:", "  ".join(f"{k} {v:.1f}" for k, v in med.items()))
        t_sk = step_us(h); h.close()
        h0 = engine(pkg, nn, without, B); t0 = step_us(h0); h0.close()
        print(f"  step time (dqn_train_steps(400), median of 5): with the connection {t_sk:.1f} us, without {t0:.1f} us (+{t_sk - t0:.1f} us)")


if __name__ == "__main__":
    main()
