// rollout_sched.h -- THE cadence of the device environment loop, stated once: when train steps and a target sync are due (src/solver.jl:134-145), and which unit of
// work starts at a vector step.  Pure C++ over dqn_rollout_cfg and host-known facts: no HIP header, so tests/host/rollout_sched_main.cpp holds it to the reference's
// own loop as a stand-alone program.  dqn_rollout_explore (feed-forward and recurrent engines) and dqn_rollout_many read every decision from here.
#pragma once
#include <algorithm>
#include "../../include/dqn_mi355x.h"

// after vector step t (counting from 1) of n copies: the train steps that run back to back, and whether the target network is synced behind them
struct RollDue { long long due; bool sync; };
static inline RollDue rollout_due(const dqn_rollout_cfg& c, long long t, long long n) {
    const long long tf = c.train_freq, tu = c.target_update_freq;
    // cadence_env_steps: the frequencies count ENV steps -- every multiple crossed by the n env steps of vector step t
    if (c.cadence_env_steps) return {tf > 0 ? (t * n) / tf - ((t - 1) * n) / tf : 0, tu > 0 && (t * n) / tu != ((t - 1) * n) / tu};
    return {tf > 0 && t % tf == 0 ? 1 : 0, tu > 0 && t % tu == 0};      // ... else VECTOR steps
}

// the unit that starts at vector step t.  PLAIN: one acting step, then rollout_due's train steps (where the replay holds a batch) and sync, each a call of its own.
// CYCLE: rollout_cycle_len acting steps + the train step due at the last of them as ONE graph.  ENVC: one acting step + its n / train_freq train steps as ONE graph
enum RollUnit { ROLL_PLAIN = 0, ROLL_CYCLE = 1, ROLL_ENVC = 2 };
struct RollFacts {
    bool graph, single, tiny, rec;      // graphs in use (use_graph, not profiling); one device, no forced communicator; the single-workgroup train step; a recurrent engine
    long long n, left;                  // copies; vector steps left in the call, step t included
    long long size, cap, B;             // the replay before step t's experiences are in, its capacity, the batch size
};
static inline int rollout_cycle_len(const dqn_rollout_cfg& c) { return c.train_freq > 0 ? c.train_freq : 4; }      // (4 acting steps when nothing trains)
static inline RollUnit rollout_unit(const dqn_rollout_cfg& c, long long t, const RollFacts& f) {
    if (f.rec || !f.graph || !f.single) return ROLL_PLAIN;      // a recurrent engine's draw is a host decision: no whole-step graphs
    const long long tf = c.train_freq, tu = c.target_update_freq;
    if (c.cadence_env_steps) {
        // every vector step owes the same number of train steps and the replay holds a batch once this step's experiences are in
        return !f.tiny && tf > 0 && f.n % tf == 0 && f.n / tf <= 64 && std::min(f.cap, f.size + f.n) >= f.B ? ROLL_ENVC : ROLL_PLAIN;
    }
    const long long F = rollout_cycle_len(c), tl = t + F - 1;      // tl: the cycle's last step
    if (F < 2 || F > 16 || f.left < F) return ROLL_PLAIN;
    // the train step due exactly at the cycle's last step, the replay holding a batch by then, no target sync before the last step
    if (tf > 0 && !(tl % tf == 0 && std::min(f.cap, f.size + F * f.n) >= f.B)) return ROLL_PLAIN;
    if (tu > 0) for (long long u = t; u < tl; u++) if (u % tu == 0) return ROLL_PLAIN;
    return ROLL_CYCLE;
}
