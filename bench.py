#!/usr/bin/env python3
"""
bench.py -- train steps/sec of the MI355X DQN engine on BASELINE.json's metric:
    "train steps/sec (batch=32, 84x84x4 obs)": Synthetic 84x84x4 image MDP (the reference's own TestMDP((84,84),4,6),
    test/test_env.jl), Nature-DQN 3-conv+2-dense dueling head, batch=32, double-Q, prioritized replay  (configs[1]).
One step = one batch_train! (src/solver.jl:191-236): sum-tree sample -> gather + IS weights -> online([s;sp]) and
target(sp) forwards -> double-Q Bellman target -> Huber(w*td)/B -> backward -> max-abs grad norm -> Adam -> priority update.

    python bench.py --gpus 1 --steps 200 --warmup 20
    python bench.py --gpus 1 --steps 200 --warmup 20 --full
    python bench.py --gpus 1 --steps 200 --warmup 20 --dump-outputs DIR
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

N > 1: one process per GPU, per-rank envs + replay (weak scaling: B=32 per rank), gradients all-reduced over RCCL
between backward and Adam.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the headline.  --full adds the untimed measurements around it: the
per-launch profile and roofline, the device env loop, the sustained region, the per-call seam, the secondary configurations and the CPU
baselines.  --dump-outputs DIR writes what the timed call left a caller after its last step as DIR/<name>.npy (dump_outputs below).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_* dense peak
PEAK_HBM_GBS = 8000.0          # HBM3E spec


def build_workload(pkg, args, rank, device):
    nn, envs = pkg.nn, pkg.envs
    chain = nn.nature_dqn(n_actions=4, in_channels=4)
    net = nn.create_dueling_network(chain)
    layers, dueling = nn.lower(net)
    hp = pkg.default_hparams(batch_size=args.batch, n_actions=4, obs_c=4, obs_h=84, obs_w=84, obs_dtype=pkg.OBS_U8 if args.u8 else pkg.OBS_F32,
                             learning_rate=1e-4, gamma=0.99, double_q=1, dueling=1, prioritized_replay=1, buffer_size=args.replay,
                             seed=1234 + rank, use_graph=0 if args.no_graph else 1, use_mfma=0 if args.no_mfma else 1, sample_distinct=1 if getattr(args, "distinct", False) else 0)
    plan = None
    if args.conv_kc:
        plan = [(args.conv_kc if (d.kind == pkg._abi.LAYER_CONV and d.cin * d.kh * d.kw > args.conv_kc) else p[0], p[1], p[2]) for d, p in zip(layers, pkg.default_plan(layers, hp))]
    if args.fc_kc:      # experiment knob: forward split-K chunk of the 3136-wide dense layers (the plan only fixes rounding order)
        plan = [(args.fc_kc if (d.kind == pkg._abi.LAYER_DENSE and d.n_in > 1024) else p[0], p[1], p[2]) for d, p in zip(layers, pkg.default_plan(layers, hp))]
    if getattr(args, "dw_wgs", 0):      # experiment knob: conv dW split -- whole positions per chunk so that (K/64 row tiles) x chunks ~ dw_wgs workgroups (default plan: 512)
        base = plan if plan is not None else pkg.default_plan(layers, hp)
        plan = []
        h = w = 84
        for d, p in zip(layers, base):
            if d.kind == pkg._abi.LAYER_CONV:
                h, w = (h - d.kh) // d.sh + 1, (w - d.kw) // d.sw + 1
                mrows = -(-(d.cin * d.kh * d.kw) // 64); st = max(1, -(-args.dw_wgs // mrows)); ppc = max(1, (h * w) // st)
                plan.append((p[0], p[1], ppc * args.batch))
            else:
                plan.append(p)
    eng = pkg.Engine(layers, hp, plan=plan, device=device)
    params = nn.glorot_params(net, seed=1)           # identical replicas on every rank
    eng.set_params(params, pkg.NET_ONLINE)
    eng.set_params(params, pkg.NET_TARGET)
    # replay pre-filled by a uniform-random policy on this rank's shard of the vectorised envs
    env = envs.TestMDP((84, 84), 4, 6, n=args.envs_per_rank, seed=7, u8=args.u8)
    env.rng = np.random.default_rng(1000 + rank)
    filled = 0
    o = env.observe()
    t_fill, n_host = time.perf_counter(), 0
    if args.device_fill:
        n_fill = min(1024, args.replay)
        eng.envs_create(env, n_envs=n_fill, max_episode_length=100, seed=1000 + rank)
        eng.rollout(-(-args.replay // n_fill), t0=1, train_freq=0, target_update_freq=0, eps=(1.0, 1.0, 1.0), stats=False)   # eps = 1: uniform-random actions
        eng.sync()
        filled = args.replay
    while filled < args.replay:
        a = env.rng.integers(0, 4, env.n)
        r = env.act(a)
        op = env.observe()
        d = env.terminated()
        eng.replay_add(o, a.astype(np.int32), r, op, d.astype(np.uint8))   # priority (|r|+eps)^alpha (...replay.jl:122)
        filled += env.n; n_host += env.n
        env.reset(d)
        o = env.observe()
    eng.sync()
    # what the boundary costs when the caller hands over HOST observation buffers (dqn_replay_add: rows copied over PCIe straight into their ring slots; the host env
    # mirror's own stepping is inside this time too).  Never part of `value`: the train step starts with everything resident in HBM.
    fill_s = time.perf_counter() - t_fill
    row_b = 2 * 4 * 84 * 84 * (1 if args.u8 else 4)
    HOST_FILL.update({"transitions_from_host": n_host, "seconds": fill_s, "transitions_per_s": n_host / fill_s if n_host else None,
                      "pcie_GBps_incl_host_env": n_host * row_b / fill_s / 1e9 if n_host else None, "bytes_per_transition": row_b})
    return eng, layers, hp, net, params, env


HOST_FILL = {}


args_ms_plain = [None]      # ms per step of the headline run (read by secondary_block's dp_model)
ADAM_SLAB_BYTES = [0.0]     # the engine's OWN overhead inside k_adam (conv dW split-K slabs it reduces): reported beside, never inside, the 8(d) floor


ARENA_ELEM_BYTES = [4]      # set from the engine (dqn_batch_arena_elem_bytes) before the launch table is priced


def op_cost(name, eng_layers, B, ncon, E, P, obs_bytes=4):
    """algorithmic (flops, bytes) of one profiled launch by its program name; names joined by '+' are one launch doing both.
    fwd_<l>      forward of layer l AND its sibling (val/adv) for the online net on [s;sp] and the target net on sp
    dw_<l>/dw2_<l>  dW+db of layer l (dw2: both sibling layers);  dx_<l>/dx_join_<l>  dX of layer l (join: both streams)
    adam         SURVEY 8(d)'s parameter-traffic floor: 28 B per parameter (p, m, v, g read; p, m, v written) -- 92 199 436 B at config 2"""
    if "+" in name:
        parts = [op_cost(n, eng_layers, B, ncon, E, P, obs_bytes) for n in name.split("+")]
        return sum(p[0] for p in parts), sum(p[1] for p in parts)
    parts = name.split("_")
    if name in ("gather", "sample_gather"):
        return 0.0, 2.0 * B * E * (obs_bytes + ARENA_ELEM_BYTES[0])   # rows read (u8 or f32) + batch arena written (fp32, or bytes for u8 replays)
    if name.startswith("adam"):
        return 0.0, P * 28.0
    digits = "".join(ch for ch in parts[-1] if ch.isdigit())
    if not digits or parts[0] not in ("fwd", "dw", "dw2", "dx"):
        return 0.0, 0.0
    li = int(digits)
    K, N, npos = eng_layers[li]
    f1 = 2.0 * K * N * npos
    nsib = sum(1 for g in eng_layers if g == eng_layers[li]) if (K, N, npos).count(0) == 0 else 1
    if parts[0] == "fwd":
        if len(parts) == 3 and parts[1] in ("on", "tg"):
            return f1 * (ncon if parts[1] == "on" else B), 0.0
        if len(parts) == 3:                       # fwd_valu_<l> / fwd_reduce_<l>: head forwards / split-K folds (negligible flops)
            return 0.0, 0.0
        return f1 * (ncon + B) * nsib, 0.0
    if parts[0] == "dw2" or (parts[0] == "dx" and len(parts) == 3 and parts[1] == "join"):
        return f1 * B * 2, 0.0
    return f1 * B, 0.0


def step_flops_analytic(eng_layers, B, ncon):
    """forward on (2B + B) columns for every layer, backward dW for every layer and dX for every layer with a producer."""
    tot = 0.0
    for i, (K, N, npos) in enumerate(eng_layers):
        f1 = 2.0 * K * N * npos
        tot += f1 * (ncon + B) + f1 * B + (f1 * B if i > 0 else 0.0)
    return tot


class quiet_stdout:
    """RCCL prints a version banner to the C stdout when a communicator is created; the driver parses ONE JSON line from this script's stdout.  File descriptor 1 points at
    /dev/null while the communicator is made, and the C stdio buffer is flushed into it before the descriptor is restored."""
    def __enter__(self):
        import ctypes
        sys.stdout.flush()
        self._libc = ctypes.CDLL(None); self._libc.fflush(None)
        self._saved = os.dup(1); dn = os.open(os.devnull, os.O_WRONLY); os.dup2(dn, 1); os.close(dn)
        return self

    def __exit__(self, *exc):
        sys.stdout.flush(); self._libc.fflush(None)
        os.dup2(self._saved, 1); os.close(self._saved)
        return False


def layer_geo(pkg, layers, hw=84):
    """(K, N, npos) per layer of an image network on hw x hw observations"""
    h = w = hw
    g2 = []
    for d in layers:
        if d.kind == pkg._abi.LAYER_CONV:
            h, w = (h - d.kh) // d.sh + 1, (w - d.kw) // d.sw + 1
            g2.append((d.cin * d.kh * d.kw, d.cout, h * w))
        else:
            g2.append((d.n_in, d.n_out, 1))
    return g2


def roofline_block(pkg, eng, layers, batch, u8, world, value, ms_per_step, prof_acc, single_gather):
    """The `roofline` object of one image-network engine: headline fraction on the TIMED rate + the per-launch table from live HIP-event durations."""
    B, ncon, E, P = batch, 2 * batch, 4 * 84 * 84, eng.P
    g2 = layer_geo(pkg, layers)
    # single-GPU path: k_adam also reduces the conv layers' dW split-K slabs (S slabs of (K+1) x N floats read once, gradient written) --
    # the engine's own overhead on top of the 8(d) floor
    ADAM_SLAB_BYTES[0] = 0.0
    if world == 1:
        for (K, N, npos), (_, _, dw_kc) in zip(g2, eng.plan()):
            S = -(-npos * B // dw_kc) if dw_kc and dw_kc < npos * B else 1
            if S > 1:
                ADAM_SLAB_BYTES[0] += (S + 1) * (K + 1) * N * 4.0
    kern = {k: v[0] / v[1] for k, v in prof_acc.items()}
    ARENA_ELEM_BYTES[0] = eng.batch_arena_elem_bytes()
    cfg2 = batch == 32 and not u8 and world == 1
    cfg5 = batch == 512 and u8 and world == 1
    PMC_OK[0] = "cfg2" if cfg2 else ("cfg5" if cfg5 else None)     # the committed PMC passes are runs of the single-GPU config-2 / config-5 bench (a replica's Adam launch is a different kernel: traffic = null)
    obs_b = 1 if u8 else 4
    step_flops = step_flops_analytic(g2, B, ncon)
    # ---- headline: the train step is a dense contraction => bound by the fp32 MFMA peak;
    #      achieved = steps/s x algorithmic FLOP per step (adv stream once, no conv1 dX), on the TIMED (graph-replay) rate
    ach = (value / world) * step_flops / 1e12
    roof = dict(bound="mfma", achieved=ach, peak=PEAK_F32_MFMA_TFLOPS, unit="TFLOP/s", frac=ach / PEAK_F32_MFMA_TFLOPS, traffic=None,
                definition="steps/s x step_flops / fp32-MFMA peak (SURVEY.md 8d); step_flops = fwd 2KN*npos x (2B online + B target) columns + dW x B + dX x B (no conv1 dX)",
                step_flops=step_flops, step_gflop=step_flops / 1e9)
    # ---- per-launch table: algorithmic MFLOP or MB, HIP-event duration (eager launches, engine stream), fraction of the bound that applies
    table = []
    for name, ms in sorted(kern.items(), key=lambda kv: -kv[1]):
        fl, by = op_cost(name, g2, B, ncon, E, P, obs_b)
        row = {"launch": name, "avg_us": round(ms * 1e3, 2)}
        if fl > 0:
            row.update(bound="mfma", mflop=round(fl / 1e6, 1), tflops=round(fl / (ms * 1e-3) / 1e12, 2), frac=round(fl / (ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4))
        elif by > 0:
            row.update(bound="hbm", mbytes=round(by / 1e6, 2), gbs=round(by / (ms * 1e-3) / 1e9, 1), frac=round(by / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4))
            if name.startswith("adam") and ADAM_SLAB_BYTES[0] > 0:
                row["overhead_mbytes"] = round(ADAM_SLAB_BYTES[0] / 1e6, 2)      # conv dW slabs: engine overhead, not in `mbytes`
            row.update(pmc_traffic(name))
        else:
            row.update(bound="latency")
        table.append(row)
    roof["launches"] = table
    roof["eager_step_us"] = round(sum(kern.values()) * 1e3, 1)
    gemm = [r for r in table if r.get("bound") == "mfma"]
    if gemm:
        roof["gemm_launches_frac"] = round(sum(r["mflop"] for r in gemm) * 1e6 / (sum(r["avg_us"] for r in gemm) * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)
        roof["longest_gemm_launch"] = dict(max(gemm, key=lambda r: r["avg_us"]))      # per-launch roofline: algorithmic FLOP / HIP-event duration
        # what the event brackets add per launch: (sum of the bracketed launches - the graph-replayed step) / launches.  rocprofv3's begin/end stamps carry none of it
        ev_over = max(0.0, (sum(kern.values()) * 1e3 - ms_per_step * 1e3) / max(1, len(kern)))
        roof["event_overhead_us_per_launch"] = round(ev_over, 2)
        roof["dominant_kernel"] = dominant_kernel(table, "cfg2" if cfg2 else ("cfg5" if cfg5 else None), ev_over)
    gk = dict(kern); gk.update({k: v[0] / v[1] for k, v in single_gather.items()})
    gname = "sample_gather" if "sample_gather" in gk else ("gather" if "gather" in gk else None)
    if gname:
        gbytes = op_cost(gname, g2, B, ncon, E, P, obs_b)[1]
        roof["gather"] = {"avg_launch_ms": gk[gname], "algorithmic_bytes": gbytes, "achieved_GBs": gbytes / (gk[gname] * 1e-3) / 1e9,
                          "frac_of_hbm_peak": gbytes / (gk[gname] * 1e-3) / 1e9 / PEAK_HBM_GBS}
        if gname not in kern:
            roof["gather"]["note"] = "launch of a single dqn_train_step; in the timed dqn_train_steps(K) loop the batch is gathered by the previous step's Adam launch (adam+gather)"
        roof["gather"].update(pmc_traffic(gname))
    adam_rows = [r for r in table if r["launch"].startswith("adam") and "traffic" in r]
    if adam_rows:
        roof["traffic"] = adam_rows[0]["traffic"]; roof["traffic_note"] = "HBM bytes per launch of the Adam kernel (the step's HBM-bound launch); " + adam_rows[0].get("traffic_source", "")
    return roof


def timed_steps(eng, steps, warmup):
    """exactly the headline's protocol on one engine: W untimed warm-up steps, sync, K steps in one call, sync"""
    import torch
    eng.train_steps(max(3, warmup)); eng.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, gn = eng.train_steps(steps)
    eng.sync(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"steps_per_s": steps / dt, "ms_per_step": dt / steps * 1e3, "steps": steps, "warmup": max(3, warmup), "last_loss": loss, "last_grad_norm": gn}


DUMP_LIMIT_BYTES = 64 << 20
RAMP_CALLS, RAMP_STEPS_PER_CALL = 6, 50      # a plain run's untimed clock ramp before its warm-up (main)


def dump_outputs(pkg, eng, out_dir, loss, grad_norm):
    """--dump-outputs: what the timed dqn_train_steps(K) call leaves its caller after the last step, as out_dir/<name>.npy in float32 / float64 --
    the returned loss and grad norm, the online parameters it trained, the replay priorities it rewrote and the indices of the last batch.
    An array over its share of DUMP_LIMIT_BYTES is replaced by a fixed, seeded sample of its elements (flat, in index order)."""
    outs = {"loss": np.array([loss], np.float32), "grad_norm": np.array([grad_norm], np.float32), "params_online": eng.get_params(pkg.NET_ONLINE),
            "replay_priorities": eng.replay_priorities(), "last_indices": eng.last_indices().astype(np.float64)}
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_LIMIT_BYTES // len(outs)
    for name, a in outs.items():
        if a.nbytes > share:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def launch_profile(eng, n, steady=True):
    acc = {}
    for _ in range(n):
        for name, ms in (eng.profile_step(steady=True) if steady else eng.profile_step()):
            a = acc.setdefault(name, [0.0, 0]); a[0] += ms; a[1] += 1
    return acc


def secondary_block(pkg, args, device):
    """BASELINE.json configs[0] (GridWorld MLP), configs[3] (DRQN, the reference's own benchmark shape benchmark/flux_dqn.jl:35-36) and configs[4] (B = 512, 1e6 u8
    transitions), each on its own engine.  `parity_gate` names the -m gpu tests that pin the configuration bit for bit against the twin (the oracle is never touched here)."""
    import argparse as _ap
    nn, envs = pkg.nn, pkg.envs
    S = __import__("importlib").import_module(pkg.__name__ + ".solver")
    out = {"note": "each entry: W warm-up steps, sync, K steps in ONE dqn_train_steps call, sync -- the protocol of `value`; engines created after the headline engine was destroyed"}
    t_all = time.perf_counter()
    # ---- config 1: SimpleGridWorld, Chain(Dense(2,32), Dense(32,4)) dueling + double-Q + prioritized replay, B = 32 (README.md:26-46); ONE launch per step (tiny_step.hip)
    try:
        net = nn.create_dueling_network(nn.Chain(nn.Dense(2, 32), nn.Dense(32, 4)))
        layers, _ = nn.lower(net)
        hp = pkg.default_hparams(batch_size=32, n_actions=4, obs_c=2, obs_h=1, obs_w=1, gamma=0.95, buffer_size=10000)
        e1 = pkg.Engine(layers, hp, device=device)
        e1.set_params(nn.glorot_params(net, seed=1), pkg.NET_ONLINE); e1.sync_target()
        e1.envs_create(envs.SimpleGridWorld(n=256), max_episode_length=100, seed=1)
        e1.rollout(40, t0=1, train_freq=0, eps=(1.0, 1.0, 1.0), stats=False)      # 10 240 transitions from the device env loop, uniform-random policy
        r = timed_steps(e1, 2000, 50)
        r.update(workload="configs[0]: SimpleGridWorld 2-D obs, Chain(Dense(2,32),Dense(32,4)) + create_dueling_network, B=32, double_q+dueling+prioritized, replay 10 240 (device env loop fill)",
                 launches_per_step=len(e1.profile_step(steady=True)), n_params=int(e1.P),
                 parity_gate="tests/test_gpu_parity.py::test_engine_matches_fp64_oracle_and_golden[cfg1_gridworld_mlp_dueling] (torch-fp64 fixture, every field) + test_hand_derived_known_answer + the bit-exact twin cases run under both schedules (DQN_NO_TINY)")
        e1.close(); out["config1"] = r
    except Exception as ex:      # a secondary entry must never take the headline down
        out["config1"] = {"error": repr(ex)}
    # ---- config 4: DRQN, TestMDP((5,5),1,6) obs 25, Chain(flattenbatch, LSTM(25,32), Dense(32,4)), trace_length 8, B = 32, double-Q (benchmark/flux_dqn.jl:35-36)
    try:
        model = nn.Chain(nn.flattenbatch, nn.LSTM(25, 32), nn.Dense(32, 4))
        layers, _ = nn.lower(model)
        hp = pkg.default_hparams(batch_size=32, n_actions=4, obs_c=1, obs_h=5, obs_w=5, gamma=0.99, double_q=1, dueling=0, prioritized_replay=0,
                                 buffer_size=1000, recurrence=1, trace_length=8, learning_rate=1e-3)
        e4 = pkg.Engine(layers, hp, device=device)
        e4.set_params(nn.glorot_params(model, seed=1), pkg.NET_ONLINE); e4.sync_target()
        env4 = envs.TestMDP((5, 5), 1, 6, n=1, seed=7)
        S.populate_episode_replay(S.HIPEpisodeReplayBuffer(e4), env4, max_pop=400, rng=np.random.default_rng(0))
        r = timed_steps(e4, 2000, 40)
        prof = launch_profile(e4, 5, steady=False)
        r.update(workload="configs[3]: recurrence=true DRQN, Chain(flattenbatch, LSTM(25,32), Dense(32,4)) on episodic replay (400 episodes), trace_length=8, B=32, double-Q (benchmark/flux_dqn.jl:35-36)",
                 sequences_per_s=r["steps_per_s"] * 32, launches={k: round(v[0] / v[1] * 1e3, 2) for k, v in prof.items()}, n_params=int(e4.P),
                 parity_gate="tests/test_drqn_gpu.py::test_drqn_bit_exact_vs_twin_and_oracle[cfg4_lstm_plain-*] + test_drqn_fused_step_long_run_wraps_the_draw_ring; bit-exact vs the twin, fp64 oracle to round-off")
        e4.close(); out["config4"] = r
    except Exception as ex:
        out["config4"] = {"error": repr(ex)}
    # ---- config 5: the headline network at B = 512 on a u8 replay of 1e6 transitions (56 GB of rows), filled by the device env loop
    try:
        a5 = _ap.Namespace(**vars(args)); a5.batch = 512; a5.u8 = True; a5.replay = 1_000_000; a5.device_fill = True; a5.distinct = False
        HOST_FILL.clear()
        e5, layers5, hp5, _, _, _ = build_workload(pkg, a5, 0, device)
        fill = dict(HOST_FILL)
        prof = launch_profile(e5, 10)
        single = {}
        for name, ms in e5.profile_step():
            if name in ("gather", "sample_gather"):
                single[name] = [ms, 1]
        r = timed_steps(e5, 100, 10)
        roof = roofline_block(pkg, e5, layers5, 512, True, 1, r["steps_per_s"], r["ms_per_step"], prof, single)
        r.update(workload=workload_name(a5, 1), samples_per_s=r["steps_per_s"] * 512, replay_rows_GB=round(2 * 28224 * 1e6 / 1e9, 1), device_fill_seconds=fill.get("seconds"),
                 roofline=roof, n_params=int(e5.P),
                 parity_gate="tests/test_gpu_parity.py::test_config5_nature_b512_u8_bit_exact (full shape, bit-exact vs the twin) + test_config5_million_transition_properties")
        e5.close(); out["config5"] = r
    except Exception as ex:
        out["config5"] = {"error": repr(ex)}
    # ---- config 5's shape with the REFERENCE's sampling semantics (hp.sample_distinct = 1, ...replay.jl:85): since r06 the priority workgroup that rides a backward launch dedupes
    # the list it pre-draws and the Adam launch pre-gathers it, as in the default mode.  200 000 transitions (11 GB of rows: the fill of a second 1e6 replay is not worth the seconds)
    try:
        a5d = _ap.Namespace(**vars(args)); a5d.batch = 512; a5d.u8 = True; a5d.replay = 200_000; a5d.device_fill = True; a5d.distinct = True
        e5d, _, _, _, _, _ = build_workload(pkg, a5d, 0, device)
        r = timed_steps(e5d, 100, 10)
        names = [n for n, _ in e5d.profile_step(steady=True)]
        a5d.distinct = False
        e5d.close()
        e5s, _, _, _, _, _ = build_workload(pkg, a5d, 0, device)
        rs = timed_steps(e5s, 100, 10)
        e5s.close()
        r.update(workload="configs[4] shape with hp.sample_distinct = 1 (the reference's replace=false draws): " + workload_name(a5d, 1), launches_per_step=len(names), launch_names=names,
                 stratified_same_replay_steps_per_s=rs["steps_per_s"], ratio_to_stratified=r["steps_per_s"] / rs["steps_per_s"],
                 parity_gate="tests/test_gpu_parity.py::test_train_steps_with_distinct_sampling_bit_exact[B512_config5_shape]")
        out["config5_distinct"] = r
    except Exception as ex:
        out["config5_distinct"] = {"error": repr(ex)}
    # ---- what a replica step costs BEFORE any wire time, measured at world 1 through a real RCCL communicator (ncclCommInitRank + ncclAllGather of one rank inside the step
    # graph): the numbers a future multi-GPU SCALE line can be checked against.  Nothing here is a scaling measurement.
    try:
        os.environ["DQN_FORCE_ALLREDUCE"] = "1"
        a3 = _ap.Namespace(**vars(args)); a3.distinct = False; a3.device_fill = True
        e3, _, _, _, _, _ = build_workload(pkg, a3, 0, device)
        with quiet_stdout():
            e3.comm_init(pkg.comm_unique_id(), 0, 1)
        os.environ.pop("DQN_FORCE_ALLREDUCE", None)
        r = timed_steps(e3, 300, 30)
        prof = launch_profile(e3, 10)
        L = {k: v[0] / v[1] * 1e3 for k, v in prof.items()}
        xb = e3.comm_exchange_bytes()
        plain_us = 1e3 * args_ms_plain[0] if args_ms_plain[0] else None
        link = 153e9      # one xGMI link, bytes/s (MI355X guide)
        def model(N):      # replica step at N ranks = measured world-1 replica step + (N - 1) more K tiles in the wide dW + the all-gather over point-to-point links
            wide = sum(v for k, v in L.items() if k.startswith("dp_dw"))
            per_tile = 2.1      # us per additional rank block (one more 32-sample K tile per workgroup): calibrated on the simulated 8-rank run (profiles/history/r01_k_dp8_*: 25.8 us at N = 8)
            ag_direct = xb / link * 1e6 if N > 1 else 0.0; ag_ring = (N - 1) * xb / link * 1e6
            return {"wide_dw_us": round(wide + per_tile * (N - 1), 1), "allgather_direct_us": round(ag_direct, 1), "allgather_ring_us": round(ag_ring, 1), "rccl_latency_us": "10-20 (not measurable at world 1)",
                    "predicted_step_us_direct": round(r["ms_per_step"] * 1e3 + per_tile * (N - 1) + ag_direct + 15.0, 1), "predicted_step_us_ring": round(r["ms_per_step"] * 1e3 + per_tile * (N - 1) + ag_ring + 15.0, 1)}
        out["dp_model"] = {"measured_world1": {"replica_step_us": round(r["ms_per_step"] * 1e3, 2), "plain_step_us": plain_us, "steps_per_s": r["steps_per_s"],
                                                "pack_us": round(sum(v for k, v in L.items() if k.startswith("dp_pack")), 2), "wide_dw_us": round(sum(v for k, v in L.items() if k.startswith("dp_dw")), 2),
                                                "unpack_sum_us": round(L.get("dp_sum_ranks", 0.0), 2), "launches": {k: round(v, 2) for k, v in L.items()}},
                           "exchange_bytes_per_rank": xb, "rccl_nranks": e3.comm_info()["rccl_nranks"],
                           "model": {f"N={N}": model(N) for N in (2, 4, 8)},
                           # weak-scaling efficiency the model implies at N = 8 (per-rank work fixed): plain single-GPU step / predicted replica step.  Both all-gather shapes are
                           # listed because which one RCCL picks on 8 point-to-point-linked GPUs is not observable at world 1.  A PREDICTION, not a measurement.
                           "efficiency_N8": ({"direct_links": round(plain_us / model(8)["predicted_step_us_direct"], 3), "ring": round(plain_us / model(8)["predicted_step_us_ring"], 3),
                                              "assumptions": "plain step measured in this run; replica step at world 1 measured through a real communicator; + 2.1 us per extra rank block in the wide dW (calibrated on the simulated 8-rank run); all-gather = exchange_bytes_per_rank / 153 GB/s (direct: every peer over its own link, concurrently; ring: N - 1 hops); + 15 us RCCL launch / protocol latency (a guess: not measurable at world 1); no overlap of the exchange with compute (DQN_DP_OVERLAP off: its fork + join cost 26 us at world 1)"}
                                             if plain_us else None),
                           "note": "world-1 measurement through a real communicator + a point-to-point xGMI model (153 GB/s per link, one link per peer pair); predicted_step_us = replica step + 2.1 us per extra rank block in the wide dW + all-gather + 15 us RCCL latency; UNMEASURED beyond world 1"}
        e3.close()
    except Exception as ex:
        os.environ.pop("DQN_FORCE_ALLREDUCE", None)
        out["dp_model"] = {"error": repr(ex)}
    # ---- the headline configuration with the REFERENCE's sampling semantics: B distinct indices per batch (sample(...; replace=false), ...replay.jl:85; hp.sample_distinct)
    try:
        a2 = _ap.Namespace(**vars(args)); a2.distinct = True; a2.device_fill = True
        e2, _, _, _, _, _ = build_workload(pkg, a2, 0, device)
        r = timed_steps(e2, 300, 30)
        for _ in range(3):
            e2.train_step(want_td=False)
        e2.sync(); t0 = time.perf_counter()
        for _ in range(300):
            e2.train_step(want_td=False)
        e2.sync(); dt = time.perf_counter() - t0
        r.update(workload="configs[1] with hp.sample_distinct = 1 (the reference's replace=false draws): " + workload_name(a2, 1), per_call_sync_us=dt / 300 * 1e6, per_call_sync_steps_per_s=300 / dt,
                 parity_gate="tests/test_gpu_parity.py::test_train_steps_with_distinct_sampling_bit_exact + test_sampler_distinct_gpu_equals_twin")
        e2.close(); out["config2_distinct"] = r
    except Exception as ex:
        out["config2_distinct"] = {"error": repr(ex)}
    out["seconds"] = time.perf_counter() - t_all
    return out



def workload_name(args, world):
    """which BASELINE.json config the flags describe (configs[] is 0-based: [1] = B=32 on one GPU, [2] = the same sharded over ranks,
    [4] = the B=512 / 1e6-transition u8 stress run); anything else is named by its parameters"""
    base = "TestMDP((84,84),4,6) image MDP, Nature-DQN 3-conv+2-dense dueling, double-Q, prioritized replay"
    if args.batch == 512 and args.u8 and args.replay >= 1_000_000:
        return f"configs[4]: large-batch stress, batch_size=512, replay {args.replay} u8 transitions; {base}"
    if args.batch == 32 and not args.u8:
        if world > 1:
            return f"configs[2]: {args.envs_per_rank * world} envs sharded {world}-way, per-rank replay, one RCCL exchange per step; {base}"
        return f"configs[1]: {base}"
    return f"non-BASELINE variant (batch={args.batch}, replay={args.replay}, {'u8' if args.u8 else 'f32'}): {base}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=80)      # >= 64: the 16-step grouped graph of dqn_train_steps is first launched by a call of 64+ steps -- with the default K = 300 that is the timed call unless the warm-up is one too (r06: one default-flag run in ~16 read 6904 instead of ~8300 steps/s, 7 ms inside the K-step call)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--replay", type=int, default=10000, help="transitions per rank (the reference fixes none for this shape)")
    ap.add_argument("--envs-per-rank", type=int, default=32, help="config 3: 256 envs / 8 ranks")
    ap.add_argument("--u8", action="store_true", help="u8 replay storage (config 5 style)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-mfma", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--profile-steps", type=int, default=20)
    ap.add_argument("--sustained-steps", type=int, default=-1, help="steps of the long-run twin of the timed region (0 = skip; -1 = as many as --sustained-seconds needs at the measured rate)")
    ap.add_argument("--sustained-seconds", type=float, default=10.0, help="GPU time of the sustained region (longer than any SMI sampler's period; runs BEFORE the CPU baseline)")
    ap.add_argument("--order", default="profile-first", choices=["profile-first", "env-first"], help="order of the two untimed secondary sections before the headline (A/B)")
    ap.add_argument("--per-call-steps", type=int, default=-1, help="calls of the per-call seam measurement (dqn_train_step with scalars returned, and its async form); -1 = --steps, 0 = skip")
    ap.add_argument("--dp-overlap", type=int, default=-1, choices=[-1, 0, 1], help="replicas: 1 = exchange the wide dense layers' operands on a third stream under the conv backward (DESIGN.md 8); -1 = engine default")
    ap.add_argument("--device-fill", action="store_true", help="fill the replay with the device-resident env loop (uniform-random policy, eps = 1) instead of host rollouts + PCIe; needed for config 5's 1e6-transition replay")
    ap.add_argument("--env-steps", type=int, default=200, help="vector steps of the device-resident env loop timed after the main metric (0 = skip)")
    ap.add_argument("--conv-kc", type=int, default=0, help="experiment: forward split-K chunk of the conv layers")
    ap.add_argument("--fc-kc", type=int, default=0, help="experiment: override fwd_kc of the wide dense layers")
    ap.add_argument("--dw-wgs", type=int, default=0, help="experiment: target workgroup count of the conv dW split (plan dw_kc)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the `secondary` block (BASELINE configs[0], [3], [4] timed like `value`; default run at N = 1 on the headline workload only)")
    ap.add_argument("--distinct", action="store_true", help="hp.sample_distinct = 1 for the headline engine (the reference's replace=false draws, ...replay.jl:85)")
    ap.add_argument("--full", action="store_true", help="also run the per-launch profile + roofline, env loop, sustained region, per-call seam, secondary configurations and CPU "
                                                          "baselines (the options above that configure them take effect only with --full)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write the timed call's outputs after its last step to DIR/<name>.npy (rank 0)")
    ap.add_argument("--cpu-worker", default="", choices=["", "twin", "torch"], help=argparse.SUPPRESS)      # internal: the CPU-baseline subprocess (cpu_worker below)
    ap.add_argument("--cpu-worker-cpus", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.cpu_worker:
        return cpu_worker(args)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("DQN_BENCH_ONE_DEVICE"):      # debugging aid: all ranks on device 0 (RCCL normally refuses duplicate devices)
        local_rank = 0
    # CI self-test of the N > 1 script path on a ONE-GPU box (tests/test_bench_multiproc_gpu.py): every rank shares device 0 and its engine is
    # created under DQN_SIM_WORLD = world, i.e. the step runs the replica program (two half graphs, pack, wide dW over world*B samples, sum over
    # ranks, Adam with g/world) with the all-gather replaced by local copies of its own block.  Rendezvous, the 128-byte id broadcast, barriers,
    # the max-over-ranks timer and the JSON line are the real ones; only ncclCommInitRank / ncclAllGather are not executed.  The line says so.
    sim_comm = bool(os.environ.get("DQN_BENCH_SIM_COMM")) and world > 1
    if sim_comm:
        local_rank = 0
        os.environ["DQN_SIM_WORLD"] = str(world)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run (one rank per GPU, loopback rendezvous on a free port); rank 0 of the
        # child prints the ONE JSON line, the child's return code is ours.  The torchrun form the driver uses for N > 1 arrives with WORLD_SIZE set and skips this.
        import socket
        import subprocess
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1", "--master-port", str(port),
               os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd, env=env).returncode)
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: a launcher's world size must equal --gpus (plain `python bench.py --gpus N` launches itself)", file=sys.stderr)
        sys.exit(2)

    if args.dp_overlap == 1:
        os.environ["DQN_DP_OVERLAP"] = "1"
    elif args.dp_overlap == 0:
        os.environ["DQN_DP_OVERLAP"] = "0"      # (unset = the engine decides from the world size and the exchange bytes, engine_program.hip)
    import torch
    if not torch.cuda.is_available():
        print("bench.py: no HIP device visible; the engine has no CPU fallback", file=sys.stderr)
        sys.exit(3)
    torch.cuda.set_device(local_rank)
    pkg = ge.load_package()
    if not os.path.exists(pkg.LIB_PATH):
        ge.build()
    import importlib
    pkg.nn = importlib.import_module(pkg.__name__ + ".nn")
    pkg.envs = importlib.import_module(pkg.__name__ + ".envs")
    par = importlib.import_module(pkg.__name__ + ".parallel")
    # control plane (rendezvous, 128-byte id broadcast, barriers, max-over-ranks timer) over gloo on the loopback interface;
    # the DATA path -- the one collective of a step (all-gather of the wide dense layers' operands + small gradients) -- is RCCL
    # over xGMI inside the engine (dqn_comm_init), on its stream.
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    group = par.Group(backend="gloo")

    eng, layers, hp, net, params, env = build_workload(pkg, args, rank, local_rank)
    with quiet_stdout():
        group.attach_engine(pkg, eng, init_comm=not sim_comm)          # RCCL communicator inside the engine (the step's collective runs on its stream)

    def barrier():
        group.barrier()
        torch.cuda.synchronize()
        eng.sync()

    env_loop = None
    prof_acc, single_gather = {}, {}

    def section_env_loop():
        nonlocal env_loop
        # ---- secondary: the device-resident env loop of config 3 (envs_per_rank copies of the image MDP per rank, eps-greedy + add_exp! in HBM)
        if args.env_steps > 0:
            eng.envs_create(env, n_envs=args.envs_per_rank, max_episode_length=100, seed=1234 + rank)
            eng.rollout(20, t0=1, train_freq=0, target_update_freq=0, stats=False)
            eng.sync()
            ta = time.perf_counter()
            eng.rollout(args.env_steps, t0=21, train_freq=0, target_update_freq=0, stats=False)      # acting only: no collective, safe on every rank
            eng.sync()
            tb = time.perf_counter()
            act_s = group.max_over_ranks(tb - ta)
            env_loop = {"envs_per_rank": args.envs_per_rank, "vector_steps": args.env_steps, "act_only_env_steps_per_s": world * args.envs_per_rank * args.env_steps / act_s,
                        "act_only_ms_per_vector_step": act_s / args.env_steps * 1e3}
            if world == 1:
                ta = time.perf_counter()
                st = eng.rollout(args.env_steps, t0=21 + args.env_steps, train_freq=4, target_update_freq=500)
                tb = time.perf_counter()
                env_loop.update({"train_freq": 4, "loop_env_steps_per_s": args.envs_per_rank * args.env_steps / (tb - ta),
                                 "loop_train_steps_per_s": st["train_steps"] / (tb - ta), "loop_ms_per_vector_step": (tb - ta) / args.env_steps * 1e3})
                # the REFERENCE's cadence (src/solver.jl:136-140: a train step every train_freq ENV steps = envs_per_rank / 4 train steps per vector step)
                nref = max(20, args.env_steps // 4)
                ta = time.perf_counter()
                st = eng.rollout(nref, t0=21 + 2 * args.env_steps, train_freq=4, target_update_freq=500, env_step_cadence=True)
                tb = time.perf_counter()
                env_loop.update({"refcadence_vector_steps": nref, "refcadence_train_steps_per_vector_step": st["train_steps"] / nref,
                                 "refcadence_env_steps_per_s": args.envs_per_rank * nref / (tb - ta), "refcadence_train_steps_per_s": st["train_steps"] / (tb - ta),
                                 "refcadence_ms_per_vector_step": (tb - ta) / nref * 1e3})
            group.barrier()


    def section_profile():
        # per-launch durations (HIP events on the engine stream, eager launches).  A profiled step is a full train step -- with its collective when
        # world > 1 -- so EVERY rank runs the same number of them; only rank 0 uses the numbers.
        for _ in range(args.profile_steps):
            for name, ms in eng.profile_step(steady=True):      # the step dqn_train_steps(n) repeats (its timed loop below runs exactly that)
                a = prof_acc.setdefault(name, [0.0, 0])
                a[0] += ms
                a[1] += 1
        # the gather launch of a SINGLE dqn_train_step (inside dqn_train_steps the previous step's Adam launch carries it: "adam+gather" above)
        for _ in range(min(5, args.profile_steps)):
            for name, ms in eng.profile_step():
                if name in ("gather", "sample_gather"):
                    a = single_gather.setdefault(name, [0.0, 0]); a[0] += ms; a[1] += 1
        group.barrier()


    if args.full:
        # the HOST-paced per-launch profile first, the GPU-paced device env loop (~35 ms of dense work) last: what runs right before the 3 ms timed region decides the clocks it sees
        if args.order == "env-first":
            section_env_loop(); section_profile()
        else:
            section_profile(); section_env_loop()
    else:
        # no untimed section runs before the headline here, so untimed steps of the same call bring the GPU to its clocks instead (~35 ms at config 2,
        # as the env loop does above; without them the 20-step region read 8096-8104 steps/s against 8472-8485 with them, same box).  Calls of fewer than 64 steps: the 16-step grouped graph's first launch stays where it is with --full.
        for _ in range(RAMP_CALLS):
            eng.train_steps(RAMP_STEPS_PER_CALL)

    # ---- the headline: W untimed warm-up steps, then EXACTLY K timed steps between barrier + synchronize.  It runs AFTER the secondary sections
    # above (real train steps and env steps, all untimed): the GPU needs ~10 ms of activity to reach its clocks, and with --steps 20 --warmup 5
    # the timed region is 3 ms -- measured straight after the idle build phase it read 160 us/step instead of 152 (tools/first_call.py).
    # (r04, measured and rejected: running the 10-second sustained region BEFORE it.  Five alternating runs with the driver's flags: 6201 / 6396 / 6931 / 7164 / 5909 steps/s
    # after the sustained region vs 7004 / 7057 / 7084 / 7048 / 6944 in this order -- the first short call after ten seconds of load is slower and far noisier.)
    eng.train_steps(max(3, args.warmup))      # >= 3 so that the three step graphs of dqn_train_steps (first / middle / last) are all captured untimed
    barrier()
    t0 = time.perf_counter()
    loss, gnorm = eng.train_steps(args.steps)       # K graph replays back to back; one host sync at the end
    t_call = time.perf_counter()
    eng.sync()
    t_sync = time.perf_counter()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    region_split = {"dqn_train_steps_call": (t_call - t0) * 1e6, "engine_stream_sync": (t_sync - t_call) * 1e6, "torch_cuda_synchronize": (t1 - t_sync) * 1e6,
                    "note": "rank 0's split of the timed region (us): the K-step call (returns when the last step's scalars are in the host mailbox), then the two synchronisations the contract asks for"}
    elapsed = group.max_over_ranks(t1 - t0)
    group.barrier()
    ms_per_step = elapsed / args.steps * 1e3
    value = world * args.steps / elapsed            # whole-job train steps/s (each rank runs its own B=32 step)
    if args.dump_outputs and rank == 0:
        dump_outputs(pkg, eng, args.dump_outputs, loss, gnorm)

    # ---- the same measurement over a LONG region (the driver's --steps 20 region is ~3 ms, shorter than its SMI sampler's period): `--sustained-seconds` of GPU time
    # (default 10 s) of the identical call, same barriers, same max-over-ranks clock, BEFORE the CPU baseline.  Reported beside `value`, never instead of it.
    sustained = None
    if args.sustained_steps < 0:
        args.sustained_steps = int(max(1000, args.sustained_seconds * value / world)) if args.sustained_seconds > 0 else 0
    if args.full and args.sustained_steps > 0:
        barrier()
        t0 = time.perf_counter()
        eng.train_steps(args.sustained_steps)
        eng.sync()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        el2 = group.max_over_ranks(t1 - t0)
        group.barrier()
        sustained = {"steps": args.sustained_steps, "seconds": el2, "value": world * args.sustained_steps / el2, "unit": "steps/s", "ms_per_step": el2 / args.sustained_steps * 1e3}

    # ---- the drop-in seam as the reference's loop drives it: ONE call per train step with (loss, grad_norm) returned every time (src/solver.jl:138,235).
    # `sync`: K calls of dqn_train_step(e, NULL, &loss, &gn, NULL) -- the host waits for every step's scalars (published by the step's last launch into a
    # mapped host ring).  `async`: K calls of dqn_train_step_async (returns once enqueued) and ONE dqn_step_scalars at the end -- what the shim's dqn_train! does
    # between two log_freq prints (src/solver.jl:154-167).  Both include the step's own sample + gather launch (nothing is pre-gathered across calls).
    per_call = None
    kpc = args.steps if args.per_call_steps < 0 else args.per_call_steps
    if args.full and kpc > 0 and world == 1:
        per_call = {}
        for _ in range(3):
            eng.train_step(want_td=False); eng.step_scalars(eng.train_step_async())
        for mode in ("sync", "async"):
            barrier()
            t0 = time.perf_counter()
            if mode == "sync":
                for _ in range(kpc):
                    lv = eng.train_step(want_td=False)
            else:
                for _ in range(kpc):
                    tk = eng.train_step_async()
                lv = eng.step_scalars(tk, wait=True)
            eng.sync()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            per_call[mode] = {"calls": kpc, "value": kpc / (t1 - t0), "unit": "steps/s", "us_per_call": (t1 - t0) / kpc * 1e6,
                              "us_over_batched_step": (t1 - t0) / kpc * 1e6 - ms_per_step * 1e3, "last_loss": lv[0]}
        per_call["note"] = ("sync = dqn_train_step(e, NULL, &loss, &gn, NULL) per step (what the shim's batch_train! method does); async = dqn_train_step_async per step + one "
                            "dqn_step_scalars (what the shim's dqn_train! loop does between log_freq prints); `value` above is dqn_train_steps(K), one call for K steps")
    comm_info = eng.comm_info()
    if world > 1 and not sim_comm:
        assert comm_info["rccl_nranks"] == world and comm_info["rccl_rank"] == rank, (comm_info, rank, world)     # the communicator itself saw WORLD_SIZE ranks

    out = None
    n_params = eng.P
    if rank == 0:
        roof = secondary = cpu = None
        if args.full:
            roof = roofline_block(pkg, eng, layers, args.batch, args.u8, world, value, ms_per_step, prof_acc, single_gather)
            # ---- BASELINE configs[0], [3], [4] on the SAME line: each timed exactly like `value` (warm-up, K steps between two syncs), on engines of
            # their own, after the headline engine has been released.  Default single-GPU run on the headline workload only.
            if world == 1 and not args.no_secondary and args.batch == 32 and not args.u8 and not args.distinct:
                eng.close()
                args_ms_plain[0] = ms_per_step
                secondary = secondary_block(pkg, args, local_rank)
            if not args.no_cpu_baseline:           # rank 0 only (this block), at any world size
                if world > 1:
                    args.cpu_seconds = min(args.cpu_seconds, 5.0)      # the other ranks wait at the final barrier meanwhile
                cpu = cpu_baseline(pkg, layers, hp, params, env, args)
        out = {
            "metric": f"train steps/sec (batch={args.batch}, 84x84x4 obs)", "value": value, "unit": "steps/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
            "timed_region_us": region_split,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": workload_name(args, world), "sampling": "distinct (replace=false, ...replay.jl:85)" if args.distinct else "stratified sum-tree (with replacement)",
                       "batch_per_rank": args.batch, "global_batch": args.batch * world, "replay_per_rank": args.replay,
                       "replay_dtype": "u8" if args.u8 else "f32", "envs_per_rank": args.envs_per_rank,
                       "parallelism": f"dp{world} (per-rank envs + replay; one RCCL all-gather per step: wide-dense operands + small gradients)" if world > 1 else "single GPU",
                       "hip_graph": not args.no_graph, "mfma": not args.no_mfma, "last_loss": loss, "last_grad_norm": gnorm, "n_params": int(n_params),
                       "rccl_nranks": comm_info["rccl_nranks"], "rccl_rank": comm_info["rccl_rank"], "rccl_device": comm_info["rccl_device"],
                       "exchange": {0: "none", 1: "all-gather (wide-dense operands + small gradients)", 2: "all-reduce (flat gradient)", -1: "undecided"}[comm_info["exchange"]],
                       "dp_overlap": bool(comm_info["dp_overlap"]),
                       **({"sim_comm": "SELF-TEST: all ranks share GPU 0, the all-gather is replaced by local copies (DQN_SIM_WORLD); not a scaling measurement"} if sim_comm else {})},
            "samples_per_s": value * args.batch, "clock_ramp_steps": 0 if args.full else RAMP_CALLS * RAMP_STEPS_PER_CALL, "host_fill": dict(HOST_FILL),
        }
        if args.full:
            out.update({"roofline": roof, "cpu_baseline": cpu, "env_loop": env_loop, "sustained": sustained, "per_call": per_call, "secondary": secondary,
                        "value_distinct": (secondary or {}).get("config2_distinct", {}).get("steps_per_s")})      # the same step with distinct sampling (secondary.config2_distinct)
        print(json.dumps(out))
    group.barrier()
    eng.close()
    group.close()


def numa_plan():
    """One NUMA node of this host and the first hardware thread of each of its physical cores (sysfs).  The CPU proxies run confined to it: on the 2-socket GPU boxes
    un-pinned OpenMP / oneDNN threads migrate across sockets and a step's time spreads 4x (driver p10 20 ms vs median 72 ms)."""
    def parse(txt):
        out = []
        for part in txt.strip().split(","):
            if not part:
                continue
            a, _, b = part.partition("-")
            out.extend(range(int(a), int(b or a) + 1))
        return out
    try:
        allowed = set(os.sched_getaffinity(0))
        nodes = sorted(int(d[4:]) for d in os.listdir("/sys/devices/system/node") if d.startswith("node") and d[4:].isdigit())
        best = None
        for nd in nodes:
            cpus = [c for c in parse(open(f"/sys/devices/system/node/node{nd}/cpulist").read()) if c in allowed]
            cores = []
            for c in cpus:
                try:
                    sib = parse(open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list").read())
                except OSError:
                    sib = [c]
                if c == min(x for x in sib if x in allowed or x == c):
                    cores.append(c)
            if best is None or len(cores) > len(best[1]):
                best = (nd, cores, len(nodes))
        if best and best[1]:
            return {"node": best[0], "cores": best[1], "nodes": best[2]}
    except OSError:
        pass
    return {"node": None, "cores": sorted(os.sched_getaffinity(0)), "nodes": 1}


def cpu_worker(args):
    """Internal (bench.py --cpu-worker twin|torch): ONE CPU proxy measured in a FRESH process, pinned to the physical cores of one NUMA node BEFORE any threaded library is
    loaded (OMP_PLACES=cores OMP_PROC_BIND=close are set by the parent; the twin worker never imports torch).  Prints one JSON object."""
    cpus = [int(c) for c in args.cpu_worker_cpus.split(",") if c]
    if cpus:
        os.sched_setaffinity(0, cpus)
    ncore = len(cpus) if cpus else (os.cpu_count() or 1)
    if args.cpu_worker == "torch":
        pkg = ge.load_package()
        hp = pkg.default_hparams(batch_size=args.batch, n_actions=4, obs_c=4, obs_h=84, obs_w=84, gamma=0.99)
        runs = []
        best_t, best_v = None, 0.0
        import torch
        for th in sorted({min(16, ncore), min(32, ncore), ncore}):
            torch.set_num_threads(th)
            r = torch_cpu_line(hp, min(1.5, args.cpu_seconds / 8))
            if r["value"] > best_v:
                best_t, best_v = th, r["value"]
        torch.set_num_threads(best_t)
        for _ in range(5):
            runs.append(torch_cpu_line(hp, min(2.0, args.cpu_seconds / 6)))
        top = sorted(runs, key=lambda r: r["value"])[2]
        top.update(threads=best_t, runs_steps_per_s=[round(r["value"], 2) for r in runs], spread=round(max(r["value"] for r in runs) / min(r["value"] for r in runs), 3),
                   protocol="fresh process pinned to one NUMA node's physical cores; thread count = best of 16/32/all by a short probe; value = MEDIAN of 5 runs")
        print(json.dumps(top))
        return 0
    # ---- the canonical-order C twin (oracle/dqn_ref.c, kind "port") on a bounded sample of the same workload: same network, batch and step, a 512-transition replay
    import importlib
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref
    pkg = ge.load_package()
    nn = importlib.import_module(pkg.__name__ + ".nn"); envs = importlib.import_module(pkg.__name__ + ".envs")
    net = nn.create_dueling_network(nn.nature_dqn(n_actions=4, in_channels=4))
    layers, _ = nn.lower(net)
    hp2 = pkg.default_hparams(batch_size=args.batch, n_actions=4, obs_c=4, obs_h=84, obs_w=84, obs_dtype=pkg.OBS_U8 if args.u8 else pkg.OBS_F32, learning_rate=1e-4, gamma=0.99,
                              double_q=1, dueling=1, prioritized_replay=1, buffer_size=512, seed=1234)
    params = nn.glorot_params(net, seed=1)
    env = envs.TestMDP((84, 84), 4, 6, n=32, seed=7, u8=args.u8); env.rng = np.random.default_rng(1000)
    tw = ref.Twin(layers, hp2, plan=None, threads=1)
    tw.set_params(params, 0); tw.set_params(params, 1)
    o = env.observe(); n = 0
    while n < 512:
        a = env.rng.integers(0, 4, env.n); r = env.act(a); op = env.observe(); d = env.terminated()
        tw.replay_add(o, a.astype(np.int32), r, op, d.astype(np.uint8)); n += env.n
        env.reset(d); o = env.observe()
    tw.train_step()
    def protocol(th, warm, k):
        tw.set_threads(th)
        for _ in range(warm):
            tw.train_step()
        dts = []
        for _ in range(k):
            t0 = time.perf_counter(); tw.train_step(); dts.append(time.perf_counter() - t0)
        dts = np.sort(np.array(dts))
        return float(np.median(dts)), float(dts[int(0.1 * (k - 1))]), float(dts[int(0.9 * (k - 1))])
    # thread count: every candidate runs a short version of the protocol (3 warm-up + 9 timed steps) and is judged by its MEDIAN and its spread -- a 5-step probe picked 32
    # threads on one box (median 78 ms, p90 / p10 = 4.3) where 16 threads gave 39 ms at 1.08 (r05): OpenMP teams wider than the loops' trip counts oversubscribe the short loops
    t0 = time.perf_counter(); tw.set_threads(1); tw.train_step(); single = 1.0 / (time.perf_counter() - t0)
    cand = {}
    for th in sorted({min(8, ncore), min(16, ncore), min(32, ncore)}):
        m, lo, hi = protocol(th, 3, 9)
        cand[th] = (m * (1.0 if hi / lo < 1.5 else hi / lo), m)      # a noisy team is penalised by its spread
    cores = min(cand, key=lambda t: cand[t][0]); best = cand[cores][1]
    # SURVEY 8(d) protocol, three times: 10 warm-up steps, then >= 30 individually timed steps; value = 1 / (the smallest of the three medians)
    k = int(max(30, min(200, args.cpu_seconds / 3 / max(best, 1e-3))))
    reps = [protocol(cores, 10, k) for _ in range(3)]
    tw.close()
    med, p10, p90 = min(reps)
    print(json.dumps({"value": 1.0 / med, "cores": cores, "single_thread_value": single, "median_ms": med * 1e3, "p10_ms": p10 * 1e3, "p90_ms": p90 * 1e3, "timed_steps": k,
                      "medians_ms": [round(r[0] * 1e3, 3) for r in reps], "p90_over_p10": p90 / p10}))
    return 0


def run_cpu_worker(kind, args, plan):
    import subprocess
    env = dict(os.environ)
    env.update(OMP_PROC_BIND="close", OMP_PLACES="cores", OMP_DYNAMIC="false", OMP_WAIT_POLICY="active", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", kind, "--cpu-worker-cpus", ",".join(str(c) for c in plan["cores"]), "--batch", str(args.batch),
           "--cpu-seconds", str(args.cpu_seconds)] + (["--u8"] if args.u8 else [])
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=max(120.0, 8 * args.cpu_seconds))
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not line:
            return {"error": f"cpu worker {kind} failed (rc {r.returncode}): {r.stderr[-400:]}"}
        return json.loads(line[-1])
    except Exception as ex:
        return {"error": repr(ex)}


def cpu_baseline(pkg, layers, hp, params, env, args):
    """Two CPU ports of the same train step on this box's host cores, each in a FRESH subprocess confined to the physical cores of ONE NUMA node (numa_plan) with
    OMP_PROC_BIND=close OMP_PLACES=cores -- the twin before any torch import (cpu_worker).  The Julia/Flux reference itself cannot run in this image."""
    ncpu = os.cpu_count() or 1
    plan = numa_plan()
    tw = run_cpu_worker("twin", args, plan)
    tc = run_cpu_worker("torch", args, plan)
    port = tw.get("value", 0.0) or 0.0
    tval = tc.get("value", 0.0) or 0.0
    # `value` is the STRONGER of the two CPU restatements of the same step: Flux's CPU path is im2col + OpenBLAS, i.e. library-class like the
    # eager PyTorch / oneDNN line, while the canonical-order twin trades speed for a fixed summation order.  Both are ports; neither is the reference.
    use_torch = tval > port
    return {"value": tval if use_torch else port, "unit": "steps/s", "cores": tc.get("threads") if use_torch else tw.get("cores"), "kind": "port",
            "value_source": "torch_cpu (eager PyTorch CPU, oneDNN)" if use_torch else "twin (oracle/dqn_ref.c)",
            # one place for "how many cores" (VERDICT r05 weak 12): the threads the quoted value USED, and what the box HAS (logical CPUs; physical cores of the NUMA node the
            # workers were pinned to x nodes).  The ports stop scaling at 16 threads (probed 1 / 8 / 16 / 32 / all): more cores are there, they do not make this step faster
            "cores_used": tc.get("threads") if use_torch else tw.get("cores"),
            "cores_available": {"logical_cpus": ncpu, "physical_cores_one_numa_node": len(plan["cores"]), "numa_nodes": plan["nodes"], "physical_cores_box": len(plan["cores"]) * plan["nodes"]},
            "port_value": port, "port_cores": tw.get("cores"), "nproc": ncpu, "numa_node": plan["node"], "numa_nodes": plan["nodes"], "pinned_physical_cores": len(plan["cores"]),
            "single_thread_value": tw.get("single_thread_value"),
            "median_ms": tw.get("median_ms"), "p10_ms": tw.get("p10_ms"), "p90_ms": tw.get("p90_ms"), "p90_over_p10": tw.get("p90_over_p10"), "medians_ms": tw.get("medians_ms"),
            "timed_steps": tw.get("timed_steps"), "twin": tw, "torch_cpu": tc,
            "sample": f"value = the faster of two CPU ports of the same train step (B={hp.batch_size}, Nature-DQN dueling, double-Q, IS-weighted Huber, backward, Adam), each in a fresh process "
                      f"pinned to the {len(plan['cores'])} physical cores of NUMA node {plan['node']} of this {ncpu}-CPU host (OMP_PROC_BIND=close, OMP_PLACES=cores): "
                      f"(a) eager PyTorch CPU / oneDNN, random batch, median of 5 runs (library-class proxy for Flux's im2col + OpenBLAS path); "
                      f"(b) port_value: oracle/dqn_ref.c (the canonical-order twin the parity tests use) on a 512-transition replay, thread count = fastest of 1/8/16/32/all by a 5-step probe, "
                      f"then 3 x (10 warm-up + >= 30 individually timed steps), 1 / smallest median.  The Julia/Flux reference itself cannot run in this image"}




PMC_OK = [True]

# kernel-symbol family of a launch of the step program (names: DESIGN.md section 6 / op_cost above)
KERNEL_FAMILIES = (("k_dwdx_lds", lambda n: "dx" in n and n.startswith("dw")), ("k_fwd_lds", lambda n: n.startswith("fwd_") and "reduce" not in n and "valu" not in n),
                   ("k_dw_lds", lambda n: n.startswith("dw") and "dx" not in n), ("k_adam", lambda n: n.startswith("adam")), ("k_head_td", lambda n: n == "head_td"), ("k_red_head", lambda n: n == "red_head"), ("k_head_cols4", lambda n: n == "head_cols4"),
                   ("k_reduce_multi", lambda n: "reduce" in n))


def dominant_kernel(table, use_profile, ev_over=0.0):
    """The dominant kernel = the kernel symbol with the largest TOTAL time in the newest committed rocprofv3 --kernel-trace summary of this bench
    (use_profile = "cfg2": profiles/*_kernel_trace_summary.txt; "cfg5": profiles/*_cfg5_kernels.txt, whose env-loop kernels -- the device fill -- belong to no family of
    the train step and are skipped; None: no profile), priced on its launches' algorithmic FLOPs (or bytes) over their LIVE HIP-event durations; the
    committed profile's average duration of the same symbol stands beside it (HIP events read ~1.2-2 us longer per launch than rocprofv3's begin/end stamps).
    Without a usable profile (other configs): the family with the largest live total."""
    import glob
    import hashlib
    fam_rows = {}
    for fam, pred in KERNEL_FAMILIES:
        rows = [r for r in table if pred(r["launch"])]
        if rows:
            fam_rows[fam] = rows
    prof = None
    if use_profile:
        pattern = "*_cfg5_kernels.txt" if use_profile == "cfg5" else "*_kernel_trace_summary.txt"      # the per-kernel table of rocprofv3 --kernel-trace --stats on the config's own bench command
        for path in sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)), reverse=True):
            if ("cfg5" in path) != (use_profile == "cfg5") or "drqn" in path:
                continue
            rows = []
            for line in open(path):
                f = line.rsplit(None, 6)
                try:
                    if len(f) == 7:
                        rows.append((f[0].strip(), int(f[1]), float(f[2]), float(f[5])))
                except ValueError:
                    pass      # header / footer lines
            if rows:
                prof = (path, rows)
                break
    if prof:
        # the top SYMBOL of the profile (rows are sorted by total time); its family's launches are the ones priced (template instances of one family that the
        # launch names cannot tell apart -- the forward tiles' NT -- are priced together)
        by_fam, symbol = {}, None
        for name, calls, avg, tot in sorted(prof[1], key=lambda r: -r[3]):
            fam0 = next((f for f in fam_rows if f in name), None)
            if fam0 is not None:
                by_fam[fam0] = [calls, tot]; symbol = name
                break
        fam = next(iter(by_fam), None)
    else:
        fam = None
    if fam is None:
        fam = max(fam_rows, key=lambda k: sum(r["avg_us"] for r in fam_rows[k]))
    rows = fam_rows[fam]
    us = sum(r["avg_us"] for r in rows)
    d = {"kernel": fam, "launches_per_step": len(rows), "launches": [r["launch"] for r in rows], "avg_us": round(us / len(rows), 2), "step_us": round(us, 2),
         "timing": "HIP events on the engine stream, live in this run (eager launches of the steady-state step)"}
    if all(r.get("bound") == "mfma" for r in rows):
        fl = sum(r["mflop"] for r in rows) * 1e6
        d.update(bound="mfma", mflop_per_step=round(fl / 1e6, 1), tflops=round(fl / (us * 1e-6) / 1e12, 2), frac=round(fl / (us * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4))
    elif all(r.get("bound") == "hbm" for r in rows):
        by = sum(r["mbytes"] for r in rows) * 1e6
        d.update(bound="hbm", mbytes_per_step=round(by / 1e6, 2), gbs=round(by / (us * 1e-6) / 1e9, 1), frac=round(by / (us * 1e-6) / 1e9 / PEAK_HBM_GBS, 4))
    if ev_over > 0 and d.get("bound") == "mfma":
        net = us - ev_over * len(rows)
        d.update(avg_us_net_of_event_overhead=round(net / len(rows), 2), frac_net_of_event_overhead=round(d["mflop_per_step"] * 1e6 / (net * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4))
    if prof:
        calls, tot = by_fam[fam]
        d.update(rocprof_symbol=symbol, rocprof_file="profiles/" + os.path.basename(prof[0]), rocprof_sha1=hashlib.sha1(open(prof[0], "rb").read()).hexdigest()[:12],
                 rocprof_avg_us=round(tot * 1e3 / calls, 2), rocprof_share_of_kernel_time=round(tot / sum(r[3] for r in prof[1]), 4),
                 chosen_by="largest total time in the committed rocprofv3 kernel-trace summary")
        if d.get("bound") == "mfma" and use_profile != "cfg5":      # (config 5: the family's launches are several template instances, the profile's average is ONE symbol's)
            # live FLOPs over the COMMITTED profile's duration: not a measurement of this run (the profile may predate the code that is running)
            d["frac_at_committed_profile_duration"] = round(d["mflop_per_step"] * 1e6 / (d["rocprof_avg_us"] * len(rows) * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)
    else:
        d["chosen_by"] = "largest live total (no committed rocprofv3 summary for this configuration)"
    return d


def pmc_traffic(op):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (profiles/*_pmc_fetch.txt / *_pmc_write.txt: separate
    --pmc FETCH_SIZE and --pmc WRITE_SIZE runs of this bench, values in KB; gfx950 reports half of wide reads, hence x2 on FETCH_SIZE as the
    MI355X guide prescribes).  bench.py cannot run the profiler itself; the newest committed pass is quoted, or null."""
    import glob
    if not PMC_OK[0]:
        return {}
    cfg5 = PMC_OK[0] == "cfg5"      # config 5 (u8 replay, byte arena): its own kernels, its own passes (profiles/*_cfg5_pmc_fetch.txt / _write.txt, tools/gpu_pmc_cfg5.sh)
    kname = ({"adam": "k_adam", "adam+gather": "k_adam_pg_u8", "gather": "k_gather_fb_u8b"} if cfg5 else
             {"adam": "k_adam", "adam+gather": "k_adam_pg", "sample_gather": "k_gather_fb", "gather": "k_gather_fb"}).get(op)
    if kname is None:
        return {}
    def last(pattern):
        for path in sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)), reverse=True):
            if ("cfg5" in os.path.basename(path)) != cfg5:
                continue
            for line in open(path):
                f = line.split()
                if f and f[0] == kname and len(f) >= 3:
                    return float(f[-1]), os.path.basename(path)
        return None, None
    fetch, pf = last("*_pmc_fetch.txt")
    write, pw = last("*_pmc_write.txt")
    if fetch is None or write is None:
        return {}
    import hashlib
    sha = lambda f: hashlib.sha1(open(os.path.join(ROOT, "profiles", f), "rb").read()).hexdigest()[:12]
    return {"traffic": (2.0 * fetch + write) * 1024.0, "traffic_unit": "bytes/launch",
            "traffic_source": f"profiles/{pf} [sha1 {sha(pf)}] (FETCH_SIZE x2) + profiles/{pw} [sha1 {sha(pw)}] (WRITE_SIZE), separate rocprofv3 --pmc passes of this bench (committed files, NOT measured by this run)"}


def torch_cpu_line(hp, seconds):
    """A "well-optimised CPU library" sanity line next to the twin: the same train step -- Nature-DQN dueling, double-Q
    target, IS-weighted Huber, backward, Adam -- in eager PyTorch on the host cores (oneDNN convolutions).  A proxy for the Flux CPU
    path, not a parity reference: random weights and batch, no replay."""
    import torch
    import torch.nn.functional as F
    B, nA = hp.batch_size, hp.n_actions

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c1, self.c2, self.c3 = torch.nn.Conv2d(4, 32, 8, 4), torch.nn.Conv2d(32, 64, 4, 2), torch.nn.Conv2d(64, 64, 3, 1)
            self.v1, self.v2 = torch.nn.Linear(3136, 512), torch.nn.Linear(512, 1)
            self.a1, self.a2 = torch.nn.Linear(3136, 512), torch.nn.Linear(512, nA)

        def forward(self, x):
            x = F.relu(self.c3(F.relu(self.c2(F.relu(self.c1(x)))))).flatten(1)
            v, a = self.v2(F.relu(self.v1(x))), self.a2(F.relu(self.a1(x)))
            return v + a - a.mean(1, keepdim=True)

    torch.manual_seed(0)
    on, tg = Net(), Net()
    opt = torch.optim.Adam(on.parameters(), lr=1e-4)
    s, sp = torch.rand(B, 4, 84, 84), torch.rand(B, 4, 84, 84)
    a, r, d, w = torch.randint(0, nA, (B,)), torch.randn(B), (torch.rand(B) < 0.2).float(), torch.rand(B) + 0.5

    def step():
        with torch.no_grad():
            best = on(sp).argmax(1)
            y = r + (1 - d) * hp.gamma * tg(sp).gather(1, best[:, None])[:, 0]
        td = on(s).gather(1, a[:, None])[:, 0] - y
        x = (w * td).abs()
        m = torch.clamp(x, max=1.0)
        loss = (0.5 * m * m + (x - m)).sum() / B
        opt.zero_grad()
        loss.backward()
        opt.step()

    step()
    t0 = time.perf_counter()
    k = 0
    while time.perf_counter() - t0 < seconds:
        step()
        k += 1
    el = time.perf_counter() - t0
    return {"value": k / el, "unit": "steps/s", "threads": torch.get_num_threads(), "steps": k, "seconds": el, "kind": "eager PyTorch CPU (oneDNN), proxy"}

if __name__ == "__main__":
    main()
