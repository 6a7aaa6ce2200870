#!/usr/bin/env python3
"""tools/program_names.py [--out FILE]  (GPU box, repo root) -- the launch names of the train step's program, in order, for a fixed table of engines, as JSON.

For every engine: the names of profile_step() and, for a feed-forward engine (the ones that pipeline), of profile_step(steady=True).  Two builds of the library
(DQN_MI355X_LIB=<the other build>) that compile the same program print the same bytes: the check of a host-side change to csrc/engine_program.hip
(docs/history/step_build.md).  The table invents no network; it is built from case tables the tests own:
  plan/   tests/plan_edges_common.CASES                    ff/ rnd/   tests/feedforward_edges_common.CASES, RANDOM
  kind/   tests/kind_traits_cases.GPU_CASES (train steps)  comp/      tests/composition_common.FF, REC
  rec/    tests/test_recurrent_edges_gpu BOUNDARY under the engine's own plan (an LSTM: the column-group step) and, LSTMs, with dw_kc >= 0; MULTI_LAUNCH_DW
  dp/     the engines of tests/test_dp_gpu.py, one child process per replica switch (the engine reads them once, at creation)
  sw/     one engine per program switch, on the first case of the tables above whose default program shows what the switch removes
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("oracle", "tests", ""):
    sys.path.insert(0, os.path.join(ROOT, d))

DP_ENVS = [{"DQN_SIM_WORLD": "2"}, {"DQN_SIM_WORLD": "3"}, {"DQN_FORCE_ALLREDUCE": "1"}, {"DQN_DP_ALLREDUCE": "1"}, {"DQN_DP_OVERLAP": "0"}, {"DQN_DP_OVERLAP": "1"}]
# (switch, value, a launch-name fragment of the default program that the switch removes)
SWITCHES = [("DQN_NO_RED_HEAD", "1", "red_head"), ("DQN_NO_HEAD_COLS4", "1", "head_cols4"), ("DQN_NO_HEAD_COLS4", "2", "head_cols4"), ("DQN_NO_SKIP_FUSE", "1", "+skip"),
            ("DQN_GRU_STEPWISE", "1", "gru_seq"), ("DQN_RNN_STEPWISE", "1", "rnn_seq"), ("DQN_NO_TINY", "1", "tiny_step")]


def observe(h, recurrent):
    out = {"step": [n for n, _ in h.profile_step(max_entries=4096)]}
    if not recurrent:
        try:
            out["steady"] = [n for n, _ in h.profile_step(max_entries=4096, steady=True)]
        except Exception as e:      # the library's own refusal (an engine that does not pipeline) is part of the record; anything else ends the run
            if type(e).__name__ != "DQNError":
                raise
            out["steady"] = ["refused: " + str(e)]
    h.close()
    return out


def dp_child():
    """the replica engines of tests/test_dp_gpu.py under this process's environment: the wide dense dueling network (B = 32), the wide first layer (B = 64, two tiles per
    rank) and Nature-DQN dueling (B = 32); without DQN_SIM_WORLD the first one also behind a communicator of world size 1"""
    import numpy as np
    import __graft_entry__ as ge
    import dqn_oracle as O
    import ref
    import test_dp_gpu as T
    from nets import nature_dueling
    pkg = ge.load_package(); pkg.lib()
    sim = "DQN_SIM_WORLD" in os.environ

    def engine(net, B, comm=False):
        layers = ref.layers_from_network(net); n = 2 * B + 8
        hp = ref.hparams_for(net, batch_size=B, buffer_size=n, learning_rate=1e-3, gamma=0.99)
        h = pkg.Engine(layers, hp, plan=pkg.default_plan(layers, hp))
        rng = np.random.default_rng(0)
        obs = lambda: rng.random((n,) + net.obs_shape, dtype=np.float32)
        h.replay_add(obs(), rng.integers(0, net.n_actions, n).astype(np.int32), rng.standard_normal(n).astype(np.float32), obs(), (rng.random(n) < 0.2).astype(np.uint8))
        p = O.Network.flatten(O.init_params(net, seed=5)); h.set_params(p, 0); h.set_params(p, 1)
        if comm:
            h.comm_init(pkg.comm_unique_id(), 0, 1)
        return h

    two_tiles = O.Network((768,), *O.create_dueling_network([O.Dense(768, 1024, T.R), O.Dense(1024, 5, T.I)]))
    out = {"wide_b32": observe(engine(T.wide_dense_dueling(), 32), False), "first_layer_b64": observe(engine(two_tiles, 64), False), "nature_b32": observe(engine(nature_dueling(), 32), False)}
    if not sim:
        out["wide_b32_comm"] = observe(engine(T.wide_dense_dueling(), 32, comm=True), False)
    json.dump(out, sys.stdout)


def table():
    """[(name, factory)]: factory(env) creates the engine with the switches `env` set and returns (handle with a filled replay, recurrent)"""
    import __graft_entry__ as ge
    import composition_common as CC
    import feedforward_edges_common as C
    import kind_traits_cases as K
    import plan_edges_common as P
    import ref
    import test_composition_gpu as TC
    import test_recurrent_edges_gpu as TR
    pkg = ge.load_package(); pkg.lib()
    mods = (pkg, importlib.import_module(pkg.__name__ + ".nn"))
    rows = []

    def ff(c, plan):
        def make(env):
            net = C.network(c); D = C._draw(c, net, c.seed, 1)
            with K._environ(env):
                return C.make_handle(pkg.Engine, c, net, D, plan=plan)[0], False
        return make

    def kind(c):
        def make(env):
            h, hp = K._engine(c, c["env"] | env); K._fill(h, hp, c)
            return h, bool(hp.recurrence)
        return make

    def comp(c):
        def make(env):
            with K._environ(env):
                return (TC.rec_engine if c.T else TC.ff_engine)(pkg, c, CC.data(c)), bool(c.T)
        return make

    def rec(c, plan):
        def make(env):
            with K._environ(env):
                return TR.make_engine(mods, c, plan=plan(c) if callable(plan) else plan)[1], True
        return make

    def own_plan(c, floor=None, kc=None):      # the engine's own plan; floor: dw_kc no lower (0: never the column-group step); kc: dw_kc on every layer
        return [(p[0], p[1], kc if kc is not None else max(p[2], floor)) for p in TR.default_plan_of(mods, c)]

    rows += [("plan/" + c.name, ff(c, P.plan_of(c))) for c in P.CASES]
    rows += [("ff/" + c.name, ff(c, ref.default_plan)) for c in C.CASES] + [("rnd/" + c.name, ff(c, ref.default_plan)) for c in C.RANDOM]
    rows += [("kind/" + n, kind(c)) for n, c in K.GPU_CASES.items() if not c["refuse"] and not c["envs"]]
    rows += [("comp/" + c.name, comp(c)) for c in CC.FF + CC.REC]
    for c in TR.BOUNDARY:
        rows.append(("rec/" + c.name, rec(c, None)))
        if c.name.startswith("lstm"):
            rows.append(("rec/" + c.name + "/dw_kc>=0", rec(c, lambda c: own_plan(c, floor=0))))
    rows += [("rec/" + c.name, rec(c, lambda c, kc=kc: own_plan(c, kc=kc))) for c, kc, _ in TR.MULTI_LAUNCH_DW]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dp-child", action="store_true")
    a = ap.parse_args()
    if a.dp_child:
        return dp_child()
    out = {}
    # the replica engines first, each in a process of its own, before this process opens the GPU; a child that fails ends the run
    for env in DP_ENVS:
        tag = ",".join(f"{k}={v}" for k, v in env.items())
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--dp-child"], env=os.environ | env, stdout=subprocess.PIPE, timeout=300, cwd=ROOT)
        if r.returncode:
            sys.exit(f"program_names: the child under {tag} ended with status {r.returncode}")
        for k, v in json.loads(r.stdout.decode().strip().splitlines()[-1]).items():
            out[f"dp/{tag}/{k}"] = v
    rows = table()
    made = {}
    for name, make in rows:
        h, recurrent = make({})
        out[name] = observe(h, recurrent); made[name] = make
        print(f"{len(out):4d} {name}", file=sys.stderr, flush=True)
    for var, val, frag in SWITCHES:
        name = next((n for n, _ in rows if any(frag in x for x in out[n]["step"])), None)
        if name is None:
            sys.exit(f"program_names: no case of the tables launches '{frag}': {var} has nothing to change")
        h, recurrent = made[name]({var: val})
        out[f"sw/{var}={val}/{name}"] = observe(h, recurrent)
    text = json.dumps(out, indent=0, sort_keys=True) + "\n"
    print(f"{len(out)} engines", file=sys.stderr)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
