"""CPU: the grouped-acting seam without a GPU -- the header, the ctypes mirror and the Julia shim agree on dqn_rollout_many / dqn_rollout_many_info (the shim cannot
be executed here: checked statically, in the style of test_engine_group_cpu.py), the library exports them, their null and argument refusals need no device, and
solver.solve_many's Python-side checks are what they were."""
import ctypes
import importlib
import os
import re

import pytest

import __graft_entry__ as ge
from engine_group_common import many_refusal_cases

pkg = ge.load_package()
abi = pkg._abi
SHIM = os.path.join(ge.ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")
HEADER = os.path.join(ge.ROOT, "include", "dqn_mi355x.h")
MANY_FNS = ("dqn_rollout_many", "dqn_rollout_many_info")
WANT = {"dqn_rollout_many": ["ptr", "i32", "ptr", "ptr", "ptr"], "dqn_rollout_many_info": ["ptr", "ptr", "ptr"]}


def header_protos():
    return {m.group(1): [x.strip() for x in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",") if x.strip()]
            for m in re.finditer(r"\bint\s+(dqn_rollout_many\w*)\s*\(([^;{]*?)\)\s*;", open(HEADER).read(), re.S)}


def c_cat(param):
    if "*" in param:
        return "ptr"
    return {"int": "i32", "int32_t": "i32", "unsigned": "u32"}[param.rsplit(" ", 1)[0].replace("const ", "").strip()]


def test_header_declares_the_two_entry_points_and_the_law():
    protos = header_protos()
    assert set(protos) == set(MANY_FNS)
    for name in MANY_FNS:
        assert [c_cat(p) for p in protos[name]] == WANT[name], (name, protos[name])
    assert "const dqn_exploration* const* explore" in protos["dqn_rollout_many"]
    text = open(HEADER).read()
    law = text[text.index("grouped acting: the device environment loop"):text.index("int dqn_rollout_many(")]
    for phrase in ("THE LAW", "bit for bit what dqn_rollout_explore(member_k", "cadence_env_steps must be 0", "members that disagree are refused", "REFUSED before anything is enqueued"):
        assert phrase in law, phrase
    # the pinned set of dqn_group_* names is untouched: the new entry points are not group-prefixed
    assert not any(n.startswith("dqn_group_") for n in MANY_FNS)


def test_ctypes_prototypes_match_the_header():
    for name in MANY_FNS:
        args = abi.PROTOS[name[len("dqn_"):]]
        cats = ["ptr" if (a is ctypes.c_void_p or issubclass(a, ctypes._Pointer)) else {ctypes.c_int: "i32"}[a] for a in args]
        assert cats == WANT[name], (name, cats)
    many = abi.PROTOS["rollout_many"]
    assert many[2]._type_ is abi.RolloutCfg and many[3]._type_._type_ is abi.Exploration and many[4]._type_ is abi.RolloutStats
    assert abi.PROTOS["rollout_many_info"][2]._type_ is ctypes.c_uint


def test_shim_ccalls_match_the_header():
    src = open(SHIM).read()
    for name in MANY_FNS:
        m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint, \(", src)
        assert m, name
        i, depth, cur, types = m.end(), 1, "", []
        while depth:                                   # the balanced argument-type tuple
            ch = src[i]; i += 1
            depth += {"(": 1, "{": 1, ")": -1, "}": -1}.get(ch, 0)
            if depth == 0:
                break
            if ch == "," and depth == 1:
                types.append(cur.strip()); cur = ""
            else:
                cur += ch
        types = [t for t in types + [cur.strip()] if t]
        cats = ["ptr" if t.startswith(("Ptr{", "Ref{")) else {"Cint": "i32"}[t] for t in types]
        assert cats == WANT[name], (name, types)
    assert re.search(r"function rollout!\(g::EngineGroup, n_steps;", src) and "Ptr{Ptr{Exploration}}" in src
    # K statistics records travel as an array: the isbits twin of RolloutStats has its fields, in its order
    fields = lambda name: re.findall(r"(\w+)::(\w+)", re.search(r"struct " + name + r"\b(.*?)\n\s*(?:RolloutStats\(\)|end)", src, re.S).group(1))
    assert fields("RolloutStatsRec") == fields("RolloutStats") == [("episodes", "Int64"), ("reward_sum", "Float64"), ("train_steps", "Int64"), ("last_loss", "Float32"), ("last_grad_norm", "Float32")]
    assert re.search(r"(?<!mutable )struct RolloutStatsRec", src)


def test_library_exports_them_and_refuses_without_a_device():
    ge.build()
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, n) for n in MANY_FNS)
    f = abi.bind(lib, "dqn_")
    cfg = (abi.RolloutCfg * 1)(abi.RolloutCfg(4, 8, 1.0, 0.1, 10.0, 0, 1))
    st = (abi.RolloutStats * 1)()
    assert f["rollout_many"](None, 1, cfg, None, st) == -1 and b"null group handle" in f["last_error"]()
    assert f["rollout_many"](None, 0, None, None, None) == -1 and b"null group handle" in f["last_error"]()
    n, lds = ctypes.c_int(-7), ctypes.c_uint(7)
    assert f["rollout_many_info"](None, ctypes.byref(n), ctypes.byref(lds)) == -1 and b"null group handle" in f["last_error"]()
    assert (n.value, lds.value) == (-7, 7)                                    # a refused call writes nothing


def test_engine_group_rollout_checks_its_lists_in_python():
    g = abi.EngineGroup.__new__(abi.EngineGroup)
    g.members, g.f, g._group = [object(), object()], {"rollout_many": None, "last_error": None}, ctypes.c_void_p(1)
    with pytest.raises(pkg.DQNError, match="3 eps schedules were given for 2 members"):
        g.rollout(1, eps=[(1.0, 0.1, 5.0)] * 3)
    with pytest.raises(pkg.DQNError, match="1 exploration entries were given for 2 members"):
        g.rollout(1, explore=[None])
    g._group = ctypes.c_void_p()                                              # (nothing to destroy)


# ---- solve_many: the refusals made in pure Python are unchanged by the grouped loop (no GPU is touched: an engine would raise "no CPU fallback" here)
def _solvers(S, nn, envs, over):
    out, es = [], []
    for k in range(3):
        o = dict(over.get(k, {}))
        n = o.pop("_env_n", 4)
        lstm = o.pop("_lstm", False)
        env = envs.SimpleGridWorld(n=n, seed=5)
        model = nn.Chain(nn.LSTM(2, 8), nn.Dense(8, env.n_actions)) if lstm else nn.Chain(nn.Dense(2, 8, nn.relu), nn.Dense(8, env.n_actions))
        kw = dict(qnetwork=model, exploration_policy=S.EpsGreedyPolicy(env, 0.1), max_steps=48, train_freq=4, target_update_freq=16, train_start=8, batch_size=8,
                  buffer_size=64, eval_freq=24, log_freq=24, save_freq=48, logdir=None, verbose=False, device_envs=True, seed=k, learning_rate=1e-3 * (k + 1))
        kw.update(o)
        out.append(S.DeepQLearningSolver(**kw)); es.append(env)
    return out, es


@pytest.mark.parametrize("field,who,over", many_refusal_cases(), ids=lambda x: x if isinstance(x, str) else None)
def test_solve_many_still_refuses_in_python_before_any_engine(field, who, over):
    S, nn, envs = (importlib.import_module(pkg.__name__ + "." + m) for m in ("solver", "nn", "envs"))
    solvers, es = _solvers(S, nn, envs, over)

    class NoEngine:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created before the refusal")

    with pytest.raises(pkg.DQNError) as ei:
        S.solve_many(solvers, es, engine_cls=NoEngine)
    msg = str(ei.value)
    assert msg.startswith("solve_many: " + field), msg
    assert [int(x) for x in re.findall(r"solvers? (\d+)(?: and (\d+))?", msg)[0] if x != ""] == list(who), msg


def test_solve_many_goes_through_the_group_rollout():
    """statically: one group.rollout per block with train_freq and target_update_freq inside the call, and the per-member loop kept as the declined path"""
    import inspect
    S = importlib.import_module(pkg.__name__ + ".solver")
    src = inspect.getsource(S.solve_many)
    assert "group.rollout_info()" in src and "group.rollout(nxt - t + 1, t0=t, train_freq=s0.train_freq, target_update_freq=s0.target_update_freq" in src
    assert "group.train_steps(1)" in src and "e.rollout(nxt - t + 1, t0=t, train_freq=0, target_update_freq=0" in src
