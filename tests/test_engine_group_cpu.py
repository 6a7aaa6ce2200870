"""CPU: the engine-group seam without a GPU -- the header, the ctypes mirror and the Julia shim agree on the four dqn_group_* prototypes (the shim cannot be
executed here: checked statically, in the style of test_shim_static_cpu.py), the ctypes struct has the header's layout, and solver.solve_many refuses in pure
Python, before any engine exists, naming the field and the solver indices."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest

import __graft_entry__ as ge
from engine_group_common import many_refusal_cases
from test_shim_static_cpu import julia_struct_layout

pkg = ge.load_package()
abi = pkg._abi
SHIM = os.path.join(ge.ROOT, "deepqlearning.jl_amd", "julia", "DeepQLearningMI355X.jl")
HEADER = os.path.join(ge.ROOT, "include", "dqn_mi355x.h")
GROUP_FNS = ("dqn_group_create", "dqn_group_train_steps", "dqn_group_info", "dqn_group_destroy")


def header_protos():
    return {m.group(1): [x.strip() for x in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",") if x.strip()]
            for m in re.finditer(r"\bint\s+(dqn_group_\w+)\s*\(([^;{]*?)\)\s*;", open(HEADER).read(), re.S)}


def c_cat(param):
    if "*" in param:
        return "ptr"
    return {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint64_t": "u64", "size_t": "u64", "float": "f32"}[param.rsplit(" ", 1)[0].replace("const ", "").strip()]


def test_header_declares_exactly_the_four_group_entry_points():
    protos = header_protos()
    assert set(protos) == set(GROUP_FNS)
    assert [len(protos[n]) for n in GROUP_FNS] == [3, 4, 2, 1]
    assert [c_cat(p) for p in protos["dqn_group_train_steps"]] == ["ptr", "i32", "ptr", "ptr"]
    assert [c_cat(p) for p in protos["dqn_group_create"]] == ["ptr", "i32", "ptr"]


def test_ctypes_prototypes_match_the_header():
    protos = header_protos()
    for name in GROUP_FNS:
        args = abi.PROTOS[name[len("dqn_"):]]
        cats = ["ptr" if (a is ctypes.c_void_p or issubclass(a, ctypes._Pointer)) else {ctypes.c_int: "i32"}[a] for a in args]
        assert cats == [c_cat(p) for p in protos[name]], (name, cats, protos[name])


def test_shim_ccalls_match_the_header():
    src = open(SHIM).read()
    protos = header_protos()
    for name in GROUP_FNS:
        m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint, \(", src)
        assert m, name
        i, depth, cur, types = m.end(), 1, "", []
        while depth:                                   # the balanced argument-type tuple: (Ptr{Ptr{Cvoid}}, Cint, ...)
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
        assert cats == [c_cat(p) for p in protos[name]], (name, types, protos[name])
    assert "finalizer(close!, g)" in src and re.search(r"function train_steps!\(g::EngineGroup, n::Integer\)", src)


def test_group_info_struct_has_the_header_layout(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dqn_mi355x.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(dqn_group_info_t), '
           'offsetof(dqn_group_info_t, n_members), offsetof(dqn_group_info_t, max_lds_bytes), offsetof(dqn_group_info_t, launches_per_step));}')
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ge.ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    G = abi.GroupInfo
    assert got == [ctypes.sizeof(G), G.n_members.offset, G.max_lds_bytes.offset, G.launches_per_step.offset]
    size, offsets = julia_struct_layout(open(SHIM).read(), "GroupInfo")
    assert size == ctypes.sizeof(G) and list(offsets) == [f[0] for f in G._fields_] and all(offsets[f[0]] == getattr(G, f[0]).offset for f in G._fields_)


def test_library_exports_the_group_symbols():
    ge.build()
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, n) for n in GROUP_FNS + ("dqn_get_last_td",))
    f = abi.bind(lib, "dqn_")
    assert f["group_destroy"](None) == 0                                   # like dqn_engine_destroy(NULL)
    assert f["group_train_steps"](None, 1, None, None) == -1 and b"null group handle" in f["last_error"]()
    out = ctypes.c_void_p(123)
    assert f["group_create"](None, 0, ctypes.byref(out)) == -1 and b"outside 1..4096" in f["last_error"]() and not out.value
    assert f["group_create"](None, 4097, ctypes.byref(out)) == -1 and b"outside 1..4096" in f["last_error"]()
    arr = (ctypes.c_void_p * 2)(None, None)
    assert f["group_create"](arr, 2, ctypes.byref(out)) == -1 and b"member 0 is a null engine handle" in f["last_error"]()


# ---- solve_many: refusals before any engine exists (no GPU is touched: an engine would raise "no CPU fallback" here)
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
def test_solve_many_refuses_in_python_naming_field_and_indices(field, who, over):
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


def test_solve_many_accepts_what_it_should_up_to_the_first_engine():
    """the same three solvers without an override pass every Python check: the first thing that fails is the engine factory"""
    S, nn, envs = (importlib.import_module(pkg.__name__ + "." + m) for m in ("solver", "nn", "envs"))
    solvers, es = _solvers(S, nn, envs, {})

    class Stop(Exception):
        pass

    def factory(*a, **k):
        raise Stop()

    with pytest.raises(Stop):
        S.solve_many(solvers, es, engine_cls=factory)
    solvers[0].logdir, solvers[1].logdir = ".", None                     # None is no directory: never "the same" as one
    with pytest.raises(Stop):
        S.solve_many(solvers, es, engine_cls=factory)
    with pytest.raises(pkg.DQNError, match="3 environments were given for 2 solvers"):
        S.solve_many(solvers[:2], es, engine_cls=factory)
