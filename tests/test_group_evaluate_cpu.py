"""CPU (-m "not gpu"): the grouped-evaluation entry points of the C ABI are declared, bound and called with matching arities (header, ctypes prototypes, Julia shim
-- the shim is not executed here: checked statically, in the style of test_shim_static_cpu.py), and the refusals made in pure Python hold before any engine exists."""
import importlib
import os
import re

import pytest

import __graft_entry__ as ge
from group_evaluate_common import header_arity

pkg = ge.load_package()
HDR = open(os.path.join(ge.ROOT, "include", "dqn_mi355x.h")).read()
SHIM = open(os.path.join(ge.PKG_DIR, "julia", "DeepQLearningMI355X.jl")).read()
NEW = {"evaluate_many": 6, "evaluate_many_info": 6}


@pytest.mark.parametrize("name", sorted(NEW))
def test_prototype_arity_matches_the_header(name):
    assert header_arity(HDR, "dqn_" + name) == NEW[name] == len(pkg._abi.PROTOS[name])


@pytest.mark.parametrize("name", sorted(NEW))
def test_shim_ccall_has_the_header_arity(name):
    m = re.search(r"ccall\(\(:dqn_" + name + r", LIB\), Cint, \(([^)]*)\),([^\n]*)\)\)", SHIM)
    assert m, name
    types = [t for t in m.group(1).split(",") if t.strip()]
    args = [a for a in m.group(2).split(",") if a.strip()]
    assert len(types) == NEW[name] == len(args), (types, args)
    assert types[0].strip() == "Ptr{Cvoid}" and args[0].strip() == "g.h"


def test_header_states_the_law_and_the_bound():
    i = HDR.index("grouped evaluation")
    text = HDR[i:HDR.index("int dqn_evaluate_many(", i)]
    for words in ("THE LAW", "bit for bit", "ascending order", "steps_per_launch", "dqn_envs_peek_q is refused", "REFUSED before anything is enqueued", "Out of scope"):
        assert words in text, words


def test_seed_list_of_the_wrong_length_is_refused_in_python():
    class FakeGroup(pkg._abi.EngineGroup):
        def __init__(self):      # no engine, no library call
            self.members, self.f = [object(), object()], {"evaluate_many": lambda *a: pytest.fail("the library was called")}

        def __del__(self):
            pass

    with pytest.raises(pkg.DQNError, match="EngineGroup.evaluate: 3 seeds were given for 2 members"):
        FakeGroup().evaluate(4, 5, [1, 2, 3])
    with pytest.raises(pkg.DQNError, match="this library does not export evaluate_many"):
        g = FakeGroup(); g.f = {}; g.evaluate(4, 5, [1, 2])


def _solvers(over):
    S, nn, envs = (importlib.import_module(pkg.__name__ + "." + m) for m in ("solver", "nn", "envs"))
    out, es = [], []
    for k in range(3):
        env = envs.SimpleGridWorld(n=4, seed=5)
        model = nn.Chain(nn.Dense(2, 8, nn.relu), nn.Dense(8, env.n_actions))
        kw = dict(qnetwork=model, exploration_policy=S.EpsGreedyPolicy(env, 0.1), max_steps=48, train_freq=4, target_update_freq=16, train_start=8, batch_size=8,
                  buffer_size=64, eval_freq=24, log_freq=24, save_freq=48, logdir=None, verbose=False, device_envs=True, seed=k, learning_rate=1e-3 * (k + 1))
        kw.update(over.get(k, {}))
        out.append(S.DeepQLearningSolver(**kw)); es.append(env)
    return S, out, es


class NoEngine:
    def __init__(self, *a, **k):
        raise AssertionError("an engine was created before the refusal")


@pytest.mark.parametrize("field", ["num_ep_eval", "max_episode_length"])
def test_solve_many_refuses_disagreeing_evaluations_by_field_and_indices(field):
    S, solvers, es = _solvers({2: {field: 7}})
    with pytest.raises(pkg.DQNError) as ei:
        S.solve_many(solvers, es, engine_cls=NoEngine)
    msg = str(ei.value)
    assert msg.startswith("solve_many: " + field + " differs between solvers 0 and 2 ("), msg
    assert "vs 7" in msg


def test_a_member_with_its_own_evaluation_policy_is_free_to_disagree():
    class Stop(Exception):
        pass

    def factory(*a, **k):
        raise Stop()

    S, solvers, es = _solvers({0: {"num_ep_eval": 7, "evaluation_policy": lambda *a: (0.0, 0, 0)}, 2: {"max_episode_length": 50, "evaluation_policy": lambda *a: (0.0, 0, 0)}})
    with pytest.raises(Stop):      # every Python check passes: the first thing that fails is the engine factory
        S.solve_many(solvers, es, engine_cls=factory)
    # ... and the refusal names the first two members that keep basic_evaluation
    S, solvers, es = _solvers({0: {"evaluation_policy": lambda *a: (0.0, 0, 0)}, 2: {"num_ep_eval": 9}})
    with pytest.raises(pkg.DQNError, match=r"solve_many: num_ep_eval differs between solvers 1 and 2 \(\d+ vs 9\)"):
        S.solve_many(solvers, es, engine_cls=NoEngine)
