"""CPU: the acting-step edge cases without a GPU.  Every case sits on the side of every rule it was written for (acting_edges_common.facts against `want`, under the
plan the case runs with); the two sides of an at / above pair differ in exactly the term the pair names; k_tiny_act's reciprocal item division equals the integer
division for every divisor and every item index the LDS rule admits; the CPU twin's ref_envs_peek_q returns, after every vector step of every case on a built-in env
kind, a Q column within E.TOL_Q of the fp64 forward of the rows the step acted on and its first-max argmax; each chunked case's Q column differs in at least one bit from
the unsplit plan's on the same parameters and states (so a wrong chunk order is visible in q); and two wrong engines -- one q value off by one ulp, last-max on an exact
tie -- fail the comparison helper the GPU file uses."""
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
import acting_edges_common as A
import ref

pkg = ge.load_package()
envs = importlib.import_module(pkg.__name__ + ".envs")
CASES = A.cases()
TWIN_CASES = [n for n, c in CASES.items() if c["twin"] and c["runs"]]
TEETH = {}      # case -> (steps compared, steps whose q differed in a bit, steps whose executed actions differed): printed, docs/history/acting_edges.md has the run


def twin_of(c, **kw):
    return A.build(c, ref.Twin, ref.default_plan, envs, threads=4, **kw)


def one_step(h, t, eps, train=True):
    return h.rollout(1, t0=t, train_freq=A.TRAIN_FREQ if train else 0, target_update_freq=A.TARGET_FREQ if train else 0, eps=eps)


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_sits_where_it_was_written_for(name):
    c = CASES[name]
    layers, hp = A.layers_hp(c)
    default = ref.default_plan(layers, hp)
    f = A.check_want(c, A.case_plan(c, default))
    assert f == A.facts(c), "the default plan cuts a contraction of this case: its facts depend on more than the case names"
    assert all(kc == 0 for kc, _, _ in default) or c["fwd_kc"] or c["last_kc"], default
    assert f["n_layers"] <= A.MAX_LAYERS and len(f["levels"]) <= A.MAX_LAYERS
    assert (f["refusal"] is None) == c["runs"]
    if c["runs"] and c["grouped"]:
        assert f["max_item"] < f["items"] <= A.MAX_ITEMS and f["lds_bytes"] + A.TAIL_LDS <= A.LDS_LIMIT
    assert c["twin"] == (not isinstance(c["env"], tuple) and name != "acts")


def test_the_case_table_covers_what_the_issue_names():
    f = {n: A.facts(c) for n, c in CASES.items()}
    assert f["lds_at"]["lds_bytes"] == 103424 and (952 // 4) & (952 // 4 - 1) != 0                     # n / 4 = 238: no power of two
    assert f["lds_at"]["lds_floats"] == 152 + 1904 + 19992 + 3808 == A.MAX_ITEMS
    assert CASES["lds_at"]["n_fill"] + CASES["lds_at"]["n"] <= CASES["lds_at"]["cap"] < CASES["lds_at"]["n_fill"] + 2 * CASES["lds_at"]["n"]      # wraps on the second step
    assert f["pxn_at"]["pxn"] == 262144 and f["pxn_above"]["pxn"] > 262144 and f["pxn_above"]["total_bytes"] <= A.LDS_LIMIT
    assert [k % 4 for k in (7, 13)] == [3, 1] and f["tails_v4"]["chunks"] == f["tails_scalar"]["chunks"] == [1, 2, 3]
    assert f["k19_scalar"]["k_tail8"][1] == 3 and f["k19_scalar"]["chunks"] == [1, 1]
    assert f["l8"]["n_layers"] == 8 and CASES["l8"]["u8"]
    assert {l.act for l in CASES["acts"]["net"].all_layers()[:-1]}.isdisjoint({A.I, A.R, A.T}) and len({l.act for l in CASES["acts"]["net"].all_layers()[:-1]}) == 3
    r2, r9 = CASES["ring_two"], CASES["ring_two_c9"]
    assert (r2["n"], r2["cap"], r2["n_fill"], r2["B"]) == (2, 8, 4, 4) and (r9["cap"], f["ring_two_c9"]["cap2"]) == (9, 16)
    assert (r2["n_fill"] + 2 * r2["n"]) == r2["cap"]                                                   # the second step ends at the ring's end without wrapping, the third starts at 0
    assert {n for n, c in CASES.items() if not c["grouped"]} == {"split_head_at", "split_head_above"}
    assert all(c["B"] <= 8 and c["n_fill"] >= c["B"] for c in CASES.values())
    assert all(c["max_len"] < sum(A.CALLS) for c in CASES.values())                                   # episodes end inside the run


@pytest.mark.parametrize("at", list(A.PAIRS))
def test_both_sides_of_a_pair_differ_in_the_term_they_name(at):
    above, term = A.PAIRS[at]
    a, b = CASES[at], CASES[above]
    fa, fb = A.facts(a), A.facts(b)
    assert b["n"] == a["n"] + 1 and fa["P"] == fb["P"] and fa["levels"] == fb["levels"] and fa["chunks"] == fb["chunks"]
    assert {k: a[k] for k in ("env", "B", "cap", "u8", "fwd_kc", "last_kc")} == {k: b[k] for k in ("env", "B", "cap", "u8", "fwd_kc", "last_kc")}
    if term == "staged":
        assert fa["staged"] and not fb["staged"] and fa["refusal"] is None and fb["refusal"] is None
        assert fa["head_floats"] <= A.HEAD_LDS < fb["head_floats"] and fb["head_floats"] - fa["head_floats"] == fa["per_col"]
    elif term == "lds":
        assert fa["refusal"] is None and fb["refusal"] == "lds" and fa["pxn_ok"] and fb["pxn_ok"]
        assert fa["total_bytes"] == A.LDS_LIMIT < fb["total_bytes"] and A.refusal_text(b) == f"it needs {fb['total_bytes']} bytes of LDS"
    else:
        assert fa["refusal"] is None and fb["refusal"] == "pxn" and fa["pxn"] == A.PXN_LIMIT < fb["pxn"]
        assert max(fa["total_bytes"], fb["total_bytes"]) <= A.LDS_LIMIT and A.refusal_text(b) == f"too many parameters for {b['n']} copies"


def test_reciprocal_item_division_is_exact_for_every_admitted_item_count():
    """k_tiny_act divides an item index x by the copy count (or a quarter of it) as int((float(x) + 0.5f) * (1.0f / float(d))).  x < 25 856 = (144 KB - 43 KB) / 4: no
    activation array is longer than the dynamic LDS the eligibility rule admits; d <= 1024 copies.  Exhaustive."""
    x = np.arange(A.MAX_ITEMS, dtype=np.int64)
    assert A.MAX_ITEMS == 25856
    bad = sum(int((A.qdiv(x, d) != x // d).sum()) for d in range(1, 1025))
    assert bad == 0, bad
    for c in A.runnable_grouped():
        f = A.facts(c)
        assert f["max_item"] < A.MAX_ITEMS and 1 <= c["n"] <= 1024


@pytest.fixture(scope="module")
def twin_runs():
    """computed ONCE per case: the twin stepped one vector step per call through the run's cadence (t = 1 .. 8, train steps and target syncs inside), each step's record
    with the parameters it acted with"""
    out = {}

    def get(name):
        if name not in out:
            c = CASES[name]
            tw = twin_of(c)
            with pytest.raises(pkg.DQNError, match="has not taken a vector step"):
                tw.envs_peek_q()
            recs, trained = [], False
            for t in range(1, sum(A.CALLS) + 1):
                p = tw.get_params(0)
                st = one_step(tw, t, c["eps"])
                trained = trained or st["train_steps"] > 0
                recs.append((A.step_record(tw, st, trained=trained, td=False), p))
            tw.close()
            out[name] = recs
        return out[name]
    return get


@pytest.mark.parametrize("name", TWIN_CASES)
def test_twin_accessor_returns_the_q_column_it_acted_on(twin_runs, name):
    c = CASES[name]
    recs = twin_runs(name)
    for t, (rec, p) in enumerate(recs, 1):
        A.check_record(c, rec, p_acting=p, what=f"twin, vector step {t}")
    assert int(recs[-1][0]["stats.episodes"]) > 0 and int(recs[-1][0]["counters.train_steps"]) == sum(A.CALLS) // A.TRAIN_FREQ
    assert any(not np.array_equal(r["peek.actions"], r["peekq.greedy"]) for r, _ in recs), "nothing explored: the run would not tell the executed action from the greedy one"


@pytest.mark.parametrize("name", TWIN_CASES)
def test_twin_actions_are_the_greedy_ones_when_nothing_explores(name):
    c = CASES[name]
    tw = twin_of(c)
    for t in (1, 2, 3):
        p = tw.get_params(0)
        st = one_step(tw, t, (0.0, 0.0, 1.0))
        A.check_record(c, A.step_record(tw, st, trained=t >= 2, td=False), p_acting=p, greedy_only=True, what=f"twin, eps = 0, vector step {t}")
    tw.evaluate(2, 3, seed=1)
    with pytest.raises(pkg.DQNError, match="vector step"):      # the evaluation's forward took the policy workspace: refused until the set steps again
        tw.envs_peek_q()
    tw.close()


@pytest.mark.parametrize("name", A.CHUNKED)
def test_a_chunked_plan_shows_in_q(name):
    """teeth: under the case's plan the twin's Q column differs in at least one bit from the unsplit plan's, on the same parameters and states -- a kernel that summed the
    chunks in another order, or not at all, would therefore show in q.  Whether the executed ACTIONS differ over the run is recorded: where they do not, nothing but the
    accessor would have noticed"""
    c = CASES[name]
    layers, hp = A.layers_hp(c)
    a, b = twin_of(c), twin_of(c, plan=A.unsplit_plan(c, ref.default_plan(layers, hp)))
    assert a.plan() != b.plan()
    compared = q_diff = act_diff = 0
    for t in range(1, sum(A.CALLS) + 1):
        same_state = all(np.array_equal(x, y) for x, y in zip(a.envs_peek(), b.envs_peek()))
        for h in (a, b):
            one_step(h, t, c["eps"], train=False)      # no training: the parameters stay the same on both sides
        if not same_state:
            break
        (qa, _), (qb, _) = a.envs_peek_q(), b.envs_peek_q()
        compared += 1; q_diff += int(not np.array_equal(qa, qb)); act_diff += int(not np.array_equal(a.envs_peek()[1], b.envs_peek()[1]))
    a.close(); b.close()
    TEETH[name] = (compared, q_diff, act_diff)
    print(f"teeth {name}: {compared} steps on the same states, q differed in {q_diff}, executed actions in {act_diff}")
    assert compared >= 1 and q_diff >= 1, TEETH[name]


class _Wrong:
    """a wrong engine: the twin with what envs_peek_q returns replaced"""

    def __init__(self, tw, peek_q):
        self._tw, self._peek_q = tw, peek_q

    def __getattr__(self, k):
        return getattr(self._tw, k)

    def envs_peek_q(self):
        return self._peek_q(*self._tw.envs_peek_q())


def test_one_ulp_in_one_q_value_fails_the_comparison():
    c = CASES["tails_scalar"]
    tw = twin_of(c)
    p = tw.get_params(0)
    st = one_step(tw, 1, c["eps"])
    good = A.step_record(tw, st, trained=False, td=False)

    def off_by_one_ulp(q, a):
        q = q.copy(); j = int(np.argmin(q[2]))      # the smallest value of copy 2: its argmax, hence every action, stays what it was
        q[2, j] = np.nextafter(q[2, j], np.float32(-np.inf))
        return q, a
    bad = A.step_record(_Wrong(tw, off_by_one_ulp), st, trained=False, td=False)
    A.check_record(c, good, want=good, p_acting=p, what="the twin against itself")
    A.check_record(c, bad, p_acting=p, what="one ulp, without a reference")      # what the suite held before: actions, and a tolerance -- both blind to one ulp
    assert all(np.array_equal(bad[k], good[k]) for k in good if k != "peekq.q")
    with pytest.raises(AssertionError, match="peekq.q"):
        A.check_record(c, bad, want=good, p_acting=p, what="one ulp")
    tw.close()


def test_last_max_on_an_exact_tie_fails_the_comparison():
    c = CASES["ring_two"]
    net = c["net"]
    ps = net.unflatten(A.initial_params(c))
    ps[-2] = np.zeros_like(ps[-2]); ps[-1] = np.full_like(ps[-1], 0.25)      # the output layer ignores its input: every action's Q is the same bias
    tw = twin_of(c, params=net.flatten(ps).astype(np.float32))
    p = tw.get_params(0)
    st = one_step(tw, 1, (0.0, 0.0, 1.0))
    good = A.step_record(tw, st, trained=False, td=False)
    assert np.array_equal(good["peekq.q"], np.full((c["n"], 4), 0.25, np.float32)) and not good["peekq.greedy"].any()
    A.check_record(c, good, p_acting=p, greedy_only=True, what="exact tie")
    last_max = lambda q, a: (q, (q.shape[1] - 1 - np.argmax(q[:, ::-1], axis=1)).astype(np.int32))
    bad = A.step_record(_Wrong(tw, last_max), st, trained=False, td=False)
    assert (bad["peekq.greedy"] == 3).all()
    with pytest.raises(AssertionError, match="first-max"):
        A.check_record(c, bad, p_acting=p, what="last-max")
    tw.close()
