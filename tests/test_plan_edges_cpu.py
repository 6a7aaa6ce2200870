"""CPU: the plan table of tests/plan_edges_common.py on the C twin (oracle/dqn_ref.c) -- feed-forward train steps under caller-supplied summation plans,
against the fp64 reference of tests/feedforward_reference.py at the tolerances of feedforward_edges_common.run_checked (none widened).  Per case: it stands
on the side of every selection rule it was written for, evaluated on the EDITED plan; the two legs of the reference agree along its trajectory; the twin
under the plan passes the checker over three steps; and the twin's record under the plan differs from its record under the default plan in at least one
bit -- or, where the edit cannot change the summation order (chunk length >= the contraction), equals it.  tests/test_plan_edges_gpu.py runs the same table
on the HIP engine and holds it to this twin bit for bit.  Figures: docs/history/plan_edges.md."""
import numpy as np
import pytest

import feedforward_edges_common as C
import plan_edges_common as P
import ref

IDS = lambda cs: [c.name for c in cs]
_REC = {}


def twin_record(c, plan, tag):
    if (c.name, tag) not in _REC:
        _REC[c.name, tag] = C.replay_steps(ref.Twin, c, threads=8, plan=plan)
    return _REC[c.name, tag]


def differs(a, b):
    for x, y in zip(a, b):
        if x["loss"] != y["loss"] or x["gn"] != y["gn"] or any(not np.array_equal(x[k], y[k]) for k in ("td", "g", "p", "pr")) or \
           any(not np.array_equal(x["q"][k], y["q"][k]) for k in ("q_on_s", "q_on_sp", "q_tg_sp", "y")):
            return True
    return False


@pytest.mark.parametrize("c", P.CASES, ids=IDS(P.CASES))
def test_case_stands_on_its_side_of_the_rule_under_its_plan(c):
    f = C.check_want(c)
    net = C.network(c); hp = C.hparams(c, net)
    plan = C.case_plan(c, C.FR.layer_descs(net), hp)
    assert [(g.fwd_kc, g.dx_kc, g.dw_kc) for g in f["G"]] == plan
    if c.edit is not None:
        assert (plan == ref.default_plan(C.FR.layer_descs(net), hp)) is False, f"{c.name}: the edit is the default plan"


def test_table_reaches_every_family_on_an_edited_plan():
    """what the table is for: every kernel family of the forward, dX and dW with MORE than one chunk, ragged last chunks in each, both slab-sum forms, both sides of the
    red_head slab cap and of U_MAX, the single-launch step with chunks"""
    fs = {c.name: C.case_facts(c) for c in P.CASES if c.edit is not None}
    B = {c.name: c.B for c in P.CASES}
    seen = {"fwd": set(), "dx": set(), "dw": set()}
    ragged = {"fwd": set(), "dx": set(), "dw": set()}
    for name, f in fs.items():
        if f["tiny"]:
            continue
        for g in f["G"]:
            for fam, K, kc in (("fwd", g.K, g.fwd_kc), ("dw", g.npos * B[name], g.dw_kc)) + ((("dx", g.N, g.dx_kc),) if g.kind == "dense" and g.src >= 0 else ()):
                if C.nchunks(K, kc) > 1 and f[f"{fam}{g.i}"] in ("lds", "mfma", "valu", "head"):
                    seen[fam].add(f[f"{fam}{g.i}"])
                    if K % kc:
                        ragged[fam].add(f[f"{fam}{g.i}"])
    assert seen["fwd"] >= {"lds", "mfma", "valu", "head"} and ragged["fwd"] >= {"lds", "mfma", "valu", "head"}, (seen, ragged)
    assert seen["dx"] >= {"lds", "mfma", "valu"} and ragged["dx"] >= {"lds", "mfma", "valu"}, (seen, ragged)
    assert seen["dw"] >= {"lds", "mfma", "valu", "head"} and ragged["dw"] >= {"lds", "mfma", "valu"}, (seen, ragged)
    assert {f["dwsum"] for f in fs.values() if not f["tiny"]} >= {"adam", "launch"}
    assert {f["head"] for n, f in fs.items() if n.startswith("plan_heads_s")} == {"red_head", "head_td"}
    assert {f["tiny"] for n, f in fs.items() if n.startswith("plan_tiny")} == {True, False}
    conv = [(C.conv_max_chunks(g), f[f"dxmode{g.i}"]) for n, f in fs.items() if n.startswith("plan_dx_conv") for g in f["G"] if g.kind == "conv" and g.src >= 0]
    assert any(n > C.U_MAX and m == -1 for n, m in conv) and any(1 < n <= C.U_MAX and m == 3 for n, m in conv)


@pytest.mark.parametrize("c", P.CASES, ids=IDS(P.CASES))
def test_reference_legs_agree_along_the_trajectory(c):
    C.check_legs_along_trajectory(c)


@pytest.mark.parametrize("c", P.CASES, ids=IDS(P.CASES))
def test_twin_under_the_plan_vs_fp64_reference(c):
    h, rec = C.run_checked(ref.Twin, c, threads=8, plan=P.plan_of(c))
    net = C.network(c)
    assert h.plan() == C.case_plan(c, C.FR.layer_descs(net), C.hparams(c, net))
    h.close()
    C.same_bits(rec, twin_record(c, P.plan_of(c), "plan"), f"{c.name}: checked run vs plain replay")


@pytest.mark.parametrize("c", P.CASES, ids=IDS(P.CASES))
def test_edit_changes_a_bit_unless_it_cannot(c):
    a, b = twin_record(c, P.plan_of(c), "plan"), twin_record(c, P.DEFAULT, "default")
    if c.same:
        C.same_bits(a, b, f"{c.name}: a chunk length >= the contraction is unsplit")
    else:
        assert differs(a, b), f"{c.name}: the edited plan gives the default plan's bits in every recorded number: the case tests nothing"


@pytest.mark.parametrize("plan, msg", [
    ([(-1, 0, 0), (0, 0, 0)], r"layer 0: fwd_kc = -1, dx_kc = 0: a chunk length must be >= 0"),
    ([(0, 0, 0), (0, -32, 0)], r"layer 1: fwd_kc = 0, dx_kc = -32: a chunk length must be >= 0"),
    ([(0, 0, -2 ** 31), (0, 0, 0)], r"layer 0: dw_kc = -2147483648: a column group \(dw_kc < 0\) holds at most batch_size = 32 columns"),
    ([(0, 0, -33), (0, 0, 0)], r"layer 0: dw_kc = -33: a column group"),
], ids=["fwd_kc<0", "dx_kc<0", "dw_kc=INT_MIN", "dw_kc<-B"])
def test_twin_refuses_what_the_engine_refuses(plan, msg):
    """the plans engine creation refuses by layer and rule (tests/test_plan_edges_gpu.py holds the engine to the same messages)"""
    net = C.network(C.case("refusal", 64, C.mlp(64, 32, 4), 32, prio=0))
    hp = ref.hparams_for(net, batch_size=32, buffer_size=40, prioritized_replay=0)
    with pytest.raises(ref.abi.DQNError, match=msg):
        ref.Twin(C.FR.layer_descs(net), hp, plan=plan)


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity this run showed (docs/history/plan_edges.md records them)"""
    import feedforward_reference as FR
    print("\nworst error / tolerance:", {k: round(v, 4) for k, v in sorted(C.WORST.items())})
    print("worst gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(FR.WORST.items()) if k.startswith(("conv", "dense"))})
    print("draws:", {c.name: C.prepare(c)[1]["tries"] for c in P.CASES if C.prepare(c)[1]["tries"]})
