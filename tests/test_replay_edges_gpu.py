"""GPU (-m gpu): the replay edge table of tests/replay_edges_common.py on the HIP engine through the C ABI, against the fp64 model and the stratified law of
tests/replay_reference.py: every draw of replay_sample and of a sampled train step (single-launch step, fused sample + gather on f32 / u8 / byte-arena rows, the
sample launch at B > 64 with the priority block in a backward launch or on the second stream, pipelined train_steps) must land within the derived slack d of where
the fp64 cumulative sum of the reported leaves puts its Philox target; leaves, IS weights, the root and the loss of sampled steps are held to fp64 too.

On top of the shared checker, per case: the engine equals the C twin bit for bit (indices, priorities, losses, td), use_graph 0 and 1 give the same bits, and the
launch names of profile_step show the sampling site the case was written for.

No case found a defect in the engine or the twin; test_zz_report_worst_margins prints the largest margin per quantity and the redraw counts of a run."""
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import ref
import replay_edges_common as C

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


def check_case(pkg, c, other_graph=True):
    C.check_want(c)
    r, rec = C.run(pkg.Engine, c, keep=True)                               # against the fp64 model and the law
    C.same_bits(rec, C.run(ref.Twin, c, judge=False, threads=8), f"{c.name}: engine vs twin")
    if other_graph:
        C.same_bits(rec, C.run(pkg.Engine, c, graph=1 - c.graph, judge=False), f"{c.name}: use_graph {c.graph} vs {1 - c.graph}")
    if c.names:                                                            # profile_step runs one more (eager, sampled) step: last
        tokens = {t for n, _ in r.h.profile_step(max_entries=512) for t in n.split("+")}
        must, never = {n for n in c.names if n[0] != "-"}, {n[1:] for n in c.names if n[0] == "-"}
        assert must <= tokens and not (never & tokens), (c.name, "missing", sorted(must - tokens), "unexpected", sorted(never & tokens), "launched", sorted(tokens))
    r.h.close()


@pytest.mark.parametrize("c", C.CASES, ids=IDS(C.CASES))
def test_case_vs_law_twin_and_schedule(pkg, c):
    check_case(pkg, c)


@pytest.mark.parametrize("c", C.DEEP, ids=IDS(C.DEEP))
def test_deep_case_vs_law_and_twin(pkg, c):
    check_case(pkg, c, other_graph=False)                                  # (4.2 M rows: one engine run; the graph companion runs on every other case)


def test_pipelined_step_takes_the_pregathered_batch(pkg):
    """the middle step of train_steps(n) on the multi-launch program gathers the next batch inside its Adam launch"""
    c = C.BY_NAME["site_pipelined"]
    r, _ = C.run(pkg.Engine, c, keep=True)
    names = [n for n, _ in r.h.profile_step(max_entries=512, steady=True)]
    assert "adam+gather" in names and "sample_gather" not in names, names
    r.h.close()


def test_chi_square_non_power_of_two_partly_filled(pkg):
    C.chi_square(pkg.Engine, cap=100, size=83, B=16, draws=2000)


def test_chi_square_b512(pkg):
    C.chi_square(pkg.Engine, cap=3000, size=2500, B=512, draws=300)


def test_zz_report_worst_margins():
    """not a check: prints the largest margin / tolerance per quantity and the wall time of this file"""
    print("\nworst margin / tolerance on the engine:", {k: float(f"{v:.3g}") for k, v in sorted(C.WORST.items())})
    print("distinct cases on the engine, (redraws judged, left out, with R < S / 4):", C.REDRAWS)
    print(f"wall time of the file: {time.time() - T0:.0f} s")
