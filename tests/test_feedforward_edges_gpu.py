"""GPU (-m gpu): the feed-forward edge table of tests/feedforward_edges_common.py on the HIP engine through the C ABI, against the fp64 reference of
tests/feedforward_reference.py: kernel-selection boundaries of the forward / dW / dX families, the single-launch step, head fusion and the byte
arena; rectangular convolutions (kh != kw, sh != sw) as first and second layers; 32 seeded random configurations; 200 Adam steps.  Per case, three
train steps on given indices, each compared at the engine's own previous parameters and batch: Q values, greedy indices (exactly), targets, td,
loss, every parameter block's gradient, grad_norm, the parameters after an fp64 Adam carried on the engine's gradients, and the priorities.

On top of the shared checker, per case: the engine equals the C twin bit for bit, use_graph 0 and 1 give the same bits, and the launch names of
profile_step show the kernel family the selection rules (restated in feedforward_edges_common.facts) give for the case.  What launch names cannot
tell: the LDS-tiled and the direct-MFMA dW (dX) launches share the name "dw_<layer>" ("dx_<layer>"), so names separate them only from the VALU
tasks; the head rule fwd_kc = 32 and the dW tile width NT are visible in the plan and the facts only.

Found by this file: a dueling join whose streams do not share one dX launch (two sources x three plan chunks, e.g. hidden layers wider than 512)
ran the second stream's dX before the first stream's LDS-tiled dX had written the sum it adds to; engine_program.hip now issues that launch first
(case dx_join_units6).

Measured on one MI355X (143 tests, 7 s for the file, 9.4 s with pytest's start-up).  Largest error as a fraction of its tolerance: q_on_s 0.12,
q_on_sp 0.13, q_tg_sp 0.23, y 0.11, td 0.12, loss 0.04, grad_norm 0.03, IS weights 0.06, beta powers 0.001; largest gradient error / block scale
(the bound is GRAD_C = 2e-5): conv W 1.55e-6, conv b 1.23e-6, dense W 3.24e-6, dense b 3.19e-6.  No case needed a tolerance of its own."""
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import feedforward_edges_common as C
import ref

pytestmark = pytest.mark.gpu
IDS = lambda cs: [c.name for c in cs]
T0 = time.time()


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package(); p.lib()
    return p


def check_case(pkg, c):
    f = C.check_want(c)                                   # the case stands on the side of the rule it was written for
    net = C.network(c); hp = C.hparams(c, net); layers = ref.layers_from_network(net)
    assert pkg.default_plan(layers, hp) == ref.default_plan(layers, hp)
    h, rec = C.run_checked(pkg.Engine, c, plan=ref.default_plan)                 # against the fp64 reference
    C.same_bits(rec, C.replay_steps(ref.Twin, c, threads=8, plan=ref.default_plan), f"{c.name}: engine vs twin")
    C.same_bits(rec, C.replay_steps(pkg.Engine, c, graph=1 - c.graph, plan=ref.default_plan), f"{c.name}: use_graph {c.graph} vs {1 - c.graph}")
    if not f["tiny"]:
        assert h.batch_arena_elem_bytes() == (1 if f["arena"] else 4), c.name
    C.assert_launches(h, f, c.name)                       # profile_step runs one more (eager) step: last
    h.close()


@pytest.mark.parametrize("c", C.CASES, ids=IDS(C.CASES))
def test_case_vs_fp64_reference_twin_and_schedule(pkg, c):
    check_case(pkg, c)


@pytest.mark.parametrize("c", C.RANDOM, ids=IDS(C.RANDOM))
def test_random_configuration_vs_fp64_reference_twin_and_schedule(pkg, c):
    check_case(pkg, c)


@pytest.mark.parametrize("c", C.LONG, ids=IDS(C.LONG))
def test_adam_over_200_steps(pkg, c):
    C.long_adam(pkg.Engine, c, plan=ref.default_plan).close()


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity and the wall time of this file (the module docstring records them)"""
    import feedforward_reference as FR
    print("\nworst error / tolerance:", {k: round(v, 4) for k, v in sorted(C.WORST.items())})
    print("worst gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(FR.WORST.items()) if k.startswith(("conv", "dense"))})
    print(f"wall time of the file: {time.time() - T0:.0f} s")
