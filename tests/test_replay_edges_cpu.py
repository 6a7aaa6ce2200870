"""CPU (-m "not gpu"): the replay edge table of tests/replay_edges_common.py on the C twin, against the fp64 model and the stratified law of
tests/replay_reference.py -- plus what pins the reference itself: its Philox4x32-10 against a table printed by ATen's engine, its leaves and IS weights
against oracle/dqn_oracle.py's PrioritizedReplay, and every case's sharpness on the model before any engine exists."""
import numpy as np
import pytest

import dqn_oracle as O
import ref
import replay_edges_common as C
import replay_reference as RR

IDS = lambda cs: [c.name for c in cs]


def test_twin_library_is_built_from_this_tree():
    """ref.fns() rebuilds a library that another commit's build left behind (the sources' hash is compiled in); the replay seams this table needs are exported"""
    f = ref.fns()
    assert ref.is_current()
    assert all(n in f for n in ref.REQUIRED)


def test_philox_matches_the_outside_table():
    fx = RR.philox_fixture()
    rows = fx["rows"]
    assert "at::Philox4_32" in fx["source"] and len(rows) >= 24
    cs = [tuple(r["counter"]) for r in rows]
    assert (0, 0, 0, 0) in cs and (0xFFFFFFFF,) * 4 in cs and any(c[1] > 0 and c[3] in (RR.TAG, RR.TAG + 1, RR.TAG + 2) for c in cs)      # all-zero, all-ones, call counters >= 2^32
    for r in rows:
        np.testing.assert_array_equal(RR.philox4x32_10(r["key"], np.array(r["counter"], np.uint64)), np.array(r["out"], np.uint32), err_msg=str(r))
    by_key = {}
    for r in rows:                                                    # and vectorised over counters, as uniforms() calls it
        by_key.setdefault(tuple(r["key"]), []).append(r)
    for k, rs in by_key.items():
        np.testing.assert_array_equal(RR.philox4x32_10(k, np.array([r["counter"] for r in rs], np.uint64)), np.array([r["out"] for r in rs], np.uint32))
    r = next(r for r in rows if r["counter"][3] == RR.TAG and r["counter"][1] > 0)
    seed, ctr = r["key"][0] | (r["key"][1] << 32), r["counter"][0] | (r["counter"][1] << 32)
    assert RR.uniforms(seed, ctr, [r["counter"][2]])[0] == (r["out"][0] >> 8) * 2.0 ** -24


def test_model_against_the_numpy_oracle():
    """the leaves and the IS weights of the model against oracle/dqn_oracle.py's PrioritizedReplay (an fp32 restatement of …replay.jl, no tree either)"""
    rng = np.random.default_rng(4)
    for alpha, beta, cap in ((0.6, 0.4, 37), (1.0, 1.0, 8), (0.0, 0.0, 5)):
        eps = np.float32(1e-3)
        m = RR.Replay(cap, np.float32(alpha), eps)
        o = O.PrioritizedReplay((2,), cap, 9, alpha=alpha, beta=beta, eps=float(eps))
        for n in (3, cap - 1, 2 * cap + 3):
            td = rng.random(n).astype(np.float32) * 5
            m.add(td)
            for i in range(n):
                o.add_exp(np.zeros(2, np.float32), 0, 0.0, np.zeros(2, np.float32), False, td_err=td[i])
            np.testing.assert_allclose(np.asarray(o.prio[:m.size], np.float64), m.live(), rtol=RR.LEAF_RTOL(alpha))
            idx = rng.integers(0, m.size, 9); tdu = rng.standard_normal(9).astype(np.float32)
            m.update(idx, tdu); o.update_priorities(idx, tdu)
            np.testing.assert_allclose(np.asarray(o.prio[:m.size], np.float64), m.live(), rtol=RR.LEAF_RTOL(alpha))
            np.testing.assert_allclose(O.is_weights(np.asarray(o.prio[:m.size])[idx], np.asarray(o.prio[:m.size]), beta, np.float64),
                                       RR.is_weights(m.live(), idx, beta), rtol=1e-6)


def test_law_can_fail():
    """a draw one leaf off is outside d on a sharp vector; a stale internal node (the law judged on other leaves than the draw was made on) too"""
    leaves = 10.0 ** (3 * np.random.default_rng(1).random(100))
    _, t, d, lo, hi = RR.strata(leaves, 5, 0, 16, 100)
    assert (lo == hi).all()
    RR.judge(leaves, lo, 5, 0, 16, 100)
    with pytest.raises(AssertionError):
        RR.judge(leaves, np.minimum(lo + 1, 99), 5, 0, 16, 100)
    with pytest.raises(AssertionError):
        RR.judge(leaves, lo, 5, 1, 16, 100)                           # another call counter


@pytest.mark.parametrize("c", C.CASES + C.DEEP, ids=IDS(C.CASES + C.DEEP))
def test_case_is_sharp_on_the_model_and_on_its_side_of_the_rules(c):
    """sharpness, and for hp.sample_distinct the omission condition and the promised number of judged redraws, from the reference alone"""
    m = C.model_sharpness(c)
    if c.distinct:
        print(f"\n{c.name}: on the model alone {m}")
    C.check_want(c)


@pytest.mark.parametrize("c", C.CASES, ids=IDS(C.CASES))
def test_case_on_twin(c):
    C.run(ref.Twin, c, threads=2)


@pytest.mark.parametrize("c", C.DEEP, ids=IDS(C.DEEP))
def test_deep_case_on_twin(c):
    C.run(ref.Twin, c, threads=2)


def test_chi_square_non_power_of_two_partly_filled_on_twin():
    C.chi_square(ref.Twin, cap=100, size=83, B=16, draws=2000, threads=1)


def test_chi_square_b512_on_twin():
    C.chi_square(ref.Twin, cap=3000, size=2500, B=512, draws=300, threads=1)


def test_zz_report_worst_margins():
    """not a check: prints the largest margin / tolerance per quantity (the module docstring of the GPU file records them)"""
    print("\nworst margin / tolerance on the twin:", {k: float(f"{v:.3g}") for k, v in sorted(C.WORST.items())})
    print("distinct cases on the twin, (redraws judged, left out, with R < S / 4):", C.REDRAWS)
