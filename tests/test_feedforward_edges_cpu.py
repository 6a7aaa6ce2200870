"""CPU: the feed-forward edge table of tests/feedforward_edges_common.py on the C twin (oracle/dqn_ref.c), against the fp64 reference of
tests/feedforward_reference.py -- kernel-selection boundaries, rectangular convolutions (kh != kw, sh != sw), 32 seeded random configurations and
200 Adam steps.  Also here, because they need no GPU: the two legs of the reference (NumPy oracle, torch autograd) agree to 1e-10 on every case,
and every case of the table stands on the side of the selection rule it was written for.  tests/test_feedforward_edges_gpu.py runs the same
checker on the HIP engine and holds the engine to the twin bit for bit.

Measured (the twin's error is the engine's, by that assertion): largest error as a fraction of its tolerance q_on_s 0.12, q_on_sp 0.13, q_tg_sp 0.23,
y 0.11, td 0.12, loss 0.04, grad_norm 0.03; largest gradient error / block scale 3.24e-6 (a Dense weight) of GRAD_C = 2e-5.  No case needed a
tolerance of its own.  Mutation check, done once by hand: with sh and sw swapped in the twin's forward input index (dqn_ref.c, `xb = oy * sh * iw +
ox * sw`), all eight rectangular cases and 13 of the 32 random seeds fail here while every square case of the table, the golden cases and the
known answers still pass."""
import numpy as np
import pytest

import feedforward_edges_common as C
import feedforward_reference as FR
import dqn_oracle as O
import ref

IDS = lambda cs: [c.name for c in cs]
TWIN = dict(threads=8, plan=ref.default_plan)      # the twin has no planner of its own: the default plan, restated in oracle/ref.py


@pytest.mark.parametrize("c", C.CASES, ids=IDS(C.CASES))
def test_case_stands_on_its_side_of_the_rule(c):
    C.check_want(c)


def test_table_covers_both_sides_of_every_rule():
    f = {c.name: C.case_facts(c) for c in C.CASES}
    seen = lambda key, val: any(any(k.rstrip("0123456789") == key and v == val for k, v in x.items()) for x in f.values())
    for key, vals in {"fwd": ("lds", "mfma", "mfma+valu", "valu"), "dw": ("lds", "mfma", "valu"), "dx": ("lds", "mfma", "valu", "join"), "dxmode": (2, 3, -1),
                      "dxred": (True, False), "dwNT": (1, 2, 4), "join": ("lds", "tmp"), "head": ("head_td", "head_cols4", "red_head", "td_huber"),
                      "tiny": (True, False), "arena": (True, False)}.items():
        for v in vals:
            assert seen(key, v), (key, v)
    assert {c.mfma for c in C.CASES} == {0, 1} and {c.u8 for c in C.CASES} == {0, 1} and {c.graph for c in C.CASES} == {0, 1}
    rect = [g for c in C.RECT for g in C.case_facts(c)["G"] if g.kind == "conv" and (g.kh != g.kw or g.sh != g.sw)]
    assert sum(1 for g in rect if g.dx_kc > 0 and g.kh != g.kw) >= 2          # raw-tap chunks with kw != kh
    assert any(g.oh == 1 for g in rect) and any(g.ow == 1 for g in rect)
    assert any(g.sh > 1 and (g.ih - g.kh) % g.sh for g in rect) and any(g.sw > 1 and (g.iw - g.kw) % g.sw for g in rect)


@pytest.mark.parametrize("c", C.CASES + C.RANDOM, ids=IDS(C.CASES + C.RANDOM))
def test_reference_legs_agree(c):
    """NumPy oracle and torch autograd, both fp64, on the case's first batch: 1e-10 relative on every quantity"""
    net, D, batch = _first_batch(c)
    args = (net, D["p_on"], D["p_tg"], batch, float(np.float32(c.gamma)), c.dq)
    FR.legs_agree(FR.step_numpy(*args), FR.step_torch(*args))


def _first_batch(c):
    net, D = C.prepare(c)
    prio = O.priority_from_td(np.abs(D["r"]), np.float32(1e-3), np.float32(0.6)).astype(np.float64)
    return net, D, C._fp64_batch(c, D, D["idx"][0], prio)


@pytest.mark.parametrize("c", C.CASES + C.RANDOM, ids=IDS(C.CASES + C.RANDOM))
def test_reference_numpy_leg_is_the_oracles_whole_step_bit_for_bit(c):
    """step_numpy is built from the oracle's layer functions, not from its batch_train_step: on a network the oracle can describe the two are the same
    operations in the same order, so every quantity of KEYS is equal bit for bit"""
    net, D, batch = _first_batch(c)
    gamma = float(np.float32(c.gamma))
    a = FR.step_numpy(net, D["p_on"], D["p_tg"], batch, gamma, c.dq)
    o = O.batch_train_step(net, net.unflatten(D["p_on"].astype(np.float64)), net.unflatten(D["p_tg"].astype(np.float64)), batch, gamma=gamma, double_q=bool(c.dq), adam=None)
    want = dict(o, q_on_s=o["q"], grads=O.Network.flatten(o["grads"]))
    assert set(a) == set(FR.KEYS)
    for k in FR.KEYS:
        np.testing.assert_array_equal(a[k], want[k], err_msg=k)


@pytest.mark.parametrize("c", C.CASES + C.RANDOM, ids=IDS(C.CASES + C.RANDOM))
def test_layer_descs_are_the_oracles_field_by_field(c):
    """feedforward_reference.layer_descs = ref.layers_from_network where there is neither pad nor pool"""
    net = C.network(c)
    a, b = FR.layer_descs(net), ref.layers_from_network(net)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert [getattr(x, f) for f, _ in x._fields_] == [getattr(y, f) for f, _ in y._fields_]


@pytest.mark.parametrize("c", C.CASES + C.RANDOM, ids=IDS(C.CASES + C.RANDOM))
def test_init_params_are_the_oracles_bit_for_bit(c):
    net = C.network(c)
    pa, pb = FR.init_params(net, c.seed), O.init_params(net, c.seed)
    assert len(pa) == len(pb)
    for x, y in zip(pa, pb):
        assert x.dtype == y.dtype and x.shape == y.shape
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("c", C.CASES, ids=IDS(C.CASES))
def test_twin_case_vs_fp64_reference(c):
    h, _ = C.run_checked(ref.Twin, c, **TWIN)
    h.close()


@pytest.mark.parametrize("c", C.RANDOM, ids=IDS(C.RANDOM))
def test_twin_random_configuration_vs_fp64_reference(c):
    h, _ = C.run_checked(ref.Twin, c, **TWIN)
    h.close()


@pytest.mark.parametrize("c", C.LONG, ids=IDS(C.LONG))
def test_twin_adam_over_200_steps(c):
    C.long_adam(ref.Twin, c, **TWIN).close()


def test_zz_report_worst_errors():
    """not a check: prints the largest error / tolerance per quantity this run showed (the module docstrings record them)"""
    print("\nworst error / tolerance:", {k: round(v, 4) for k, v in sorted(C.WORST.items())})
    print("worst gradient error / scale per block kind:", {k: float(f"{v:.3g}") for k, v in sorted(FR.WORST.items()) if k.startswith(("conv", "dense"))})
