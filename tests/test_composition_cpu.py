"""CPU: the tables of tests/composition_common.py -- 64 feed-forward and 16 recurrent networks drawn from the module's own grammar over every layer kind -- before anything
is compared with the GPU (tests/test_composition_gpu.py): the draw is deterministic and the seeds are what the search returns; every case lowers through nn.lower and the
library's host-side build_layers accepts it (dqn_plan_default, no GPU); every kind nn can build, every adjacent pair the grammar declares legal, every activation code and
every option the GPU file promises has a case; the margins hold at twice their value along the fp64 trajectory and every parameter block is live; every parameter layer is
VISIBLE (a relative change of 1e-3 in its parameters moves Q or the gradients by more than ten tolerances, so a wrong kernel at that layer would be seen); the fp64 step
is well conditioned (one fp32 ulp moves it by less than a quarter of a tolerance); the NumPy legs agree with the default leg; and two wrong engines -- the skip join without
+ x, a fused activation taken from the neighbouring layer -- land more than a hundred tolerances off on every case that holds the construct."""
import numpy as np
import pytest

import __graft_entry__ as ge
import activation_layer_reference as AL
import composition_common as C
import dropout_reference as DR
import groupnorm_reference as GR
import layernorm_reference as LN
import step_reference as S
from test_step_reference_cpu import _buildable_kinds

nn = C.nn
ALL = C.FF + C.REC
IDS = lambda cs: [c.name for c in cs]


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


# ------------------------------------------------------------------ determinism and seeds
def test_the_draw_is_deterministic():
    for s in range(C.N_FF):
        a, b = C.draw(s), C.draw(s)
        assert (a.specs, a.tokens, a.B, a.obs, a.nA, a.dueling, a.dq, a.prio, a.u8, a.T, a.gamma, a.pscale) == (b.specs, b.tokens, b.B, b.obs, b.nA, b.dueling, b.dq, b.prio, b.u8, b.T, b.gamma, b.pscale)
        assert a.specs == C.FF[s].specs and a.name == C.FF[s].name
    for s in range(C.N_REC):
        a, b = C.draw_rec(s), C.draw_rec(s)
        assert (a.specs, a.tokens, a.B, a.obs, a.T, a.dueling, a.dq) == (b.specs, b.tokens, b.B, b.obs, b.T, b.dueling, b.dq) and a.specs == C.REC[s].specs
    for c in (C.FF[0], C.FF[3], C.REC[0]):
        D1, D2 = C.data(c), C.data(c)
        np.testing.assert_array_equal(D1.p_on, D2.p_on); np.testing.assert_array_equal(D1.p_tg, D2.p_tg)
        if c.T:
            assert all(np.array_equal(x, y) for e1, e2 in zip(D1.eps, D2.eps) for t1, t2 in zip(e1, e2) for x, y in zip(t1, t2))
        else:
            np.testing.assert_array_equal(D1.s, D2.s); np.testing.assert_array_equal(D1.idx[1], D2.idx[1])
    assert len(C.FF) == 64 and len(C.REC) == 16 and len(C.BY_NAME) == 80


def test_the_seeds_are_the_smallest_that_pass_the_screens():
    """find_seed, re-run: the smallest data seed that keeps twice every margin on every step, leaves no dead block, passes the one-ulp screen and shows every layer.
    No seed lies above SEED_CAP = 8 -- by construction, not by luck: the network screen (ALTS, next test) redraws a network that has none, so the bound "at most 4 of the
    80 cases need a seed above 8" cannot fail here and is not asserted; what the screen costs is stated by ALTS itself (how many networks gave way, and how often)"""
    for c in ALL:
        assert C.find_seed(c) == c.seed <= C.SEED_CAP, c.name
    assert set(C.SEEDS) <= set(C.BY_NAME) and all(v != 1 for v in C.SEEDS.values())


def test_the_alternatives_are_the_first_that_pass_the_network_screen():
    """ALTS, re-run: every alternative in front of a case's own either does not fit its shapes or has no data seed up to SEED_CAP that passes the screens"""
    assert set(C.ALTS) <= set(C.BY_NAME) and all(C.BY_NAME[n].alt == a > 0 for n, a in C.ALTS.items())
    for c in ALL:
        one = C.draw_rec_at if c.T else C.draw_at
        for alt in range(c.alt):
            other = one(int(c.name[-2:]), alt)
            if other is not None:
                with pytest.raises(AssertionError, match="no seed below"):
                    C.find_seed(other)


# ------------------------------------------------------------------ lowering and host validation
def _n_params(d, abi):
    """the parameter count of one descriptor, from the descriptor alone"""
    if d.kind == abi.LAYER_DENSE:
        return d.n_in * d.n_out + d.n_out
    if d.kind == abi.LAYER_CONV:
        return d.cout * d.cin * d.kh * d.kw + d.cout
    if d.kind == abi.LAYER_CONV_DG:
        return d.cout * (d.cin // (d.n_out >> 16)) * d.kh * d.kw + d.cout
    if d.kind == abi.LAYER_LAYERNORM:
        return 2 * d.n_out
    if d.kind == abi.LAYER_GROUPNORM:
        return 2 * d.cout
    if d.kind in (abi.LAYER_LSTM, abi.LAYER_GRU, abi.LAYER_RNN):
        g = {abi.LAYER_LSTM: 4, abi.LAYER_GRU: 3, abi.LAYER_RNN: 1}[d.kind]; h = d.n_out
        return g * h * (d.n_in + h + 1) + h * (2 if d.kind == abi.LAYER_LSTM else 1)
    return 0


@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_every_case_lowers_and_the_host_side_validation_accepts_it(pkg, c):
    """the grammar is a restatement: nn.lower and build_layers (through dqn_plan_default) must admit what it admits"""
    abi = nn._abi; net = c.mk()
    layers, dueling = nn.lower(net)
    assert dueling == c.dueling and len(layers) == C.n_descs(c.specs, c.dueling) <= C.MAX_DESCS
    o = tuple(c.obs) + (1,) * (3 - len(c.obs))
    hp = pkg.default_hparams(batch_size=c.B, n_actions=c.nA, obs_c=o[0], obs_h=o[1], obs_w=o[2], dueling=int(dueling), buffer_size=c.B + 24, recurrence=int(bool(c.T)), trace_length=max(c.T, 1),
                             prioritized_replay=c.prio, obs_dtype=c.u8, double_q=c.dq)
    plan = pkg.default_plan(layers, hp)
    assert len(plan) == len(layers)
    blks = S.blocks(net); P = nn.glorot_params(net).size
    assert blks[0][1].start == 0 and blks[-1][1].stop == P and all(a[1].stop == b[1].start for a, b in zip(blks, blks[1:]))
    assert sum(_n_params(d, abi) for d in layers) == P


# ------------------------------------------------------------------ coverage
def _layers(c):
    return nn.all_layers(c.mk())


def test_every_kind_and_every_declared_pair_has_a_case():
    kinds = set()
    for c in ALL:
        kinds |= S.kinds(c.mk()) - {"act"}
    assert kinds == _buildable_kinds(), _buildable_kinds() ^ kinds
    seen = set().union(*(C.pairs_of(c.tokens) for c in C.FF))
    assert len(C.PAIRS) == 93 and not set(C.PAIRS) - seen, sorted(set(C.PAIRS) - seen)
    for c in C.FF:      # ... and no case holds a pair the grammar does not declare
        assert C.pairs_of(c.tokens) <= set(C.PAIRS), (c.name, C.pairs_of(c.tokens) - set(C.PAIRS))
    cell = lambda t: "cell" if t in C.CELLS else t
    rec_seen = set().union(*(C.pairs_of([cell(t) for t in c.tokens]) for c in C.REC))
    assert not set(C.REC_PAIRS) - rec_seen, sorted(set(C.REC_PAIRS) - rec_seen)
    firsts = {next(t for t in c.tokens if t in C.CELLS) for c in C.REC}
    seconds = {[t for t in c.tokens if t in C.CELLS][1] for c in C.REC if sum(t in C.CELLS for t in c.tokens) == 2}
    assert firsts == set(C.CELLS) and seconds == set(C.CELLS)
    assert {c.T for c in C.REC} == {2, 3} and {c.B for c in C.REC} == {2, 4} and {c.dueling for c in C.REC} == {False, True}


def test_every_kind_stands_in_a_dueling_base():
    base = set()
    for c in ALL:
        if c.dueling:
            base |= C.base_kinds(c.mk())
    assert base == _buildable_kinds(), _buildable_kinds() ^ base


def test_the_options_and_shapes_the_gpu_file_promises():
    for image in (True, False):
        cs = [c for c in C.FF if c.image == image]
        assert any(c.B == 5 for c in cs) and any(c.u8 for c in cs) and any(not c.prio for c in cs) and any(not c.dq for c in cs), image
        assert any(c.prio for c in cs) and any(c.dq for c in cs) and any(c.dueling for c in cs) and any(not c.dueling for c in cs)
    assert {c.B for c in C.FF} == {5, 16, 32} and len([c for c in C.FF if c.image]) == 48
    assert 8 <= sum(c.u8 for c in C.FF if c.image) <= 16 and 24 <= sum(c.dueling for c in C.FF) <= 40
    ls = [l for c in ALL for l in _layers(c)]
    convs = [l for l in ls if l.kind == "conv"]
    assert any(l.ph or l.pw for l in convs) and any(not (l.ph or l.pw) for l in convs) and any(l.dh == 2 for l in convs) and any(l.sh == 2 for l in convs)
    assert any(l.groups == 2 for l in convs) and any(l.groups == l.cin > 1 for l in convs) and {(l.kh, l.kw) for l in convs} == {(1, 1), (2, 2), (3, 3), (3, 2)}
    assert any(c.B == 32 and l.kind == "conv" and l.cout in (16, 32) for c in C.FF for l in _layers(c)[:1])      # the MFMA-sized draw
    assert any(l.kind == "dense" and l.n_out == C.SPLIT_WIDTH for l in ls)      # a split-sum width
    assert {(l.kh, l.kw) for l in ls if l.kind in ("maxpool", "meanpool")} == {(2, 2), (2, 1)}
    assert {(l.oh, l.ow) for l in ls if l.kind in ("adaptivemaxpool", "adaptivemeanpool")} == {(2, 2), (1, 2), (1, 1)}
    assert {l.p for l in ls if l.kind == "dropout"} == {0.25, 0.5} and min(l.n for l in ls if l.kind == "layernorm") >= 7
    chains = [(c.mk().base if c.dueling else c.mk()).layers for c in ALL]
    relu_pool = [(a.kind, b.kind) for ch in chains for a, b in zip(ch, ch[1:]) if b.kind in ("maxpool", "adaptivemaxpool") and (a.code if a.kind == "activation" else a.act) == nn.relu]
    assert {("conv", "maxpool"), ("conv", "adaptivemaxpool"), ("groupnorm", "adaptivemaxpool"), ("activation", "adaptivemaxpool")} <= set(relu_pool), relu_pool      # relu directly in front of a max-type pool (the margin exempts its exact zeros)
    assert {l.act for l in ls if l.kind in S.FUSED} == set(range(11)), "every fused activation code"
    assert {l.code for l in ls if l.kind == "activation"} == set(range(15)), "every standalone activation code"
    on_map = lambda c: {type(l).__name__ for l in c.mk().layers} if not c.dueling else {type(l).__name__ for l in c.mk().base.layers}
    assert any("SkipConnection" in on_map(c) for c in C.FF if "skip:map" in c.tokens) and any("skip:vec" in c.tokens for c in C.FF)


# ------------------------------------------------------------------ margins, live blocks, visibility, conditioning, legs
@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_margins_at_twice_their_value_and_every_block_live(c):
    D = C.prepare(c)
    for k, p, batch, o in C.trajectory(c, D):
        m = C.margins(c, D.net, p, D.p_tg, batch, k)
        assert C.holds(m, 2.0), (c.name, k, m)
        if k == 0:
            C.check_grads(D.net, o["grads"], o["grads"], live=True)


def test_the_scale_invariant_layers_are_decided_from_the_structure():
    """composition_common.scale_invariant: the layer's own activation is homogeneous and nothing but Dropout, pools and homogeneous Activation layers stand between it and a
    LayerNorm / GroupNorm of the same chain.  Nothing else is excused: not a squashing layer in front of a normalisation, not the last inner layer of a block, not a head"""
    D, LNm, A = nn.Dense, nn.LayerNorm, nn.Activation
    net = nn.Chain(D(6, 8), LNm(8, nn.relu), nn.Dropout(0.5), LNm(8), D(8, 8, nn.tanh), LNm(8), D(8, 8, nn.leakyrelu), A(nn.relu), LNm(8), D(8, 8), A(nn.tanh), LNm(8),
                   nn.SkipConnection(nn.Chain(D(8, 8), LNm(8), D(8, 8)), "+"), LNm(8), D(8, 4))
    kinds = [l.kind for l in nn.all_layers(net)]
    assert kinds == ["dense", "layernorm", "dropout", "layernorm", "dense", "layernorm", "dense", "activation", "layernorm", "dense", "activation", "layernorm", "dense", "layernorm", "dense", "layernorm", "dense"]
    assert C.scale_invariant(net) == {0, 1, 6, 12}      # Dense -> LN; LN(relu) -> Dropout -> LN; Dense(leakyrelu) -> Activation(relu) -> LN; the block's first Dense -> LN
    cm = nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.MaxPool(2), nn.GroupNorm(4, 2), nn.MeanPool(1), nn.GroupNorm(4, 1, nn.elu), nn.Conv(1, 4, 4), nn.flattenbatch, D(36, 4))
    assert C.scale_invariant(cm) == {0, 2}
    duel = nn.create_dueling_network(nn.Chain(D(6, 8), LNm(8), D(8, 8), D(8, 4)))
    assert C.scale_invariant(duel) == {0}      # no layer of a value / advantage stream
    for c in ALL:      # ... and in the tables every excused layer is a Dense, Conv, LayerNorm or GroupNorm with a homogeneous activation, followed in its chain by a normalisation
        net = c.mk(); ls = nn.all_layers(net)
        for i in C.scale_invariant(net):
            assert ls[i].kind in S.FUSED and ls[i].act in C.HOMOGENEOUS and any(l.kind in ("layernorm", "groupnorm") for l in ls[i + 1:]), (c.name, i)


@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_every_parameter_layer_is_visible(c):
    """scaling one layer's parameters by (1 + 1e-3) moves q_on_s (a recurrent step: td) or the gradients by more than 10 tolerances: no layer could be wrong unseen.
    The one exception is the law's and not the data's: a layer of composition_common.scale_invariant(net) -- and no other -- moves by 1e-3 / (GRAD_RTOL + GRAD_C) = 8.33
    tolerances at the very most under a pure rescaling, and is asked the same bound under the same factor on the first half of each of its arrays"""
    D = C.prepare(c); _, p, batch, o = next(C.trajectory(c, D))
    seen = C.visibility(c, D, p, batch, o)
    assert set(seen) == {i for i, l in enumerate(nn.all_layers(D.net)) if l.shapes()}      # every parameter layer was asked
    assert C.VISIBLE == 10.0 and C.VIS_STEP == 1e-3 and min(seen.values()) > C.VISIBLE, (c.name, {i: (nn.all_layers(D.net)[i].kind, round(v, 2)) for i, v in seen.items() if v <= C.VISIBLE})
    for i in set(seen) - C.scale_invariant(D.net):      # every other layer: the issue's bound under the UNIFORM scaling, stated here without the helper
        p2 = p.copy(); p2[C.layer_slices(D.net)[i]] *= 1.0 + 1e-3
        d = S.distance(C.step(c, D.net, p2, D.p_tg, batch), o, D.net)
        assert max(d["td"] if c.T else d["q_on_s"], d["grads"]) > 10.0, (c.name, i, d)


@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_one_ulp_moves_the_fp64_step_by_less_than_a_quarter_tolerance(c):
    assert C.conditioning(c, C.prepare(c)) < C.COND_BOUND


@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_the_numpy_legs_agree_with_the_default_leg(c):
    D = C.prepare(c); have = S.kinds(D.net)
    leg = {k: v for legs in (LN.LEGS["numpy"], GR.LEGS["numpy"], AL.LEGS["numpy"], DR.LEGS["numpy"]) for k, v in legs.items() if k in have}
    for k, p, batch, o in C.trajectory(c, D):
        if leg:
            S.legs_agree(o, C.step(c, D.net, p, D.p_tg, batch, k, leg))


# ------------------------------------------------------------------ the tests can tell
def _neighbour_act(net):
    """a law for "act" under which every fused layer takes the activation of the fused layer behind it (the last one: the first one's); None where all are the same"""
    fused = [l for l in nn.all_layers(net) if l.kind in S.FUSED]
    if len({l.act for l in fused}) < 2:
        return None
    other = {id(a): b for a, b in zip(fused, fused[1:] + fused[:1])}; real = S.default_laws()["act"]
    return lambda l, x, _a, cx: real(other[id(l)], x, _a, cx)


@pytest.mark.parametrize("c", ALL, ids=IDS(ALL))
def test_two_wrong_engines_are_a_hundred_tolerances_off(c):
    D = C.prepare(c); _, p, batch, o = next(C.trajectory(c, D))
    if "skip" in S.kinds(D.net):
        d = S.distance(C.step(c, D.net, p, D.p_tg, batch, leg={"skip": lambda l, x, a, cx: a}), o, D.net)
        assert max(d.values()) > 100.0, (c.name, "the join without + x", d)
    law = _neighbour_act(D.net)
    if law is not None:
        d = S.distance(C.step(c, D.net, p, D.p_tg, batch, leg={"act": law}), o, D.net)
        assert max(d.values()) > 100.0, (c.name, "a fused activation taken from the neighbour", d)
