"""fp64 reference of ONE batch_train! for networks with Flux SkipConnection(layers, +) blocks (TEST INFRASTRUCTURE), feed-forward (src/solver.jl:191-236) and recurrent
(src/solver.jl:239-287), over the package's nn descriptors: what dropout_reference.py covers (Dense, LSTM / GRU, LayerNorm, Dropout, plain or dueling) plus the block.

The block (Flux 0.14; recalled, not executed): SkipConnection(layers, +)(x) = layers(x) .+ x, no parameters, no activation.  In the engine's words (DESIGN.md section 4
"Skip connections"): y_join = y_K + y_P with K the last inner layer and P the producer the first inner layer F reads; backwards dact[K] = dY .* act_K'(y_K) at the join and
dact[P] = (dF + dY) .* act_P'(y_P) at the entry -- P's derivative once, after the sum.

Two legs:
  * "law"    torch float64 autograd through `layers(x) + x` written out;
  * "numpy"  feed-forward steps: a NumPy forward and a HAND-WRITTEN backward of the whole step in the engine's order (np_step: one dact per layer, the join and entry
             rules above, ln_backward_np / do_backward_np for the two layer kinds that have one); recurrent steps: the torch graph with the join entered as a NumPy
             torch.autograd.Function whose backward hands dY to both operands (JOIN_NUMPY, the one override of the leg).
The step and the walker are step_reference's.
np_step also runs the WRONG engines test_skip_cpu.test_the_tests_can_tell shows apart (WRONG); its LayerNorm and Dropout are layernorm_reference's / dropout_reference's
NumPy forward and backward, by import.

A Dropout layer's mask is keyed by the layer's ENGINE index (its descriptor's position: every join in front of it counts), while the reference's arrays are indexed in
Flux.params order (nn.all_layers: inner layers in place, no join); engine_index maps one to the other.

Data rule: the margins of layernorm_reference (SIGMA_MIN, RELU_MARGIN, GAP) on the masked s pass and the unmasked s' passes, no dead gradient block, and every wrong
engine at least 2 * TELL tolerances away.  Seeds are fixed in the table and were found with this module alone (find_seed, dropout_reference's cap)."""
import types

import numpy as np
import torch

import dropout_reference as DR
import layernorm_reference as LR
import step_reference as STEP
from gru_reference import param_arrays
from step_reference import blocks, check_grads, ff_batch, ff_data, grad_distance, legs_agree, rec_data      # noqa: F401

nn = LR.nn
F64 = torch.float64
ENGINE_SEED = DR.ENGINE_SEED
# the wrong engines: (name, changes the forward)
WRONG = (("entry_without_dY", False), ("p_derivative_before_the_sum", False), ("p_derivative_twice", False), ("k_derivative_omitted", False),
         ("k_preactivation_added", True), ("skip_read_from_f", True))


# ------------------------------------------------------------------ structure
def program(net):
    """the engine's descriptor list as data: [(kind 'layer' | 'join', layer, flat index (Flux.params order) or None, src, stream, P or None)], src / P = program
    indices (-1: the observation); the join's src is the block's last inner layer K, P the block's entry"""
    prog = []

    def walk(chain, fi, src, stream):
        for l in chain:
            if l.kind == "skip":
                entry = src
                fi, src = walk(l.layers, fi, src, stream)
                prog.append(types.SimpleNamespace(kind="join", l=l, fi=None, src=src, stream=stream, P=entry)); src = len(prog) - 1
            else:
                prog.append(types.SimpleNamespace(kind="layer", l=l, fi=fi, src=src, stream=stream, P=None)); src = len(prog) - 1; fi += 1
        return fi, src
    if isinstance(net, nn.DuelingNetwork):
        fi, sb = walk(net.base, 0, -1, 0)
        fi, _ = walk(net.val, fi, sb, 1)
        walk(net.adv, fi, sb, 2)
    else:
        walk(net, 0, -1, 0)
    return prog


def engine_index(net):
    """{flat index: engine layer index}"""
    return {e.fi: i for i, e in enumerate(program(net)) if e.kind == "layer"}


def masks_for(net, k, B, T=0, seed=ENGINE_SEED):
    """dropout_reference.masks_for, keyed by the FLAT index and drawn under the layer's ENGINE index.  An Activation layer keeps the width of the layer in front; a layer
    on a map (Conv, pools, GroupNorm) has none, and no Dropout layer stands behind one"""
    prog, out, width = program(net), {}, {}
    for i, e in enumerate(prog):
        w = width.get(e.src)
        if e.kind == "layer" and e.l.kind == "dropout":
            m = DR.keep_mask(seed, k, i, w, (T or 1) * B, e.l.p)
            out[e.fi] = m.reshape(T, B, w) if T else m
        elif e.kind == "layer" and e.l.kind != "activation":
            w = e.l.n if e.l.kind == "layernorm" else getattr(e.l, "n_out", None)
        width[i] = w
    return out


# ------------------------------------------------------------------ the join in NumPy (the recurrent "numpy" leg), and the step
class _JoinNumpy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, x):
        return torch.tensor(a.detach().numpy() + x.detach().numpy(), dtype=F64)

    @staticmethod
    def backward(ctx, dy):
        g = dy.numpy()
        return torch.tensor(g.copy()), torch.tensor(g.copy())      # the join hands dY to the inner chain AND to the entry


JOIN_NUMPY = {"skip": lambda l, x, a, cx: _JoinNumpy.apply(a, x)}      # the override of step_reference's `layers(x) + x`; a: the inner chain's output


# ------------------------------------------------------------------ the "numpy" leg: the engine's order, by hand (feed-forward)
def act_np(pre, act):
    if act == nn.relu:
        return np.maximum(pre, 0.0)
    if act == nn.tanh:
        return np.tanh(pre)
    if act == nn.sigmoid:
        return 1.0 / (1.0 + np.exp(-pre))
    if act == nn.elu:
        return np.where(pre >= 0, pre, np.expm1(np.minimum(pre, 0.0)))
    assert act == nn.identity, act
    return pre


def dact_np(d, y, act):
    """d .* act'(.) from the STORED output y, as the engine takes every derivative"""
    if act == nn.relu:
        return np.where(y > 0, d, 0.0)
    if act == nn.tanh:
        return d * (1.0 - y * y)
    if act == nn.sigmoid:
        return d * (y * (1.0 - y))
    if act == nn.elu:
        return np.where(y >= 0, d, d * (y + 1.0))
    assert act == nn.identity, act
    return d


def np_forward(prog, arrs, x, masks, wrong=None):
    """stored outputs y[i], pre-activations and caches of every program entry"""
    ys, pres, cache = [], [], []
    for i, e in enumerate(prog):
        xin = x.reshape(x.shape[0], -1) if e.src < 0 else ys[e.src]
        pre, c = None, None
        if e.kind == "join":
            a = pres[e.src] if wrong == "k_preactivation_added" and pres[e.src] is not None else ys[e.src]
            xs = ys[_first_inner(prog, i)] if wrong == "skip_read_from_f" else ys[e.P]
            y = a + xs
        elif e.l.kind == "dense":
            pre = xin @ arrs[e.fi][0] + arrs[e.fi][1]; y = act_np(pre, e.l.act)
        elif e.l.kind == "layernorm":
            pre, c = LR.ln_forward_np(xin, arrs[e.fi][0], arrs[e.fi][1], float(np.float32(e.l.eps))); y = act_np(pre, e.l.act)
        else:
            assert e.l.kind == "dropout", e.l.kind
            y = DR.do_forward_np(xin, masks[e.fi], DR.do_scale(e.l.p)) if masks is not None else xin
        ys.append(y); pres.append(pre); cache.append(c)
    return ys, pres, cache


def _first_inner(prog, j):
    """program index of the first inner layer F of the block that joins at j: the entry that reads P and lies inside the block"""
    k = prog[j].src      # K; walk back along src until the entry P
    while prog[k].src != prog[j].P:
        k = prog[k].src
    return k


def np_q(net, prog, ys):
    if isinstance(net, nn.DuelingNetwork):
        lv = max(i for i, e in enumerate(prog) if e.stream == 1); la = max(i for i, e in enumerate(prog) if e.stream == 2)
        return ys[lv] + ys[la] - ys[la].mean(axis=1, keepdims=True), (lv, la)
    return ys[-1], (None, len(prog) - 1)


def np_step(net, p_on, p_tg, batch, gamma, double_q, masks, wrong=None):
    """one feed-forward batch_train! in NumPy with the backward written out layer by layer: D[i] = dL / d(pre-activation of entry i), the engine's dact"""
    s, a, r, sp, done, w = (np.asarray(x, np.float64) if k != 1 else np.asarray(x, np.int64) for k, x in enumerate(batch))
    B = s.shape[0]; prog = program(net)
    aon = [[t.numpy() for t in la] for la in param_arrays(net, nn, np.asarray(p_on, np.float64))]
    atg = [[t.numpy() for t in la] for la in param_arrays(net, nn, np.asarray(p_tg, np.float64))]
    q_tg_sp = np_q(net, prog, np_forward(prog, atg, sp, None, wrong)[0])[0]
    q_on_sp = np_q(net, prog, np_forward(prog, aon, sp, None, wrong)[0])[0] if double_q else q_tg_sp
    best = q_on_sp.argmax(axis=1)      # NumPy's argmax is Julia's: the smallest index among the maxima
    y = r + (1.0 - done) * float(gamma) * q_tg_sp[np.arange(B), best]
    ys, pres, cache = np_forward(prog, aon, s, masks, wrong)
    q, (lv, la) = np_q(net, prog, ys)
    td = q[np.arange(B), a] - y
    x = w * td; ab = np.abs(x); qd = np.minimum(ab, 1.0)
    loss = float((0.5 * qd * qd + (ab - qd)).sum() / B)
    dq = np.zeros_like(q); dq[np.arange(B), a] = w * np.clip(x, -1.0, 1.0) / B
    D = [None] * len(prog); g = [None] * len(aon)
    if lv is None:
        D[la] = dact_np(dq, ys[la], prog[la].l.act)
    else:      # Q = V + A - mean(A)
        D[lv] = dact_np(dq.sum(axis=1, keepdims=True), ys[lv], prog[lv].l.act)
        D[la] = dact_np(dq - dq.mean(axis=1, keepdims=True), ys[la], prog[la].l.act)
    first_of = {_first_inner(prog, j): j for j, e in enumerate(prog) if e.kind == "join"}
    for i in range(len(prog) - 1, -1, -1):
        e = prog[i]; xin = s.reshape(B, -1) if e.src < 0 else ys[e.src]
        if e.kind == "join":      # at the join: dact[K] = dY .* act_K'(y_K)
            K = prog[e.src]
            D[e.src] = D[i] if wrong == "k_derivative_omitted" else dact_np(D[i], ys[e.src], K.l.act if K.kind == "layer" else nn.identity)
            continue
        if e.l.kind == "dense":
            g[e.fi] = [xin.T @ D[i], D[i].sum(axis=0)]; dx = D[i] @ aon[e.fi][0].T
        elif e.l.kind == "layernorm":
            dx, ds, db = LR.ln_backward_np(cache[i], D[i]); g[e.fi] = [ds, db]
        else:
            g[e.fi] = []; dx = DR.do_backward_np(masks[e.fi], DR.do_scale(e.l.p), D[i]) if masks is not None else D[i]
        if e.src < 0:
            continue
        src = prog[e.src]; act_s = src.l.act if src.kind == "layer" else nn.identity
        if i in first_of:      # at the entry: dact[P] = (dF + dY) .* act_P'(y_P), the derivative once, after the sum
            dY = D[first_of[i]]
            if wrong == "entry_without_dY":
                D[e.src] = dact_np(dx, ys[e.src], act_s)
            elif wrong == "p_derivative_before_the_sum":
                D[e.src] = dact_np(dx, ys[e.src], act_s) + dY
            elif wrong == "p_derivative_twice":
                D[e.src] = dact_np(dact_np(dx + dY, ys[e.src], act_s), ys[e.src], act_s)
            else:
                D[e.src] = dact_np(dx + dY, ys[e.src], act_s)
        else:      # one consumer -- or the dueling split, where the two streams' gradients meet
            d = dact_np(dx, ys[e.src], act_s); D[e.src] = d if D[e.src] is None else D[e.src] + d
    gv = np.concatenate([x.reshape(-1) for la_ in g for x in la_])
    return dict(q_on_s=q, q_on_sp=q_on_sp, q_tg_sp=q_tg_sp, best_a=best, y=y, td=td, loss=loss, grads=gv, grad_norm=float(np.abs(gv).max()))


# the legs: "law" is step_reference's walker as it stands; "numpy" is np_step for a feed-forward step and the NumPy join for a recurrent one
q_values = STEP.bound(STEP.q_values, {"law": {}, "numpy": JOIN_NUMPY}, "masks")
ff_step = STEP.bound(STEP.ff_step, {"law": {}, "numpy": np_step}, "masks")
rec_step = STEP.bound(STEP.rec_step, {"law": {}, "numpy": JOIN_NUMPY}, "masks")
distance = lambda net, a, b: STEP.distance(a, b, net)


# ------------------------------------------------------------------ the case table
case = LR.case


def S(*inner):
    return nn.SkipConnection(nn.Chain(*inner), "+")


def _net(n, *blocks_, p_act=nn.relu, nA=4, E=6):
    return lambda: nn.Chain(nn.Dense(E, n, p_act), *[b() for b in blocks_], nn.Dense(n, nA))


one_dense = lambda n: lambda: S(nn.Dense(n, n))
two_dense = lambda n, h=None: lambda: S(nn.Dense(n, h or 2 * n, nn.relu), nn.Dense(h or 2 * n, n))
ends_tanh = lambda n: lambda: S(nn.Dense(n, n, nn.tanh))
pre_norm = lambda n: lambda: S(nn.LayerNorm(n), nn.Dense(n, 2 * n, nn.relu), nn.Dense(2 * n, n))
do_first = lambda n, p=0.5: lambda: S(nn.Dropout(p), nn.Dense(n, n, nn.relu), nn.Dense(n, n))
do_last = lambda n, p=0.5: lambda: S(nn.Dense(n, n, nn.relu), nn.Dense(n, n), nn.Dropout(p))

# B = 4 / 32: the 16-byte form; B = 5: ten [s ; s'] columns, unaligned rows, the scalar form; B = 6: a column count that is no multiple of 4 (scalar form, aligned rows);
# B = 128: dx_mode 2 on F.  n = 5 / 33: features that are no multiple of anything; n = 64 at B = 32: more than one workgroup per launch
CASES = [
    case("one_dense_n5_b4", _net(5, one_dense(5)), 4, seed=1),                                   # F == K, the join's backward an alias
    case("one_dense_n8_b5", _net(8, one_dense(8), p_act=nn.tanh), 5, seed=1),                    # P with tanh
    case("two_dense_n33_b6", _net(33, two_dense(33, 16)), 6, seed=1),                            # Dense(relu) -> Dense; P with relu
    case("two_dense_n64_b32", _net(64, two_dense(64)), 32, seed=1),
    case("two_dense_n64_b32_valu", _net(64, two_dense(64)), 32, mfma=0, seed=1),
    case("two_dense_n64_b128", _net(64, two_dense(64)), 128, seed=6),                            # dx_mode 2 on F
    case("ends_tanh_n33_b5", _net(33, ends_tanh(33)), 5, seed=1),                                # the join's launch is no alias
    case("ends_tanh_n8_b32", _net(8, ends_tanh(8), p_act=nn.elu), 32, seed=1),                   # ... and P with an out-of-line activation
    case("pre_norm_n33_b32", _net(33, pre_norm(33)), 32, seed=1),                                # LayerNorm -> Dense(relu) -> Dense: LayerNorm is F
    case("pre_norm_n8_b6", _net(8, pre_norm(8), p_act=nn.elu), 6, seed=1),
    case("do_first_n33_b4", _net(33, do_first(33)), 4, seed=1),                                  # Dropout is F: its backward leaves the raw dF
    case("do_last_n8_b5", _net(8, do_last(8)), 5, seed=1),                                       # Dropout is K: a = its masked output on s, its producer's elsewhere
    case("two_blocks_n33_b32", _net(33, two_dense(33, 16), pre_norm(33)), 32, seed=1),           # P is a join
    case("two_blocks_n5_b6", _net(5, one_dense(5), ends_tanh(5), p_act=nn.tanh), 6, seed=1),
    case("p_layernorm_n33_b5", lambda: nn.Chain(nn.Dense(6, 33, nn.relu), nn.LayerNorm(33, nn.tanh), two_dense(33, 16)(), nn.Dense(33, 4)), 5, seed=1),      # P a LayerNorm
    case("p_dropout_n64_b32", lambda: nn.Chain(nn.Dense(6, 64, nn.relu), nn.Dropout(0.5), two_dense(64, 32)(), nn.Dense(64, 4)), 32, seed=1),                # P a Dropout
    case("dueling_prio", lambda: nn.create_dueling_network(nn.Chain(nn.Dense(6, 32, nn.relu), pre_norm(32)(), nn.Dense(32, 4))), 32, dueling=True, prio=1, seed=1),      # the block directly in front of the split
    case("single_q_n8_b4", _net(8, two_dense(8)), 4, dq=0, seed=1),                              # four columns in the forward
]
REC_CASES = [
    case("lstm_block", lambda: nn.Chain(nn.LSTM(6, 8), two_dense(8)(), nn.Dense(8, 3)), 4, nA=3, T=3, seed=1, pscale=3.0),                      # P recurrent: dact[P] is the cell's dH
    case("dense_block_gru", lambda: nn.Chain(nn.Dense(6, 8, nn.relu), ends_tanh(8)(), nn.GRU(8, 8), nn.Dense(8, 3)), 4, nA=3, T=3, seed=1, pscale=3.0),
]
BY_NAME = {c.name: c for c in CASES + REC_CASES}
assert len(BY_NAME) == len(CASES) + len(REC_CASES)
def first_step(c, seed=None):
    """(network data, fp64 batch, masks) of the case's first step"""
    D, batch = STEP.first_step(c, seed)
    return D, batch, masks_for(D.net, 0, c.B, c.T)


def step(c, D, batch, masks, p_on=None, leg="law"):
    return (rec_step if c.T else ff_step)(D.net, D.p_on if p_on is None else p_on, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq), masks, leg=leg)


def case_margins(c, seed=None):
    """(sigma_min, relu margin, argmax gap) of the first step in fp64, as dropout_reference.case_margins takes them"""
    D, batch, masks = first_step(c, seed); probe = DR.new_probe()
    q_values(D.net, D.p_on, batch[0], masks, probe=probe)
    qon = q_values(D.net, D.p_on, batch[3], probe=probe); qtg = q_values(D.net, D.p_tg, batch[3], probe=probe)
    qsel = qon if c.dq else qtg
    return probe["sigma"], probe["relu"], LR._gap(np.concatenate(qsel) if c.T else qsel)


def margins_ok(c, seed=None, k=2.0):
    sg, rm, gap = case_margins(c, seed)
    if not (sg >= k * LR.SIGMA_MIN and rm > k * LR.RELU_MARGIN and gap > k * LR.GAP):
        return False
    D, batch, masks = first_step(c, seed)
    return not STEP.dead_blocks(D.net, step(c, D, batch, masks)["grads"])


TELL = 100.0      # a wrong engine must move a compared quantity by this many of its tolerances


def applies(c, wrong):
    """which wrong engines a case can show: the feed-forward ones (np_step); P's derivative before the sum needs a P with an activation, twice one whose derivative is not
    0 / 1; K's derivative omitted / K's pre-activation added need a K with an activation; the skip read from F's output needs that output to have the block's width"""
    if c.T:
        return False
    prog = program(c.mk())
    joins = [e for e in prog if e.kind == "join"]
    act_of = lambda i: prog[i].l.act if prog[i].kind == "layer" else nn.identity
    if wrong == "p_derivative_before_the_sum":
        return any(act_of(e.P) != nn.identity for e in joins)
    if wrong == "p_derivative_twice":      # relu' is 0 or 1: applied twice it is itself
        return any(act_of(e.P) not in (nn.identity, nn.relu) for e in joins)
    if wrong in ("k_derivative_omitted", "k_preactivation_added"):
        return any(act_of(e.src) != nn.identity for e in joins)
    if wrong == "skip_read_from_f":      # F's output must have the block's width to be added at all
        width = lambda i: (prog[i].l.n if prog[i].l.kind == "layernorm" else prog[i].l.n_out) if prog[i].kind == "layer" and prog[i].l.kind != "dropout" else width(prog[i].src)
        return all(width(_first_inner(prog, j)) == width(e.P) for j, e in enumerate(prog) if e.kind == "join")
    return True


def tell_distances(c, seed=None):
    """{wrong engine: the largest distance over the compared quantities, in tolerances} on the case's first step, for the wrong engines that apply"""
    if c.T:
        return {}
    D, batch, masks = first_step(c, seed); g = float(np.float32(c.gamma))
    a = np_step(D.net, D.p_on, D.p_tg, batch, g, bool(c.dq), masks)
    return {w: max(distance(D.net, np_step(D.net, D.p_on, D.p_tg, batch, g, bool(c.dq), masks, wrong=w), a).values()) for w, _ in WRONG if applies(c, w)}


def tells_ok(c, seed=None, k=2.0):
    return all(d >= k * TELL for d in tell_distances(c, seed).values())


find_seed = lambda c, cap=200: STEP.find_seed(c, lambda c, seed: margins_ok(c, seed) and tells_ok(c, seed), cap)
