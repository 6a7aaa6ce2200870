"""fp64 reference of ONE batch_train! for networks with CONVOLUTIONAL Flux SkipConnection(layers, +) blocks (TEST INFRASTRUCTURE): x + Conv(Conv(x)) on a (c, h, w) map,
feed-forward (src/solver.jl:191-236) and in front of an LSTM (src/solver.jl:239-287), over the package's nn descriptors: padded and pad-0 Conv layers, MaxPool / MeanPool,
Dense, LSTM, plain or dueling, plus the block.

The block (Flux 0.14; recalled, not executed): SkipConnection(layers, +)(x) = layers(x) .+ x.  In the engine's words (DESIGN.md section 4 "Skip connections" and
"Convolutional skip blocks"): y_join = y_K + y_P, K the last inner layer, P the producer the first inner layer F reads; backwards dact[K] = dY .* act_K'(y_K) at the join
and dact[P] = (dF + dY) .* act_P'(y_P) at the entry -- P's derivative once, after the sum; for a pool P the derivative is the identity and the pool's own backward reads
dact[P].

Two legs that share no join code:
  * "law"    torch float64 autograd through F.conv2d(padding = ...) on the flipped kernel, F.max_pool2d / F.avg_pool2d and `layers(x) + x` written out;
  * "numpy"  feed-forward steps: feedforward_reference's conv forward / backward BY IMPORT (the oracle's pad-0 conv on the np.pad-ed input, the input gradient cropped; the
             pools' stacked taps) under a HAND-WRITTEN backward of the whole step in the engine's order (np_step: one dact per program entry, the join and the entry as
             stated above); recurrent steps: the torch graph with the join entered as skip_reference's NumPy autograd Function, which hands dY to both operands.
np_step also runs the WRONG engines test_conv_skip_cpu.test_the_tests_can_tell shows apart (WRONG).  The step and the walker are step_reference's.

Tolerances, the gradient check and Adam are the project's one set (re-exported below).  Data rule: every relu pre-activation of the online network on s at least
RELU_MARGIN off the kink, every MaxPool window's top two taps at least RELU_MARGIN apart (feedforward_reference.margins' rule: a window whose maximum is a relu's exact 0
is exempt), the argmax gap of the selecting network at least GAP, no dead gradient block, every wrong engine at least 2 * TELL tolerances away -- all with a factor 2 at
the table's seeds, which were found with this module alone (find_seed).  No case is skipped and no element is masked out."""
import numpy as np
import torch

import dqn_oracle as O
import feedforward_reference as FR
import layernorm_reference as LR
import recurrent_reference as R
import skip_reference as SR
import step_reference as STEP
from feedforward_reference import GRAD_C, GRAD_RTOL, RELU_MARGIN, Adam, check_params      # noqa: F401  (re-exported: one set of constants)
from gru_reference import param_arrays
from layernorm_reference import GAP, TOL_GN, TOL_LOSS, TOL_Q, TOL_TD      # noqa: F401
from step_reference import blocks, check_grads, ff_batch, ff_data, grad_distance, legs_agree, rec_data      # noqa: F401

nn = LR.nn
F64 = torch.float64
ENGINE_SEED = SR.ENGINE_SEED
TELL = SR.TELL
# the wrong engines: (name, changes the forward)
WRONG = (("entry_without_dY", False), ("p_derivative_before_the_sum", False), ("p_derivative_twice", False), ("k_derivative_omitted", False), ("skip_read_from_f", True))
program, _first_inner = SR.program, SR._first_inner


# ------------------------------------------------------------------ the "numpy" leg: the engine's order, by hand (feed-forward)
def _lin(l):
    """the layer's linear part as feedforward_reference's own descriptor (IDENTITY activation: the activations are taken here, from the stored output)"""
    if l.kind == "conv":
        return FR.PConv((l.kh, l.kw), l.cin, l.cout, FR.I, (l.sh, l.sw), (l.ph, l.pw))
    if l.kind in ("maxpool", "meanpool"):
        return FR.Pool(l.kind, (l.kh, l.kw), (l.sh, l.sw))
    return O.Dense(l.n_in, l.n_out, FR.I)


def np_forward(prog, arrs, x, wrong=None, probe=None):
    """stored outputs y[i] (maps keep (B, c, h, w)) and the caches of every program entry.  probe: dict(relu, pool) lowered to the smallest |relu pre-activation| and the
    smallest top-two gap of a MaxPool window (feedforward_reference.margins' rule)"""
    ys, cache = [], []
    for i, e in enumerate(prog):
        xin = x if e.src < 0 else ys[e.src]
        c = None
        if e.kind == "join":
            xs = ys[_first_inner(prog, i)] if wrong == "skip_read_from_f" else ys[e.P]
            y = ys[e.src] + xs
        elif e.l.kind == "conv":
            L = _lin(e.l); xp = FR._padded(L, xin)
            pre, cols = O.layer_forward(FR._plain(L), xp, arrs[e.fi][0], arrs[e.fi][1]); y = SR.act_np(pre, e.l.act); c = (cols, xp.shape)
            if probe is not None and e.l.act == nn.relu:
                probe["relu"] = min(probe["relu"], float(np.abs(pre).min()))
        elif e.l.kind in ("maxpool", "meanpool"):
            L = _lin(e.l)
            if probe is not None and e.l.kind == "maxpool" and e.l.kh * e.l.kw > 1:
                t = np.sort(FR._taps(L, xin)[0], axis=0); gap = t[-1] - t[-2]
                src = prog[e.src] if e.src >= 0 else None
                if src is not None and src.kind == "layer" and src.l.act == nn.relu:      # a window of relu zeros: the first tap takes dY and relu' = 0 drops it in both precisions
                    gap = np.where(t[-1] == 0.0, np.inf, gap)
                probe["pool"] = min(probe["pool"], float(gap.min()))
            y, c = FR.pool_forward(L, xin)
        else:
            assert e.l.kind == "dense", e.l.kind
            pre = xin.reshape(xin.shape[0], -1) @ arrs[e.fi][0] + arrs[e.fi][1]; y = SR.act_np(pre, e.l.act)
            if probe is not None and e.l.act == nn.relu:
                probe["relu"] = min(probe["relu"], float(np.abs(pre).min()))
        ys.append(y); cache.append(c)
    return ys, cache


def np_step(net, p_on, p_tg, batch, gamma, double_q, wrong=None):
    """one feed-forward batch_train! in NumPy with the backward written out entry by entry: D[i] = dL / d(pre-activation of entry i), the engine's dact"""
    s, a, r, sp, done, w = (np.asarray(x, np.float64) if k != 1 else np.asarray(x, np.int64) for k, x in enumerate(batch))
    B = s.shape[0]; prog = program(net)
    aon = [[t.numpy() for t in la] for la in param_arrays(net, nn, np.asarray(p_on, np.float64))]
    atg = [[t.numpy() for t in la] for la in param_arrays(net, nn, np.asarray(p_tg, np.float64))]
    q_tg_sp = SR.np_q(net, prog, np_forward(prog, atg, sp, wrong)[0])[0]
    q_on_sp = SR.np_q(net, prog, np_forward(prog, aon, sp, wrong)[0])[0] if double_q else q_tg_sp
    best = q_on_sp.argmax(axis=1)      # NumPy's argmax is Julia's: the smallest index among the maxima
    y = r + (1.0 - done) * float(gamma) * q_tg_sp[np.arange(B), best]
    ys, cache = np_forward(prog, aon, s, wrong)
    q, (lv, la) = SR.np_q(net, prog, ys)
    td = q[np.arange(B), a] - y
    x = w * td; ab = np.abs(x); qd = np.minimum(ab, 1.0)
    loss = float((0.5 * qd * qd + (ab - qd)).sum() / B)
    dq = np.zeros_like(q); dq[np.arange(B), a] = w * np.clip(x, -1.0, 1.0) / B
    D = [None] * len(prog); g = [None] * len(aon)
    act_of = lambda i: prog[i].l.act if prog[i].kind == "layer" else nn.identity
    if lv is None:
        D[la] = SR.dact_np(dq, ys[la], act_of(la))
    else:      # Q = V + A - mean(A)
        D[lv] = SR.dact_np(dq.sum(axis=1, keepdims=True), ys[lv], act_of(lv))
        D[la] = SR.dact_np(dq - dq.mean(axis=1, keepdims=True), ys[la], act_of(la))
    first_of = {_first_inner(prog, j): j for j, e in enumerate(prog) if e.kind == "join"}
    for i in range(len(prog) - 1, -1, -1):
        e = prog[i]; xin = s if e.src < 0 else ys[e.src]
        if e.kind == "join":      # at the join: dact[K] = dY .* act_K'(y_K)
            D[e.src] = D[i] if wrong == "k_derivative_omitted" else SR.dact_np(D[i], ys[e.src], act_of(e.src))
            continue
        if e.l.kind == "conv":
            L = _lin(e.l); cols, pshape = cache[i]; Bx, C, H, Wd = xin.shape
            dxp, dW, db = O.layer_backward(FR._plain(L), cols, pshape, ys[i], D[i], aon[e.fi][0])      # (IDENTITY: D[i] is the pre-activation gradient already)
            dx = dxp[:, :, L.ph:L.ph + H, L.pw:L.pw + Wd]; g[e.fi] = [dW, db]      # the interior crop of the extended map's input gradient
        elif e.l.kind in ("maxpool", "meanpool"):
            dx = FR.pool_backward(_lin(e.l), cache[i], xin.shape, D[i]); g[e.fi] = []
        else:
            x2 = xin.reshape(B, -1); g[e.fi] = [x2.T @ D[i], D[i].sum(axis=0)]; dx = (D[i] @ aon[e.fi][0].T).reshape(xin.shape)
        if e.src < 0:
            continue
        act_s = act_of(e.src)
        if i in first_of:      # at the entry: dact[P] = (dF + dY) .* act_P'(y_P), the derivative once, after the sum
            dY = D[first_of[i]]
            if wrong == "entry_without_dY":
                D[e.src] = SR.dact_np(dx, ys[e.src], act_s)
            elif wrong == "p_derivative_before_the_sum":
                D[e.src] = SR.dact_np(dx, ys[e.src], act_s) + dY
            elif wrong == "p_derivative_twice":
                D[e.src] = SR.dact_np(SR.dact_np(dx + dY, ys[e.src], act_s), ys[e.src], act_s)
            else:
                D[e.src] = SR.dact_np(dx + dY, ys[e.src], act_s)
        else:      # one consumer -- or the dueling split, where the two streams' gradients meet
            d = SR.dact_np(dx, ys[e.src], act_s); D[e.src] = d if D[e.src] is None else D[e.src] + d
    gv = np.concatenate([np.asarray(x).reshape(-1) for la_ in g for x in la_])
    return dict(q_on_s=q, q_on_sp=q_on_sp, q_tg_sp=q_tg_sp, best_a=best, y=y, td=td, loss=loss, grads=gv, grad_norm=float(np.abs(gv).max()))


# the legs: "law" is step_reference's walker as it stands; "numpy" is np_step for a feed-forward step and skip_reference's NumPy join for a recurrent one
q_values = STEP.bound(STEP.q_values, {"law": {}, "numpy": SR.JOIN_NUMPY}, "leg")
ff_step = STEP.bound(STEP.ff_step, {"law": {}, "numpy": np_step}, "leg")
rec_step = STEP.bound(STEP.rec_step, {"law": {}, "numpy": SR.JOIN_NUMPY}, "leg")
distance = SR.distance


# ------------------------------------------------------------------ the case table
case = LR.case
S = SR.S
CV = lambda c, act=nn.identity, k=3, pad=1, cin=None: nn.Conv(k, cin or c, c, act, 1, pad)


def block(c, k=3, pad=1, act_k=nn.identity, m=2, act_mid=nn.relu):
    """x + Conv(... Conv(x)): m padded convs c => c, act_mid (relu) between them, act_k on the last"""
    return lambda: S(*[CV(c, act_mid, k, pad) for _ in range(m - 1)], CV(c, act_k, k, pad))


def trunk(c, hw, *mid, stem=None, nA=4, cin=2, tail=None):
    """Conv(3, cin => c, relu; pad = 1) (or `stem`) -> mid... -> flattenbatch -> Dense(c * h * w, nA) (or `tail`)"""
    return lambda: nn.Chain(stem() if stem else nn.Conv(3, cin, c, nn.relu, 1, 1), *[b() for b in mid], nn.flattenbatch, *(tail() if tail else [nn.Dense(c * hw[0] * hw[1], nA)]))


# the smallest shapes at which each path can go wrong (the issue's table, in its order)
CASES = [
    case("valu_c4_5x5_b5", trunk(4, (5, 5), block(4)), 5, obs=(2, 5, 5), seed=1),                                            # 1: c = 4: the VALU forms; ten unaligned [s ; s'] columns
    case("mfma_c16_6x6_b32", trunk(16, (6, 6), block(16)), 32, obs=(2, 6, 6), seed=2),                                      # 2: MFMA tiles
    # 3: sample-cut dW chunks.  (tanh in front of the block: with a relu there too a step has 221 184 relu units, and no seed below 200 keeps all of them RELU_MARGIN off the kink on three steps)
    case("mfma_c16_6x6_b128", trunk(16, (6, 6), block(16), stem=lambda: nn.Conv(3, 2, 16, nn.tanh, 1, 1)), 128, obs=(2, 6, 6), seed=86),
    case("single_inner_c16_b32", trunk(16, (6, 6), block(16, m=1)), 32, obs=(2, 6, 6), seed=1),                             # 4: F == K: both epilogues on one layer, dpre aliases dY
    case("rect_6x7_k3x5_b32", trunk(16, (6, 7), block(16, (3, 5), (1, 2)), stem=lambda: nn.Conv((3, 5), 2, 16, nn.relu, 1, (1, 2))), 32, obs=(2, 6, 7), seed=6),      # 5
    case("k_tanh_c16_b32", trunk(16, (6, 6), block(16, act_k=nn.tanh)), 32, obs=(2, 6, 6), seed=3),                         # 6: the unfused join + bwd_join
    case("p_pad0_tanh_c16_b32", trunk(16, (6, 6), block(16), stem=lambda: nn.Conv(3, 2, 16, nn.tanh)), 32, obs=(2, 8, 8), seed=3),      # 7: P a pad-0 Conv with tanh: the derivative after the sum
    case("p_maxpool_c16_b32", trunk(16, (4, 4), lambda: nn.MaxPool(2), block(16)), 32, obs=(2, 8, 8), seed=4),              # 8: the entry's derivative is the identity; the pool's backward reads dact[P]
    case("two_blocks_c16_b32", trunk(16, (6, 6), block(16), block(16)), 32, obs=(2, 6, 6), seed=7),                         # 9: P is a join
    case("meanpool_behind_c16_b32", trunk(16, (3, 3), block(16), lambda: nn.MeanPool(2)), 32, obs=(2, 6, 6), seed=6),       # 10: a pool consumes the join
    case("dueling_prio_u8", lambda: nn.create_dueling_network(trunk(16, (6, 6), block(16), tail=lambda: [nn.Dense(576, 32, nn.relu), nn.Dense(32, 4)])()), 32, obs=(2, 6, 6),
         dueling=True, prio=1, u8=1, seed=61),                                                                  # 11: the split and the byte arena
]
REC_CASES = [
    case("conv_block_lstm", lambda: nn.Chain(nn.Conv(3, 2, 4, nn.relu, 1, 1), block(4)(), nn.flattenbatch, nn.LSTM(100, 8), nn.Dense(8, 3)), 4, obs=(2, 5, 5), nA=3, T=3, seed=1),      # 12: the block over T * B columns
]
ALL = CASES + REC_CASES


def readout_net(c, hw, blocks=2, m=2):
    """the network of the exact check: Conv(3, c => c; pad = 1) -> `blocks` blocks of m Conv(3, c => c; pad = 1) -> flattenbatch -> Dense(n, n), n = c * h * w, every conv
    without activation, its kernel the centre-tap identity (W[co, ci, 1, 1] = [co == ci], which the flip of a true convolution leaves alone), the Dense weight the identity, every bias zero:
    each block doubles its input exactly, Q = 2^blocks * x.  Returns (net, flat fp32 parameters, n)"""
    n = c * hw[0] * hw[1]
    net = nn.Chain(CV(c), *[block(c, m=m, act_mid=nn.identity)() for _ in range(blocks)], nn.flattenbatch, nn.Dense(n, n))
    W = np.zeros((c, c, 3, 3), np.float32); W[np.arange(c), np.arange(c), 1, 1] = 1.0
    conv = [W.ravel(), np.zeros(c, np.float32)]
    return net, np.concatenate(conv * (1 + blocks * m) + [np.eye(n, dtype=np.float32).ravel(), np.zeros(n, np.float32)]), n
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)
first_step = STEP.first_step      # (network data, fp64 batch) of the case's first step


def step(c, D, batch, p_on=None, leg="law"):
    return (rec_step if c.T else ff_step)(D.net, D.p_on if p_on is None else p_on, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq), leg=leg)


def margins_at(c, net, p_on, p_tg, batch):
    """(relu margin, MaxPool margin, argmax gap) of one step in fp64: the relu and pool margins on the s columns under the online parameters (where the derivatives are
    taken; a recurrent case: over the columns the mask keeps, whose trunk does not depend on the hidden state), the gap over the columns of the selecting network"""
    probe = dict(relu=np.inf, pool=np.inf)
    arrs = [[t.numpy() for t in la] for la in param_arrays(net, nn, np.asarray(p_on, np.float64))]
    s = np.asarray(batch[0], np.float64)
    if c.T:
        s = s.reshape((-1,) + tuple(c.obs))[np.asarray(batch[5]).reshape(-1) > 0]
        prog = program(net); cut = next(i for i, e in enumerate(prog) if e.kind == "layer" and e.l.kind == "lstm")
        np_forward(prog[:cut], arrs, s, probe=probe)
        qsel = np.concatenate(q_values(net, p_on if c.dq else p_tg, batch[3]))
    else:
        np_forward(program(net), arrs, s, probe=probe)
        qsel = q_values(net, p_on if c.dq else p_tg, batch[3])
    return probe["relu"], probe["pool"], LR._gap(qsel)


def case_margins(c, seed=None):
    D, batch = first_step(c, seed)
    return margins_at(c, D.net, D.p_on, D.p_tg, batch)


def trajectory(c, seed=None):
    """the fp64 trajectory of the case's three steps with the reference alone (fp64 Adam on the reference's own gradients; a prioritized case: the IS weights of the
    priorities the steps before left behind, (|td| + eps)^alpha) -> [(margins, step outputs)] per step"""
    out = []
    if c.T:
        D = rec_data(c, seed); batches = [R.sample_batch(D.ring, idx, start, c.T, c.obs) for idx, start in D.draws]
    else:
        D = ff_data(c, seed); prio = O.priority_from_td(np.abs(D.r), np.float32(1e-3), np.float32(0.6)).astype(np.float64)
    p = D.p_on.astype(np.float64); adam = Adam(p.size, lr=LR.LR)
    for k in range(3):
        if c.T:
            batch = batches[k]
        else:
            batch = ff_batch(c, D, D.idx[k])[:5] + (O.is_weights(prio[D.idx[k]], prio, 0.4, np.float64),)
        o = step(c, D, batch, p_on=p)
        out.append((margins_at(c, D.net, p, D.p_tg, batch), o))
        if not c.T and c.prio:
            prio[D.idx[k]] = O.priority_from_td(np.abs(o["td"]), np.float32(1e-3), np.float32(0.6)).astype(np.float64)
        p = adam.step(p, o["grads"])
    return out


def margins_ok(c, seed=None, k=2.0):
    """k times the margins on the first step (the find_seed pattern of the other tables) and the margins themselves on the two steps the fp64 trajectory takes from
    there -- the engine's own trajectory lies within round-off of it --; no dead gradient block on the first step"""
    tr = trajectory(c, seed)
    for i, (rm, pm, gap) in enumerate(m for m, _ in tr):
        f = k if i == 0 else 1.0
        if not (rm > f * RELU_MARGIN and pm > f * RELU_MARGIN and gap > f * GAP):
            return False
    D, _ = first_step(c, seed)
    return not STEP.dead_blocks(D.net, tr[0][1]["grads"])


def applies(c, wrong):
    """which wrong engines a case can show: the feed-forward ones (np_step); P's derivative before the sum needs a P with an activation, twice one whose derivative is not
    0 / 1; K's derivative omitted needs a K with an activation; the skip read from F's output needs that output to have the block's shape"""
    if c.T:
        return False
    prog = program(c.mk()); joins = [(j, e) for j, e in enumerate(prog) if e.kind == "join"]
    act_of = lambda i: prog[i].l.act if prog[i].kind == "layer" else nn.identity
    if wrong == "p_derivative_before_the_sum":
        return any(act_of(e.P) != nn.identity for _, e in joins)
    if wrong == "p_derivative_twice":      # relu' is 0 or 1: applied twice it is itself
        return any(act_of(e.P) not in (nn.identity, nn.relu) for _, e in joins)
    if wrong == "k_derivative_omitted":
        return any(act_of(e.src) != nn.identity for _, e in joins)
    if wrong == "skip_read_from_f":      # every inner conv of the table's blocks keeps (c, h, w)
        return all(prog[_first_inner(prog, j)].l.cout == prog[e.src].l.cout for j, e in joins)
    return True


def tell_distances(c, seed=None):
    """{wrong engine: the largest distance over the compared quantities, in tolerances} on the case's first step, for the wrong engines that apply"""
    if c.T:
        return {}
    D, batch = first_step(c, seed); g = float(np.float32(c.gamma))
    a = np_step(D.net, D.p_on, D.p_tg, batch, g, bool(c.dq))
    return {w: max(distance(D.net, np_step(D.net, D.p_on, D.p_tg, batch, g, bool(c.dq), wrong=w), a).values()) for w, _ in WRONG if applies(c, w)}


def tells_ok(c, seed=None, k=2.0):
    return all(d >= k * TELL for d in tell_distances(c, seed).values())


find_seed = lambda c, cap=200: STEP.find_seed(c, lambda c, seed: margins_ok(c, seed) and tells_ok(c, seed), cap)
