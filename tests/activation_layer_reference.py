"""fp64 reference of ONE batch_train! for networks with the standalone activation layer nn.Activation(σ) (TEST INFRASTRUCTURE: layer kind 14, csrc/act_layer.hip; Julia's
Base.Broadcast.BroadcastFunction(σ) in a Chain), feed-forward (src/solver.jl:191-236) and recurrent (src/solver.jl:239-287), over the package's nn descriptors: Dense, Conv
(pad included), MaxPool / MeanPool, GroupNorm, SkipConnection(+) on vectors and on maps, LSTM, GRU and Activation layers, plain or dueling.

The law of the layer: y = σ.(x); σ is one of the eleven codes of activation_reference (their laws are imported, not restated) or one of
    gelu 11       0.5 x (1 + tanh(sqrt(2/π) (x + 0.044715 x³)))      NNlib's tanh form, NOT the erf form
    swish 12      x sigm(x)
    mish 13       x tanh(softplus(x))
    hardswish 14  x clamp((x + 3) / 6, 0, 1)
The codes are restated here as plain integers (the header's values): the reference does not read them from the package it checks.

Two legs that share no code of the layer:
  * "torch"  torch float64 autograd with F.gelu(approximate="tanh"), F.silu, F.mish, F.hardswish and, for the eleven, activation_reference.act_torch (torch.nn.functional's own);
  * "numpy"  the closed forms above in NumPy with a HAND-WRITTEN backward, entered into the graph as a torch.autograd.Function: for the eleven the derivative as a function
             of the layer's own OUTPUT (activation_reference.dact_np -- the column the engine runs), for the four the derivative from the INPUT:
             gelu′ = 0.5 (1 + t) + 0.5 x (1 - t²) sqrt(2/π) (1 + 3·0.044715 x²), swish′ = s (1 + x (1 - s)), mish′ = t + x (1 - t²) sigm(x),
             hardswish′ = 0 below -3, 1 above 3, (2x + 3) / 6 between.
tests/test_activation_layer_cpu.py holds the two to 1e-10 of each other on every case before anything is compared with the GPU.  Everything that is no Activation layer is
imported: the GroupNorm law (groupnorm_reference), the cells, the Huber loss, the batches, Adam, the gradient and parameter checks and their constants.  No tolerance is
introduced here.

Data rules, asserted by prepare() on the first step and by the GPU test on every step it runs: every fp64 input of an Activation layer and every pre-activation of a fused
activation on s stays RELU_MARGIN away from each kink of its σ (relu, leakyrelu, selu: 0; relu6: 0 and 6; hardtanh: -1 and 1; hardswish: -3 and 3 -- which value a kink
takes is NNlib's rule and unpinned); every MaxPool window keeps its top-two gap above RELU_MARGIN; every argmax column keeps GAP.  Seeds are fixed in the table and were
found on the CPU with this module alone (find_seed: the smallest seed that keeps TWICE the margins); no case is skipped at run time."""
import types

import numpy as np
import torch
import torch.nn.functional as F

import activation_reference as AR
import dqn_oracle as O
import groupnorm_reference as GR
import layernorm_reference as LR
import recurrent_reference as R
from drqn_common import draws, make_episodes      # noqa: F401
from feedforward_edges_common import GAP, TOL_GN, TOL_LOSS, TOL_Q, TOL_TD      # noqa: F401  (one set of constants)
from feedforward_reference import GRAD_C, GRAD_RTOL, RELU_MARGIN, Adam, check_params      # noqa: F401
from gru_reference import gru_cell, param_arrays

nn = LR.nn
F64 = torch.float64
LRATE = LR.LR
GELU, SWISH, MISH, HARDSWISH = 11, 12, 13, 14
NAMES = AR.NAMES + ("gelu", "swish", "mish", "hardswish")      # index = the code on an Activation layer
NEW = (GELU, SWISH, MISH, HARDSWISH)
KINKS = dict(AR.KINKS); KINKS[HARDSWISH] = (-3.0, 3.0)
GELU_C, GELU_A = float(np.sqrt(2.0 / np.pi)), 0.044715
SENTINEL = {GELU: nn.gelu, SWISH: nn.swish, MISH: nn.mish, HARDSWISH: nn.hardswish}


def A(code):
    """nn.Activation(σ) by code: the four new ones through the mirror's sentinels, as a user writes them"""
    return nn.Activation(SENTINEL.get(code, code))


# ------------------------------------------------------------------ the two legs of the layer
def actl_torch(x, a):
    if a <= 10:
        return AR.act_torch(x, a)
    return {GELU: lambda v: F.gelu(v, approximate="tanh"), SWISH: F.silu, MISH: F.mish, HARDSWISH: F.hardswish}[a](x)


def _sigm(x):
    return 1.0 / (1.0 + np.exp(-x))


def _softplus(x):
    return np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0.0)


def actl_np(x, a):
    x = np.asarray(x, np.float64)
    if a <= 10:
        return AR.act_np(x, a)
    if a == GELU:
        return 0.5 * x * (1.0 + np.tanh(GELU_C * (x + GELU_A * x ** 3)))
    if a == SWISH:
        return x * _sigm(x)
    if a == MISH:
        return x * np.tanh(_softplus(x))
    assert a == HARDSWISH, a
    return x * np.clip((x + 3.0) / 6.0, 0.0, 1.0)


def dactl_np(dy, x, y, a):
    """dL/dx: from the OUTPUT y for the eleven (the engine's column), from the INPUT x for the four"""
    if a <= 10:
        return AR.dact_np(dy, y, a)
    if a == GELU:
        t = np.tanh(GELU_C * (x + GELU_A * x ** 3))
        return dy * (0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * GELU_C * (1.0 + 3.0 * GELU_A * x * x))
    if a == SWISH:
        s = _sigm(x)
        return dy * (s * (1.0 + x * (1.0 - s)))
    if a == MISH:
        t = np.tanh(_softplus(x))
        return dy * (t + x * (1.0 - t * t) * _sigm(x))
    assert a == HARDSWISH, a
    return dy * np.where(x < -3.0, 0.0, np.where(x > 3.0, 1.0, (2.0 * x + 3.0) / 6.0))


class _ActNumpy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a):
        xn = x.detach().numpy(); y = actl_np(xn, a)
        ctx.saved = (xn, y, a)
        return torch.tensor(y, dtype=F64)

    @staticmethod
    def backward(ctx, dy):
        xn, y, a = ctx.saved
        return torch.tensor(dactl_np(dy.numpy(), xn, y, a)), None


LEGS = {"torch": actl_torch, "numpy": _ActNumpy.apply}


# ------------------------------------------------------------------ chains of nn descriptors
def new_probe():
    return dict(kink=np.inf, pool=np.inf)


def _kink(probe, x, a):
    for k in KINKS.get(a, ()):
        probe["kink"] = min(probe["kink"], GR._min((x.detach()[GR._rows(probe, x)] - k).abs()))


def _run(layers, it, x, hs, leg, probe, st):
    """one (time) step through a chain; `it` yields (flat layer index, parameter arrays) in nn.all_layers order; st['relu']: x holds the exact zeros of a relu"""
    for l in layers:
        if l.kind == "skip":
            x = _run(l.layers.layers, it, x, hs, leg, probe, st) + x
            st["relu"] = False
            continue
        k, a = next(it)
        if l.kind == "activation":
            if probe is not None:
                _kink(probe, x, l.code)
            x = LEGS[leg](x, l.code); st["relu"] = l.code == AR.RELU
            continue
        if l.kind == "lstm":
            hs[k] = R.lstm_cell(x.reshape(x.shape[0], -1), hs[k][0], hs[k][1], a[0], a[1], a[2]); x = hs[k][0]; st["relu"] = False
            continue
        if l.kind == "gru":
            hs[k] = gru_cell(x.reshape(x.shape[0], -1), hs[k], a[0], a[1], a[2]); x = hs[k]; st["relu"] = False
            continue
        if l.kind in ("maxpool", "meanpool"):
            if l.kind == "maxpool" and probe is not None:
                probe["pool"] = min(probe["pool"], GR._pool_gap(l, x.detach()[GR._rows(probe, x)], st["relu"]))
            x = (F.max_pool2d if l.kind == "maxpool" else F.avg_pool2d)(x, (l.kh, l.kw), stride=(l.sh, l.sw))
            st["relu"] = st["relu"] and l.kind == "maxpool"
            continue
        if l.kind == "adaptivemeanpool":      # GlobalMeanPool() only: the mean over the whole map (kinds 12 / 13 have their own table: adaptive_pool_reference)
            assert (l.oh, l.ow) == (1, 1)
            x = x.mean(dim=(2, 3), keepdim=True); st["relu"] = False
            continue
        if l.kind == "conv":      # a true convolution is the cross-correlation with the flipped kernel (feedforward_reference._layer_t)
            pre = F.conv2d(x, a[0].flip(2, 3), a[1], stride=(l.sh, l.sw), padding=(l.ph, l.pw))
        elif l.kind == "groupnorm":
            pre = GR.gn_torch(x, a[0], a[1], l.G, float(np.float32(l.eps)))      # Flux.params order: beta, gamma
        else:
            assert l.kind == "dense", l.kind
            pre = x.reshape(x.shape[0], -1) @ a[0] + a[1]
        if probe is not None:
            _kink(probe, pre, l.act)
        x = AR.act_torch(pre, l.act); st["relu"] = l.act == AR.RELU
    return x


def q_step(net, arrs, x, hs, leg="torch", probe=None):
    it = iter(enumerate(arrs)); st = dict(relu=False)
    if isinstance(net, nn.DuelingNetwork):
        y = _run(net.base.layers, it, x, hs, leg, probe, st)
        v = _run(net.val.layers, it, y, hs, leg, probe, dict(st))
        a = _run(net.adv.layers, it, y, hs, leg, probe, dict(st))
        return v + a - a.mean(dim=1, keepdim=True)      # src/dueling.jl:10
    return _run(net.layers, it, x, hs, leg, probe, st)


def is_recurrent(net):
    return any(l.kind in ("lstm", "gru") for l in nn.all_layers(net))


def q_values(net, p, x, leg="torch", probe=None, mask=None):
    """Q (B, nA) as fp64 NumPy of a feed-forward network on x (B, ...); a recurrent network: x (T, B, ...) from the reset state -> [T] of (B, nA)"""
    arrs = param_arrays(net, nn, np.asarray(p, np.float64))
    with torch.no_grad():
        if not is_recurrent(net):
            return q_step(net, arrs, LR._t64(x), {}, leg, probe).numpy()
        hs = LR.init_state(net, arrs, np.asarray(x).shape[1]); out = []
        for t, xt in enumerate(x):
            if probe is not None and mask is not None:
                probe["rows"] = torch.tensor(np.asarray(mask[t]) > 0)
            out.append(q_step(net, arrs, LR._t64(xt), hs, leg, probe).numpy())
        return out


def probe_of(net, p, s, mask=None):
    pr = new_probe(); q_values(net, p, s, probe=pr, mask=mask)
    return pr


def ff_step(net, p_on, p_tg, batch, gamma, double_q, leg="torch"):
    """layernorm_reference.ff_step over this module's chain.  batch = (s, a, r, sp, done, w) as get_batch returns it"""
    s, a, r, sp, done, w = batch
    s, sp, r, done, w = (LR._t64(v) for v in (s, sp, r, done, w))
    a = torch.tensor(np.asarray(a, np.int64)); B = s.shape[0]
    aon, atg = param_arrays(net, nn, np.asarray(p_on, np.float64)), param_arrays(net, nn, np.asarray(p_tg, np.float64))
    with torch.no_grad():       # the targets are constants of the loss (src/solver.jl:209-217)
        q_tg_sp = q_step(net, atg, sp, {}, leg)
        q_on_sp = q_step(net, aon, sp, {}, leg) if double_q else q_tg_sp
        best = (q_on_sp == q_on_sp.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)      # Julia's argmax: the smallest index among the maxima
        y = r + (1.0 - done) * float(gamma) * q_tg_sp[torch.arange(B), best]
    leaves = [x for la in aon for x in la]
    for x in leaves:
        x.requires_grad_(True)
    q = q_step(net, aon, s, {}, leg)
    td = q[torch.arange(B), a] - y
    loss = LR._huber(w * td).sum() / B        # src/solver.jl:223-224
    loss.backward()
    g = np.concatenate([x.grad.numpy().reshape(-1) for x in leaves])
    return dict(q_on_s=q.detach().numpy(), q_on_sp=q_on_sp.numpy(), q_tg_sp=q_tg_sp.numpy(), best_a=best.numpy(), y=y.numpy(), td=td.detach().numpy(),
                loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()))


def rec_step(net, p_on, p_tg, batch, gamma, double_q, leg="torch"):
    """layernorm_reference.rec_step over this module's chain.  batch = (s, a, r, sp, done, mask), each (T, B, ...)"""
    s, a, r, sp, d, m = batch; T, B = s.shape[0], s.shape[1]
    q_tg = q_values(net, p_tg, sp, leg)
    q_on = q_values(net, p_on, sp, leg) if double_q else q_tg
    ys = [O.bellman_targets(q_on[t], q_tg[t], r[t].astype(np.float64), d[t].astype(np.float64), gamma, double_q)[0] for t in range(T)]
    arrs = param_arrays(net, nn, np.asarray(p_on, np.float64)); leaves = [x for la in arrs for x in la]
    for x in leaves:
        x.requires_grad_(True)
    hs = LR.init_state(net, arrs, B); loss = torch.zeros((), dtype=F64); tds = []
    for t in range(T):
        q = q_step(net, arrs, LR._t64(s[t]), hs, leg)
        td = q[torch.arange(B), torch.tensor(a[t].astype(np.int64))] - LR._t64(ys[t]); tds.append(td.detach().numpy())
        loss = loss + LR._huber(LR._t64(m[t]) * td).sum() / B
    loss = loss / T
    loss.backward()
    g = np.concatenate([x.grad.numpy().reshape(-1) for x in leaves])
    return dict(loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()), q_on_sp=q_on, q_tg_sp=q_tg, td=np.stack(tds))


legs_agree = LR.legs_agree
BLOCK_NAMES = {"lstm": ("Wi", "Wh", "b", "h0", "c0"), "gru": ("Wi", "Wh", "b", "h0"), "dense": ("W", "b"), "conv": ("W", "b"), "groupnorm": ("beta", "gamma"), "maxpool": (), "meanpool": (),
               "adaptivemeanpool": (), "activation": ()}


def blocks(net):
    """[(name, slice into the flat Flux.params vector)]; an Activation layer holds nothing"""
    out, off = [], 0
    for li, l in enumerate(nn.all_layers(net)):
        for nm, shp in zip(BLOCK_NAMES[l.kind], l.shapes()):
            k = int(np.prod(shp)); out.append((f"{'gn' if l.kind == 'groupnorm' else l.kind}{li}.{nm}", slice(off, off + k))); off += k
    return out


def check_grads(net, got, want, live=True):
    """recurrent_reference.check_grads per block (GRAD_C, GRAD_RTOL unchanged); live: no block's fp64 gradient is negligible"""
    R.check_grads(net, nn, got, want, live=live, blks=blocks(net))


# ------------------------------------------------------------------ the case table: the smallest shapes at which each path of act_layer.hip and each placement can go wrong
def case(name, mk, B, obs=(6,), nA=4, dueling=False, dq=1, prio=1, T=0, seed=1, pscale=2.0, plain=None, codes=()):
    """plain: the same network with every Activation(σ) folded into the layer in front (Dense(…, σ) / Conv(…, σ)), where that is expressible -- the exact companion.
    pscale: the glorot draw is multiplied by it, so that hidden pre-activations have O(1) spread and reach past the kinks at ±1 and ±3"""
    return types.SimpleNamespace(name=name, mk=mk, B=B, obs=tuple(obs), nA=nA, dueling=dueling, dq=dq, prio=prio, u8=0, mfma=1, T=T, seed=seed, gamma=0.95, pscale=pscale, plain=plain,
                                 codes=tuple(codes))


def _vec(a, n=16):
    return lambda: nn.Chain(nn.Dense(6, n), A(a), nn.Dense(n, 4))


def _vec_plain(a, n=16):
    return lambda: nn.Chain(nn.Dense(6, n, a), nn.Dense(n, 4))


IMG = (1, 6, 6)


def _map(a, pad=0):
    feat = 4 * (4 + 2 * pad) ** 2
    return lambda: nn.Chain(nn.Conv(3, 1, 4, pad=pad), A(a), nn.flattenbatch, nn.Dense(feat, 4))


def _map_plain(a, pad=0):
    feat = 4 * (4 + 2 * pad) ** 2
    return lambda: nn.Chain(nn.Conv(3, 1, 4, a, pad=pad), nn.flattenbatch, nn.Dense(feat, 4))


def _vblock():
    return nn.SkipConnection(nn.Chain(nn.Dense(16, 16, nn.relu), nn.Dense(16, 16)), "+")


def _mblock():
    return nn.SkipConnection(nn.Chain(nn.Conv(3, 4, 4, nn.relu, pad=1), nn.Conv(3, 4, 4, pad=1)), "+")


# seeds: found with find_seed on the CPU, with this module alone; fixed here.  Every case of the tables keeps twice the margins at seed 1 already (the largest seed is 1:
# docs/history/activation_layer.md; tests/test_activation_layer_cpu.py re-runs the search), so the dictionary names no exception
SEEDS = {}
_c = lambda name, mk, B, **kw: case(name, mk, B, seed=SEEDS.get(name, 1), **kw)


def _table():
    t = []
    # 1. vectors, Dense(6, n) -> Activation(σ) -> Dense(n, 4): all fifteen σ at B = 16, n = 16 (one 16-byte access per thread, one workgroup); the eleven have a fused companion
    for a in range(15):
        t.append(_c(f"vec_{NAMES[a]}", _vec(a), 16, plain=_vec_plain(a) if a <= 10 else None, codes=(a,)))
    # 2. the four new ones at B = 5 (ten columns: the one-column walk; the target pass starts at column 5) with n = 7 (a ragged last workgroup), and one case at B = 128
    for a in NEW:
        t.append(_c(f"vec_{NAMES[a]}_b5_n7", _vec(a, 7), 5, codes=(a,)))
    t.append(_c("vec_gelu_b128", _vec(GELU), 128, codes=(GELU,)))
    # 3. maps on a 6x6x1 observation: Conv(3, 1 => 4) -> Activation(σ) -> Dense for the four new codes and relu (the eleven: exact companions only, below)
    for a in NEW + (AR.RELU,):
        t.append(_c(f"map_{NAMES[a]}", _map(a), 16, obs=IMG, plain=_map_plain(a) if a <= 10 else None, codes=(a,)))
    t.append(_c("map_gn_swish", lambda: nn.Chain(nn.Conv(3, 1, 4), nn.GroupNorm(4, 2), A(SWISH), nn.flattenbatch, nn.Dense(64, 4)), 16, obs=IMG, codes=(SWISH,)))
    t.append(_c("map_maxpool_mish", lambda: nn.Chain(nn.Conv(3, 1, 4), nn.MaxPool(2), A(MISH), nn.flattenbatch, nn.Dense(16, 4)), 16, obs=IMG, codes=(MISH,)))
    t.append(_c("map_gelu_cpad", lambda: nn.Chain(nn.Conv(3, 1, 4), A(GELU), nn.Conv(3, 4, 4, pad=1), nn.flattenbatch, nn.Dense(64, 4)), 16, obs=IMG, codes=(GELU,)))
    # 3b. behind a global pool (the (4, 1, 1) map of GlobalMeanPool), and directly behind another Activation -- whose fused companion is Dense(6, 16, tanh) -> Activation(relu)
    t.append(_c("map_gmean_hardswish", lambda: nn.Chain(nn.Conv(3, 1, 4), nn.GlobalMeanPool(), A(HARDSWISH), nn.flattenbatch, nn.Dense(4, 4)), 16, obs=IMG, pscale=4.0, codes=(HARDSWISH,)))
    t.append(_c("vec_tanh_then_relu", lambda: nn.Chain(nn.Dense(6, 16), A(AR.TANH), A(AR.RELU), nn.Dense(16, 4)), 16,
                plain=lambda: nn.Chain(nn.Dense(6, 16, nn.tanh), A(AR.RELU), nn.Dense(16, 4)), codes=(AR.TANH, AR.RELU)))
    # 4. the post-add relu of ResNet-v1, the reason for the layer: on vectors (skip.hip) and on maps (conv_pad.hip epilogues)
    t.append(_c("postadd_vec", lambda: nn.Chain(nn.Dense(6, 16), _vblock(), A(AR.RELU), _vblock(), nn.Dense(16, 4)), 16, pscale=1.0, codes=(AR.RELU,)))
    t.append(_c("postadd_map", lambda: nn.Chain(nn.Conv(3, 1, 4), _mblock(), A(AR.RELU), _mblock(), nn.flattenbatch, nn.Dense(64, 4)), 16, obs=IMG, pscale=1.0, codes=(AR.RELU,)))
    # 5. dueling: the base chain ENDS in Activation(swish); the join's summed dX is the layer's dY
    t.append(_c("dueling_swish", lambda: nn.create_dueling_network(nn.Chain(nn.Dense(6, 16), A(SWISH), nn.Dense(16, 8, nn.relu), nn.Dense(8, 4))), 16, dueling=True, codes=(SWISH,)))
    return t


def _rec_table():
    return [
        _c("rec_conv_gelu_gru", lambda: nn.Chain(nn.Conv(2, 1, 4), A(GELU), nn.flattenbatch, nn.GRU(64, 8), nn.Dense(8, 3)), 4, obs=(1, 5, 5), nA=3, T=3, prio=0, pscale=3.0, codes=(GELU,)),
        _c("rec_lstm_tanh", lambda: nn.Chain(nn.LSTM(6, 8), A(AR.TANH), nn.Dense(8, 3)), 4, nA=3, T=3, prio=0, pscale=3.0, codes=(AR.TANH,)),
    ]


# exact companions only (engine against engine, no fp64 step): the eleven codes on a map, and one padded Conv
def _exact_table():
    return [_c(f"exact_map_{NAMES[a]}", _map(a), 16, obs=IMG, plain=_map_plain(a), codes=(a,)) for a in range(11) if a != AR.RELU] + \
           [_c("exact_cpad_tanh", _map(AR.TANH, pad=1), 16, obs=IMG, plain=_map_plain(AR.TANH, pad=1), codes=(AR.TANH,))]


def _build():
    global CASES, REC_CASES, EXACT_ONLY, BY_NAME
    CASES, REC_CASES, EXACT_ONLY = _table(), _rec_table(), _exact_table()
    BY_NAME = {c.name: c for c in CASES + REC_CASES + EXACT_ONLY}
    assert len(BY_NAME) == len(CASES) + len(REC_CASES) + len(EXACT_ONLY)


_build()
STEPS = 2      # train steps the GPU test runs per feed-forward case (the draws of layernorm_reference.ff_data)
ff_data, ff_batch, rec_data = LR.ff_data, LR.ff_batch, LR.rec_data


def trajectory(c, D=None, steps=STEPS, seed=None, leg="torch"):
    """the fp64 trajectory of a case: yields (k, fp64 online parameters before step k, batch, step outputs); the parameters move by fp64 Adam"""
    D = D or (rec_data(c, seed) if c.T else ff_data(c, seed))
    p = D.p_on.astype(np.float64); adam = Adam(p.size, lr=LRATE)
    for k in range(1 if c.T else steps):
        if c.T:
            idx, start = D.draws[k]; batch = R.sample_batch(D.ring, idx, start, c.T, c.obs)
            o = rec_step(D.net, p, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq), leg)
        else:
            batch = ff_batch(c, D, D.idx[k])
            o = ff_step(D.net, p, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq), leg)
        yield k, p, batch, o
        p = adam.step(p, o["grads"])


def margins(c, net, p_on, p_tg, batch):
    """(kink margin, MaxPool margin, argmax gap) of one step in fp64: kinks and windows on s under the online parameters (where the derivatives are taken), the gap over the
    columns of the network that picks the action"""
    s, sp = batch[0], batch[3]; mask = batch[5] if c.T else None
    pr = probe_of(net, p_on, s, mask)
    qsel = q_values(net, p_on if c.dq else p_tg, sp)
    return pr["kink"], pr["pool"], LR._gap(np.concatenate(qsel) if c.T else qsel)


def margins_ok(c, seed=None, k=2.0):
    D = rec_data(c, seed) if c.T else ff_data(c, seed)
    for _, p, batch, _ in trajectory(c, D):
        km, pm, gap = margins(c, D.net, p, D.p_tg, batch)
        if not (km > k * RELU_MARGIN and pm > k * RELU_MARGIN and gap > k * GAP):
            return False
    return True


def find_seed(c, cap=64):
    """the smallest seed that keeps twice the margins along the case's fp64 trajectory (how the table's seeds were chosen, on the CPU, with this module alone)"""
    for seed in range(1, cap):
        if margins_ok(c, seed):
            return seed
    raise AssertionError(f"{c.name}: no seed below {cap} keeps the margins")


_PREPARED = {}


def prepare(c):
    """the case's data, computed once and shared: asserts the margins on the first step (the GPU test asserts them again on every step it runs, on the engine's own parameters)"""
    if c.name not in _PREPARED:
        D = rec_data(c) if c.T else ff_data(c)
        _, p, batch, _ = next(trajectory(c, D))
        km, pm, gap = margins(c, D.net, p, D.p_tg, batch)
        assert km > RELU_MARGIN and pm > RELU_MARGIN and gap > GAP, (c.name, km, pm, gap)
        _PREPARED[c.name] = D
    return _PREPARED[c.name]


def activations(net):
    """[(descriptor index, code)] of the network's Activation layers, in the engine's layer numbering"""
    return [(i, d.act) for i, d in enumerate(nn.lower(net)[0]) if d.kind == 14]
