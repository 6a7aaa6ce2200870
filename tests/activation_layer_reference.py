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
import groupnorm_reference as GR
import layernorm_reference as LR
import recurrent_reference as R
import step_reference as S
from feedforward_edges_common import GAP, TOL_GN, TOL_LOSS, TOL_Q, TOL_TD      # noqa: F401  (one set of constants)
from feedforward_reference import GRAD_C, GRAD_RTOL, RELU_MARGIN, Adam, check_params      # noqa: F401
from step_reference import blocks, check_grads, ff_batch, ff_data, legs_agree, rec_data      # noqa: F401

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


LEGS = {"torch": {}, "numpy": {"activation": S.activation_law(_ActNumpy.apply)}}


# ------------------------------------------------------------------ the observers, and the step (step_reference's, bound to the legs)
def _kink(probe, x, a, cx):
    for k in KINKS.get(a, ()):
        probe["kink"] = min(probe["kink"], GR._min((S.kept(cx, x.detach()) - k).abs()))


def _see_input(probe, l, x, cx):
    if l.kind == "activation":
        _kink(probe, x, l.code, cx)
    elif l.kind == "maxpool":
        probe["pool"] = min(probe["pool"], GR._pool_gap(l, S.kept(cx, x.detach()), cx.relu))


# "kink": the smallest distance of an Activation layer's input, or of a fused layer's pre-activation, from a kink of its σ; "pool": the MaxPool margin
OBSERVERS = {"in": _see_input, "pre": lambda probe, l, pre, cx: _kink(probe, pre, l.act, cx)}


def new_probe():
    return S.Probe(OBSERVERS, kink=np.inf, pool=np.inf)


q_values = S.bound(S.q_values, LEGS, "leg", "probe", "mask")
ff_step, rec_step = S.bound(S.ff_step, LEGS, "leg"), S.bound(S.rec_step, LEGS, "leg")


def probe_of(net, p, s, mask=None):
    return S.probed(new_probe(), q_values, net, p, s, mask=mask)


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
    # 4. the post-add relu of ResNet-v1, the reason for the layer: on vectors (skip.hip) and on maps (conv_own.hip epilogues)
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


find_seed = lambda c, cap=64: S.find_seed(c, margins_ok, cap)


_PREPARED = {}


def prepare(c, cache=_PREPARED):
    """the case's data, computed once and shared: asserts the margins on the first step (the GPU test asserts them again on every step it runs, on the engine's own parameters)"""
    if c.name not in cache:
        D = rec_data(c) if c.T else ff_data(c)
        _, p, batch, _ = next(trajectory(c, D))
        km, pm, gap = margins(c, D.net, p, D.p_tg, batch)
        assert km > RELU_MARGIN and pm > RELU_MARGIN and gap > GAP, (c.name, km, pm, gap)
        cache[c.name] = D
    return cache[c.name]


def activations(net):
    """[(descriptor index, code)] of the network's Activation layers, in the engine's layer numbering"""
    return [(i, d.act) for i, d in enumerate(nn.lower(net)[0]) if d.kind == 14]
