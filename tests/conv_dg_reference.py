"""fp64 reference of ONE batch_train! for networks with a dilated, grouped or depthwise convolution -- nn.Conv(...; dilation, groups), nn.DepthwiseConv (TEST INFRASTRUCTURE: layer
kind 15, csrc/conv_own.hip) --, feed-forward (src/solver.jl:191-236) and recurrent (src/solver.jl:239-287), over the package's nn descriptors.

The law of the layer (Flux 0.14 over NNlib, recalled): output channel n of group j = n ÷ (cout/g) reads input channels [j cin/g, (j + 1) cin/g); tap (ky, kx) of the FLIPPED
kernel reads iy = oy sh + ky dh - ph, ix = ox sw + kx dw - pw of the zero-extended map.

Two legs of the layer that share no conv code:
  * "torch"  torch.nn.functional.conv2d(dilation=, groups=, padding=) on the flipped kernel under float64 autograd;
  * "numpy"  a hand-written NumPy forward (one strided slice of the np.pad-ed map per tap, one matrix product per group) and backward (dW per tap, dX scattered into the padded
             map and cropped), entered into the graph as a torch.autograd.Function.
Everything that is no such convolution -- Dense, the plain and padded Conv, pools, GroupNorm, Activation, SkipConnection, LSTM, the dueling join, the Huber loss, the batches,
Adam, the margins, the gradient and parameter checks and their constants -- is step_reference's and activation_layer_reference's: a leg of this module overrides the "conv"
entry of step_reference's table of laws and nothing else, so no law is restated and no tolerance is introduced here.

WRONG ENGINES (tests/test_conv_dg_cpu.py, "the tests can tell"): legs that make one plausible mistake each -- the dilation ignored, the groups ignored (a dense conv whose
off-block weights are not zero), the group-to-channel map interleaved, the dX validity test without the dilation.

expand() / expand_params(): the exact companion -- the groups = 1, dilation = 1 network whose conv holds the zero-stuffed, block-diagonal kernel."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

import activation_layer_reference as AL
import step_reference as S
from activation_layer_reference import (GAP, GRAD_C, GRAD_RTOL, LRATE, RELU_MARGIN, TOL_GN, TOL_LOSS, TOL_Q, TOL_TD, Adam, blocks, check_grads, check_params, ff_batch, ff_data,      # noqa: F401
                                        legs_agree, rec_data)

nn = AL.nn
F64 = torch.float64
WRONG = ("no_dilation", "dense_groups", "interleaved", "dx_no_dilation")


def out_hw(l, h, w):
    return (h + 2 * l.ph - (l.kh - 1) * l.dh - 1) // l.sh + 1, (w + 2 * l.pw - (l.kw - 1) * l.dw - 1) // l.sw + 1


# ------------------------------------------------------------------ the torch leg, and the wrong engines that are expressible in torch
def conv_torch(x, W, b, l, mode="torch"):
    """W (cout, cin/g, kh, kw), un-flipped: a true convolution is the cross-correlation with the flipped kernel"""
    Wf = W.flip(2, 3); g = l.groups; ng = l.cout // g
    oh, ow = out_hw(l, x.shape[2], x.shape[3])
    if mode == "no_dilation":      # the taps of the undilated kernel on the layer's own output geometry (what the shim did: the dilation dropped)
        return F.conv2d(x, Wf, b, stride=(l.sh, l.sw), padding=(l.ph, l.pw), groups=g)[:, :, :oh, :ow]
    if mode == "dense_groups":      # groups ignored: every output channel reads every input channel.  Block (jo, ji) of the dense kernel is group ji's own block: the diagonal
        row = torch.cat([Wf[ji * ng:(ji + 1) * ng] for ji in range(g)], dim=1)      # is the layer's, the off-block weights are weights too, not zeros
        return F.conv2d(x, torch.cat([row] * g, dim=0), b, stride=(l.sh, l.sw), padding=(l.ph, l.pw), dilation=(l.dh, l.dw))
    if mode == "interleaved":      # output channel n reads group n % g instead of n ÷ (cout/g)
        sigma = torch.tensor([(m % ng) * g + m // ng for m in range(l.cout)])
        y = F.conv2d(x, Wf[sigma], b[sigma], stride=(l.sh, l.sw), padding=(l.ph, l.pw), dilation=(l.dh, l.dw), groups=g)
        return y[:, torch.argsort(sigma)]
    return F.conv2d(x, Wf, b, stride=(l.sh, l.sw), padding=(l.ph, l.pw), dilation=(l.dh, l.dw), groups=g)


# ------------------------------------------------------------------ the NumPy leg: hand-written forward and backward
def _tap(l, xp, ky, kx, oh, ow, dh, dw):
    return xp[:, :, ky * dh:ky * dh + l.sh * (oh - 1) + 1:l.sh, kx * dw:kx * dw + l.sw * (ow - 1) + 1:l.sw]


def conv_np_forward(l, x, W, b):
    B, _, H, Wd = x.shape; g = l.groups; cg, ng = l.cin // g, l.cout // g
    oh, ow = out_hw(l, H, Wd)
    xp = np.pad(x, ((0, 0), (0, 0), (l.ph, l.ph), (l.pw, l.pw))); Wf = W[:, :, ::-1, ::-1]
    y = np.zeros((B, l.cout, oh, ow))
    for ky in range(l.kh):
        for kx in range(l.kw):
            xs = _tap(l, xp, ky, kx, oh, ow, l.dh, l.dw)
            for j in range(g):
                y[:, j * ng:(j + 1) * ng] += np.einsum("bchw,oc->bohw", xs[:, j * cg:(j + 1) * cg], Wf[j * ng:(j + 1) * ng, :, ky, kx])
    return y + b.reshape(1, -1, 1, 1)


def conv_np_backward(l, x, W, dy, dx_dilation=True):
    """-> dX, dW, db.  dx_dilation = False: the wrong engine whose input gradient places tap (ky, kx) at (ky, kx) instead of (ky dh, kx dw)"""
    B, _, H, Wd = x.shape; g = l.groups; cg, ng = l.cin // g, l.cout // g
    oh, ow = dy.shape[2:]
    xp = np.pad(x, ((0, 0), (0, 0), (l.ph, l.ph), (l.pw, l.pw))); Wf = W[:, :, ::-1, ::-1]
    dxp = np.zeros_like(xp); dWf = np.zeros_like(Wf)
    ddh, ddw = (l.dh, l.dw) if dx_dilation else (1, 1)
    for ky in range(l.kh):
        for kx in range(l.kw):
            xs = _tap(l, xp, ky, kx, oh, ow, l.dh, l.dw); dst = _tap(l, dxp, ky, kx, oh, ow, ddh, ddw)
            for j in range(g):
                d = dy[:, j * ng:(j + 1) * ng]
                dWf[j * ng:(j + 1) * ng, :, ky, kx] = np.einsum("bohw,bchw->oc", d, xs[:, j * cg:(j + 1) * cg])
                dst[:, j * cg:(j + 1) * cg] += np.einsum("bohw,oc->bchw", d, Wf[j * ng:(j + 1) * ng, :, ky, kx])
    return dxp[:, :, l.ph:l.ph + H, l.pw:l.pw + Wd], dWf[:, :, ::-1, ::-1].copy(), dy.sum(axis=(0, 2, 3))


class _ConvNumpy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, l, dx_dilation):
        xn, Wn = x.detach().numpy(), W.detach().numpy()
        ctx.saved = (xn, Wn, l, dx_dilation)
        return torch.tensor(conv_np_forward(l, xn, Wn, b.detach().numpy()), dtype=F64)

    @staticmethod
    def backward(ctx, dy):
        xn, Wn, l, dx_dilation = ctx.saved
        dx, dW, db = conv_np_backward(l, xn, Wn, dy.numpy(), dx_dilation)
        return torch.tensor(dx), torch.tensor(dW), torch.tensor(db), None, None


def _general_only(mode):
    """a wrong engine is wrong at the general layer only"""
    return lambda x, W, b, l: _ConvNumpy.apply(x, W, b, l, False) if (mode == "dx_no_dilation" and l.general) else conv_torch(x, W, b, l, mode if l.general else "torch")


def _numpy(l, x, a, cx):
    """the hand-written forward and backward for every Conv of the chain, general or not; a SkipConnection block (which holds no general conv) stays with conv_torch"""
    return conv_torch(x, a[0], a[1], l) if cx.inner else _ConvNumpy.apply(x, a[0], a[1], l, True)


# the legs: overrides of step_reference's "conv" entry (which is conv_torch)
LEGS = {"torch": {}, "numpy": {"conv": _numpy}} | {w: {"conv": S.conv_law(_general_only(w))} for w in WRONG}


def trajectory(c, D=None, steps=AL.STEPS, seed=None, leg="torch"):
    """activation_layer_reference.trajectory under this module's legs"""
    return AL.trajectory(c, D, steps, seed, LEGS[leg])


# everything else is activation_layer_reference's as it stands: the default leg of both modules is step_reference's table
q_values, probe_of, margins, margins_ok, find_seed, STEPS = AL.q_values, AL.probe_of, AL.margins, AL.margins_ok, AL.find_seed, AL.STEPS
ff_step, rec_step = S.bound(S.ff_step, LEGS, "leg"), S.bound(S.rec_step, LEGS, "leg")
prepare = functools.partial(AL.prepare, cache={})


# ------------------------------------------------------------------ the exact companion: the kind-1 network on the zero-stuffed, block-diagonal kernel
def general_layers(net):
    """[(index into nn.all_layers, layer)] of the network's general convolutions"""
    return [(i, l) for i, l in enumerate(nn.all_layers(net)) if l.kind == "conv" and l.general]


def _expanded(l):
    return nn.Conv(((l.kh - 1) * l.dh + 1, (l.kw - 1) * l.dw + 1), l.cin, l.cout, l.act, (l.sh, l.sw), (l.ph, l.pw)) if l.kind == "conv" and l.general else l


def expand(net):
    """the same network with every general Conv replaced by Conv(((kh-1) dh + 1, (kw-1) dw + 1), cin => cout; stride, pad) (general convs stand in a base chain, never in a block)"""
    if isinstance(net, nn.DuelingNetwork):
        return nn.DuelingNetwork(nn.Chain(*[_expanded(l) for l in net.base.layers]), net.val, net.adv)
    return nn.Chain(*[_expanded(l) for l in net.layers])


def _segments(net):
    out, off = [], 0
    for l in nn.all_layers(net):
        segs = []
        for shp in l.shapes():
            k = int(np.prod(shp)); segs.append((off, shp)); off += k
        out.append(segs)
    return out, off


def live_index(net):
    """per layer of nn.all_layers(net): (slice of the layer's W in the flat vector of `net`, the flat positions of the same weights in the flat vector of expand(net))"""
    a, _ = _segments(net); b, _ = _segments(expand(net)); out = {}
    for i, l in general_layers(net):
        (o0, shp), (o1, shp1) = a[i][0], b[i][0]
        cg, ng = l.cin // l.groups, l.cout // l.groups
        co, ci, ky, kx = np.meshgrid(np.arange(l.cout), np.arange(cg), np.arange(l.kh), np.arange(l.kw), indexing="ij")
        pos = np.ravel_multi_index((co, (co // ng) * cg + ci, ky * l.dh, kx * l.dw), shp1)      # un-flipped indices: the flip maps tap ky d of the flipped extent to ky d here
        out[i] = (slice(o0, o0 + int(np.prod(shp))), o1 + pos.reshape(-1))
    return out


def expand_params(net, p):
    """the flat parameters of expand(net) that compute the same function: the layer's weights at the live taps, exact zeros elsewhere; every other array as it is"""
    a, _ = _segments(net); b, n1 = _segments(expand(net)); live = live_index(net)
    q = np.zeros(n1, np.asarray(p).dtype)
    for i, (sa, sb) in enumerate(zip(a, b)):
        for j, ((o0, shp), (o1, shp1)) in enumerate(zip(sa, sb)):
            k = int(np.prod(shp))
            if i in live and j == 0:
                q[live[i][1]] = p[o0:o0 + k]
            else:
                q[o1:o1 + k] = p[o0:o0 + k]
    return q


def contract_grads(net, g1):
    """the flat gradient of expand(net) read at the positions `net` has: dW of a general conv at its live taps, everything else as it is"""
    a, n0 = _segments(net); b, _ = _segments(expand(net)); live = live_index(net)
    g = np.zeros(n0, g1.dtype)
    for i, (sa, sb) in enumerate(zip(a, b)):
        for j, ((o0, shp), (o1, shp1)) in enumerate(zip(sa, sb)):
            k = int(np.prod(shp))
            g[o0:o0 + k] = g1[live[i][1]] if (i in live and j == 0) else g1[o1:o1 + k]
    return g


# ------------------------------------------------------------------ the case table: 6x6 .. 9x9 maps, the smallest shapes at which the index arithmetic of conv_own.hip can go wrong
def case(name, mk, B, obs, nA=4, dueling=False, u8=0, T=0, seed=1, pscale=2.0, wrong=()):
    """wrong: the wrong engines that apply to the case (each must land >= 100 tolerances off)"""
    return types.SimpleNamespace(name=name, mk=mk, B=B, obs=tuple(obs), nA=nA, dueling=dueling, dq=1, prio=0 if T else 1, u8=u8, mfma=1, T=T, seed=seed, gamma=0.95, pscale=pscale,
                                 wrong=tuple(wrong), plain=None, codes=())


C, DW, D, A = nn.Conv, nn.DepthwiseConv, nn.Dense, nn.Activation
RELU, TANH, SIG = nn.relu, nn.tanh, nn.sigmoid
# seeds: found with find_seed on the CPU, with this module alone (tests/test_conv_dg_cpu.py re-runs the search); fixed here
SEEDS = {"dw_4to8_pad_b32": 2, "u8_dil2": 12}
_c = lambda name, mk, B, obs, **kw: case(name, mk, B, obs, seed=SEEDS.get(name, 1), **kw)


def _table():
    t = []
    # dilation 2 on 7x7 -> 3x3, B = 5: ten columns, the one-column walk, the target pass starts at column 5.  K = 9: the thin kernels
    t.append(_c("dil2_b5", lambda: nn.Chain(C(3, 1, 4, RELU, dilation=2), D(36, 4)), 5, (1, 7, 7), wrong=("no_dilation",)))
    # kernel (3, 2), dilation (2, 1), stride (2, 1), pad (2, 0) on 9x6 -> 5x5, behind a 1x1 conv: the dX validity test with stride, dilation and pad on one axis
    t.append(_c("rect_aniso", lambda: nn.Chain(C(1, 1, 2, TANH), C((3, 2), 2, 4, RELU, stride=(2, 1), pad=(2, 0), dilation=(2, 1)), D(100, 4)), 16, (1, 9, 6),
                wrong=("no_dilation", "dx_no_dilation")))
    # "same": k = 3, dilation 2, pad 2 on 6x6 -> 6x6, behind a conv: every border tap
    t.append(_c("same_dil2", lambda: nn.Chain(C(1, 1, 2, TANH), C(3, 2, 4, RELU, pad=nn.SamePad(), dilation=2), D(144, 4)), 16, (1, 6, 6), wrong=("no_dilation", "dx_no_dilation")))
    # groups = 2, 4 => 6: three channels per group, no tile; K = 18: the VALU form
    t.append(_c("groups2_4to6", lambda: nn.Chain(C(3, 4, 6, RELU, groups=2), D(96, 4)), 16, (4, 6, 6), wrong=("dense_groups", "interleaved")))
    # depthwise 4 => 4, and 4 => 8 (multiplier 2) with pad 1, at B = 5 (one column at a time) and 32 (16-byte accesses)
    t.append(_c("dw_4to4", lambda: nn.Chain(DW(3, 4, 4, RELU), D(64, 4)), 32, (4, 6, 6), wrong=("dense_groups",)))
    t.append(_c("dw_4to8_pad_b5", lambda: nn.Chain(DW(3, 4, 8, TANH, pad=1), D(288, 4)), 5, (4, 6, 6), wrong=("dense_groups", "interleaved")))
    t.append(_c("dw_4to8_pad_b32", lambda: nn.Chain(C(1, 4, 4, TANH), DW(3, 4, 8, RELU, pad=1), D(288, 4)), 32, (4, 6, 6), wrong=("dense_groups", "interleaved")))
    # the MFMA forms: groups = 2 on 32 => 32 (16 channels per group), dilation 2 on 16 => 16, B = 32, each behind a conv (the MFMA dX).  Smooth activations: thousands of
    # relu units per step leave no seed with every unit off its kink (tests/conv_pad_reference.py, stack_same)
    t.append(_c("mfma_groups2", lambda: nn.Chain(C(3, 1, 32, TANH), C(3, 32, 32, SIG, groups=2), D(128, 4)), 32, (1, 6, 6), wrong=("dense_groups", "interleaved")))
    t.append(_c("mfma_dil2", lambda: nn.Chain(C(3, 1, 16, TANH), C(3, 16, 16, SIG, pad=2, dilation=2), D(400, 4)), 32, (1, 7, 7), wrong=("no_dilation", "dx_no_dilation")))
    # first layer on a u8 replay, with dilation: the byte arena (cout 16, K = 36: the MFMA forms read bytes)
    t.append(_c("u8_dil2", lambda: nn.Chain(C(3, 4, 16, RELU, pad=2, dilation=2), D(576, 4)), 32, (4, 6, 6), u8=1, pscale=1.0, wrong=("no_dilation",)))
    # behind a MaxPool: 8x8 -> 4x4 -> dilation 2 with pad 1 -> 2x2.  (the 1x1 conv in front has no activation: a tanh at this weight scale saturates, and the top two taps of
    # a window then lie 1e-10 apart -- no seed keeps the MaxPool margin)
    t.append(_c("behind_maxpool", lambda: nn.Chain(C(1, 1, 2), nn.MaxPool(2), C(3, 2, 4, RELU, pad=1, dilation=2), D(16, 4)), 16, (1, 8, 8), wrong=("no_dilation", "dx_no_dilation")))
    # the depthwise-separable stem: DepthwiseConv -> Conv 1x1 -> GroupNorm
    t.append(_c("separable_gn", lambda: nn.Chain(DW(3, 4, 4, pad=1), C(1, 4, 8), nn.GroupNorm(8, 2, RELU), D(288, 4)), 16, (4, 6, 6), wrong=("dense_groups",)))
    # in front of an Activation(gelu)
    t.append(_c("before_gelu", lambda: nn.Chain(C(3, 2, 4, groups=2, dilation=2), A(nn.gelu), D(16, 4)), 16, (2, 6, 6), wrong=("no_dilation", "dense_groups", "interleaved")))
    # as the entry P of a convolutional skip block
    t.append(_c("skip_entry", lambda: nn.Chain(C(3, 2, 4, TANH, pad=2, dilation=2, groups=2),
                                               nn.SkipConnection(nn.Chain(C(3, 4, 4, RELU, pad=1), C(3, 4, 4, pad=1)), "+"), D(144, 4)), 16, (2, 6, 6), pscale=1.0,
                wrong=("no_dilation", "dense_groups", "interleaved")))
    # dueling, the layer in the base chain
    t.append(_c("dueling", lambda: nn.create_dueling_network(nn.Chain(C(1, 2, 2, TANH), C(3, 2, 4, RELU, dilation=2, groups=2), D(16, 8, RELU), D(8, 4))), 16, (2, 6, 6), dueling=True,
                wrong=("no_dilation", "dense_groups", "interleaved", "dx_no_dilation")))
    return t


def _rec_table():
    # Conv(dilation = 2) -> LSTM, T = 3, B = 4: the layer runs once over the T B = 12 columns
    return [_c("rec_dil2_lstm", lambda: nn.Chain(C(3, 1, 4, RELU, dilation=2), nn.LSTM(36, 8), D(8, 3)), 4, (1, 7, 7), nA=3, T=3, pscale=3.0, wrong=("no_dilation",))]


CASES, REC_CASES = _table(), _rec_table()
BY_NAME = {c.name: c for c in CASES + REC_CASES}
assert len(BY_NAME) == len(CASES) + len(REC_CASES)


def general_descs(net):
    """[descriptor index] of the network's kind-15 layers, in the engine's layer numbering"""
    return [i for i, d in enumerate(nn.lower(net)[0]) if d.kind == 15]
