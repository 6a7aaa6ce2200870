"""fp64 reference of ONE batch_train! for networks with Flux GroupNorm layers (TEST INFRASTRUCTURE), feed-forward (src/solver.jl:191-236) and recurrent
(src/solver.jl:239-287), over the package's nn descriptors: Conv (padded or not), MaxPool / MeanPool, convolutional SkipConnection(+) blocks, GroupNorm, Dense and
LSTM, plain or dueling.

The law (Flux 0.14 `_norm_layer_forward`; recalled, not executed): per sample and group of chs / G contiguous channels, over the group's n_g = (chs / G) * h * w elements,
mu = mean(x), var = mean((x - mu)^2), y = act(gamma_ch * (x - mu) / sqrt(var + eps) + beta_ch) -- eps INSIDE the root.  Flux.params: beta, THEN gamma.
torch.nn.functional.group_norm computes exactly this law (biased variance, sqrt(var + eps), contiguous groups): an independent second leg.

Legs:
  * "torch"   float64 autograd with F.group_norm;
  * "numpy"   the same step with every GroupNorm layer replaced by a hand-written NumPy forward and backward (gn_forward_np / gn_backward_np), entered into the graph
              as a torch.autograd.Function;
  * "ln_law"  the OTHER law, (x - mu) / (sigma + eps) as LayerNorm's `normalise` has it: only the tell-apart test of test_groupnorm_cpu calls it.
tests/test_groupnorm_cpu.py holds the first two to 1e-10 of each other on every case and checks the hand-written gradient against central differences.

Everything but the layer -- the walker and the step, the constants, the cells, the batches, the gradient check per block, the fp64 Adam -- is that of step_reference /
layernorm_reference / recurrent_reference / feedforward_edges_common, imported, not restated.  No tolerance is introduced here.

Data rule: beside the relu margin and the argmax gap, every non-degenerate group keeps sqrt(var) >= SIGMA_MIN (the LayerNorm table's value; a group that is identically
0 -- case dead_group -- is degenerate on purpose), and every MaxPool window keeps its top-two gap above RELU_MARGIN unless its maximum is an exact 0 out of a relu.
Seeds are fixed in the table and were found with this module alone (find_seed), on the CPU."""
import types

import numpy as np
import torch
import torch.nn.functional as F

import layernorm_reference as LR
import recurrent_reference as R
import step_reference as S
from gru_reference import param_arrays      # noqa: F401
from layernorm_reference import GAP, GRAD_C, GRAD_RTOL, RELU_MARGIN, SIGMA_MIN, TOL_GN, TOL_LOSS, TOL_Q, TOL_TD, Adam, check_params      # noqa: F401  (one set of constants)
from step_reference import _gap, _t64, blocks, check_grads, dead_blocks, ff_batch, legs_agree      # noqa: F401

nn = LR.nn
F64 = torch.float64
LRATE = LR.LR
GN_R = 64      # rows per chunk of csrc/groupnorm.hip (GN_R, common.h): the table's chunk cases are built around it


# ------------------------------------------------------------------ the layer
def _sigma(x, G):
    B = x.shape[0]
    return x.reshape(B, G, -1).var(dim=2, unbiased=False).sqrt()


def gn_torch(x, beta, gamma, G, eps):
    """x (B, C, H, W) -> the pre-activation under Flux's law, by torch's own group_norm"""
    return F.group_norm(x, G, gamma, beta, eps)


def gn_ln_law(x, beta, gamma, G, eps):
    """the OTHER law: eps added to sigma outside the root (LayerNorm's `normalise`)"""
    B, C = x.shape[0], x.shape[1]
    xg = x.reshape(B, G, -1); mu = xg.mean(dim=2, keepdim=True)
    sg = ((xg - mu) ** 2).mean(dim=2, keepdim=True).sqrt()
    return gamma.reshape(1, C, 1, 1) * ((xg - mu) / (sg + eps)).reshape(x.shape) + beta.reshape(1, C, 1, 1)


def gn_forward_np(x, beta, gamma, G, eps):
    """NumPy: x (B, C, H, W) -> pre-activation, cache"""
    B, C = x.shape[0], x.shape[1]
    xg = x.reshape(B, G, -1); n = xg.shape[2]
    mu = xg.sum(axis=2, keepdims=True) / n
    d = xg - mu
    var = (d * d).sum(axis=2, keepdims=True) / n
    r = 1.0 / np.sqrt(var + eps)
    xh = (d * r).reshape(x.shape)
    return gamma.reshape(1, C, 1, 1) * xh + beta.reshape(1, C, 1, 1), (xh, r, gamma, G)


def gn_backward_np(cache, dy):
    """dy = dL/d(pre-activation) -> dx, dbeta, dgamma.  With g = dy * gamma_ch, per sample and group:  dx = r (g - mean g - x_hat mean(g x_hat))
    (d x_hat_j / d var = -x_hat_j r^2 / 2 and d var / d x_i = 2 (x_i - mu) / n = 2 x_hat_i / (n r))"""
    xh, r, gamma, G = cache
    B, C = dy.shape[0], dy.shape[1]
    g = (dy * gamma.reshape(1, C, 1, 1)).reshape(B, G, -1); xg = xh.reshape(B, G, -1)
    dx = r * (g - g.mean(axis=2, keepdims=True) - xg * (g * xg).mean(axis=2, keepdims=True))
    return dx.reshape(dy.shape), dy.sum(axis=(0, 2, 3)), (dy * xh).sum(axis=(0, 2, 3))


class _GnNumpy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, beta, gamma, G, eps):
        y, cache = gn_forward_np(x.detach().numpy(), beta.detach().numpy(), gamma.detach().numpy(), G, eps)
        ctx.cache = cache
        return torch.tensor(y, dtype=F64)

    @staticmethod
    def backward(ctx, dy):
        dx, db, dg = gn_backward_np(ctx.cache, dy.numpy())
        return torch.tensor(dx), torch.tensor(db), torch.tensor(dg), None, None


LEGS = {"torch": {}, "numpy": {"groupnorm": S.groupnorm_law(_GnNumpy.apply)}, "ln_law": {"groupnorm": S.groupnorm_law(gn_ln_law)}}


# ------------------------------------------------------------------ the observers, and the step (step_reference's, bound to the legs)
def _pool_gap(l, x, relu_out):
    """the smallest top-two gap over the MaxPool windows of x, except windows whose maximum is an exact 0 out of a relu (feedforward_reference.margins' rule)"""
    if l.kh * l.kw == 1 or not x.numel():      # (no column: a time step of a recurrent batch whose every column is padding)
        return np.inf
    t = F.unfold(x.reshape(-1, 1, x.shape[2], x.shape[3]), (l.kh, l.kw), stride=(l.sh, l.sw)).sort(dim=1).values
    gap = t[:, -1] - t[:, -2]
    if relu_out:
        gap = torch.where(t[:, -1] == 0.0, torch.full_like(gap, np.inf), gap)
    return float(gap.min())


def _min(t):
    return float(t.min()) if t.numel() else np.inf


def _see_input(probe, l, x, cx):
    if l.kind == "maxpool":
        probe["pool"] = min(probe["pool"], _pool_gap(l, x.detach(), cx.relu))
    elif l.kind == "groupnorm":
        sg = S.kept(cx, _sigma(x.detach(), l.G)); dead = sg == 0.0
        probe["dead"] += int(dead.sum())
        if (~dead).any():
            probe["sigma"] = min(probe["sigma"], _min(sg[~dead]))


def _see_relu(probe, l, pre, cx):
    if l.act == nn.relu:
        probe["relu"] = min(probe["relu"], _min(S.kept(cx, pre.detach()).abs()))


# "sigma": the smallest sqrt(var) over the non-degenerate groups, "dead": the number of degenerate ones, "relu" / "pool": the relu and MaxPool margins
OBSERVERS = {"in": _see_input, "pre": _see_relu}


def new_probe():
    return S.Probe(OBSERVERS, sigma=np.inf, relu=np.inf, pool=np.inf, dead=0)


q_values = S.bound(S.q_values, LEGS, "leg", "probe", "mask")
ff_step, rec_step = S.bound(S.ff_step, LEGS, "leg"), S.bound(S.rec_step, LEGS, "leg")


def probe_of(net, p, s, mask=None):
    return S.probed(new_probe(), q_values, net, p, s, mask=mask)


# ------------------------------------------------------------------ the case table
def _net(gn):
    """Conv(3, 1 => 4, relu) -> gn -> Dense on the (4, 4, 4) map of a 6x6 observation"""
    return lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu), gn(), nn.flattenbatch, nn.Dense(64, 4))


def _block():
    return nn.SkipConnection(nn.Chain(nn.Conv(3, 4, 4, nn.relu, pad=1), nn.Conv(3, 4, 4, pad=1)), "+")


def case(name, mk, B, obs=(1, 6, 6), nA=4, dueling=False, dq=1, prio=0, u8=0, mfma=1, T=0, seed=1, pscale=1.0, dead=0, c0scale=1.0):
    """dead: the number of leading conv channels of layer 0 whose kernel is 0 and whose bias is -1 in both networks (their relu output is identically 0).  pscale: the
    glorot draw is multiplied by it; c0scale: the kernel of layer 0 (a Conv) is multiplied by it in both networks -- [0, 1) observations (u8 replay, the recurrent tables'
    episodes) through glorot weights give a map of sigma ~0.03, and the layer's output does not depend on the scale of its input"""
    return types.SimpleNamespace(name=name, mk=mk, B=B, obs=tuple(obs), nA=nA, dueling=dueling, dq=dq, prio=prio, u8=u8, mfma=mfma, T=T, seed=seed, gamma=0.95, pscale=pscale, dead=dead, c0scale=c0scale)


_duel = lambda: nn.create_dueling_network(nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.GroupNorm(4, 2, nn.relu), nn.flattenbatch, nn.Dense(64, 16, nn.relu), nn.Dense(16, 4)))
CASES = [
    case("g2_b5", _net(lambda: nn.GroupNorm(4, 2, nn.relu)), 5, seed=1),                # ten columns: the one-column path; n_g = 32
    case("g1", _net(lambda: nn.GroupNorm(4, 1)), 8, seed=1),                             # one group: LayerNorm over the whole map; the four-column path
    case("gc", _net(lambda: nn.GroupNorm(4, 4)), 8, seed=1),                             # instance normalisation: n_g = h * w
    # n_g = 2 R + 3 = 131 (a prime: 131 channels per group on a 1x1 map): three chunks with a ragged last one, a channel boundary at every row; both column paths
    case("chunks_b5", lambda: nn.Chain(nn.Conv(3, 1, 262, nn.relu), nn.GroupNorm(262, 2), nn.flattenbatch, nn.Dense(262, 4)), 5, obs=(1, 3, 3), seed=1),
    case("chunks_b8", lambda: nn.Chain(nn.Conv(3, 1, 262, nn.relu), nn.GroupNorm(262, 2), nn.flattenbatch, nn.Dense(262, 4)), 8, obs=(1, 3, 3), seed=4),
    # n_g = R - 1 = 63 = 7 channels x (3 x 3): the single-chunk case, channel boundaries inside it
    case("one_chunk", lambda: nn.Chain(nn.Conv(3, 1, 14, nn.relu), nn.GroupNorm(14, 2, nn.relu), nn.flattenbatch, nn.Dense(126, 4)), 8, obs=(1, 5, 5), seed=1),
    # h * w = 15 (a 3 x 5 map): neither a multiple of 4 nor of 16; the per-channel gamma / beta index
    case("hw_odd", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.GroupNorm(4, 2, nn.relu), nn.flattenbatch, nn.Dense(60, 4)), 8, obs=(1, 5, 7), seed=1),
    case("eps_half", _net(lambda: nn.GroupNorm(4, 2, eps=0.5)), 8, seed=1),              # sqrt(var + eps) against sigma + eps
    case("dead_group", _net(lambda: nn.GroupNorm(4, 2, nn.leakyrelu)), 8, seed=1, dead=2),      # group 0 is identically 0: y = act(beta_ch) exactly, every gradient finite
    case("behind_pool", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.MaxPool(2), nn.GroupNorm(4, 2, nn.relu), nn.flattenbatch, nn.Dense(36, 4)), 8, obs=(1, 8, 8), seed=1),
    case("behind_cpad", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu, pad=1), nn.GroupNorm(4, 2, nn.relu), nn.flattenbatch, nn.Dense(144, 4)), 8, seed=1),
    case("behind_block", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu), _block(), nn.GroupNorm(4, 2, nn.relu), nn.flattenbatch, nn.Dense(64, 4)), 8, seed=1),
    case("gn_gn", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.GroupNorm(4, 2, nn.relu), nn.GroupNorm(4, 1), nn.flattenbatch, nn.Dense(64, 4)), 8, seed=1),
    case("then_conv", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.GroupNorm(4, 2), nn.Conv(3, 4, 4, nn.relu), nn.flattenbatch, nn.Dense(64, 4)), 8, obs=(1, 8, 8), seed=1),
    case("then_pool", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.GroupNorm(4, 2, nn.relu), nn.MeanPool(2), nn.flattenbatch, nn.Dense(36, 4)), 8, obs=(1, 8, 8), seed=1),
    case("then_block", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.GroupNorm(4, 2), _block(), nn.flattenbatch, nn.Dense(64, 4)), 8, seed=1),
    case("act_tanh", _net(lambda: nn.GroupNorm(4, 2, nn.tanh)), 8, seed=1),
    case("act_leakyrelu", _net(lambda: nn.GroupNorm(4, 2, nn.leakyrelu)), 8, seed=1),
    case("dueling", _duel, 8, dueling=True, prio=1, seed=1),                            # the head schedules; IS weights from unequal priorities
    case("u8", _duel, 8, dueling=True, prio=1, u8=1, seed=3, c0scale=10.0),               # a u8 replay in front of the layer (it always reads floats)
    case("valu", _net(lambda: nn.GroupNorm(4, 2, nn.relu)), 8, mfma=0, seed=1),
    case("b32", _net(lambda: nn.GroupNorm(4, 2, nn.relu)), 32, seed=1),
]
REC_CASES = [
    case("then_lstm", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.GroupNorm(4, 2, nn.relu), nn.flattenbatch, nn.LSTM(64, 8), nn.Dense(8, 3)), 4, nA=3, T=3, seed=1, c0scale=10.0),
]
BY_NAME = {c.name: c for c in CASES + REC_CASES}
assert len(BY_NAME) == len(CASES) + len(REC_CASES)


def _kill(c, net, p):
    """case.c0scale, then case.dead: kernel 0 and bias -1 on the leading conv channels of layer 0"""
    l0 = nn.all_layers(net)[0]; per = l0.cin * l0.kh * l0.kw; nw = l0.cout * per
    p[:nw] *= np.float32(c.c0scale)
    if c.dead:
        p[:c.dead * per] = 0.0; p[nw:nw + c.dead] = -1.0
    return p


def _data(data):
    """layernorm_reference's data of a case, plus the case's c0scale and dead channels"""
    def make(c, seed=None):
        D = data(c, seed)
        _kill(c, D.net, D.p_on); _kill(c, D.net, D.p_tg)
        return D
    return make


ff_data, rec_data = _data(S.ff_data), _data(S.rec_data)


def case_margins(c, seed=None):
    """(sigma_min over the non-degenerate groups, relu margin, MaxPool margin, argmax gap) of the case's FIRST step in fp64: sigma over the s and s' columns and both
    networks; the relu and MaxPool margins on s under the online parameters (where the derivatives are taken); the gap over the columns of the network that picks the action"""
    if c.T:
        D = rec_data(c, seed); idx, start = D.draws[0]
        s, a, r, sp, d, m = R.sample_batch(D.ring, idx, start, c.T, c.obs)
        qsel = np.concatenate(q_values(D.net, D.p_on if c.dq else D.p_tg, sp)); mk = m
    else:
        D = ff_data(c, seed); s, a, r, sp, d, w = ff_batch(c, D, D.idx[0])
        qsel = q_values(D.net, D.p_on if c.dq else D.p_tg, sp); mk = None
    on_s = probe_of(D.net, D.p_on, s, mk)
    sg = min(on_s["sigma"], probe_of(D.net, D.p_on, sp, mk)["sigma"], probe_of(D.net, D.p_tg, sp, mk)["sigma"])
    return sg, on_s["relu"], on_s["pool"], _gap(qsel)


def margins_ok(c, seed=None, k=2.0):
    sg, rm, pm, gap = case_margins(c, seed)
    return sg >= k * SIGMA_MIN and rm > k * RELU_MARGIN and pm > k * RELU_MARGIN and gap > k * GAP


find_seed = lambda c, cap=200: S.find_seed(c, margins_ok, cap)
