"""fp64 reference of ONE batch_train! for networks with Flux LayerNorm layers (TEST INFRASTRUCTURE), feed-forward (src/solver.jl:191-236) and recurrent
(src/solver.jl:239-287), over the package's nn descriptors: Dense, pad-0 Conv, LSTM / GRU and LayerNorm, plain or dueling.

The law (Flux 0.14 `normalise`; recalled, not executed): per batch column mu = mean(x), sigma = sqrt(mean((x - mu)^2)), y = act(scale * (x - mu) / (sigma + eps) + bias)
-- eps is added to sigma OUTSIDE the root.  torch.nn.LayerNorm / F.layer_norm compute sqrt(var + eps), a different law, and are not used anywhere here
(ln_torchs_law restates that other law only so that a test can show the two apart).

Two legs:
  * "law"    torch float64 autograd through the law written out (ln_law);
  * "numpy"  the same step with every LayerNorm layer replaced by a hand-written NumPy forward and backward (ln_forward_np / ln_backward_np), entered into the
             graph as a torch.autograd.Function -- an independent derivation of the layer's gradient, including the path through sigma.
tests/test_layernorm_cpu.py holds them to 1e-10 of each other on every case and checks the hand-written gradient against central differences.

Data rule: beside the relu margin and the argmax gap of the feed-forward tables (feedforward_edges_common.RELU_MARGIN, GAP) every case keeps
sigma_min >= SIGMA_MIN: the layer divides by sigma, so an fp32 error in x is amplified by 1 / sigma, and the gradient by 1 / sigma^2; at sigma >= 0.05 and O(1)
activations that stays inside the tolerances the other tables use.  Seeds are fixed in the table and were found with this module alone (find_seed)."""
import types

import numpy as np
import torch

import recurrent_reference as R
import step_reference as S
from feedforward_edges_common import GAP, RELU_MARGIN, TOL_GN, TOL_LOSS, TOL_Q, TOL_TD      # noqa: F401  (one set of constants, with the meaning they have there)
from recurrent_reference import GRAD_C, GRAD_RTOL, Adam, check_params      # noqa: F401
from step_reference import F64, LR, _gap, blocks, check_grads, dead_blocks, ff_batch, ff_data, legs_agree, nn, rec_data      # noqa: F401  (what this table's tests reach through here)

SIGMA_MIN = 0.05


# ------------------------------------------------------------------ the layer
def ln_law(x, scale, bias, eps):
    """x (B, n) -> the pre-activation scale * x_hat + bias under Flux's law; also sigma (B, 1)"""
    mu = x.mean(dim=1, keepdim=True)
    sigma = ((x - mu) ** 2).mean(dim=1, keepdim=True).sqrt()
    return scale * ((x - mu) / (sigma + eps)) + bias, sigma


def ln_torchs_law(x, scale, bias, eps):
    """the OTHER law, sqrt(var + eps): what torch.nn.LayerNorm computes.  Only test_layernorm_cpu's tell-apart test calls it"""
    mu = x.mean(dim=1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=1, keepdim=True)
    return scale * ((x - mu) / (var + eps).sqrt()) + bias, var.sqrt()


def ln_forward_np(x, scale, bias, eps):
    """NumPy: x (B, n) -> pre-activation (B, n), cache"""
    n = x.shape[1]
    mu = x.sum(axis=1, keepdims=True) / n
    d = x - mu
    sigma = np.sqrt((d * d).sum(axis=1, keepdims=True) / n)
    r = 1.0 / (sigma + eps)
    xh = d * r
    return scale * xh + bias, (xh, sigma, r, scale)


def ln_backward_np(cache, dy):
    """dy = dL/d(pre-activation) -> dx, dscale, dbias.  With g = dy * scale:  dx = r (g - mean g) - x_hat mean(g x_hat) / sigma  (the second term is the path through sigma:
    d x_hat_j / d sigma = -x_hat_j r and d sigma / d x_i = (x_i - mu) / (n sigma) = x_hat_i / (n sigma r))"""
    xh, sigma, r, scale = cache
    g = dy * scale
    dx = r * (g - g.mean(axis=1, keepdims=True)) - xh * ((g * xh).mean(axis=1, keepdims=True) / sigma)
    return dx, (dy * xh).sum(axis=0), dy.sum(axis=0)


class _LnNumpy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, bias, eps):
        y, cache = ln_forward_np(x.detach().numpy(), scale.detach().numpy(), bias.detach().numpy(), eps)
        ctx.cache = cache
        return torch.tensor(y, dtype=F64)

    @staticmethod
    def backward(ctx, dy):
        dx, ds, db = ln_backward_np(ctx.cache, dy.numpy())
        return torch.tensor(dx), torch.tensor(ds), torch.tensor(db), None


def _ln_numpy(x, scale, bias, eps):
    return _LnNumpy.apply(x, scale, bias, eps), torch.tensor(_LnNumpy_sigma(x, eps))


def _LnNumpy_sigma(x, eps):
    return ln_forward_np(x.detach().numpy(), 1.0, 0.0, eps)[1][1]


# ------------------------------------------------------------------ the legs, the observers and the step (step_reference's, bound to them)
LEGS = {"law": {}, "numpy": {"layernorm": S.layernorm_law(_ln_numpy)}, "torchs_law": {"layernorm": S.layernorm_law(ln_torchs_law)}}


def _see_sigma(probe, l, sigma, cx):
    probe["sigma"] = min(probe["sigma"], float(sigma.min()))


def _see_relu(probe, l, pre, cx):
    if l.act == nn.relu:
        probe["relu"] = min(probe["relu"], float(pre.detach().abs().min()))


OBSERVERS = {"sigma": _see_sigma, "pre": _see_relu}      # -> the smallest LayerNorm sigma / |relu pre-activation| seen so far


def new_probe():
    return S.Probe(OBSERVERS, sigma=np.inf, relu=np.inf)


q_values = S.bound(S.q_values, LEGS, "leg", "probe")
ff_step, rec_step = S.bound(S.ff_step, LEGS, "leg"), S.bound(S.rec_step, LEGS, "leg")


def sigma_min(net, p, s):
    """the smallest fp64 sigma over every LayerNorm layer and every column of s under the parameters p (s: (B, ...), or (T, B, ...) for a recurrent network).
    A case's bound covers the s and s' columns and both networks: case_margins"""
    return S.probed(new_probe(), q_values, net, p, s)["sigma"]


def relu_margin(net, p, s):
    return S.probed(new_probe(), q_values, net, p, s)["relu"]


# ------------------------------------------------------------------ the case table
def _mlp(n, hid_act=nn.relu, ln_act=nn.identity, eps=1e-5, nA=4, E=6):
    return lambda: nn.Chain(nn.Dense(E, n, hid_act), nn.LayerNorm(n, ln_act, eps=eps), nn.Dense(n, nA))


def case(name, mk, B, obs=(6,), nA=4, dueling=False, dq=1, prio=0, u8=0, mfma=1, T=0, seed=1, pscale=1.0, dead=()):
    """dead: blocks whose gradient is negligible BY THE LAW, not by the data (only n = 2, see the table).  pscale: the glorot draw is multiplied by it (O(1) activations in front of the LayerNorm where glorot weights on [0, 1) inputs or a gated cell give ~0.1)"""
    return types.SimpleNamespace(name=name, mk=mk, B=B, obs=tuple(obs), nA=nA, dueling=dueling, dq=dq, prio=prio, u8=u8, mfma=mfma, T=T, seed=seed, gamma=0.95, pscale=pscale, dead=tuple(dead))


CASES = [
    # 1: minimum width; ten columns: the scalar column path.  Over two features x_hat = (+a, -a) with a = sigma / (sigma + eps) whatever x is, so the input gradient is
    # dx_1 = -dx_2 = (g_1 - g_2) / 2 * eps / (sigma + eps)^2: at eps = 1f-5 and sigma >= 0.05 the blocks IN FRONT of the layer carry < 1e-2 of a live block's gradient by the
    # law itself (test_layernorm_cpu checks the identity), and in fp32 the two terms of dx cancel to that size: the seed keeps sigma >= 0.5, where the
    # round-off of that difference, ~2^-24 / sigma of a live gradient, stays inside the blocks' tolerance.  They are compared like every block but cannot be asked to be live; ln1.scale / ln1.bias / dense2 are
    case("n2_b5", _mlp(2), 5, seed=5930, dead=("dense0.W", "dense0.b")),
    case("n5_b32", _mlp(5), 32, seed=7),                                                 # 2: n neither a multiple of 4 nor of the 16 slots
    case("n64_b32", _mlp(64), 32, seed=1), case("n65_b32", _mlp(65), 32, seed=1), case("n100_b32", _mlp(100), 32, seed=1),      # 3
    case("n512_b32", _mlp(512), 32, seed=10), case("n512_b128", _mlp(512), 128, seed=4, pscale=3.0), case("n512_b32_valu", _mlp(512), 32, mfma=0, seed=10),      # 4
    case("relu_tanh", _mlp(16, nn.tanh, nn.relu), 32, seed=1), case("tanh_tanh", _mlp(16, nn.tanh, nn.tanh), 32, seed=1),      # 5
    case("sigmoid_tanh", _mlp(16, nn.tanh, nn.sigmoid), 32, seed=1), case("identity_identity", _mlp(16, nn.identity, nn.identity), 32, seed=1),
    case("eps_half", _mlp(16, eps=0.5), 32, seed=1),                                     # 6: Flux's law against torch's
    case("two_layers", lambda: nn.Chain(nn.Dense(6, 24, nn.relu), nn.LayerNorm(24), nn.Dense(24, 16, nn.relu), nn.LayerNorm(16), nn.Dense(16, 4)), 32, seed=1),      # 7
    case("dueling_prio", lambda: nn.create_dueling_network(_mlp(32)()), 32, dueling=True, prio=1, seed=1),      # 8: the join's dX into the layer; IS weights from unequal priorities
    case("single_q", _mlp(16), 32, dq=0, seed=1),                                        # 9
    case("conv_u8", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.flattenbatch, nn.Dense(64, 16, nn.relu), nn.LayerNorm(16), nn.Dense(16, 4)), 32, obs=(1, 6, 6), u8=1, seed=1, pscale=3.0),      # 10
]
REC_CASES = [
    case("lstm_b4", lambda: nn.Chain(nn.LSTM(6, 8), nn.LayerNorm(8), nn.Dense(8, 3)), 4, nA=3, T=3, seed=6, pscale=3.0),                    # 11: per-step recurrence launches (H * B = 32)
    case("lstm_b8", lambda: nn.Chain(nn.LSTM(6, 8), nn.LayerNorm(8), nn.Dense(8, 3)), 8, nA=3, T=3, seed=6, pscale=3.0),                    # ... and the whole-sequence kernels (H * B = 64)
    case("gru_b4", lambda: nn.create_dueling_network(nn.Chain(nn.GRU(6, 8), nn.LayerNorm(8, nn.tanh), nn.Dense(8, 3))), 4, nA=3, T=3, dueling=True, seed=6, pscale=3.0),      # 12
    case("gru_b8", lambda: nn.create_dueling_network(nn.Chain(nn.GRU(6, 8), nn.LayerNorm(8, nn.tanh), nn.Dense(8, 3))), 8, nA=3, T=3, dueling=True, seed=10, pscale=3.0),
]
BY_NAME = {c.name: c for c in CASES + REC_CASES}
assert len(BY_NAME) == len(CASES) + len(REC_CASES)


def case_margins(c, seed=None):
    """(sigma_min, relu margin, argmax gap) of the case's FIRST step in fp64: sigma over the s and s' columns and both networks; the relu margin on s under the online
    parameters (where relu' is taken); the gap over the columns of the network that picks the action"""
    if c.T:
        D = rec_data(c, seed); idx, start = D.draws[0]
        s, a, r, sp, d, m = R.sample_batch(D.ring, idx, start, c.T, c.obs)
        qsel = np.concatenate(q_values(D.net, D.p_on if c.dq else D.p_tg, sp))
    else:
        D = ff_data(c, seed); s, a, r, sp, d, w = ff_batch(c, D, D.idx[0])
        qsel = q_values(D.net, D.p_on if c.dq else D.p_tg, sp)
    sg = min(sigma_min(D.net, D.p_on, s), sigma_min(D.net, D.p_on, sp), sigma_min(D.net, D.p_tg, sp))
    return sg, relu_margin(D.net, D.p_on, s), _gap(qsel)


def margins_ok(c, seed=None, k=2.0):
    sg, rm, gap = case_margins(c, seed)
    return sg >= k * SIGMA_MIN and rm > k * RELU_MARGIN and gap > k * GAP


find_seed = lambda c, cap=200: S.find_seed(c, margins_ok, cap)
