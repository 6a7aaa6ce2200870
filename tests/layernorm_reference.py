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
import importlib
import types

import numpy as np
import torch
import torch.nn.functional as F

import __graft_entry__ as ge
import dqn_oracle as O
import recurrent_reference as R
from drqn_common import draws, make_episodes
from feedforward_edges_common import GAP, RELU_MARGIN, TOL_GN, TOL_LOSS, TOL_Q, TOL_TD      # noqa: F401  (one set of constants, with the meaning they have there)
from gru_reference import gru_cell, param_arrays
from recurrent_reference import GRAD_C, GRAD_RTOL, Adam, check_params      # noqa: F401

nn = importlib.import_module(ge.load_package().__name__ + ".nn")
F64 = torch.float64
SIGMA_MIN = 0.05
LR = 1e-3
RECURRENT = ("lstm", "gru")


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


LEGS = {"law": ln_law, "numpy": _ln_numpy, "torchs_law": ln_torchs_law}


# ------------------------------------------------------------------ chains of nn descriptors
def _act(y, act):
    return {0: lambda v: v, 1: torch.relu, 2: torch.tanh, 3: torch.sigmoid}[act](y)


def _chain(layers, arrs, x, hs, li0, leg, probe):
    """one (time) step through a chain.  probe (or None): dict with 'sigma' / 'relu' -> the smallest LayerNorm sigma / |relu pre-activation| seen so far"""
    for i, l in enumerate(layers):
        a, k = arrs[li0 + i], li0 + i
        if l.kind == "lstm":
            hs[k] = R.lstm_cell(x.reshape(x.shape[0], -1), hs[k][0], hs[k][1], a[0], a[1], a[2]); x = hs[k][0]
            continue
        if l.kind == "gru":
            hs[k] = x = gru_cell(x.reshape(x.shape[0], -1), hs[k], a[0], a[1], a[2])
            continue
        if l.kind == "conv":      # a true convolution is the cross-correlation with the flipped kernel (feedforward_reference._layer_t)
            assert (l.ph, l.pw) == (0, 0)
            pre = F.conv2d(x, a[0].flip(2, 3), a[1], stride=(l.sh, l.sw))
        elif l.kind == "layernorm":
            pre, sigma = LEGS[leg](x.reshape(x.shape[0], -1), a[0], a[1], float(np.float32(l.eps)))
            if probe is not None:
                probe["sigma"] = min(probe["sigma"], float(sigma.min()))
        else:
            assert l.kind == "dense", l.kind
            pre = x.reshape(x.shape[0], -1) @ a[0] + a[1]
        if probe is not None and l.act == nn.relu:
            probe["relu"] = min(probe["relu"], float(pre.detach().abs().min()))
        x = _act(pre, l.act)
    return x


def q_step(net, arrs, x, hs, leg="law", probe=None):
    if isinstance(net, nn.DuelingNetwork):
        nb, nv = len(net.base.layers), len(net.val.layers)
        y = _chain(net.base.layers, arrs, x, hs, 0, leg, probe)
        v = _chain(net.val.layers, arrs, y, hs, nb, leg, probe)
        a = _chain(net.adv.layers, arrs, y, hs, nb + nv, leg, probe)
        return v + a - a.mean(dim=1, keepdim=True)      # src/dueling.jl:10
    return _chain(net.layers, arrs, x, hs, 0, leg, probe)


def is_recurrent(net):
    return any(l.kind in RECURRENT for l in nn.all_layers(net))


def init_state(net, arrs, n):
    out = {}
    for i, l in enumerate(nn.all_layers(net)):
        if l.kind in RECURRENT:
            h = arrs[i][3].reshape(1, -1).expand(n, -1).clone()
            out[i] = (h, arrs[i][4].reshape(1, -1).expand(n, -1).clone()) if l.kind == "lstm" else h
    return out


def _t64(x):
    return torch.tensor(np.asarray(x, np.float64))


def q_values(net, p, x, leg="law", probe=None):
    """Q (B, nA) as fp64 NumPy of a feed-forward network on observations x (B, ...); a recurrent network: x (T, B, ...) from the reset state -> [T] of (B, nA)"""
    arrs = param_arrays(net, nn, np.asarray(p, np.float64))
    with torch.no_grad():
        if not is_recurrent(net):
            return q_step(net, arrs, _t64(x), {}, leg, probe).numpy()
        hs = init_state(net, arrs, np.asarray(x).shape[1])
        return [q_step(net, arrs, _t64(xt), hs, leg, probe).numpy() for xt in x]


def sigma_min(net, p, s):
    """the smallest fp64 sigma over every LayerNorm layer and every column of s under the parameters p (s: (B, ...), or (T, B, ...) for a recurrent network).
    A case's bound covers the s and s' columns and both networks: case_margins"""
    probe = dict(sigma=np.inf, relu=np.inf)
    q_values(net, p, s, probe=probe)
    return probe["sigma"]


def relu_margin(net, p, s):
    probe = dict(sigma=np.inf, relu=np.inf)
    q_values(net, p, s, probe=probe)
    return probe["relu"]


def _huber(x):
    ab = x.abs(); qd = torch.clamp(ab, max=1.0)
    return 0.5 * qd * qd + (ab - qd)        # src/helpers.jl:14-19


def ff_step(net, p_on, p_tg, batch, gamma, double_q, leg="law"):
    """batch = (s, a, r, sp, done, w) as get_batch returns it; everything the engine reports of one feed-forward batch_train!"""
    s, a, r, sp, done, w = batch
    s, sp, r, done, w = _t64(s), _t64(sp), _t64(r), _t64(done), _t64(w)
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
    loss = _huber(w * td).sum() / B        # src/solver.jl:223-224
    loss.backward()
    g = np.concatenate([x.grad.numpy().reshape(-1) for x in leaves])
    return dict(q_on_s=q.detach().numpy(), q_on_sp=q_on_sp.numpy(), q_tg_sp=q_tg_sp.numpy(), best_a=best.numpy(), y=y.numpy(), td=td.detach().numpy(),
                loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()))


def rec_step(net, p_on, p_tg, batch, gamma, double_q, leg="law"):
    """batch = (s, a, r, sp, done, mask), each (T, B, ...), as episode_get_batch returns it: recurrent_reference.train_grads (mask inside the Huber, /B per step, /T)"""
    s, a, r, sp, d, m = batch; T, B = s.shape[0], s.shape[1]
    q_tg = q_values(net, p_tg, sp, leg)
    q_on = q_values(net, p_on, sp, leg) if double_q else q_tg
    ys = [O.bellman_targets(q_on[t], q_tg[t], r[t].astype(np.float64), d[t].astype(np.float64), gamma, double_q)[0] for t in range(T)]
    arrs = param_arrays(net, nn, np.asarray(p_on, np.float64)); leaves = [x for la in arrs for x in la]
    for x in leaves:
        x.requires_grad_(True)
    hs = init_state(net, arrs, B); loss = torch.zeros((), dtype=F64); tds = []
    for t in range(T):
        q = q_step(net, arrs, _t64(s[t]), hs, leg)
        td = q[torch.arange(B), torch.tensor(a[t].astype(np.int64))] - _t64(ys[t]); tds.append(td.detach().numpy())
        loss = loss + _huber(_t64(m[t]) * td).sum() / B
    loss = loss / T
    loss.backward()
    g = np.concatenate([x.grad.numpy().reshape(-1) for x in leaves])
    return dict(loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()), q_on_sp=q_on, q_tg_sp=q_tg, td=np.stack(tds))


def legs_agree(a, b, rel=1e-10):
    """two legs on one step: every quantity both report within rel of its own scale (gradients: of max |g|); best_a equal"""
    if "best_a" in a:
        np.testing.assert_array_equal(a["best_a"], b["best_a"])
    for k in ("q_on_s", "q_on_sp", "q_tg_sp", "y", "td", "grads"):
        if k in a:
            x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
            assert x.shape == y.shape, k
            scale = max(np.abs(x).max(), 1e-300)
            assert np.abs(x - y).max() <= rel * scale, f"{k}: the legs differ by {np.abs(x - y).max() / scale:.3g} relative"
    for k in ("loss", "grad_norm"):
        assert abs(a[k] - b[k]) <= rel * max(abs(a[k]), 1e-300), k


def blocks(net):
    """[(name, slice into the flat Flux.params vector)]; a LayerNorm layer i holds ln<i>.scale and ln<i>.bias"""
    names = {"lstm": ("Wi", "Wh", "b", "h0", "c0"), "gru": ("Wi", "Wh", "b", "h0"), "dense": ("W", "b"), "conv": ("W", "b"), "layernorm": ("scale", "bias")}
    out, off = [], 0
    for li, l in enumerate(nn.all_layers(net)):
        for nm, shp in zip(names[l.kind], l.shapes()):
            k = int(np.prod(shp)); out.append((f"{'ln' if l.kind == 'layernorm' else l.kind}{li}.{nm}", slice(off, off + k))); off += k
    return out


def dead_blocks(net, g, exempt=()):
    return [nm for nm in R.dead_blocks(net, nn, g, blks=blocks(net)) if nm not in exempt]


def check_grads(net, got, want, live=True, exempt=()):
    """recurrent_reference.check_grads per block (GRAD_C, GRAD_RTOL unchanged); live: no block's fp64 gradient is negligible, except the blocks named in
    `exempt` -- which are still held to the tolerance (see Case.dead)"""
    R.check_grads(net, nn, got, want, live=False, blks=blocks(net))
    assert not live or not dead_blocks(net, want, exempt), dead_blocks(net, want, exempt)


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


def _params(net, rng, pscale=1.0):
    """glorot weights (times pscale) + noise everywhere (non-zero biases and state0; LayerNorm scale around pscale, bias around 0)"""
    p_on = nn.glorot_params(net, seed=3); p_on = (np.float32(pscale) * p_on + 0.05 * rng.standard_normal(p_on.size)).astype(np.float32)
    p_tg = (p_on + 0.05 * rng.standard_normal(p_on.size)).astype(np.float32)
    return p_on, p_tg


def ff_data(c, seed=None):
    """the case's network, replay rows, parameters and step indices: deterministic from the seed"""
    rng = np.random.default_rng(c.seed if seed is None else seed); net = c.mk(); n = c.B + 24
    if c.u8:
        s, sp = (rng.integers(0, 256, (n,) + c.obs).astype(np.uint8) for _ in range(2))
    else:
        s, sp = ((2 * rng.standard_normal((n,) + c.obs)).astype(np.float32) for _ in range(2))
    a = rng.integers(0, c.nA, n).astype(np.int32); r = (2 * rng.standard_normal(n)).astype(np.float32); d = (rng.random(n) < 0.2).astype(np.uint8)
    p_on, p_tg = _params(net, rng, c.pscale)
    idx = [rng.choice(n, c.B, replace=False).astype(np.int64) for _ in range(3)]
    return types.SimpleNamespace(net=net, s=s, sp=sp, a=a, r=r, d=d, p_on=p_on, p_tg=p_tg, idx=idx)


def ff_batch(c, D, ix):
    """get_batch in fp64 from the drawn rows; IS weights from the priorities replay_add gave the rows (|r| as TD error)"""
    f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
    prio = O.priority_from_td(np.abs(D.r), np.float32(1e-3), np.float32(0.6)).astype(np.float64)
    return f(D.s[ix]), D.a[ix], D.r[ix], f(D.sp[ix]), D.d[ix].astype(np.float64), O.is_weights(prio[ix], prio, 0.4, np.float64)


def rec_data(c, seed=None):
    seed = c.seed if seed is None else seed
    net = c.mk(); cap = max(12, c.B + 4)
    eps = make_episodes(types.SimpleNamespace(obs_shape=c.obs, n_actions=c.nA), cap + 3, c.T, np.random.default_rng(seed))
    ring = [None] * cap
    for i, ep in enumerate(eps):
        ring[i % cap] = ep
    rng = np.random.default_rng(seed); p_on, p_tg = _params(net, rng, c.pscale)
    rng = np.random.default_rng(seed + 100)
    return types.SimpleNamespace(net=net, cap=cap, eps=eps, ring=ring, p_on=p_on, p_tg=p_tg, draws=[draws(ring, c.B, rng) for _ in range(3)])


def _gap(q):
    t = np.sort(q, axis=1)[:, -2:]
    return float((t[:, 1] - t[:, 0]).min())


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


def find_seed(c, cap=200):
    """the smallest seed that keeps twice the margins (how the table's seeds were chosen, on the CPU, with this module alone)"""
    for seed in range(1, cap):
        if margins_ok(c, seed):
            return seed
    raise AssertionError(f"{c.name}: no seed below {cap} keeps the margins")
