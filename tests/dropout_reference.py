"""fp64 reference of ONE batch_train! for networks with Flux Dropout layers (TEST INFRASTRUCTURE), feed-forward (src/solver.jl:191-236) and recurrent
(src/solver.jl:239-287), over the package's nn descriptors: what layernorm_reference.py covers (Dense, pad-0 Conv, LSTM / GRU, LayerNorm, plain or dueling) plus Dropout.

The layer (Flux 0.14 automatic mode; recalled, not executed): ACTIVE only in the forward Flux.gradient differentiates -- the online network on s --, where
y = keep ? x * scale : 0 with scale = Float32(1 / (1 - p)); the identity in every other pass (online on s', target, acting).  The masks are DATA here: a step takes
{layer index: keep (B, n) bool} (recurrent: (T, B, n)).  keep_mask restates the engine's mask law in NumPy on top of replay_reference.philox4x32_10 (DESIGN.md section 4
"Dropout layers"): Philox4x32-10 keyed by the engine seed on {k lo, k hi, q, 0x44520000 | layer}, k = train steps completed before, q = f * ceil(C / 4) + col / 4,
the four words for columns 4 (col / 4) + 0..3, u = (word >> 8) * 2^-24, keep <=> u >= p.  Julia's RNG is not matched and nothing here pretends to.

Two legs:
  * "law"    torch float64 autograd through torch.where(keep, x * scale, 0);
  * "numpy"  the same step with every Dropout layer a hand-written NumPy forward and backward (do_forward_np / do_backward_np) entered as a torch.autograd.Function.
Everything that is not a Dropout layer runs through layernorm_reference._chain (its "law" leg).  `where` says which passes are masked: ("s",) is the law; ("s", "sp") and
("s", "tg") are the two WRONG engines (the layer active in the online pass on s' / in the target pass) the CPU tests show apart from it.

Data rule: the margins of layernorm_reference (SIGMA_MIN, RELU_MARGIN, GAP), taken on the masked s pass and the unmasked s' passes.  Seeds are fixed in the table and were
found with this module alone (find_seed)."""
import types

import numpy as np
import torch

import dqn_oracle as O
import layernorm_reference as LR
import recurrent_reference as R
import replay_reference as RR
from gru_reference import param_arrays

nn = LR.nn
F64 = torch.float64
DO_TAG = 0x44520000
ENGINE_SEED = 5      # hparams.seed of every engine the GPU tests build for these tables (the mask's key)
LAW = ("s",)


# ------------------------------------------------------------------ the mask law
def do_scale(p):
    return float(np.float32(1.0 / (1.0 - float(p))))      # the quotient in Float64, rounded once


def uniforms(seed, k, layer, n, C):
    """u (C, n) float64, exact: column col of feature f"""
    nq = (C + 3) // 4
    q = (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(nq) + np.arange(nq, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)      # (n, nq)
    c = np.empty((n, nq, 4), np.uint64)
    c[..., 0], c[..., 1], c[..., 2], c[..., 3] = int(k) & 0xFFFFFFFF, (int(k) >> 32) & 0xFFFFFFFF, q, DO_TAG | int(layer)
    w = RR.philox4x32_10((int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF), c)      # (n, nq, 4): word j of quad qd is column 4 qd + j
    u = (w >> np.uint32(8)).astype(np.float64) * RR.U24
    return u.reshape(n, 4 * nq)[:, :C].T.copy()


def keep_mask(seed, k, layer, n, C, p):
    return uniforms(seed, k, layer, n, C) >= float(p)


def widths(net):
    """{layer index: n} of every Dropout layer: the producing layer's output width"""
    out, n = {}, None
    for i, l in enumerate(nn.all_layers(net)):
        if l.kind == "dropout":
            out[i] = n
        else:
            n = l.n if l.kind == "layernorm" else l.n_out if l.kind != "conv" else None
    assert all(v for v in out.values())
    return out


def masks_for(net, k, B, T=0, seed=ENGINE_SEED):
    """the engine's masks of train step k (k steps completed before): {layer: (B, n)}, recurrent {layer: (T, B, n)} with col = t * B + b"""
    layers = nn.all_layers(net); out = {}
    for i, n in widths(net).items():
        m = keep_mask(seed, k, i, n, (T or 1) * B, layers[i].p)
        out[i] = m.reshape(T, B, n) if T else m
    return out


# ------------------------------------------------------------------ the layer
def do_law(x, keep, scale):
    return torch.where(keep, x * scale, torch.zeros((), dtype=F64))


def do_forward_np(x, keep, scale):
    return np.where(keep, x * scale, 0.0)


def do_backward_np(keep, scale, dy):
    return np.where(keep, dy * scale, 0.0)


class _DoNumpy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, keep, scale):
        ctx.keep, ctx.scale = keep.numpy(), scale
        return torch.tensor(do_forward_np(x.detach().numpy(), ctx.keep, scale), dtype=F64)

    @staticmethod
    def backward(ctx, dy):
        return torch.tensor(do_backward_np(ctx.keep, ctx.scale, dy.numpy())), None, None


LEGS = {"law": do_law, "numpy": _DoNumpy.apply}


def _chain(layers, arrs, x, hs, li0, masks, leg, probe):
    """layernorm_reference._chain over the runs between Dropout layers; masks: {layer index: keep (B, n)} or None = every Dropout layer inactive"""
    i = 0
    while i < len(layers):
        j = i
        while j < len(layers) and layers[j].kind != "dropout":
            j += 1
        if j > i:
            x = LR._chain(layers[i:j], arrs, x, hs, li0 + i, "law", probe)
        if j < len(layers):
            x = x.reshape(x.shape[0], -1)
            if probe is not None:
                probe.setdefault("do_in", {})[li0 + j] = x.detach().numpy().copy()
            if masks is not None:
                x = LEGS[leg](x, torch.tensor(masks[li0 + j]), do_scale(layers[j].p))
            j += 1
        i = j
    return x


def q_step(net, arrs, x, hs, masks=None, leg="law", probe=None):
    if isinstance(net, nn.DuelingNetwork):
        nb, nv = len(net.base.layers), len(net.val.layers)
        y = _chain(net.base.layers, arrs, x, hs, 0, masks, leg, probe)
        v = _chain(net.val.layers, arrs, y, hs, nb, masks, leg, probe)
        a = _chain(net.adv.layers, arrs, y, hs, nb + nv, masks, leg, probe)
        return v + a - a.mean(dim=1, keepdim=True)      # src/dueling.jl:10
    return _chain(net.layers, arrs, x, hs, 0, masks, leg, probe)


def _at(masks, t):
    return None if masks is None else {k: v[t] for k, v in masks.items()}


def q_values(net, p, x, masks=None, leg="law", probe=None):
    """Q (B, nA) fp64 of a feed-forward network on x (B, ...); recurrent: x (T, B, ...) from the reset state -> [T] of (B, nA).  masks None: the inactive layer"""
    arrs = param_arrays(net, nn, np.asarray(p, np.float64))
    with torch.no_grad():
        if not LR.is_recurrent(net):
            return q_step(net, arrs, LR._t64(x), {}, masks, leg, probe).numpy()
        hs = LR.init_state(net, arrs, np.asarray(x).shape[1])
        return [q_step(net, arrs, LR._t64(xt), hs, _at(masks, t), leg, probe).numpy() for t, xt in enumerate(x)]


def ff_step(net, p_on, p_tg, batch, gamma, double_q, masks, leg="law", where=LAW):
    """layernorm_reference.ff_step with the Dropout layers active, under `masks`, in the passes `where` names ("s": the law)"""
    s, a, r, sp, done, w = batch
    s, sp, r, done, w = LR._t64(s), LR._t64(sp), LR._t64(r), LR._t64(done), LR._t64(w)
    a = torch.tensor(np.asarray(a, np.int64)); B = s.shape[0]
    aon, atg = param_arrays(net, nn, np.asarray(p_on, np.float64)), param_arrays(net, nn, np.asarray(p_tg, np.float64))
    with torch.no_grad():
        q_tg_sp = q_step(net, atg, sp, {}, masks if "tg" in where else None, leg)
        q_on_sp = q_step(net, aon, sp, {}, masks if "sp" in where else None, leg) if double_q else q_tg_sp
        best = (q_on_sp == q_on_sp.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)
        y = r + (1.0 - done) * float(gamma) * q_tg_sp[torch.arange(B), best]
    leaves = [x for la in aon for x in la]
    for x in leaves:
        x.requires_grad_(True)
    q = q_step(net, aon, s, {}, masks if "s" in where else None, leg)
    td = q[torch.arange(B), a] - y
    loss = LR._huber(w * td).sum() / B
    loss.backward()
    g = np.concatenate([x.grad.numpy().reshape(-1) for x in leaves])
    return dict(q_on_s=q.detach().numpy(), q_on_sp=q_on_sp.numpy(), q_tg_sp=q_tg_sp.numpy(), best_a=best.numpy(), y=y.numpy(), td=td.detach().numpy(),
                loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()))


def rec_step(net, p_on, p_tg, batch, gamma, double_q, masks, leg="law", where=LAW):
    """layernorm_reference.rec_step: the target loop (both networks over s') unmasked, the BPTT loop over s with a fresh mask per time step (masks[layer][t])"""
    s, a, r, sp, d, m = batch; T, B = s.shape[0], s.shape[1]
    q_tg = q_values(net, p_tg, sp, masks if "tg" in where else None, leg)
    q_on = q_values(net, p_on, sp, masks if "sp" in where else None, leg) if double_q else q_tg
    ys = [O.bellman_targets(q_on[t], q_tg[t], r[t].astype(np.float64), d[t].astype(np.float64), gamma, double_q)[0] for t in range(T)]
    arrs = param_arrays(net, nn, np.asarray(p_on, np.float64)); leaves = [x for la in arrs for x in la]
    for x in leaves:
        x.requires_grad_(True)
    hs = LR.init_state(net, arrs, B); loss = torch.zeros((), dtype=F64); tds = []
    for t in range(T):
        q = q_step(net, arrs, LR._t64(s[t]), hs, _at(masks, t) if "s" in where else None, leg)
        td = q[torch.arange(B), torch.tensor(a[t].astype(np.int64))] - LR._t64(ys[t]); tds.append(td.detach().numpy())
        loss = loss + LR._huber(LR._t64(m[t]) * td).sum() / B
    loss = loss / T
    loss.backward()
    g = np.concatenate([x.grad.numpy().reshape(-1) for x in leaves])
    return dict(loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()), q_on_sp=q_on, q_tg_sp=q_tg, y=np.stack(ys), td=np.stack(tds))


def blocks(net):
    """[(name, slice into the flat Flux.params vector)]: layernorm_reference.blocks; a Dropout layer holds nothing"""
    names = {"lstm": ("Wi", "Wh", "b", "h0", "c0"), "gru": ("Wi", "Wh", "b", "h0"), "dense": ("W", "b"), "conv": ("W", "b"), "layernorm": ("scale", "bias"), "dropout": ()}
    out, off = [], 0
    for li, l in enumerate(nn.all_layers(net)):
        for nm, shp in zip(names[l.kind], l.shapes()):
            k = int(np.prod(shp)); out.append((f"{'ln' if l.kind == 'layernorm' else l.kind}{li}.{nm}", slice(off, off + k))); off += k
    return out


def check_grads(net, got, want, live=True):
    R.check_grads(net, nn, got, want, live=live, blks=blocks(net))


def distance(a, b):
    """{quantity: the largest |a - b| / tolerance} over what the GPU tests compare with the project's constants (1.0 = at the bound)"""
    out = {}
    for k, tol in (("q_on_s", LR.TOL_Q), ("q_on_sp", LR.TOL_Q), ("q_tg_sp", LR.TOL_Q), ("y", LR.TOL_TD), ("td", LR.TOL_TD)):
        if k in a and k in b:
            x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
            out[k] = float((np.abs(x - y) / (tol["atol"] + tol["rtol"] * np.abs(y))).max())
    out["loss"] = abs(a["loss"] - b["loss"]) / (LR.TOL_LOSS["atol"] + LR.TOL_LOSS["rtol"] * abs(b["loss"]))
    return out


# ------------------------------------------------------------------ the case table
def _mlp(n, p, act=nn.relu, nA=4, E=6):
    return lambda: nn.Chain(nn.Dense(E, n, act), nn.Dropout(p), nn.Dense(n, nA))


def case(name, mk, B, **kw):
    c = LR.case(name, mk, B, **kw)
    c.ps = tuple(l.p for l in nn.all_layers(mk()) if l.kind == "dropout")
    return c


# B = 5: ten columns, unaligned rows (one column per thread); B = 6: the quad that straddles s | s'; B = 4 / 32: the 16-byte path; n = 7 / 33: features that are no multiple
# of anything; n = 512: more than one workgroup per launch at any B.  Every p = 0 case is single-Q (masking s' with an all-keep mask is the identity: no test could tell)
CASES = [
    case("relu_n7_b4", _mlp(7, 0.5), 4, seed=1),                                         # behind Dense(relu)
    case("tanh_n33_b5", _mlp(33, 0.1, nn.tanh), 5, seed=2),                              # behind Dense(tanh): the producer's derivative comes from its unmasked y
    case("relu_n33_b6", _mlp(33, 0.5), 6, seed=1),
    case("n512_b32", _mlp(512, 0.5), 32, seed=1),
    case("n512_b32_valu", _mlp(512, 0.1), 32, mfma=0, seed=1),
    case("p0_n33_b32", _mlp(33, 0.0), 32, dq=0, seed=1),                                 # p = 0: the identity without a special case
    case("p0_n7_b5", _mlp(7, 0.0, nn.tanh), 5, dq=0, seed=1),
    case("do_ln", lambda: nn.Chain(nn.Dense(6, 33), nn.Dropout(0.5), nn.LayerNorm(33, nn.relu), nn.Dense(33, 4)), 32, seed=1),      # the DroQ block
    case("ln_do", lambda: nn.Chain(nn.Dense(6, 16, nn.relu), nn.LayerNorm(16, nn.tanh), nn.Dropout(0.1), nn.Dense(16, 4)), 6, seed=1),
    case("two_do", lambda: nn.Chain(nn.Dense(6, 33, nn.relu), nn.Dropout(0.5), nn.Dense(33, 16, nn.tanh), nn.Dropout(0.1), nn.Dense(16, 4)), 5, seed=1),
    case("dueling_prio", lambda: nn.create_dueling_network(_mlp(32, 0.5)()), 32, dueling=True, prio=1, seed=1),      # the last base layer: the join's dX lands in the layer
    case("single_q_b6", _mlp(33, 0.5), 6, dq=0, seed=1),                                 # 6 columns in the forward too
    case("conv_u8", lambda: nn.Chain(nn.Conv(3, 1, 4, nn.relu), nn.flattenbatch, nn.Dense(64, 16, nn.relu), nn.Dropout(0.1), nn.Dense(16, 4)), 32, obs=(1, 6, 6), u8=1, seed=1, pscale=3.0),
]
REC_CASES = [
    case("lstm_do", lambda: nn.Chain(nn.LSTM(6, 8), nn.Dropout(0.5), nn.Dense(8, 3)), 4, nA=3, T=3, seed=1, pscale=3.0),
    case("do_gru", lambda: nn.Chain(nn.Dense(6, 8, nn.relu), nn.Dropout(0.5), nn.GRU(8, 8), nn.Dense(8, 3)), 4, nA=3, T=3, seed=1, pscale=3.0),
]
BY_NAME = {c.name: c for c in CASES + REC_CASES}
assert len(BY_NAME) == len(CASES) + len(REC_CASES)
ff_data, ff_batch, rec_data = LR.ff_data, LR.ff_batch, LR.rec_data


def first_step(c, seed=None):
    """(network data, fp64 batch, masks) of the case's first step"""
    if c.T:
        D = rec_data(c, seed); idx, start = D.draws[0]
        return D, R.sample_batch(D.ring, idx, start, c.T, c.obs), masks_for(D.net, 0, c.B, c.T)
    D = ff_data(c, seed)
    return D, ff_batch(c, D, D.idx[0]), masks_for(D.net, 0, c.B)


def step(c, D, batch, masks, **kw):
    return (rec_step if c.T else ff_step)(D.net, D.p_on, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq), masks, **kw)


def case_margins(c, seed=None):
    """(sigma_min, relu margin, argmax gap) of the first step in fp64: sigma and the relu margin over the MASKED s pass under the online parameters and the unmasked s'
    passes of both networks; the gap over the columns of the network that picks the action"""
    D, batch, masks = first_step(c, seed); probe = dict(sigma=np.inf, relu=np.inf)
    q_values(D.net, D.p_on, batch[0], masks, probe=probe)
    qon = q_values(D.net, D.p_on, batch[3], probe=probe); qtg = q_values(D.net, D.p_tg, batch[3], probe=probe)
    qsel = qon if c.dq else qtg
    return probe["sigma"], probe["relu"], LR._gap(np.concatenate(qsel) if c.T else qsel)


def margins_ok(c, seed=None, k=2.0):
    sg, rm, gap = case_margins(c, seed)
    return sg >= k * LR.SIGMA_MIN and rm > k * LR.RELU_MARGIN and gap > k * LR.GAP


TELL = 100.0      # a wrong mask element / a wrongly active pass must move a compared quantity by this many of its tolerances


def tell_distances(c, seed=None):
    """what the wrong engines are off by on the case's first step, in tolerances: (one flipped mask element: the largest over the compared quantities; the layer active
    on s': the larger of y and td; the layer active in the target pass: likewise) -- the last two None for a single-Q case, whose s' pass IS the target pass"""
    D, batch, masks = first_step(c, seed); a = step(c, D, batch, masks)
    out = [max(distance(step(c, D, batch, flip_one(c, D, batch, masks)[0]), a).values())]
    for w in (("s", "sp"), ("s", "tg")):
        d = distance(step(c, D, batch, masks, where=w), a) if c.dq else None
        out.append(max(d["y"], d["td"]) if d else None)
    return tuple(out)


def tells_ok(c, seed=None, k=2.0):
    return all(d is None or d >= k * TELL for d in tell_distances(c, seed))


def find_seed(c, cap=200):
    """the smallest seed that keeps twice the margins and twice the tell distances (how the table's seeds were chosen, on the CPU, with this module alone)"""
    for seed in range(1, cap):
        if margins_ok(c, seed) and tells_ok(c, seed):
            return seed
    raise AssertionError(f"{c.name}: no seed below {cap} keeps the margins")


def flip_one(c, D, batch, masks):
    """the masks with ONE element flipped: in the first Dropout layer, column 0 (recurrent: t = 0, b = 0), the feature where the layer's input is largest in magnitude
    (an element whose input is 0 -- a dead relu -- changes nothing under any mask)"""
    probe = dict(sigma=np.inf, relu=np.inf); l = min(masks)
    q_values(D.net, D.p_on, batch[0][:1] if c.T else batch[0], _at_first(masks) if c.T else masks, probe=probe)      # recurrent: the first time step alone
    x = probe["do_in"][l]
    f = int(np.abs(x[0]).argmax())
    out = {k: v.copy() for k, v in masks.items()}
    if c.T:
        out[l][0, 0, f] ^= True
    else:
        out[l][0, f] ^= True
    return out, (l, f)


def _at_first(masks):
    return {k: v[:1] for k, v in masks.items()}
