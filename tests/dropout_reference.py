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
The step, the walker and every other layer's law are step_reference's; a leg here overrides the Dropout law alone.  `where` says which passes are masked: ("s",) is the law; ("s", "sp") and
("s", "tg") are the two WRONG engines (the layer active in the online pass on s' / in the target pass) the CPU tests show apart from it.

Data rule: the margins of layernorm_reference (SIGMA_MIN, RELU_MARGIN, GAP), taken on the masked s pass and the unmasked s' passes.  Seeds are fixed in the table and were
found with this module alone (find_seed)."""
import numpy as np
import torch

import layernorm_reference as LR
import replay_reference as RR
import step_reference as S
from step_reference import blocks, check_grads, distance, ff_batch, ff_data, rec_data      # noqa: F401

nn = LR.nn
F64 = torch.float64
DO_TAG = 0x44520000
ENGINE_SEED = 5      # hparams.seed of every engine the GPU tests build for these tables (the mask's key)


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


LEGS = {"law": {}, "numpy": {"dropout": S.dropout_law(_DoNumpy.apply, do_scale)}}


def _see_input(probe, l, x, cx):
    if l.kind == "dropout":
        probe.setdefault("do_in", {})[cx.k] = x.reshape(x.shape[0], -1).detach().numpy().copy()


OBSERVERS = LR.OBSERVERS | {"in": _see_input}      # sigma, relu margin, and "do_in": {layer index: the layer's input}


def new_probe():
    return S.Probe(OBSERVERS, sigma=np.inf, relu=np.inf)


q_values = S.bound(S.q_values, LEGS, "masks")
ff_step, rec_step = S.bound(S.ff_step, LEGS, "masks"), S.bound(S.rec_step, LEGS, "masks")


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


def first_step(c, seed=None):
    """(network data, fp64 batch, masks) of the case's first step"""
    D, batch = S.first_step(c, seed)
    return D, batch, masks_for(D.net, 0, c.B, c.T)


def step(c, D, batch, masks, **kw):
    return (rec_step if c.T else ff_step)(D.net, D.p_on, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq), masks, **kw)


def case_margins(c, seed=None):
    """(sigma_min, relu margin, argmax gap) of the first step in fp64: sigma and the relu margin over the MASKED s pass under the online parameters and the unmasked s'
    passes of both networks; the gap over the columns of the network that picks the action"""
    D, batch, masks = first_step(c, seed); probe = new_probe()
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


find_seed = lambda c, cap=200: S.find_seed(c, lambda c, seed: margins_ok(c, seed) and tells_ok(c, seed), cap)


def flip_one(c, D, batch, masks):
    """the masks with ONE element flipped: in the first Dropout layer, column 0 (recurrent: t = 0, b = 0), the feature where the layer's input is largest in magnitude
    (an element whose input is 0 -- a dead relu -- changes nothing under any mask)"""
    probe = new_probe(); l = min(masks)
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
