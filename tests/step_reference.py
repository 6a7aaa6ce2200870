"""fp64 reference of ONE batch_train! over the package's nn descriptors (TEST INFRASTRUCTURE), feed-forward (src/solver.jl:191-236) and recurrent (src/solver.jl:239-287),
stated ONCE: one walker through a chain of descriptors (SkipConnection recursion, the dueling join), one feed-forward and one recurrent step, the gradient blocks and their
check, the data of a case.  The per-kind modules (layernorm_reference, dropout_reference, activation_reference, skip_reference, conv_skip_reference, groupnorm_reference,
activation_layer_reference, conv_dg_reference) keep what is their own -- the law of their layer in two legs, the wrong engines, their observers, case tables and margins --
and bind the functions here to their legs (bound).

LAWS.  The walker dispatches on l.kind through one table {kind: law}, law(l, x, a, cx) -> the layer's output (a FUSED kind -- Dense, Conv, LayerNorm, GroupNorm: its
pre-activation; the walker then applies the entry "act", the fused activation).  x: the layer's input; a: its parameter arrays in Flux.params order (a "skip" entry: the
output of the block's inner chain, and the law is the join); cx: the context of the pass --
    cx.k      the layer's flat index (nn.all_layers order: what the arrays, the hidden states and the Dropout masks are keyed by)
    cx.inner  how many SkipConnection blocks the layer stands inside
    cx.hs     {flat index: hidden state} of the recurrent layers, advanced in place
    cx.masks  {flat index: keep (B, n)} of this pass's Dropout layers, or None: every Dropout layer inactive
    cx.relu   x holds the exact zeros of a relu (through MaxPools): what the MaxPool margin exempts
    cx.rows   the columns a recurrent batch's mask keeps at this time step (a bool tensor), or None: all
    cx.see    reports a tensor to the pass's probe
The default table (default_laws) covers every kind nn can build; the law code is imported from the module that states it and is not restated here.

LEGS.  A leg is a mapping {kind: law} of overrides on the default table: {} is the reference itself, {"layernorm": layernorm_law(f)} the same step with another LayerNorm.
A leg that overrides a kind the network does not hold is refused (a misspelt override would test nothing), and so is a chain with a kind the table does not know.

PROBES.  A Probe is the dict of values a pass leaves behind plus the observers that fill them, {point: fn(probe, l, t, cx)}.  The walker reports at fixed points: "in"
(every layer's input, before its law), "pre" (a fused layer's pre-activation), and a law may report what only it knows ("sigma": LayerNorm's)."""
import functools
import importlib
import types

import numpy as np
import torch
import torch.nn.functional as F

import __graft_entry__ as ge
import dqn_oracle as O
import recurrent_reference as R
from drqn_common import draws, make_episodes
from feedforward_edges_common import TOL_LOSS, TOL_Q, TOL_TD
from gru_reference import gru_cell, param_arrays
from rnn_reference import rnn_cell

nn = importlib.import_module(ge.load_package().__name__ + ".nn")
F64 = torch.float64
LR = 1e-3
RELU = 1      # DQN_ACT_RELU
RECURRENT = ("lstm", "gru", "rnn")
FUSED = ("dense", "conv", "layernorm", "groupnorm")      # the kinds that carry a fused activation l.act


# ------------------------------------------------------------------ the table of layer laws
def layernorm_law(f):
    """the table entry of a LayerNorm law f(x, scale, bias, eps) -> (pre-activation, sigma)"""
    def law(l, x, a, cx):
        pre, sigma = f(x.reshape(x.shape[0], -1), a[0], a[1], float(np.float32(l.eps)))
        cx.see("sigma", l, sigma)
        return pre
    return law


def groupnorm_law(f):
    """... of a GroupNorm law f(x, beta, gamma, G, eps) (Flux.params order: beta, THEN gamma)"""
    return lambda l, x, a, cx: f(x, a[0], a[1], l.G, float(np.float32(l.eps)))


def dropout_law(f, scale):
    """... of a Dropout law f(x, keep, scale(p)): active only where the pass has masks"""
    def law(l, x, a, cx):
        x = x.reshape(x.shape[0], -1)
        return x if cx.masks is None else f(x, torch.tensor(cx.masks[cx.k]), scale(l.p))
    return law


def act_law(f):
    """... of the fused activation f(pre-activation, code)"""
    return lambda l, x, a, cx: f(x, l.act)


def activation_law(f):
    """... of the standalone Activation layer f(x, code)"""
    return lambda l, x, a, cx: f(x, l.code)


def conv_law(f):
    """... of a convolution f(x, W, b, l), W un-flipped"""
    return lambda l, x, a, cx: f(x, a[0], a[1], l)


def _dense(l, x, a, cx):
    return x.reshape(x.shape[0], -1) @ a[0] + a[1]


def _pool(l, x, a, cx):
    return (F.max_pool2d if l.kind == "maxpool" else F.avg_pool2d)(x, (l.kh, l.kw), stride=(l.sh, l.sw))


def _adaptive_pool(l, x, a, cx):
    """GlobalMeanPool: the mean over the whole map; else Flux's rule per axis (stride = in ÷ out, k = in - (out - 1) stride: adaptive_pool_reference.resolve), then the pool"""
    if (l.kind, l.oh, l.ow) == ("adaptivemeanpool", 1, 1):
        return x.mean(dim=(2, 3), keepdim=True)
    from adaptive_pool_reference import resolve
    (kh, sh), (kw, sw) = resolve(x.shape[2], l.oh), resolve(x.shape[3], l.ow)
    return (F.max_pool2d if l.kind == "adaptivemaxpool" else F.avg_pool2d)(x, (kh, kw), stride=(sh, sw))


def _lstm(l, x, a, cx):
    h, c = cx.hs[cx.k]
    cx.hs[cx.k] = R.lstm_cell(x.reshape(x.shape[0], -1), h, c, a[0], a[1], a[2])
    return cx.hs[cx.k][0]


def _gru(l, x, a, cx):
    cx.hs[cx.k] = gru_cell(x.reshape(x.shape[0], -1), cx.hs[cx.k], a[0], a[1], a[2])
    return cx.hs[cx.k]


def _rnn(l, x, a, cx):
    cx.hs[cx.k] = rnn_cell(x.reshape(x.shape[0], -1), cx.hs[cx.k], a[0], a[1], a[2], l.act)
    return cx.hs[cx.k]


@functools.cache
def default_laws():
    """{kind: law} of every kind nn can build, plus "act", the fused activation.  (The imports stand here and not at the top: those modules import this one.)"""
    import activation_layer_reference as XR
    import activation_reference as AR
    import conv_dg_reference as CD
    import dropout_reference as DR
    import groupnorm_reference as GR
    import layernorm_reference as LN
    return {"dense": _dense, "conv": conv_law(CD.conv_torch),      # pad, dilation and groups: the general law (dilation = 1, groups = 1 is F.conv2d's default)
            "maxpool": _pool, "meanpool": _pool, "adaptivemaxpool": _adaptive_pool, "adaptivemeanpool": _adaptive_pool,
            "layernorm": layernorm_law(LN.ln_law), "groupnorm": groupnorm_law(GR.gn_torch), "dropout": dropout_law(DR.do_law, DR.do_scale),
            "activation": activation_law(XR.actl_torch), "act": act_law(AR.act_torch), "skip": lambda l, x, a, cx: a + x,      # SkipConnection(layers, +)(x) = layers(x) .+ x
            "lstm": _lstm, "gru": _gru, "rnn": _rnn}


# what cx.relu becomes behind a layer that is not FUSED (a fused one: l.act == RELU); every kind not named here: False
_KEEPS_RELU = {"maxpool": lambda l, r: r, "adaptivemaxpool": lambda l, r: r, "activation": lambda l, r: l.code == RELU}


def _chains(net):
    return (net.base, net.val, net.adv) if isinstance(net, nn.DuelingNetwork) else (net,)


def kinds(net):
    """the table entries a pass through the network reaches"""
    out = set()

    def visit(chain):
        for l in chain.layers:
            out.add(l.kind)
            if l.kind == "skip":
                visit(l.layers)
    for ch in _chains(net):
        visit(ch)
    return out | ({"act"} if out & set(FUSED) else set())


def laws_for(net, leg=None):
    """the default table under the leg's overrides; refuses a kind without a law and an override of a kind the network does not hold"""
    table, have = default_laws(), kinds(net)
    if have - set(table):
        raise ValueError(f"no law for layer kind {sorted(have - set(table))}: known are {sorted(table)}")
    if set(leg or ()) - have:
        raise ValueError(f"the leg overrides {sorted(set(leg) - have)}, which the network does not hold (it holds {sorted(have)})")
    return table | dict(leg or ())


# ------------------------------------------------------------------ probes
class Probe(dict):
    """the values a pass leaves behind, and the observers {point: fn(probe, l, t, cx)} that fill them"""

    def __init__(self, observers, **values):
        super().__init__(values)
        self.observers = observers


def kept(cx, t):
    """the columns of t a probe looks at: all, or those a recurrent batch's mask keeps (a padded column -- an all-zero observation -- carries mask 0 inside the Huber: no
    gradient reaches it and nothing of it is compared, as feedforward_reference.rec_margins has it)"""
    return t if cx.rows is None else t[cx.rows]


def probed(probe, q_values, net, p, s, **kw):
    """the probe after one pass of the module's q_values"""
    q_values(net, p, s, probe=probe, **kw)
    return probe


# ------------------------------------------------------------------ the walker
def _walk(chain, arrs, x, cx, laws):
    """one (time) step through a chain"""
    for l in chain.layers:
        if l.kind == "skip":
            x = x.view(x.shape)      # the block reads ONE tensor: the inner chain's gradient and the join's are summed, dF + dY, before they reach the producer (the engine's entry rule)
            cx.inner += 1; a = _walk(l.layers, arrs, x, cx, laws); cx.inner -= 1
            x = laws["skip"](l, x, a, cx); cx.relu = False
            continue
        cx.see("in", l, x)
        y = laws[l.kind](l, x, arrs[cx.k], cx)
        if l.kind in FUSED:
            cx.see("pre", l, y)
            x = laws["act"](l, y, None, cx); cx.relu = l.act == RELU
        else:
            x = y; cx.relu = _KEEPS_RELU.get(l.kind, lambda l, r: False)(l, cx.relu)
        cx.k += 1
    return x


def q_step(net, arrs, x, hs, *, leg=None, masks=None, probe=None, rows=None):
    """Q (B, nA) of one (time) step as a torch tensor; advances hs"""
    laws = laws_for(net, leg)
    def see(point, l, t):
        if probe is not None and point in probe.observers:
            probe.observers[point](probe, l, t, cx)
    cx = types.SimpleNamespace(k=0, inner=0, hs=hs, masks=masks, relu=False, rows=rows, see=see)
    if isinstance(net, nn.DuelingNetwork):
        y = _walk(net.base, arrs, x, cx, laws); relu = cx.relu
        v = _walk(net.val, arrs, y, cx, laws); cx.relu = relu
        a = _walk(net.adv, arrs, y, cx, laws)
        return v + a - a.mean(dim=1, keepdim=True)      # src/dueling.jl:10
    return _walk(net, arrs, x, cx, laws)


def is_recurrent(net):
    return any(l.kind in RECURRENT for l in nn.all_layers(net))


def init_state(net, arrs, n):
    """Flux.reset!: every recurrent layer's state0, broadcast over n streams"""
    out = {}
    for i, l in enumerate(nn.all_layers(net)):
        if l.kind in RECURRENT:
            h = arrs[i][3].reshape(1, -1).expand(n, -1).clone()
            out[i] = (h, arrs[i][4].reshape(1, -1).expand(n, -1).clone()) if l.kind == "lstm" else h
    return out


def _t64(x):
    return torch.tensor(np.asarray(x, np.float64))


def _at(masks, t):
    return None if masks is None else {k: v[t] for k, v in masks.items()}


def q_values(net, p, x, *, leg=None, masks=None, probe=None, mask=None):
    """Q (B, nA) as fp64 NumPy of a feed-forward network on observations x (B, ...); a recurrent network: x (T, B, ...) from the reset state -> [T] of (B, nA), with
    masks[layer][t] the Dropout mask of time step t and mask (T, B) the columns a probe looks at"""
    arrs = param_arrays(net, nn, np.asarray(p, np.float64))
    with torch.no_grad():
        if not is_recurrent(net):
            return q_step(net, arrs, _t64(x), {}, leg=leg, masks=masks, probe=probe).numpy()
        hs = init_state(net, arrs, np.asarray(x).shape[1])
        return [q_step(net, arrs, _t64(xt), hs, leg=leg, masks=_at(masks, t), probe=probe, rows=None if mask is None else torch.tensor(np.asarray(mask[t]) > 0)).numpy()
                for t, xt in enumerate(x)]


# ------------------------------------------------------------------ the two steps
def _huber(x):
    ab = x.abs(); qd = torch.clamp(ab, max=1.0)
    return 0.5 * qd * qd + (ab - qd)        # src/helpers.jl:14-19


def _grads(leaves):
    """the flat gradient in Flux.params order; an array the loss does not reach (a dead group's input) has gradient 0"""
    return np.concatenate([(x.grad if x.grad is not None else torch.zeros_like(x)).numpy().reshape(-1) for x in leaves])


def ff_step(net, p_on, p_tg, batch, gamma, double_q, *, leg=None, masks=None, where=("s",)):
    """batch = (s, a, r, sp, done, w) as get_batch returns it; everything the engine reports of one feed-forward batch_train!.  The Dropout layers are active, under
    `masks`, in the passes `where` names: ("s",), the online pass on s, is the law; "sp" (online on s') and "tg" (target) are wrong engines"""
    s, a, r, sp, done, w = batch
    s, sp, r, done, w = _t64(s), _t64(sp), _t64(r), _t64(done), _t64(w)
    a = torch.tensor(np.asarray(a, np.int64)); B = s.shape[0]
    aon, atg = param_arrays(net, nn, np.asarray(p_on, np.float64)), param_arrays(net, nn, np.asarray(p_tg, np.float64))
    at = lambda name: masks if name in where else None
    with torch.no_grad():       # the targets are constants of the loss (src/solver.jl:209-217)
        q_tg_sp = q_step(net, atg, sp, {}, leg=leg, masks=at("tg"))
        q_on_sp = q_step(net, aon, sp, {}, leg=leg, masks=at("sp")) if double_q else q_tg_sp
        best = (q_on_sp == q_on_sp.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)      # Julia's argmax: the smallest index among the maxima
        y = r + (1.0 - done) * float(gamma) * q_tg_sp[torch.arange(B), best]
    leaves = [x for la in aon for x in la]
    for x in leaves:
        x.requires_grad_(True)
    q = q_step(net, aon, s, {}, leg=leg, masks=at("s"))
    td = q[torch.arange(B), a] - y
    loss = _huber(w * td).sum() / B        # src/solver.jl:223-224
    loss.backward()
    g = _grads(leaves)
    return dict(q_on_s=q.detach().numpy(), q_on_sp=q_on_sp.numpy(), q_tg_sp=q_tg_sp.numpy(), best_a=best.numpy(), y=y.numpy(), td=td.detach().numpy(),
                loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()))


def rec_step(net, p_on, p_tg, batch, gamma, double_q, *, leg=None, masks=None, where=("s",)):
    """batch = (s, a, r, sp, done, mask), each (T, B, ...), as episode_get_batch returns it: the target loop over s' (both networks), the BPTT loop over s with a fresh
    Dropout mask per time step (masks[layer][t]); the mask inside the Huber, / B per step, / T (recurrent_reference.train_grads)"""
    s, a, r, sp, d, m = batch; T, B = s.shape[0], s.shape[1]
    at = lambda name: masks if name in where else None
    q_tg = q_values(net, p_tg, sp, leg=leg, masks=at("tg"))
    q_on = q_values(net, p_on, sp, leg=leg, masks=at("sp")) if double_q else q_tg
    ys = [O.bellman_targets(q_on[t], q_tg[t], r[t].astype(np.float64), d[t].astype(np.float64), gamma, double_q)[0] for t in range(T)]
    arrs = param_arrays(net, nn, np.asarray(p_on, np.float64)); leaves = [x for la in arrs for x in la]
    for x in leaves:
        x.requires_grad_(True)
    hs = init_state(net, arrs, B); loss = torch.zeros((), dtype=F64); tds = []
    for t in range(T):
        q = q_step(net, arrs, _t64(s[t]), hs, leg=leg, masks=_at(at("s"), t))
        td = q[torch.arange(B), torch.tensor(a[t].astype(np.int64))] - _t64(ys[t]); tds.append(td.detach().numpy())
        loss = loss + _huber(_t64(m[t]) * td).sum() / B
    loss = loss / T
    loss.backward()
    g = _grads(leaves)
    return dict(loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()), q_on_sp=q_on, q_tg_sp=q_tg, y=np.stack(ys), td=np.stack(tds))


def bound(fn, legs, *names, **fixed):
    """fn as a per-kind module exports it.  legs: the module's legs by name, each {kind: law} -- or a function that takes the whole step in fn's place (a step written out
    by hand); names: the keyword arguments of fn that the module's callers give by position, behind fn's own; a leg may also be given as the mapping itself"""
    n = fn.__code__.co_argcount

    def call(*args, **kw):
        kw = fixed | dict(zip(names, args[n:])) | kw
        assert len(args) <= n + len(names), fn.__name__
        leg = kw.pop("leg", None)
        leg = legs[leg] if isinstance(leg, str) else leg
        return leg(*args[:n], **kw) if callable(leg) else fn(*args[:n], leg=leg, **kw)
    call.__name__, call.__doc__ = fn.__name__, fn.__doc__
    return call


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


# ------------------------------------------------------------------ the gradient blocks
BLOCK_NAMES = {"dense": ("W", "b"), "conv": ("W", "b"), "lstm": ("Wi", "Wh", "b", "h0", "c0"), "gru": ("Wi", "Wh", "b", "h0"), "rnn": ("Wi", "Wh", "b", "h0"),
               "layernorm": ("scale", "bias"), "groupnorm": ("beta", "gamma"),      # Flux.params order: a GroupNorm layer holds beta, THEN gamma
               "maxpool": (), "meanpool": (), "adaptivemaxpool": (), "adaptivemeanpool": (), "dropout": (), "activation": (), "skip": ()}
_PREFIX = {"layernorm": "ln", "groupnorm": "gn"}


def blocks(net):
    """[(name, slice into the flat Flux.params vector)] in nn.all_layers order (the inner layers of a block in place, nothing for the join): <kind><i>.<array>, a LayerNorm
    layer i ln<i>.scale / ln<i>.bias, a GroupNorm layer gn<i>.beta / gn<i>.gamma"""
    out, off = [], 0
    for li, l in enumerate(nn.all_layers(net)):
        for nm, shp in zip(BLOCK_NAMES[l.kind], l.shapes()):
            k = int(np.prod(shp)); out.append((f"{_PREFIX.get(l.kind, l.kind)}{li}.{nm}", slice(off, off + k))); off += k
    return out


def dead_blocks(net, g, exempt=()):
    return [nm for nm in R.dead_blocks(net, nn, g, blks=blocks(net)) if nm not in exempt]


def check_grads(net, got, want, live=True, exempt=()):
    """recurrent_reference.check_grads per block (GRAD_C, GRAD_RTOL unchanged); live: no block's fp64 gradient is negligible, except the blocks named in `exempt` -- which
    are still held to the tolerance"""
    R.check_grads(net, nn, got, want, live=False, blks=blocks(net))
    assert not live or not dead_blocks(net, want, exempt), dead_blocks(net, want, exempt)


def grad_distance(net, got, want):
    """the largest gradient error in units of recurrent_reference.check_grads's bound (1.0 = at the bound)"""
    gmax = np.abs(want).max(); worst = 0.0
    for nm, sl in blocks(net):
        wv = want[sl]; scale = max(np.abs(wv).max(), 1e-2 * gmax)
        worst = max(worst, float((np.abs(got[sl] - wv) / (R.GRAD_C * scale + R.GRAD_RTOL * np.abs(wv))).max()))
    return worst


def distance(a, b, net=None):
    """{quantity: the largest |a - b| / tolerance} over what the GPU tests compare with the project's constants (1.0 = at the bound); with net: the gradients too, per block"""
    out = {}
    for k, tol in (("q_on_s", TOL_Q), ("q_on_sp", TOL_Q), ("q_tg_sp", TOL_Q), ("y", TOL_TD), ("td", TOL_TD)):
        if k in a and k in b:
            x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
            out[k] = float((np.abs(x - y) / (tol["atol"] + tol["rtol"] * np.abs(y))).max())
    out["loss"] = abs(a["loss"] - b["loss"]) / (TOL_LOSS["atol"] + TOL_LOSS["rtol"] * abs(b["loss"]))
    if net is not None:
        out["grads"] = grad_distance(net, a["grads"], b["grads"])
    return out


# ------------------------------------------------------------------ the data of a case
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


def first_step(c, seed=None):
    """(network data, fp64 batch) of the case's first step"""
    if c.T:
        D = rec_data(c, seed); idx, start = D.draws[0]
        return D, R.sample_batch(D.ring, idx, start, c.T, c.obs)
    D = ff_data(c, seed)
    return D, ff_batch(c, D, D.idx[0])


def _gap(q):
    t = np.sort(q, axis=1)[:, -2:]
    return float((t[:, 1] - t[:, 0]).min())


def find_seed(c, ok, cap=200):
    """the smallest seed at which the module's own predicate ok(c, seed) holds (how every table's seeds were chosen, on the CPU, with the reference alone)"""
    for seed in range(1, cap):
        if ok(c, seed):
            return seed
    raise AssertionError(f"{c.name}: no seed below {cap} keeps the margins")
