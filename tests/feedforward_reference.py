"""fp64 reference for ONE feed-forward batch_train! (src/solver.jl:191-236) of any network of the vocabulary (TEST INFRASTRUCTURE): Dense layers, Conv
layers with rectangular kernels (kh, kw), anisotropic strides (sh, sw) and symmetric zero padding (ph, pw), MaxPool / MeanPool layers, the four
activations, plain or dueling.  oracle/dqn_oracle.py knows neither pad nor pools (its chains index two parameter arrays per layer), so the vocabulary
beyond it lives here -- PConv, Pool -- held in an oracle Network for shapes and parameter order.  Two independent legs that share no padding code and
no pooling code:

  * step_numpy -- the oracle's layer_forward / layer_backward (im2col forward, hand-written backward) for Dense and Conv, a padded Conv as the pad-0
    oracle conv on the np.pad-ed input with the input gradient cropped to the interior; pools as a stack of the window's taps in (ky, kx) order with a
    hand-written backward (MaxPool: dY to the FIRST tap that holds the maximum, np.argmax's rule and torch's; MeanPool: dY / (kh*kw) to every tap).
    On a network the oracle can describe it is oracle/dqn_oracle.batch_train_step operation for operation (tests/test_feedforward_edges_cpu.py: bit for bit);
  * step_torch -- torch float64 autograd: F.conv2d on the flipped kernel with stride=(sh, sw), padding=(ph, pw) (the chain of
    oracle/make_golden.py::torch_chain), F.max_pool2d / F.avg_pool2d.

Both return q_on_s, q_on_sp, q_tg_sp, best_a, y, td, loss, the flat gradient in Flux.params order and grad_norm; the CPU tests of the three case tables
(feedforward_edges_common, pool_reference, conv_pad_reference) hold them to 1e-10 of each other on every case.  The gradient check per parameter block,
the fp64 Adam and the parameter check are those of recurrent_reference.py (one set of constants), given this module's blocks().

relu and MaxPool are not smooth: margins() states the rule test data must satisfy.  The last section is the same trunk in front of an LSTM, over the
package's nn descriptors (torch autograd only, as recurrent_reference)."""
import types

import numpy as np
import torch
import torch.nn.functional as F

import dqn_oracle as O
import ref
from gru_reference import param_arrays
from recurrent_reference import GRAD_C, GRAD_RTOL, LIVE_BLOCK, WORST, Adam, check_params      # noqa: F401  (re-exported: one set of constants)
import recurrent_reference as R

abi = ref.abi
I, RELU = O.ACT_IDENTITY, O.ACT_RELU
KEYS = ("q_on_s", "q_on_sp", "q_tg_sp", "best_a", "y", "td", "loss", "grads", "grad_norm")
RELU_MARGIN = 1e-5                           # |fp64 pre-activation| of every relu unit on s: the absolute error a Q value -- a pre-activation like any other -- is held to


# ------------------------------------------------------------------ the vocabulary beyond the oracle's Dense and Conv
class Pool:
    """Flux MaxPool / MeanPool((kh, kw); pad = 0, stride = window by default): no parameters, no activation"""

    def __init__(self, kind, k, stride=None):
        self.kind = kind
        self.kh, self.kw = (k, k) if np.isscalar(k) else k
        stride = (self.kh, self.kw) if stride is None else stride
        self.sh, self.sw = (stride, stride) if np.isscalar(stride) else stride
        self.act = I

    def param_shapes(self):
        return []

    def out_shape(self, s):
        c, h, w = s
        return (c, (h - self.kh) // self.sh + 1, (w - self.kw) // self.sw + 1)


MaxPool = lambda k, stride=None: Pool("maxpool", k, stride)
MeanPool = lambda k, stride=None: Pool("meanpool", k, stride)
is_pool = lambda l: l.kind in ("maxpool", "meanpool")


class PConv(O.Conv):
    """oracle Conv + symmetric zero padding (ph, pw)"""

    def __init__(self, k, cin, cout, act=I, stride=1, pad=0):
        super().__init__(k, cin, cout, act, stride)
        self.ph, self.pw = (pad, pad) if np.isscalar(pad) else pad

    def out_shape(self, s):
        c, h, w = s
        assert c == self.cin
        return (self.cout, (h + 2 * self.ph - self.kh) // self.sh + 1, (w + 2 * self.pw - self.kw) // self.sw + 1)


pad_of = lambda l: (getattr(l, "ph", 0), getattr(l, "pw", 0))


def layer_descs(net, pad=True):
    """the network as dqn_layer_desc records; a Conv's pad rides in n_in / n_out (pad = False: the same layers with pad 0 -- the network of the exact check)"""
    out = []
    for layers, stream in ((net.base, abi.STREAM_BASE),) + (((net.val, abi.STREAM_VAL), (net.adv, abi.STREAM_ADV)) if net.dueling else ()):
        shp = net.obs_shape if stream == abi.STREAM_BASE else net.base_out_shape
        for l in layers:
            d = abi.LayerDesc(); d.act, d.stream = l.act, stream
            if l.kind == "dense":
                d.kind, d.n_in, d.n_out = abi.LAYER_DENSE, l.n_in, l.n_out
            elif is_pool(l):
                d.kind = abi.LAYER_MAXPOOL if l.kind == "maxpool" else abi.LAYER_MEANPOOL
                d.cin = d.cout = shp[0]; d.kh, d.kw, d.sh, d.sw = l.kh, l.kw, l.sh, l.sw
            else:
                d.kind = abi.LAYER_CONV; d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = l.cin, l.cout, l.kh, l.kw, l.sh, l.sw
                if pad:
                    d.n_in, d.n_out = pad_of(l)
            shp = l.out_shape(shp)
            out.append(d)
    return out


def init_params(net, seed):
    rng = np.random.default_rng(seed); ps = []
    for l in net.all_layers():
        if l.kind == "dense":
            ps += [O.glorot_uniform(rng, (l.n_in, l.n_out), l.n_in, l.n_out), np.zeros(l.n_out, np.float32)]
        elif l.kind == "conv":
            kk = l.kh * l.kw
            ps += [O.glorot_uniform(rng, (l.cout, l.cin, l.kh, l.kw), kk * l.cin, kk * l.cout), np.zeros(l.cout, np.float32)]
    return ps


def blocks(net):
    """[(name, slice into the flat Flux.params vector)]: W and b of every Conv and Dense layer, base then val then adv"""
    out, off = [], 0
    for li, l in enumerate(net.all_layers()):
        for nm, s in zip(("W", "b"), l.param_shapes()):
            k = int(np.prod(s))
            out.append((f"{l.kind}{li}.{nm}", slice(off, off + k)))
            off += k
    return out


def check_grads(net, got, want, c=GRAD_C, rtol=GRAD_RTOL, live=True):
    R.check_grads(net, None, got, want, c=c, rtol=rtol, live=live, blks=blocks(net))


def dead_blocks(net, g):
    return R.dead_blocks(net, None, g, blks=blocks(net))


# ------------------------------------------------------------------ NumPy leg: np.pad, the oracle's pad-0 conv, crop; the window's taps stacked
def _plain(l, act=None):
    return O.Conv((l.kh, l.kw), l.cin, l.cout, l.act if act is None else act, (l.sh, l.sw))


def _padded(l, x):
    ph, pw = pad_of(l)
    return np.pad(x, ((0, 0), (0, 0), (ph, ph), (pw, pw)))


def _taps(l, x):
    oh, ow = l.out_shape(x.shape[1:])[1:]
    return np.stack([x[:, :, ky:ky + l.sh * oh:l.sh, kx:kx + l.sw * ow:l.sw] for ky in range(l.kh) for kx in range(l.kw)]), oh, ow


def pool_forward(l, x):
    t, _, _ = _taps(l, x)
    return (t.max(0), t.argmax(0)) if l.kind == "maxpool" else (t.sum(0) / (l.kh * l.kw), None)      # argmax: the first tap holding the maximum


def pool_backward(l, arg, x_shape, dy):
    dx = np.zeros(x_shape, dy.dtype); oh, ow = dy.shape[2:]
    for t, (ky, kx) in enumerate((ky, kx) for ky in range(l.kh) for kx in range(l.kw)):
        dx[:, :, ky:ky + l.sh * oh:l.sh, kx:kx + l.sw * ow:l.sw] += dy * (arg == t) if l.kind == "maxpool" else dy / (l.kh * l.kw)
    return dx


def _fwd(layers, ps, x, hook=None):
    """-> output, caches, parameters consumed.  hook(layer, input, pre-activation or None): the margins look at every layer"""
    caches, k = [], 0
    for l in layers:
        shp = x.shape
        if is_pool(l):
            if hook:
                hook(l, x, None)
            y, c = pool_forward(l, x)
            caches.append((c, shp, y, None))
        else:
            W, b = ps[k], ps[k + 1]; k += 2
            xin = _padded(l, x) if l.kind == "conv" else x
            if hook:
                hook(l, x, O.layer_forward(O.Dense(l.n_in, l.n_out, I) if l.kind == "dense" else _plain(l, I), xin, W, b)[0])
            y, c = O.layer_forward(_plain(l) if l.kind == "conv" else l, xin, W, b)
            caches.append((c, shp, y, W))
        x = y
    return x, caches, k


def _bwd(layers, caches, dy):
    grads = []
    for l, (c, shp, y, W) in zip(reversed(layers), reversed(caches)):
        if is_pool(l):
            dy = pool_backward(l, c, shp, dy.reshape(y.shape))
        elif l.kind == "conv":
            ph, pw = pad_of(l); B, C, H, Wd = shp
            dxp, dW, db = O.layer_backward(_plain(l), c, (B, C, H + 2 * ph, Wd + 2 * pw), y, dy.reshape(y.shape), W)
            dy = dxp[:, :, ph:ph + H, pw:pw + Wd]      # the interior crop of the extended map's input gradient
            grads = [dW, db] + grads
        else:
            dy, dW, db = O.layer_backward(l, c, shp, y, dy.reshape(y.shape), W)
            grads = [dW, db] + grads
    return dy, grads


def q_numpy(net, ps, x, hook=None):
    """-> Q (B, nA), the caches of the backward"""
    xb, cb, k = _fwd(net.base, ps, x, hook)
    if not net.dueling:
        return xb, (cb,)
    v, cv, kv = _fwd(net.val, ps[k:], xb, hook)
    a, ca, _ = _fwd(net.adv, ps[k + kv:], xb, hook)
    return v + a - a.mean(axis=1, keepdims=True), (cb, cv, ca, xb.shape)      # src/dueling.jl:10


def step_numpy(net, p_on, p_tg, batch, gamma, double_q):
    """batch = (s, a, r, sp, done, w) as get_batch returns it; p_on, p_tg flat"""
    s, a, r, sp, done, w = batch
    f = lambda x: np.asarray(x, np.float64)
    s, sp, w, r, done = f(s), f(sp), f(w), f(r), f(done); B = s.shape[0]
    pon, ptg = net.unflatten(f(p_on)), net.unflatten(f(p_tg))
    q_tg_sp = q_numpy(net, ptg, sp)[0]
    q_on_sp = q_numpy(net, pon, sp)[0] if double_q else q_tg_sp
    y, best = O.bellman_targets(q_on_sp, q_tg_sp, r, done, float(gamma), bool(double_q))
    q, cache = q_numpy(net, pon, s)
    td = q[np.arange(B), a] - y; x = w * td
    loss = O.huber_loss(x).sum() / B
    dq = np.zeros_like(q); dq[np.arange(B), a] = w * np.clip(x, -1, 1) / B
    if net.dueling:
        cb, cv, ca, xs = cache
        dxv, gv = _bwd(net.val, cv, dq.sum(axis=1, keepdims=True)); dxa, ga = _bwd(net.adv, ca, dq - dq.mean(axis=1, keepdims=True))
        grads = _bwd(net.base, cb, (dxv + dxa).reshape(xs))[1] + gv + ga
    else:
        grads = _bwd(net.base, cache[0], dq)[1]
    g = O.Network.flatten(grads)
    return dict(q_on_s=q, q_on_sp=q_on_sp, q_tg_sp=q_tg_sp, best_a=best, y=y, td=td, loss=float(loss), grads=g, grad_norm=float(np.abs(g).max()))


# ------------------------------------------------------------------ torch leg: F.conv2d's own padding, F.max_pool2d / F.avg_pool2d
def _act(x, act):
    return {O.ACT_IDENTITY: lambda v: v, O.ACT_RELU: torch.relu, O.ACT_TANH: torch.tanh, O.ACT_SIGMOID: torch.sigmoid}[act](x)


def _layer_t(l, x, W=None, b=None):
    """one pool / Conv / Dense layer; W is (cout, cin, kh, kw): a true convolution is the cross-correlation with the flipped kernel"""
    if is_pool(l):
        return (F.max_pool2d if l.kind == "maxpool" else F.avg_pool2d)(x, (l.kh, l.kw), stride=(l.sh, l.sw))
    if l.kind == "conv":
        return _act(F.conv2d(x, W.flip(2, 3), b, stride=(l.sh, l.sw), padding=pad_of(l)), l.act)
    return _act(x.reshape(x.shape[0], -1) @ W + b, l.act)


def _chain_t(layers, ps, x):
    k = 0
    for l in layers:
        n = len(l.param_shapes())
        x = _layer_t(l, x, *ps[k:k + n]); k += n
    return x, k


def q_torch(net, ps, x):
    xb, k = _chain_t(net.base, ps, x)
    if not net.dueling:
        return xb
    v, kv = _chain_t(net.val, ps[k:], xb)
    a, _ = _chain_t(net.adv, ps[k + kv:], xb)
    return v + a - a.mean(dim=1, keepdim=True)      # src/dueling.jl:10


def _huber_t(x):
    ab = x.abs(); qd = torch.clamp(ab, max=1.0)
    return 0.5 * qd * qd + (ab - qd)        # src/helpers.jl:14-19


def step_torch(net, p_on, p_tg, batch, gamma, double_q):
    s, a, r, sp, done, w = batch
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    s, sp, r, done, w = t(s), t(sp), t(r), t(done), t(w)
    a = torch.tensor(np.asarray(a, np.int64))
    B = s.shape[0]
    pon = [t(p).requires_grad_(True) for p in net.unflatten(np.asarray(p_on, np.float64))]
    ptg = [t(p) for p in net.unflatten(np.asarray(p_tg, np.float64))]
    with torch.no_grad():       # the targets are constants of the loss (src/solver.jl:209-217)
        q_tg_sp = q_torch(net, ptg, sp)
        q_on_sp = q_torch(net, pon, sp) if double_q else q_tg_sp
        best = (q_on_sp == q_on_sp.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)      # first-max tie rule of Julia's argmax: the smallest index among the maxima
        y = r + (1.0 - done) * float(gamma) * q_tg_sp[torch.arange(B), best]
    q = q_torch(net, pon, s)
    td = q[torch.arange(B), a] - y
    loss = _huber_t(w * td).sum() / B        # src/solver.jl:223-224
    loss.backward()
    g = np.concatenate([p.grad.numpy().reshape(-1) for p in pon])
    return dict(q_on_s=q.detach().numpy(), q_on_sp=q_on_sp.numpy(), q_tg_sp=q_tg_sp.numpy(), best_a=best.numpy(), y=y.numpy(), td=td.detach().numpy(),
                loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()))


def legs_agree(a, b, rel=1e-10):
    """the two legs on one step: every quantity within rel of its own scale (gradients: of max |g|); best_a equal"""
    np.testing.assert_array_equal(a["best_a"], b["best_a"])
    for k in ("q_on_s", "q_on_sp", "q_tg_sp", "y", "td", "grads"):
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        assert x.shape == y.shape, k
        scale = max(np.abs(x).max(), 1e-300)
        assert np.abs(x - y).max() <= rel * scale, f"{k}: numpy and torch legs differ by {np.abs(x - y).max() / scale:.3g} relative"
    for k in ("loss", "grad_norm"):
        assert abs(a[k] - b[k]) <= rel * max(abs(a[k]), 1e-300), k


# ------------------------------------------------------------------ the margins
def _margins(forward):
    """forward(hook) runs a NumPy forward that shows hook every layer -> (relu margin, MaxPool margin)"""
    best = [np.inf, np.inf]; relu_out = [False]

    def hook(l, x, pre):
        if pre is not None:
            if l.act == RELU:
                best[0] = min(best[0], float(np.abs(pre).min()))
            relu_out[0] = l.act == RELU
        elif l.kind == "maxpool" and l.kh * l.kw > 1:
            t = np.sort(_taps(l, x)[0], axis=0)
            gap = t[-1] - t[-2]
            if relu_out[0]:
                gap = np.where(t[-1] == 0.0, np.inf, gap)
            best[1] = min(best[1], float(gap.min()))
        # (a MeanPool keeps relu_out: zeros stay zeros only if all taps are; a MaxPool of relu outputs is >= 0 with exact zeros only from zeros)
        if pre is None and l.kind == "meanpool":
            relu_out[0] = False
    forward(hook)
    return tuple(best)


def margins(net, p_on, s):
    """(relu margin, MaxPool margin) of the online net on s in fp64; inf without such layers.  relu: the smallest |pre-activation| over the relu units.
    relu' jumps at 0: a unit whose fp64 pre-activation is within fp32 round-off of 0 may be on in one precision and off in the other, and its whole
    gradient contribution with it -- no tolerance covers that, so test data must keep this margin above the error a pre-activation may carry (RELU_MARGIN).
    MaxPool: over all windows, the gap between the top two taps -- except windows whose maximum is an exact 0 out of a relu (every tap of such a window is that
    relu's 0, the first takes dY and relu' = 0 drops it in both precisions; the relu's own margin keeps its units off the kink)."""
    return _margins(lambda hook: q_numpy(net, net.unflatten(np.asarray(p_on, np.float64)), np.asarray(s, np.float64), hook))


# ------------------------------------------------------------------ the same trunk in front of an LSTM: Conv / pool -> LSTM -> Dense chains of package nn descriptors (as recurrent_reference)
# spec: a table's namespace (obs, nA, B, T, gamma, double_q, seed, steps; net: nn -> the chain)
def rec_q(net, nn, arrs, x, hs):
    """one time step of a plain chain; x (B, C, H, W); hs as recurrent_reference.init_state gives it"""
    for i, l in enumerate(net.layers):
        a = arrs[i]
        if l.kind == "lstm":
            hs[i] = R.lstm_cell(x.reshape(x.shape[0], -1), hs[i][0], hs[i][1], a[0], a[1], a[2]); x = hs[i][0]
        else:
            x = _layer_t(l, x, *a)
    return x


def _rec_seq(net, nn, arrs, xs):
    hs = R.init_state(net, nn, arrs, xs[0].shape[0])
    return [rec_q(net, nn, arrs, x, hs) for x in xs]


def rec_train_grads(net, nn, p_on, p_tg, batch, gamma, double_q):
    """recurrent_reference.train_grads (src/solver.jl:239-287: mask inside the Huber, /B per step, /T) for a chain with Conv and pool layers"""
    s, a, r, sp, d, m = batch; T, B = s.shape[0], s.shape[1]
    t64 = lambda x: torch.tensor(np.asarray(x, np.float64))
    xs, xsp = [t64(s[t]) for t in range(T)], [t64(sp[t]) for t in range(T)]
    with torch.no_grad():
        q_tg = [q.numpy() for q in _rec_seq(net, nn, param_arrays(net, nn, p_tg), xsp)]
        q_on = [q.numpy() for q in _rec_seq(net, nn, param_arrays(net, nn, p_on), xsp)] if double_q else q_tg
    ys = [O.bellman_targets(q_on[t], q_tg[t], r[t].astype(np.float64), d[t].astype(np.float64), gamma, double_q)[0] for t in range(T)]
    arrs = param_arrays(net, nn, p_on); leaves = [x for la in arrs for x in la]
    for x in leaves:
        x.requires_grad_(True)
    qs = _rec_seq(net, nn, arrs, xs); loss = torch.zeros((), dtype=torch.float64)
    for t in range(T):
        loss = loss + _huber_t(t64(m[t]) * (qs[t][torch.arange(B), torch.tensor(a[t].astype(np.int64))] - t64(ys[t]))).sum() / B
    loss = loss / T
    loss.backward()
    g = np.concatenate([x.grad.numpy().reshape(-1) for x in leaves])
    return dict(loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()))


def rec_blocks(net, nn):
    names = {"lstm": ("Wi", "Wh", "b", "h0", "c0"), "dense": ("W", "b"), "conv": ("W", "b"), "maxpool": (), "meanpool": ()}
    out, off = [], 0
    for li, l in enumerate(nn.all_layers(net)):
        for nm, shp in zip(names[l.kind], l.shapes()):
            k = int(np.prod(shp)); out.append((f"{l.kind}{li}.{nm}", slice(off, off + k))); off += k
    return out


def rec_margins(net, nn, spec, p_on, s, mask):
    """(relu, MaxPool) margins of the Conv / pool layers in front of the first recurrent layer on the s columns (T, B, C, H, W), as margins() states them -- over the
    columns the mask keeps: a padded column (all-zero observation, every window tied at the bias) carries mask 0 inside the Huber, so no gradient reaches its windows"""
    trunk, ps = [], []
    for l, a in zip(net.layers, param_arrays(net, nn, p_on)):
        if l.kind not in ("conv", "maxpool", "meanpool"):
            break
        trunk.append(Pool(l.kind, (l.kh, l.kw), (l.sh, l.sw)) if is_pool(l) else PConv((l.kh, l.kw), l.cin, l.cout, l.act, (l.sh, l.sw), pad_of(l)))
        ps += [x.numpy() for x in a]
    x = np.asarray(s, np.float64).reshape((-1,) + tuple(spec.obs))[np.asarray(mask).reshape(-1) > 0]
    return _margins(lambda hook: _fwd(trunk, ps, x, hook))


def rec_data(nn, spec, seed=None):
    """episodes, the ring they end up in, parameters and the draws of the steps: deterministic from the seed (as test_recurrent_edges_gpu builds its cases)"""
    from drqn_common import draws, make_episodes
    seed = spec.seed if seed is None else seed
    net = spec.net(nn); cap = 12
    eps = make_episodes(types.SimpleNamespace(obs_shape=spec.obs, n_actions=spec.nA), cap + 3, spec.T, np.random.default_rng(seed))
    ring = [None] * cap
    for i, ep in enumerate(eps):
        ring[i % cap] = ep
    rng = np.random.default_rng(seed); n = nn.glorot_params(net, seed=3).size
    p_on = (nn.glorot_params(net, seed=3) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    p_tg = (nn.glorot_params(net, seed=4) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    rng = np.random.default_rng(seed + 100)
    return net, cap, eps, ring, p_on, p_tg, [draws(ring, spec.B, rng) for _ in range(spec.steps)]


def rec_trajectory_ok(nn, spec, seed=None):
    """the margins (2x) along the fp64 trajectory of the spec's steps, with the reference alone"""
    net, cap, eps, ring, p_on, p_tg, dr = rec_data(nn, spec, seed)
    p = p_on.astype(np.float64); adam = R.Adam(p.size)
    for idx, start in dr:
        batch = R.sample_batch(ring, idx, start, spec.T, spec.obs)
        rm, pm = rec_margins(net, nn, spec, p, batch[0], batch[5])
        if not (rm > 2 * RELU_MARGIN and pm > 2 * RELU_MARGIN):
            return False
        p = adam.step(p, rec_train_grads(net, nn, p, p_tg, batch, float(np.float32(spec.gamma)), True)["grads"])
    return True
