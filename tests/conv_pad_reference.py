"""fp64 reference for networks with a PADDED convolution -- Flux Conv((kh, kw), cin => cout, act; stride, pad = (ph, pw)), symmetric zero padding -- (TEST
INFRASTRUCTURE, modelled on pool_reference.py).  oracle/dqn_oracle.Conv knows no pad, so this module carries PConv (an oracle Conv with ph, pw and the padded
output shape) and two fp64 legs that share no padding code:

  * step_torch -- torch float64 autograd: F.conv2d(x, W.flip(2, 3), b, stride, padding=(ph, pw));
  * step_numpy -- oracle layer_forward / layer_backward (im2col, hand-written backward) on the np.pad-ed input, the input gradient cropped to the interior.

Pools may stand beside the conv (pool_reference's NumPy pool and its margin rule).  tests/test_conv_pad_cpu.py holds the legs to 1e-10 of each other on every case.
Tolerances are feedforward_edges_common's, unchanged.  relu and MaxPool kinks follow pool_reference.margins' rule: prepare() draws from the case's FIXED seed and
asserts the margins (no redraw, no skip at run time); the seeds were found on the CPU with this reference alone (find_seed)."""
import types

import numpy as np
import torch
import torch.nn.functional as F

import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_reference as FR
import pool_reference as PR
import ref
from test_twin_vs_oracle import check_priorities_after_step

abi = ref.abi
I, RELU, TANH, SIG = O.ACT_IDENTITY, O.ACT_RELU, O.ACT_TANH, O.ACT_SIGMOID
LR = E.LR
MaxPool, MeanPool, is_pool = PR.MaxPool, PR.MeanPool, PR.is_pool


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


# ------------------------------------------------------------------ NumPy leg: np.pad, the oracle's pad-0 conv, crop
def _plain(l, act=None):
    return O.Conv((l.kh, l.kw), l.cin, l.cout, l.act if act is None else act, (l.sh, l.sw))


def _padded(l, x):
    ph, pw = pad_of(l)
    return np.pad(x, ((0, 0), (0, 0), (ph, ph), (pw, pw)))


def _fwd(layers, ps, x, hook=None):
    caches, k = [], 0
    for l in layers:
        shp = x.shape
        if is_pool(l):
            if hook:
                hook(l, x, None)
            y, c = PR.pool_forward(l, x)
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
            dy = PR.pool_backward(l, c, shp, dy.reshape(y.shape))
        elif l.kind == "conv":
            ph, pw = pad_of(l); B, C, H, Wd = shp
            dxp, dW, db = O.layer_backward(_plain(l), c, (B, C, H + 2 * ph, Wd + 2 * pw), y, dy.reshape(y.shape), W)
            dy = dxp[:, :, ph:ph + H, pw:pw + Wd]      # the interior crop of the extended map's input gradient
            grads = [dW, db] + grads
        else:
            dy, dW, db = O.layer_backward(l, c, shp, y, dy.reshape(y.shape), W)
            grads = [dW, db] + grads
    return dy, grads


def _q_np(net, ps, x, hook=None):
    xb, cb, k = _fwd(net.base, ps, x, hook)
    if not net.dueling:
        return xb, (cb,)
    v, cv, kv = _fwd(net.val, ps[k:], xb, hook)
    a, ca, _ = _fwd(net.adv, ps[k + kv:], xb, hook)
    return v + a - a.mean(axis=1, keepdims=True), (cb, cv, ca, xb.shape)


def step_numpy(net, p_on, p_tg, batch, gamma, double_q):
    s, a, r, sp, done, w = batch
    f = lambda x: np.asarray(x, np.float64)
    s, sp, w, r, done = f(s), f(sp), f(w), f(r), f(done); B = s.shape[0]
    pon, ptg = net.unflatten(f(p_on)), net.unflatten(f(p_tg))
    q_tg_sp = _q_np(net, ptg, sp)[0]
    q_on_sp = _q_np(net, pon, sp)[0] if double_q else q_tg_sp
    y, best = O.bellman_targets(q_on_sp, q_tg_sp, r, done, float(gamma), bool(double_q))
    q, cache = _q_np(net, pon, s)
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


# ------------------------------------------------------------------ torch leg: F.conv2d's own padding
def _chain_t(layers, ps, x):
    k = 0
    for l in layers:
        if is_pool(l):
            x = (F.max_pool2d if l.kind == "maxpool" else F.avg_pool2d)(x, (l.kh, l.kw), stride=(l.sh, l.sw))
        elif l.kind == "conv":
            x = FR._act(F.conv2d(x, ps[k].flip(2, 3), ps[k + 1], stride=(l.sh, l.sw), padding=pad_of(l)), l.act); k += 2
        else:
            x = FR._act(x.reshape(x.shape[0], -1) @ ps[k] + ps[k + 1], l.act); k += 2
    return x, k


def _q_t(net, ps, x):
    xb, k = _chain_t(net.base, ps, x)
    if not net.dueling:
        return xb
    v, kv = _chain_t(net.val, ps[k:], xb)
    a, _ = _chain_t(net.adv, ps[k + kv:], xb)
    return v + a - a.mean(dim=1, keepdim=True)


def step_torch(net, p_on, p_tg, batch, gamma, double_q):
    s, a, r, sp, done, w = batch
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    s, sp, r, done, w = t(s), t(sp), t(r), t(done), t(w)
    a = torch.tensor(np.asarray(a, np.int64)); B = s.shape[0]
    pon = [t(p).requires_grad_(True) for p in net.unflatten(np.asarray(p_on, np.float64))]
    ptg = [t(p) for p in net.unflatten(np.asarray(p_tg, np.float64))]
    with torch.no_grad():
        q_tg_sp = _q_t(net, ptg, sp)
        q_on_sp = _q_t(net, pon, sp) if double_q else q_tg_sp
        best = (q_on_sp == q_on_sp.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)
        y = r + (1.0 - done) * float(gamma) * q_tg_sp[torch.arange(B), best]
    q = _q_t(net, pon, s)
    td = q[torch.arange(B), a] - y
    x = w * td; ab = x.abs(); qd = torch.clamp(ab, max=1.0)
    loss = (0.5 * qd * qd + (ab - qd)).sum() / B
    loss.backward()
    g = np.concatenate([p.grad.numpy().reshape(-1) for p in pon])
    return dict(q_on_s=q.detach().numpy(), q_on_sp=q_on_sp.numpy(), q_tg_sp=q_tg_sp.numpy(), best_a=best.numpy(), y=y.numpy(), td=td.detach().numpy(),
                loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()))


# ------------------------------------------------------------------ the margins: pool_reference.margins' rule over this module's forward
def margins(net, p_on, s):
    best = [np.inf, np.inf]; relu_out = [False]

    def hook(l, x, pre):
        if pre is not None:
            if l.act == RELU:
                best[0] = min(best[0], float(np.abs(pre).min()))
            relu_out[0] = l.act == RELU
        elif l.kind == "maxpool" and l.kh * l.kw > 1:
            t = np.sort(PR._taps(l, x)[0], axis=0)
            gap = t[-1] - t[-2]
            if relu_out[0]:
                gap = np.where(t[-1] == 0.0, np.inf, gap)
            best[1] = min(best[1], float(gap.min()))
        if pre is None and l.kind == "meanpool":
            relu_out[0] = False
    _q_np(net, net.unflatten(np.asarray(p_on, np.float64)), np.asarray(s, np.float64), hook)
    return tuple(best)


# ------------------------------------------------------------------ cases
def case(name, obs, layers, B, seed, dueling=False, u8=0, graph=1, live=True):
    return types.SimpleNamespace(name=name, obs=tuple(obs), layers=layers, B=B, seed=seed, dueling=dueling, u8=u8, graph=graph, live=live, zero_conv=False,
                                 mfma=1, prio=1, dq=1, gamma=0.95, dup=False)


def network(c):
    ls = c.layers()
    return O.Network(c.obs, *O.create_dueling_network(ls)) if c.dueling else O.Network(c.obs, ls)


def hparams(c, net, graph=None, mfma=None):
    return ref.hparams_for(net, batch_size=c.B, buffer_size=c.B + 24, learning_rate=LR, gamma=c.gamma, double_q=c.dq, prioritized_replay=c.prio, obs_dtype=c.u8,
                           use_mfma=c.mfma if mfma is None else mfma, use_graph=c.graph if graph is None else graph, seed=5)


def trajectory_ok(c, net, D, steps):
    """along an fp64 trajectory of the steps: argmax gaps > 2 GAP, relu and MaxPool margins > 2 RELU_MARGIN, (first step) no dead gradient block"""
    p = D["p_on"].astype(np.float64); adam = FR.Adam(p.size, lr=LR)
    prio = O.priority_from_td(np.abs(D["r"]), np.float32(1e-3), np.float32(0.6)).astype(np.float64)
    for k in range(steps):
        batch = E._fp64_batch(c, D, D["idx"][k], prio)
        o = step_numpy(net, p, D["p_tg"], batch, float(np.float32(c.gamma)), c.dq)
        rm, pm = margins(net, p, batch[0])
        if not (E._gap(o["q_on_sp"]) > 2 * E.GAP and rm > 2 * E.RELU_MARGIN and pm > 2 * E.RELU_MARGIN and (k > 0 or not c.live or not FR.dead_blocks(net, o["grads"]))):
            return False
        prio[D["idx"][k]] = O.priority_from_td(np.abs(o["td"]), np.float32(1e-3), np.float32(0.6), np.float64)
        p = adam.step(p, o["grads"])
    return True


_PREP = {}


def prepare(c, steps=3):
    """the case's data from its FIXED seed (pool_reference._draw: the same generator); the margins are asserted, never redrawn"""
    if c.name not in _PREP:
        net = network(c); D = PR._draw(c, net, c.seed, steps)
        assert trajectory_ok(c, net, D, steps), f"{c.name}: seed {c.seed} does not keep the margins (conv_pad_reference.find_seed)"
        _PREP[c.name] = (net, D)
    return _PREP[c.name]


def find_seed(c, steps=3, cap=400):
    net = network(c)
    for seed in range(1, cap):
        if trajectory_ok(c, net, PR._draw(c, net, seed, steps), steps):
            return seed
    raise AssertionError(f"{c.name}: no seed below {cap} keeps the margins")


def make_handle(Engine, c, net, D, graph=None, mfma=None, layers=None, plan=None, s=None, sp=None, hp_net=None):
    """layers / plan / s / sp / hp_net: the exact check's second engine (the pad-0 network on the zero-extended observations, under the padded engine's plan)"""
    hp = hparams(c, hp_net or net, graph, mfma)
    h = Engine(layer_descs(net) if layers is None else layers, hp, plan=plan)
    h.replay_add(D["s"] if s is None else s, D["a"], D["r"], D["sp"] if sp is None else sp, D["d"])
    h.set_params(D["p_on"], 0); h.set_params(D["p_tg"], 1)
    return h, hp


def run_checked(Engine, c, steps=3):
    """feedforward_edges_common.run_checked -- the same per-step checks and tolerances -- against this module's step_numpy and margins"""
    net, D = prepare(c, steps)
    h, hp = make_handle(Engine, c, net, D)
    gamma = float(np.float32(c.gamma)); adam = FR.Adam(D["p_on"].size, lr=LR); rec = []
    for k in range(steps):
        msg = f"{c.name} step {k}"; idx = D["idx"][k]
        p_prev = h.get_params(0)
        np.testing.assert_array_equal(h.get_params(1), D["p_tg"])
        batch = h.get_batch(idx)
        o = step_numpy(net, p_prev, D["p_tg"], batch, gamma, c.dq)
        pr_before = h.replay_priorities()
        E._close("is_weights", batch[5], O.is_weights(pr_before[idx], pr_before, hp.prio_beta, np.float64), rtol=2e-6, msg=msg)
        rm, pm = margins(net, p_prev, batch[0])
        assert rm > E.RELU_MARGIN, f"{msg}: a relu unit of the fp64 reference sits on its kink"
        assert pm > E.RELU_MARGIN, f"{msg}: a MaxPool window of the fp64 reference is a near-tie"
        loss, gn, td = h.train_step(idx)
        q = h.last_q()
        for key in ("q_on_s", "q_tg_sp", "q_on_sp"):
            E._close(key, q[key], o[key], msg=msg, **E.TOL_Q)
        assert E._gap(o["q_on_sp"]) > E.GAP, f"{msg}: an argmax column of the fp64 reference is a near-tie"
        np.testing.assert_array_equal(q["best_a"], o["best_a"], err_msg=msg)
        E._close("y", q["y"], o["y"], msg=msg, **E.TOL_TD)
        E._close("td", td, o["td"], msg=msg, **E.TOL_TD)
        E._close("loss", loss, o["loss"], msg=msg, **E.TOL_LOSS)
        g = h.get_grads()
        FR.check_grads(net, g, o["grads"], live=k == 0 and c.live)
        E._close("grad_norm", gn, o["grad_norm"], msg=msg, **E.TOL_GN)
        newp = h.get_params(0)
        FR.check_params(newp, adam.step(p_prev, g))
        check_priorities_after_step(h, hp, idx, pr_before, td, o["td"], batch[5])
        rec.append(dict(loss=loss, gn=gn, td=td, g=g, p=newp, q=q, pr=h.replay_priorities()))
    return h, rec


def replay_steps(Engine, c, steps=3, **kw):
    """the case's steps on another handle, unchecked: the record only"""
    net, D = prepare(c, steps)
    h, _ = make_handle(Engine, c, net, D, **kw)
    rec = []
    for k in range(steps):
        loss, gn, td = h.train_step(D["idx"][k])
        rec.append(dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities()))
    h.close()
    return rec


def extended(c, net, D):
    """the exact check's second network: the case's first (padded) conv with pad 0 on observations zero-extended by (ph, pw) -- a 0 byte border for u8.  -> (layer descs, the
    hyper-parameter view with the extended observation shape, s, sp)"""
    ph, pw = pad_of(net.base[0]); C, H, W = net.obs_shape
    ext = lambda x: np.pad(x, ((0, 0), (0, 0), (ph, ph), (pw, pw)))
    view = types.SimpleNamespace(obs_shape=(C, H + 2 * ph, W + 2 * pw), n_actions=net.n_actions, dueling=net.dueling)
    return layer_descs(net, pad=False), view, ext(D["s"]), ext(D["sp"])


# ------------------------------------------------------------------ the table: the smallest shapes at which the index math of conv_pad.hip / the program can go wrong
# seeds: found with find_seed on the CPU, with this reference alone; fixed here
SEEDS = {'same3': 1, 'all_border': 1, 'rect': 1, 'one_axis': 2, 'stride2': 1, 'aniso': 1, 'interior': 683, 'interior_tanh': 1, 'stack_same': 1, 'pool_after': 1, 'pool_before': 1, 'dueling_u8': 13}


def _c(name, obs, layers, B, **kw):
    return case(name, obs, layers, B, SEEDS.get(name, 1), **kw)


CASES = [
    # the basic border, an odd batch (ten columns, the target pass starts at column 5)
    _c("same3", (1, 5, 5), lambda: [PConv(3, 1, 4, RELU, pad=1), O.Dense(100, 4)], 5),
    # every window touches padding: 2x2 map, 3x3 kernel, pad 1 -> 2x2
    _c("all_border", (2, 2, 2), lambda: [PConv(3, 2, 3, TANH, pad=1), O.Dense(12, 4)], 8),
    # ph != pw, rectangular kernel and map: 6x7 -> 6x7
    _c("rect", (2, 6, 7), lambda: [PConv((3, 5), 2, 4, RELU, pad=(1, 2)), O.Dense(168, 4)], 16),
    # an unpadded axis beside a padded one: 6x6 -> 6x4
    _c("one_axis", (1, 6, 6), lambda: [PConv(3, 1, 4, RELU, pad=(1, 0)), O.Dense(96, 4)], 8),
    # stride 2: the extended map is 9x10, the last column of the trailing padding is dropped; dX tap divisibility.  7x8 -> 4x4
    _c("stride2", (2, 7, 8), lambda: [PConv(3, 2, 4, RELU, stride=2, pad=1), O.Dense(64, 4)], 16),
    # anisotropic stride with pad: kernel (4,3), stride (2,1), pad (1,1): 8x6 -> 4x6
    _c("aniso", (1, 8, 6), lambda: [PConv((4, 3), 1, 4, RELU, stride=(2, 1), pad=(1, 1)), O.Dense(96, 4)], 8),
    # dX THROUGH a padded conv into a relu epilogue; 16-channel MFMA tiles: 8x8 -> 6x6 -> 6x6
    _c("interior", (1, 8, 8), lambda: [O.Conv(3, 1, 16, RELU), PConv(3, 16, 16, RELU, pad=1), O.Dense(576, 4)], 32),
    # the dact_f kinds, cout 32, stride 2 on the padded layer: 8x8 -> 6x6 -> 3x3
    _c("interior_tanh", (1, 8, 8), lambda: [O.Conv(3, 1, 16, TANH), PConv(3, 16, 32, SIG, stride=2, pad=1), O.Dense(288, 4)], 16),
    # three pad-1 3x3 convs at B = 128: the dW sample-chunk path.  (smooth activations: 128 x 720 relu units per step leave no seed with every unit off its kink;
    # the relu epilogues are the other cases')
    _c("stack_same", (4, 6, 6), lambda: [PConv(3, 4, 4, TANH, pad=1), PConv(3, 4, 8, SIG, pad=1), PConv(3, 8, 8, TANH, pad=1), O.Dense(288, 4)], 128),
    # the neighbours that launch alone
    _c("pool_after", (1, 6, 6), lambda: [PConv(3, 1, 4, RELU, pad=1), MaxPool(2), O.Dense(36, 4)], 16),
    _c("pool_before", (2, 8, 8), lambda: [MeanPool(2), PConv(3, 2, 4, RELU, pad=1), O.Dense(64, 4)], 16),
    # first-layer pad 1, dueling streams, u8 replay: the byte arena, the dueling join's dX.  cout 16, K = 36: the MFMA forms read bytes
    _c("dueling_u8", (4, 6, 6), lambda: [PConv(3, 4, 16, RELU, pad=1), O.Dense(576, 16, RELU), O.Dense(16, 4)], 32, dueling=True, u8=1),
    # beyond the issue's table: 16 output channels at B = 128 -- the default plan cuts the dW chains in SAMPLES (32-aligned chunks that start inside a position) and the
    # MFMA dW walks them; smooth activation for the reason given at stack_same
    _c("b128_c16", (4, 6, 6), lambda: [PConv(3, 4, 16, TANH, pad=1), O.Dense(576, 4)], 128),
]
BY_NAME = {c.name: c for c in CASES}
FIRST_LAYER = ["same3", "all_border", "rect", "one_axis", "stride2", "aniso", "dueling_u8", "b128_c16"]      # the padded conv is the first layer: the exact check's cases


# ------------------------------------------------------------------ recurrent: Conv(3, 1=>8, relu; pad=1) -> LSTM -> Dense, T = 3, B = 4 (package nn descriptors, as pool_reference's case 11)
import recurrent_reference as R      # noqa: E402
from gru_reference import param_arrays      # noqa: E402

REC = types.SimpleNamespace(obs=(1, 5, 5), nA=4, B=4, T=3, gamma=0.95, double_q=1, seed=1, steps=3)


def rec_net(nn):
    return nn.Chain(nn.Conv(3, 1, 8, nn.relu, pad=1), nn.LSTM(200, 8), nn.Dense(8, REC.nA))


def _rec_q(net, nn, arrs, x, hs):
    for i, l in enumerate(net.layers):
        a = arrs[i]
        if l.kind == "conv":
            x = FR._act(F.conv2d(x, a[0].flip(2, 3), a[1], stride=(l.sh, l.sw), padding=(l.ph, l.pw)), l.act)
        elif l.kind == "lstm":
            hs[i] = R.lstm_cell(x.reshape(x.shape[0], -1), hs[i][0], hs[i][1], a[0], a[1], a[2]); x = hs[i][0]
        else:
            x = FR._act(x.reshape(x.shape[0], -1) @ a[0] + a[1], l.act)
    return x


def rec_train_grads(net, nn, p_on, p_tg, batch, gamma, double_q):
    """pool_reference.rec_train_grads around this module's chain (its body is bound to that module's _rec_q)"""
    s, a, r, sp, d, m = batch; T, B = s.shape[0], s.shape[1]
    t64 = lambda x: torch.tensor(np.asarray(x, np.float64))
    seq = lambda arrs, xs: (lambda hs: [_rec_q(net, nn, arrs, x, hs) for x in xs])(R.init_state(net, nn, arrs, xs[0].shape[0]))
    xs, xsp = [t64(s[t]) for t in range(T)], [t64(sp[t]) for t in range(T)]
    with torch.no_grad():
        q_tg = [q.numpy() for q in seq(param_arrays(net, nn, p_tg), xsp)]
        q_on = [q.numpy() for q in seq(param_arrays(net, nn, p_on), xsp)] if double_q else q_tg
    ys = [O.bellman_targets(q_on[t], q_tg[t], r[t].astype(np.float64), d[t].astype(np.float64), gamma, double_q)[0] for t in range(T)]
    arrs = param_arrays(net, nn, p_on); leaves = [x for la in arrs for x in la]
    for x in leaves:
        x.requires_grad_(True)
    qs = seq(arrs, xs); loss = torch.zeros((), dtype=torch.float64)
    for t in range(T):
        x = t64(m[t]) * (qs[t][torch.arange(B), torch.tensor(a[t].astype(np.int64))] - t64(ys[t]))
        ab = x.abs(); q = torch.clamp(ab, max=1.0)
        loss = loss + (0.5 * q * q + (ab - q)).sum() / B
    loss = loss / T
    loss.backward()
    g = np.concatenate([x.grad.numpy().reshape(-1) for x in leaves])
    return dict(loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()))


def rec_margin(net, nn, p_on, s, mask):
    """relu margin of the padded conv trunk on the s columns the mask keeps (pool_reference.rec_margins' rule)"""
    l0 = net.layers[0]; arrs = param_arrays(net, nn, p_on)
    x = np.asarray(s, np.float64).reshape((-1,) + tuple(REC.obs))[np.asarray(mask).reshape(-1) > 0]
    pre = O.layer_forward(O.Conv((l0.kh, l0.kw), l0.cin, l0.cout, I, (l0.sh, l0.sw)), np.pad(x, ((0, 0), (0, 0), (l0.ph, l0.ph), (l0.pw, l0.pw))), arrs[0][0].numpy(), arrs[0][1].numpy())[0]
    return float(np.abs(pre).min())


def rec_data(nn, seed=None):
    from drqn_common import draws, make_episodes
    seed = REC.seed if seed is None else seed
    net = rec_net(nn); cap = 12
    eps = make_episodes(types.SimpleNamespace(obs_shape=REC.obs, n_actions=REC.nA), cap + 3, REC.T, np.random.default_rng(seed))
    ring = [None] * cap
    for i, ep in enumerate(eps):
        ring[i % cap] = ep
    rng = np.random.default_rng(seed); n = nn.glorot_params(net, seed=3).size
    p_on = (nn.glorot_params(net, seed=3) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    p_tg = (nn.glorot_params(net, seed=4) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    rng = np.random.default_rng(seed + 100)
    return net, cap, eps, ring, p_on, p_tg, [draws(ring, REC.B, rng) for _ in range(REC.steps)]


def rec_trajectory_ok(nn, seed=None):
    net, cap, eps, ring, p_on, p_tg, dr = rec_data(nn, seed)
    p = p_on.astype(np.float64); adam = R.Adam(p.size)
    for idx, start in dr:
        batch = R.sample_batch(ring, idx, start, REC.T, REC.obs)
        if not rec_margin(net, nn, p, batch[0], batch[5]) > 2 * E.RELU_MARGIN:
            return False
        p = adam.step(p, rec_train_grads(net, nn, p, p_tg, batch, float(np.float32(REC.gamma)), True)["grads"])
    return True
