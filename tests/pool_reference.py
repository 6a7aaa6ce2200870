"""fp64 reference for networks with Flux MaxPool / MeanPool layers (TEST INFRASTRUCTURE).  oracle/dqn_oracle.Network cannot describe a pool (its chains
index two parameter arrays per layer), so this module carries a network description of its own -- oracle Dense / Conv layers plus Pool, held in an
oracle Network for shapes and parameter order -- and two fp64 legs that share no pooling code:

  * step_torch -- torch float64 autograd: F.max_pool2d / F.avg_pool2d inside the flipped-kernel conv chain of feedforward_reference._chain;
  * step_numpy -- a NumPy forward (the window's taps stacked in (ky, kx) order) and a hand-written backward (MaxPool: dY to the FIRST tap that holds
    the maximum, np.argmax's rule and torch's; MeanPool: dY / (kh*kw) to every tap), around oracle layer_forward / layer_backward for Dense and Conv.

tests/test_pool_cpu.py holds the legs to 1e-10 of each other on every case of the table below.  Tolerances are those of feedforward_edges_common and
recurrent_reference, unchanged.  A MaxPool is a second non-smooth point beside relu: margins() states the rule test data must satisfy, prepare() draws
from the case's FIXED seed and asserts it (no redraw, no skip at run time); the seeds were found on the CPU with this reference alone (find_seed)."""
import types

import numpy as np
import torch
import torch.nn.functional as F

import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_reference as FR
import ref
from test_twin_vs_oracle import check_priorities_after_step

abi = ref.abi
I, RELU, TANH, SIG = O.ACT_IDENTITY, O.ACT_RELU, O.ACT_TANH, O.ACT_SIGMOID
LR = E.LR


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


def layer_descs(net):
    """the network as dqn_layer_desc records (ref.layers_from_network knows no pool)"""
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


# ------------------------------------------------------------------ NumPy leg
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
            if hook:
                lin = O.Dense(l.n_in, l.n_out, I) if l.kind == "dense" else O.Conv((l.kh, l.kw), l.cin, l.cout, I, (l.sh, l.sw))
                hook(l, x, O.layer_forward(lin, x, W, b)[0])
            y, c = O.layer_forward(l, x, W, b)
            caches.append((c, shp, y, W))
        x = y
    return x, caches, k


def _bwd(layers, caches, dy):
    grads = []
    for l, (c, shp, y, W) in zip(reversed(layers), reversed(caches)):
        if is_pool(l):
            dy = pool_backward(l, c, shp, dy.reshape(y.shape))
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


# ------------------------------------------------------------------ torch leg: feedforward_reference.step_torch with a chain that knows pools
def _chain_t(layers, ps, x):
    k = 0
    for l in layers:
        if is_pool(l):
            x = (F.max_pool2d if l.kind == "maxpool" else F.avg_pool2d)(x, (l.kh, l.kw), stride=(l.sh, l.sw))
        else:
            x = FR._chain([l], ps[k:k + 2], x); k += 2
    return x, k


def _q_t(net, ps, x):
    xb, k = _chain_t(net.base, ps, x)
    if not net.dueling:
        return xb
    v, kv = _chain_t(net.val, ps[k:], xb)
    a, _ = _chain_t(net.adv, ps[k + kv:], xb)
    return v + a - a.mean(dim=1, keepdim=True)


def step_torch(net, p_on, p_tg, batch, gamma, double_q):
    """feedforward_reference.step_torch, restated around _q_t (that function is bound to its module's pool-less forward)"""
    s, a, r, sp, done, w = batch
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    s, sp, r, done, w = t(s), t(sp), t(r), t(done), t(w)
    a = torch.tensor(np.asarray(a, np.int64)); B = s.shape[0]
    pon = [t(p).requires_grad_(True) for p in net.unflatten(np.asarray(p_on, np.float64))]
    ptg = [t(p) for p in net.unflatten(np.asarray(p_tg, np.float64))]
    with torch.no_grad():       # the targets are constants of the loss (src/solver.jl:209-217)
        q_tg_sp = _q_t(net, ptg, sp)
        q_on_sp = _q_t(net, pon, sp) if double_q else q_tg_sp
        best = (q_on_sp == q_on_sp.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)      # first-max rule of Julia's argmax
        y = r + (1.0 - done) * float(gamma) * q_tg_sp[torch.arange(B), best]
    q = _q_t(net, pon, s)
    td = q[torch.arange(B), a] - y
    x = w * td; ab = x.abs(); qd = torch.clamp(ab, max=1.0)
    loss = (0.5 * qd * qd + (ab - qd)).sum() / B        # src/helpers.jl:14-19, src/solver.jl:223-224
    loss.backward()
    g = np.concatenate([p.grad.numpy().reshape(-1) for p in pon])
    return dict(q_on_s=q.detach().numpy(), q_on_sp=q_on_sp.numpy(), q_tg_sp=q_tg_sp.numpy(), best_a=best.numpy(), y=y.numpy(), td=td.detach().numpy(),
                loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()))


# ------------------------------------------------------------------ the margins
def margins(net, p_on, s):
    """(relu margin, pool margin) of the online net on s in fp64.  relu: the smallest |pre-activation| over the relu units (feedforward_reference.relu_margin).
    MaxPool: over all windows, the gap between the top two taps -- except windows whose maximum is an exact 0 out of a relu (every tap of such a window is that
    relu's 0, the first takes dY and relu' = 0 drops it in both precisions; the relu's own margin keeps its units off the kink)."""
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
    _q_np(net, net.unflatten(np.asarray(p_on, np.float64)), np.asarray(s, np.float64), hook)
    return tuple(best)


# ------------------------------------------------------------------ cases
def case(name, obs, layers, B, seed, dueling=False, u8=0, graph=1, live=True, zero_conv=False):
    return types.SimpleNamespace(name=name, obs=tuple(obs), layers=layers, B=B, seed=seed, dueling=dueling, u8=u8, graph=graph, live=live, zero_conv=zero_conv,
                                 mfma=1, prio=1, dq=1, gamma=0.95, dup=False)


def network(c):
    ls = c.layers()
    return O.Network(c.obs, *O.create_dueling_network(ls)) if c.dueling else O.Network(c.obs, ls)


def hparams(c, net, graph=None):
    return ref.hparams_for(net, batch_size=c.B, buffer_size=c.B + 24, learning_rate=LR, gamma=c.gamma, double_q=c.dq, prioritized_replay=c.prio, obs_dtype=c.u8,
                           use_mfma=c.mfma, use_graph=c.graph if graph is None else graph, seed=5)


def _draw(c, net, seed, steps):
    """feedforward_edges_common._draw with this module's init_params"""
    rng = np.random.default_rng(seed); n = c.B + 24
    if c.u8:
        s, sp = (rng.integers(0, 256, (n,) + net.obs_shape).astype(np.uint8) for _ in range(2))
    else:
        s, sp = (rng.random((n,) + net.obs_shape, dtype=np.float32) for _ in range(2))
    a = rng.integers(0, net.n_actions, n).astype(np.int32); r = (2 * rng.standard_normal(n)).astype(np.float32); d = (rng.random(n) < 0.2).astype(np.uint8)
    p_on = O.Network.flatten(init_params(net, seed)); p_on = (p_on + 0.02 * rng.standard_normal(p_on.shape)).astype(np.float32)
    if c.zero_conv:      # the exact-tie case: the first conv has all-zero weights and a non-zero bias, so every window of the pool behind it ties in both precisions
        l0 = net.base[0]; nw = int(np.prod(l0.param_shapes()[0]))
        p_on[:nw] = 0.0; p_on[nw:nw + l0.cout] = np.linspace(0.25, 0.75, l0.cout, dtype=np.float32)
    p_tg = (p_on + 0.05 * rng.standard_normal(p_on.shape)).astype(np.float32)
    return dict(s=s, sp=sp, a=a, r=r, d=d, p_on=p_on, p_tg=p_tg, idx=[rng.choice(n, c.B, replace=False).astype(np.int64) for _ in range(steps)])


def trajectory_ok(c, net, D, steps):
    """along an fp64 trajectory of the steps: argmax gaps > 2 GAP, relu and MaxPool margins > 2 RELU_MARGIN, (first step) no dead gradient block"""
    p = D["p_on"].astype(np.float64); adam = FR.Adam(p.size, lr=LR)
    prio = O.priority_from_td(np.abs(D["r"]), np.float32(1e-3), np.float32(0.6)).astype(np.float64)
    for k in range(steps):
        batch = E._fp64_batch(c, D, D["idx"][k], prio)
        o = step_numpy(net, p, D["p_tg"], batch, float(np.float32(c.gamma)), c.dq)
        rm, pm = margins(net, p, batch[0])
        if not (E._gap(o["q_on_sp"]) > 2 * E.GAP and rm > 2 * E.RELU_MARGIN and (c.zero_conv or pm > 2 * E.RELU_MARGIN) and (k > 0 or not c.live or not FR.dead_blocks(net, o["grads"]))):
            return False
        prio[D["idx"][k]] = O.priority_from_td(np.abs(o["td"]), np.float32(1e-3), np.float32(0.6), np.float64)
        p = adam.step(p, o["grads"])
    return True


_PREP = {}


def prepare(c, steps=3):
    """the case's data from its FIXED seed; the margins are asserted, never redrawn"""
    if c.name not in _PREP:
        net = network(c); D = _draw(c, net, c.seed, steps)
        assert trajectory_ok(c, net, D, steps), f"{c.name}: seed {c.seed} does not keep the margins (pool_reference.find_seed)"
        _PREP[c.name] = (net, D)
    return _PREP[c.name]


def find_seed(c, steps=3, cap=400):
    net = network(c)
    for seed in range(1, cap):
        if trajectory_ok(c, net, _draw(c, net, seed, steps), steps):
            return seed
    raise AssertionError(f"{c.name}: no seed below {cap} keeps the margins")


def make_handle(Engine, c, net, D, graph=None):
    hp = hparams(c, net, graph)
    h = Engine(layer_descs(net), hp)
    h.replay_add(D["s"], D["a"], D["r"], D["sp"], D["d"])
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
        assert c.zero_conv or pm > E.RELU_MARGIN, f"{msg}: a MaxPool window of the fp64 reference is a near-tie"
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


def replay_steps(Engine, c, steps=3, graph=None, net_D=None):
    """the case's steps on another handle, unchecked: the record only (net_D: another network on the case's data -- the 1x1-window case)"""
    net, D = net_D or prepare(c, steps)
    h, _ = make_handle(Engine, c, net, D, graph=graph)
    rec = []
    for k in range(steps):
        loss, gn, td = h.train_step(D["idx"][k])
        rec.append(dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities()))
    h.close()
    return rec


# ------------------------------------------------------------------ the table: the smallest shapes at which each path of pool.hip / the program can go wrong
# seeds: found with find_seed on the CPU, with this reference alone; fixed here
SEEDS = {'max_c16': 2400, 'max_c3': 2, 'mean_c16': 1584, 'between': 303, 'overlap_max': 3, 'overlap_mean': 2, 'gaps_max': 1, 'gaps_mean': 2, 'whole_max': 1, 'whole_mean': 1,
         'one_max': 1, 'one_mean': 1, 'first_max_f32': 3, 'first_mean_u8': 1, 'dueling_max': 21, 'b5_max': 1, 'b5_mean': 1, 'b16_max': 2, 'b128_max': 6, 'b128_mean': 4, 'ties': 1}


def _net(conv, pool, feat, nA=4, hidden=32):
    """Conv -> pool -> Dense(feat, hidden, relu) -> Dense(hidden, nA)"""
    return lambda: [conv(), pool(), O.Dense(feat, hidden, RELU), O.Dense(hidden, nA)]


def _c(name, obs, layers, B, **kw):
    return case(name, obs, layers, B, SEEDS.get(name, 1), **kw)


c3 = lambda cin, cout, act=RELU: (lambda: O.Conv(3, cin, cout, act))
CASES = [
    # 1. Conv(3, 1=>16, relu) -> pool(2) -> Dense -> Dense on 1x10x10 (8x8 map -> 4x4), B = 32: the LDS / MFMA conv family; cout = 3: the VALU family; MeanPool
    _c("max_c16", (1, 10, 10), _net(c3(1, 16), lambda: MaxPool(2), 256), 32),
    _c("max_c3", (1, 10, 10), _net(c3(1, 3), lambda: MaxPool(2), 48), 32),
    _c("mean_c16", (1, 10, 10), _net(c3(1, 16), lambda: MeanPool(2), 256), 32),
    # 2. pools between convs on 2x15x14: 13x12 -> 6x6 -> 4x4 -> 2x2; the upper conv's dX lands in a pool's dY
    _c("between", (2, 15, 14), lambda: [O.Conv(3, 2, 8, RELU), MaxPool(2), O.Conv(3, 8, 8, RELU), MeanPool(2), O.Dense(32, 4)], 32),
    # 3. overlapping rectangular windows and an uncovered edge behind a conv whose map is 8x7 (MaxPool (3,2)/(2,1): row 7 is in no window)
    _c("overlap_max", (1, 10, 9), _net(c3(1, 4), lambda: MaxPool((3, 2), (2, 1)), 4 * 3 * 6), 32),
    _c("overlap_mean", (1, 10, 9), _net(c3(1, 4), lambda: MeanPool((2, 3), (1, 2)), 4 * 7 * 3), 32),
    # 4. gaps: window 2, stride 3 (8x8 -> 3x3; rows / columns 2 and 5 are in no window)
    _c("gaps_max", (1, 10, 10), _net(c3(1, 4), lambda: MaxPool(2, 3), 36), 32),
    _c("gaps_mean", (1, 10, 10), _net(c3(1, 4), lambda: MeanPool(2, 3), 36), 32),
    # 5. the window is the whole map: 1x1 output
    _c("whole_max", (1, 10, 10), _net(c3(1, 4), lambda: MaxPool(8), 4), 32),
    _c("whole_mean", (1, 10, 10), _net(c3(1, 4), lambda: MeanPool(8), 4), 32),
    # 6. window 1x1, stride 1: bit for bit the network without the layer (test_pool_gpu.py)
    _c("one_max", (1, 10, 10), _net(c3(1, 4), lambda: MaxPool(1), 256), 32),
    _c("one_mean", (1, 10, 10), _net(c3(1, 4), lambda: MeanPool(1), 256), 32),
    # 7. a pool as the first layer (fp32 arena; no input gradient), with an f32 and with a u8 replay
    _c("first_max_f32", (2, 8, 8), lambda: [MaxPool(2), O.Conv(3, 2, 4, RELU), O.Dense(16, 4)], 32),
    _c("first_mean_u8", (2, 8, 8), lambda: [MeanPool(2), O.Conv(3, 2, 4, RELU), O.Dense(16, 4)], 32, u8=1),
    # 8. dueling: the pool is the last base layer, the join's summed dX is its dY
    _c("dueling_max", (1, 10, 10), lambda: [O.Conv(3, 1, 4, RELU), MaxPool(2), O.Dense(64, 16, RELU), O.Dense(16, 4)], 32, dueling=True),
    # 9. column edges: B = 5 (ten columns, the target pass starts at column 5: the scalar path), 16, and 128 (the large-batch schedule)
    _c("b5_max", (1, 6, 6), _net(c3(1, 3), lambda: MaxPool(2), 12, hidden=16), 5),
    _c("b5_mean", (1, 6, 6), _net(c3(1, 3), lambda: MeanPool(2), 12, hidden=16), 5),
    _c("b16_max", (1, 6, 6), _net(c3(1, 3), lambda: MaxPool(2), 12, hidden=16), 16),
    _c("b128_max", (1, 6, 6), _net(c3(1, 3), lambda: MaxPool(2), 12, hidden=16), 128),
    _c("b128_mean", (1, 6, 6), _net(c3(1, 3), lambda: MeanPool(2), 12, hidden=16), 128),
    # 10. exact ties: an all-zero conv with a non-zero bias and identity activation -- every MaxPool window ties in both precisions.  This case PINS the tie
    #     rule: both legs (np.argmax, torch) route dY to the first tap, and the conv's dW / db must match them
    _c("ties", (1, 10, 10), _net(c3(1, 4, I), lambda: MaxPool(2), 64), 32, zero_conv=True),
]
BY_NAME = {c.name: c for c in CASES}


def without_pool(c):
    """the network of a 1x1-window case with the pool layer taken out (same parameters, same data)"""
    ls = [l for l in c.layers() if not is_pool(l)]
    return O.Network(c.obs, *O.create_dueling_network(ls)) if c.dueling else O.Network(c.obs, ls)


# ------------------------------------------------------------------ recurrent chains with a conv trunk: Conv -> pool -> LSTM -> Dense (package nn descriptors, as recurrent_reference)
import recurrent_reference as R      # noqa: E402
from gru_reference import param_arrays      # noqa: E402


def _rec_q(net, nn, arrs, x, hs):
    """one time step of a plain chain; x (B, C, H, W); hs as recurrent_reference.init_state gives it"""
    for i, l in enumerate(net.layers):
        a = arrs[i]
        if l.kind == "conv":
            x = FR._act(F.conv2d(x, a[0].flip(2, 3), a[1], stride=(l.sh, l.sw)), l.act)
        elif l.kind in ("maxpool", "meanpool"):
            x = (F.max_pool2d if l.kind == "maxpool" else F.avg_pool2d)(x, (l.kh, l.kw), stride=(l.sh, l.sw))
        elif l.kind == "lstm":
            hs[i] = R.lstm_cell(x.reshape(x.shape[0], -1), hs[i][0], hs[i][1], a[0], a[1], a[2]); x = hs[i][0]
        else:
            x = FR._act(x.reshape(x.shape[0], -1) @ a[0] + a[1], l.act)
    return x


def _rec_seq(net, nn, arrs, xs):
    hs = R.init_state(net, nn, arrs, xs[0].shape[0])
    return [_rec_q(net, nn, arrs, x, hs) for x in xs]


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
        x = t64(m[t]) * (qs[t][torch.arange(B), torch.tensor(a[t].astype(np.int64))] - t64(ys[t]))
        ab = x.abs(); q = torch.clamp(ab, max=1.0)
        loss = loss + (0.5 * q * q + (ab - q)).sum() / B
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


def rec_margins(net, nn, p_on, s, mask):
    """(relu, MaxPool) margins of the conv trunk on the s columns (T, B, C, H, W), as margins() states them -- over the columns the mask keeps: a padded
    column (all-zero observation, every window tied at the bias) carries mask 0 inside the Huber, so no gradient reaches its windows"""
    l0, l1 = net.layers[0], net.layers[1]
    arrs = param_arrays(net, nn, p_on)
    x = np.asarray(s, np.float64).reshape((-1,) + tuple(REC.obs))[np.asarray(mask).reshape(-1) > 0]
    pre = O.layer_forward(O.Conv((l0.kh, l0.kw), l0.cin, l0.cout, I, (l0.sh, l0.sw)), x, arrs[0][0].numpy(), arrs[0][1].numpy())[0]
    t = np.sort(_taps(Pool(l1.kind, (l1.kh, l1.kw), (l1.sh, l1.sw)), np.maximum(pre, 0.0))[0], axis=0)
    gap = np.where(t[-1] == 0.0, np.inf, t[-1] - t[-2])
    return float(np.abs(pre).min()), float(gap.min())


REC = types.SimpleNamespace(obs=(1, 5, 5), nA=4, B=4, T=3, gamma=0.95, double_q=1, seed=3, steps=3)      # case 11: Conv(2, 1=>8, relu) -> MaxPool(2) -> LSTM(32, 8) -> Dense(8, 4)


def rec_net(nn):
    return nn.Chain(nn.Conv(2, 1, 8, nn.relu), nn.MaxPool(2), nn.LSTM(32, 8), nn.Dense(8, REC.nA))


def rec_data(nn, seed=None):
    """episodes, the ring they end up in, parameters and the draws of the steps: deterministic from the seed (as test_recurrent_edges_gpu builds its cases)"""
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
    """the margins (2x) along the fp64 trajectory of the case's steps, with the reference alone"""
    net, cap, eps, ring, p_on, p_tg, dr = rec_data(nn, seed)
    p = p_on.astype(np.float64); adam = R.Adam(p.size)
    for idx, start in dr:
        batch = R.sample_batch(ring, idx, start, REC.T, REC.obs)
        rm, pm = rec_margins(net, nn, p, batch[0], batch[5])
        if not (rm > 2 * E.RELU_MARGIN and pm > 2 * E.RELU_MARGIN):
            return False
        p = adam.step(p, rec_train_grads(net, nn, p, p_tg, batch, float(np.float32(REC.gamma)), True)["grads"])
    return True
