"""fp64 torch reference for recurrent Q-networks of ANY recurrent chain (TEST INFRASTRUCTURE): plain or dueling chains that mix nn.Dense,
nn.LSTM, nn.GRU and nn.RNN (any σ), with any number of recurrent layers in the base chain.  The state is per layer: (h, c) for an LSTM, h for a
GRU or an RNN.  It provides the recurrent batch_train! of src/solver.jl:239-287 on a given sampled batch (mask inside the Huber, /B then /T,
state reset for every sequence set; autograd through the whole sequence), the policy's q_step / init_state and the dqn_get_hidden layout, an
fp64 Adam carried across steps, and a gradient check per parameter block.  The GRU and RNN cells are those of gru_reference.py and
rnn_reference.py; the LSTM cell is the oracle's (dqn_oracle._seq_forward: gates i, f, g, o)."""
import numpy as np
import torch

import dqn_oracle as O
from gru_reference import _act, gru_cell, param_arrays
from rnn_reference import rnn_cell

F64 = torch.float64
RECURRENT = ("lstm", "gru", "rnn")


def lstm_cell(x, h, c, Wi, Wh, b):
    """x: (B, in), h, c: (B, H); Wi: (in, 4H), Wh: (H, 4H), b: (4H,) -- the C-order views of Flux's Wi (4H, in), Wh (4H, H); gates i, f, g, o"""
    H = h.shape[1]
    g = x @ Wi + h @ Wh + b
    i, f, gc, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
    c = f * c + i * gc
    return o * torch.tanh(c), c


def _chain_step(layers, arrs, x, hs, li0):
    """one time step through a chain; hs: dict layer index -> state (h for a GRU / RNN, (h, c) for an LSTM), updated in place"""
    for i, l in enumerate(layers):
        a, k = arrs[li0 + i], li0 + i
        if l.kind == "lstm":
            hs[k] = lstm_cell(x, hs[k][0], hs[k][1], a[0], a[1], a[2])
            x = hs[k][0]
        elif l.kind == "gru":
            hs[k] = x = gru_cell(x, hs[k], a[0], a[1], a[2])
        elif l.kind == "rnn":
            hs[k] = x = rnn_cell(x, hs[k], a[0], a[1], a[2], l.act)
        else:
            x = _act(x @ a[0] + a[1], l.act)
    return x


def recurrent_layers(net, nn):
    return [i for i, l in enumerate(nn.all_layers(net)) if l.kind in RECURRENT]


def init_state(net, nn, arrs, n):
    """Flux.reset!: every layer's state0, broadcast over n streams"""
    out = {}
    for i in recurrent_layers(net, nn):
        h = arrs[i][3].reshape(1, -1).expand(n, -1).clone()
        out[i] = (h, arrs[i][4].reshape(1, -1).expand(n, -1).clone()) if nn.all_layers(net)[i].kind == "lstm" else h
    return out


def q_step(net, nn, arrs, x, hs):
    """Q(s) for one step (B, nA); advances hs"""
    if isinstance(net, nn.DuelingNetwork):
        nb, nv = len(net.base.layers), len(net.val.layers)
        y = _chain_step(net.base.layers, arrs, x, hs, 0)
        v = _chain_step(net.val.layers, arrs, y, hs, nb)
        a = _chain_step(net.adv.layers, arrs, y, hs, nb + nv)
        return v + a - a.mean(dim=1, keepdim=True)      # src/dueling.jl:10
    return _chain_step(net.layers, arrs, x, hs, 0)


def seq_q(net, nn, arrs, xs):
    hs = init_state(net, nn, arrs, xs[0].shape[0])
    return [q_step(net, nn, arrs, x, hs) for x in xs], hs


def hidden_layout(net, nn, hs):
    """hs -> what dqn_get_hidden returns: per recurrent layer in layer order, (h, c) for an LSTM, h for a GRU or an RNN, each (out, streams) fp64"""
    out = []
    for i in recurrent_layers(net, nn):
        st = hs[i]
        out.append((st[0].numpy().T, st[1].numpy().T) if isinstance(st, tuple) else st.numpy().T)
    return out


def state_from_layout(net, nn, saved):
    """the inverse of hidden_layout (an engine's get_hidden list -> hs, fp64)"""
    hs = {}
    for i, st in zip(recurrent_layers(net, nn), saved):
        t = lambda m: torch.tensor(np.asarray(m, np.float64).T.copy())
        hs[i] = (t(st[0]), t(st[1])) if isinstance(st, tuple) else t(st)
    return hs


def sample_batch(ring, idx, start, T, obs_shape):
    """the batch dqn_episode_get_batch returns for the given draws, (s, a, r, sp, done, mask) each (T, B, ...), from the episodes themselves"""
    return tuple(np.stack(x) for x in O.episode_sample(ring, idx, start, T, obs_shape))


def _tensors(batch):
    s, a, r, sp, d, m = batch
    T, B = s.shape[0], s.shape[1]
    xs = [torch.tensor(s[t].reshape(B, -1), dtype=F64) for t in range(T)]
    xsp = [torch.tensor(sp[t].reshape(B, -1), dtype=F64) for t in range(T)]
    return xs, xsp, T, B


def targets(net, nn, p_on, p_tg, batch, gamma, double_q):
    """the Bellman targets y[t] (B,): both nets over sp from the reset state (src/solver.jl:249-269); constants of the loss"""
    s, a, r, sp, d, m = batch
    xs, xsp, T, B = _tensors(batch)
    with torch.no_grad():
        q_tg = [q.numpy() for q in seq_q(net, nn, param_arrays(net, nn, p_tg), xsp)[0]]
        q_on_sp = [q.numpy() for q in seq_q(net, nn, param_arrays(net, nn, p_on), xsp)[0]] if double_q else q_tg
    return [O.bellman_targets(q_on_sp[t], q_tg[t], r[t].astype(np.float64), d[t].astype(np.float64), gamma, double_q)[0] for t in range(T)]


def batch_loss(net, nn, arrs, batch, ys):
    """the recurrent loss over s from the reset state (src/solver.jl:271-282): mask inside huber, /B per step, /T at the end"""
    s, a, r, sp, d, m = batch
    xs, xsp, T, B = _tensors(batch)
    qs, _ = seq_q(net, nn, arrs, xs)
    loss = torch.zeros((), dtype=F64)
    for t in range(T):
        td = qs[t][torch.arange(B), torch.tensor(a[t].astype(np.int64))] - torch.tensor(ys[t], dtype=F64)
        x = torch.tensor(m[t].astype(np.float64), dtype=F64) * td
        ab = x.abs(); q = torch.clamp(ab, max=1.0)
        loss = loss + (0.5 * q * q + (ab - q)).sum() / B       # src/helpers.jl:14-19
    return loss / T


def train_grads(net, nn, p_on, p_tg, batch, gamma, double_q):
    """loss, flat gradient (Flux.params order) and grad_norm (max |g|, src/helpers.jl:38-46) of one recurrent batch_train! at p_on"""
    ys = targets(net, nn, p_on, p_tg, batch, gamma, double_q)
    arrs = param_arrays(net, nn, p_on)
    leaves = [x for la in arrs for x in la]
    for x in leaves:
        x.requires_grad_(True)
    loss = batch_loss(net, nn, arrs, batch, ys)
    loss.backward()
    g = np.concatenate([x.grad.numpy().reshape(-1) for x in leaves])
    return dict(loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()), ys=ys)


def drqn_train_step(net, nn, p_on, p_tg, batch, gamma, double_q, lr=1e-3):
    """train_grads plus the first fp64 Adam step from p_on.  batch = (s, a, r, sp, done, mask) as returned by Engine.episode_get_batch: s, sp [T][B][obs...], the rest [T][B]"""
    o = train_grads(net, nn, p_on, p_tg, batch, gamma, double_q)
    p64 = np.asarray(p_on, np.float64)
    o["new_params"] = O.adam_update([p64], [o["grads"]], O.AdamState([p64], lr))[0]
    return o


def check_step(h, net, nn, batch, ep_idx, ep_start, gamma, double_q, p_on, p_tg):
    """one engine train step on the given draws against the fp64 reference, at check_against_oracle's tolerances (tests/drqn_common.py)"""
    o = drqn_train_step(net, nn, p_on, p_tg, batch, gamma, double_q)
    loss, gn = h.train_step_drqn(ep_idx, ep_start)
    np.testing.assert_allclose(loss, o["loss"], rtol=2e-5, atol=1e-7)
    g = h.get_grads(); sc = np.abs(o["grads"]).max() + 1e-30
    np.testing.assert_allclose(g, o["grads"], atol=3e-5 * sc, rtol=1e-4)
    np.testing.assert_allclose(gn, o["grad_norm"], rtol=1e-4)
    diff = np.abs(h.get_params(0) - o["new_params"])
    assert diff.max() <= 2.1e-3 and (diff > 5e-6).mean() < 1e-3     # Adam at |g| ~ eps moves a parameter by up to lr (tests/drqn_common.py)
    return loss, gn


def blocks(net, nn):
    """[(name, slice into the flat vector)]: the Wi, Wh, b, h0 (, c0) of each recurrent layer, the W and b of each Dense: step_reference.blocks, the one table of block names
    (imported here: that module imports this one)"""
    from step_reference import blocks
    return blocks(net)


# gradient tolerance per block: atol = GRAD_C * max(max |g_block|, 1e-2 * max |g|) plus rtol GRAD_RTOL.  GRAD_C is 4x the largest
# error / scale the MI355X showed over tests/test_recurrent_edges_gpu.py (4.8e-6, a Dense bias; recurrent blocks up to 2.4e-6, an RNN's h0)
GRAD_C, GRAD_RTOL = 2e-5, 1e-4
LIVE_BLOCK = 1e-4      # a checked block's fp64 gradient must reach this fraction of max |g|: else the block could pass vacuously
WORST = {}             # largest error / scale seen per block name while checking (for choosing GRAD_C)


def dead_blocks(net, nn, g, blks=None):
    """the blocks whose fp64 gradient is negligible (see LIVE_BLOCK); a test config must have none.  blks: the [(name, slice)] list of a network
    that blocks() does not describe (feedforward_reference.blocks: Conv and Dense layers of an oracle Network)"""
    gmax = np.abs(g).max()
    return [nm for nm, sl in (blocks(net, nn) if blks is None else blks) if not np.abs(g[sl]).max() > LIVE_BLOCK * gmax]


def check_grads(net, nn, got, want, c=GRAD_C, rtol=GRAD_RTOL, live=True, blks=None):
    """got (engine) against want (fp64) block by block.  live: also assert that no block's fp64 gradient is negligible (a config's first
    step; training may kill a block later -- a dead relu stream -- and the block is then still held to c * 1e-2 * max |g|).  blks: as in dead_blocks"""
    gmax = np.abs(want).max()
    assert gmax > 0
    for nm, sl in (blocks(net, nn) if blks is None else blks):
        w = want[sl]; bmax = np.abs(w).max()
        assert not live or bmax > LIVE_BLOCK * gmax, f"{nm}: fp64 gradient {bmax:.3g} is negligible against max |g| = {gmax:.3g}"
        scale = max(bmax, 1e-2 * gmax)
        err = np.abs(got[sl] - w)
        key = nm.split(".")[0].rstrip("0123456789") + "." + nm.split(".")[1]      # e.g. "gru.h0"
        WORST[key] = max(WORST.get(key, 0.0), float((err / (scale + rtol / c * np.abs(w))).max()))      # the smallest c that passes
        bad = err > c * scale + rtol * np.abs(w)
        assert not bad.any(), f"{nm}: {int(bad.sum())} of {w.size} elements off; worst |err| {err.max():.3g} at scale {scale:.3g} (atol {c * scale:.3g})"


class Adam:
    """Flux 0.14 Adam in fp64 throughout (m, v and the step count t kept here), applied to the engine's own gradients and previous parameters"""

    def __init__(self, n, lr=1e-3, beta=(0.9, 0.999), eps=1e-8):
        self.m, self.v, self.t = np.zeros(n), np.zeros(n), 0
        self.lr, self.b1, self.b2, self.eps = float(np.float32(lr)), beta[0], beta[1], eps

    def step(self, p, g):
        g = np.asarray(g, np.float64)
        self.t += 1
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        mh, vh = self.m / (1 - self.b1 ** self.t), self.v / (1 - self.b2 ** self.t)
        return np.asarray(p, np.float64) - mh / (np.sqrt(vh) + self.eps) * self.lr


def check_params(got, want):
    """engine parameters after Adam (fp32 m, v, rounded on store) against the fp64 Adam on the same inputs: within one fp32 spacing of the
    parameter plus 1e-8 (the m, v roundings move a step of at most a few lr by ~1e-7 of itself)"""
    tol = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 1e-8
    err = np.abs(np.asarray(got, np.float64) - want)
    assert (err <= tol).all(), f"{int((err > tol).sum())} parameters off; worst {err.max():.3g} (tol there {tol[err.argmax()]:.3g})"
