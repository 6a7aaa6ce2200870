"""fp64 torch reference for recurrent Q-networks with Flux RNN layers (TEST INFRASTRUCTURE): the plain RNN cell (Flux 0.14 RNNCell,
h' = σ.(Wi*x .+ Wh*h .+ b)), the recurrent batch_train! of src/solver.jl:239-287 on a given sampled batch (autograd through the whole
sequence), and the policy's Recur state.  Networks are the package's own nn descriptors (nn.Chain / nn.DuelingNetwork with nn.Dense and
nn.RNN layers).  The cell-agnostic helpers come from gru_reference.py."""
import numpy as np
import torch

import dqn_oracle as O
from gru_reference import _act, param_arrays

F64 = torch.float64


def rnn_cell(x, h, Wi, Wh, b, act):
    """x: (B, in), h: (B, H); Wi: (in, H), Wh: (H, H), b: (H,) -- the C-order views of Flux's Wi (H, in), Wh (H, H); act: DQN_ACT_* code"""
    return _act(x @ Wi + h @ Wh + b, act)


def _chain_step(layers, arrs, x, hs, li0):
    """one time step through a chain; hs: dict layer index -> hidden state (updated in place)"""
    for i, l in enumerate(layers):
        a = arrs[li0 + i]
        if l.kind == "rnn":
            hs[li0 + i] = rnn_cell(x, hs[li0 + i], a[0], a[1], a[2], l.act)
            x = hs[li0 + i]
        else:
            x = _act(x @ a[0] + a[1], l.act)
    return x


def init_state(net, nn, arrs, n):
    return {i: arrs[i][3].reshape(1, -1).expand(n, -1).clone() for i, l in enumerate(nn.all_layers(net)) if l.kind == "rnn"}


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


def drqn_train_step(net, nn, p_on, p_tg, batch, gamma, double_q, lr=1e-3):
    """batch = (s, a, r, sp, done, mask) as returned by Engine.episode_get_batch: s, sp [T][B][obs...], the rest [T][B]"""
    s, a, r, sp, d, m = batch
    T, B = s.shape[0], s.shape[1]
    xs = [torch.tensor(s[t].reshape(B, -1), dtype=F64) for t in range(T)]
    xsp = [torch.tensor(sp[t].reshape(B, -1), dtype=F64) for t in range(T)]
    with torch.no_grad():
        at = param_arrays(net, nn, p_tg); ao = param_arrays(net, nn, p_on)
        q_tg = [q.numpy() for q in seq_q(net, nn, at, xsp)[0]]
        q_on_sp = [q.numpy() for q in seq_q(net, nn, ao, xsp)[0]] if double_q else q_tg
    ys = [O.bellman_targets(q_on_sp[t], q_tg[t], r[t].astype(np.float64), d[t].astype(np.float64), gamma, double_q)[0] for t in range(T)]
    arrs = param_arrays(net, nn, p_on)
    leaves = [x for la in arrs for x in la]
    for x in leaves:
        x.requires_grad_(True)
    qs, _ = seq_q(net, nn, arrs, xs)
    loss = torch.zeros((), dtype=F64)
    for t in range(T):
        td = qs[t][torch.arange(B), torch.tensor(a[t].astype(np.int64))] - torch.tensor(ys[t], dtype=F64)
        x = torch.tensor(m[t].astype(np.float64), dtype=F64) * td
        ab = x.abs(); q = torch.clamp(ab, max=1.0)
        loss = loss + (0.5 * q * q + (ab - q)).sum() / B       # src/helpers.jl:14-19, mask inside huber
    loss = loss / T
    loss.backward()
    g = np.concatenate([x.grad.numpy().reshape(-1) for x in leaves])
    p64 = np.asarray(p_on, np.float64)
    st = O.AdamState([p64], lr)
    newp = O.adam_update([p64], [g], st)[0]
    return dict(loss=float(loss.detach()), grads=g, grad_norm=float(np.abs(g).max()), new_params=newp)


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
