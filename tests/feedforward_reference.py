"""fp64 reference for ONE feed-forward batch_train! (src/solver.jl:191-236) of any network of the vocabulary (TEST INFRASTRUCTURE): Dense and Conv
layers with rectangular kernels (kh, kw) and anisotropic strides (sh, sw), the four activations, plain or dueling.  Two independent legs:

  * step_numpy -- oracle/dqn_oracle.batch_train_step in float64 (im2col forward, hand-written backward);
  * step_torch -- torch float64 autograd: F.conv2d on the flipped kernel with stride=(sh, sw) (the chain of oracle/make_golden.py::torch_chain).

Both return q_on_s, q_on_sp, q_tg_sp, best_a, y, td, loss, the flat gradient in Flux.params order and grad_norm; tests/test_feedforward_edges_cpu.py
holds them to 1e-10 of each other on every case of the edge table, which pins the reference itself for rectangular kernels.  The gradient check per
parameter block, the fp64 Adam and the parameter check are those of recurrent_reference.py (one set of constants), given this module's blocks()."""
import numpy as np
import torch
import torch.nn.functional as F

import dqn_oracle as O
from recurrent_reference import GRAD_C, GRAD_RTOL, LIVE_BLOCK, WORST, Adam, check_params      # noqa: F401  (re-exported: one set of constants)
import recurrent_reference as R

F64 = torch.float64
KEYS = ("q_on_s", "q_on_sp", "q_tg_sp", "best_a", "y", "td", "loss", "grads", "grad_norm")


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


def step_numpy(net, p_on, p_tg, batch, gamma, double_q):
    """batch = (s, a, r, sp, done, w) as get_batch returns it; p_on, p_tg flat"""
    o = O.batch_train_step(net, net.unflatten(np.asarray(p_on, np.float64)), net.unflatten(np.asarray(p_tg, np.float64)), batch,
                           gamma=float(gamma), double_q=bool(double_q), adam=None)
    return dict(q_on_s=o["q"], q_on_sp=o["q_on_sp"], q_tg_sp=o["q_tg_sp"], best_a=o["best_a"], y=o["y"], td=o["td"], loss=float(o["loss"]),
                grads=O.Network.flatten(o["grads"]), grad_norm=float(o["grad_norm"]))


def relu_margin(net, p_on, s):
    """the smallest |pre-activation| over the relu units of the online net on s (fp64; inf without relu layers).  relu' jumps at 0: a unit whose fp64
    pre-activation is within fp32 round-off of 0 may be on in one precision and off in the other, and its whole gradient contribution with it -- no
    tolerance covers that, so test data is drawn until this margin clears the error a pre-activation may carry (feedforward_edges_common.RELU_MARGIN)"""
    ps = [np.asarray(x, np.float64) for x in net.unflatten(np.asarray(p_on, np.float64))]
    lin = lambda l: O.Dense(l.n_in, l.n_out, O.ACT_IDENTITY) if l.kind == "dense" else O.Conv((l.kh, l.kw), l.cin, l.cout, O.ACT_IDENTITY, (l.sh, l.sw))
    best = np.inf

    def chain(layers, ps, x):
        nonlocal best
        for i, l in enumerate(layers):
            pre, _ = O.layer_forward(lin(l), x, ps[2 * i], ps[2 * i + 1])
            if l.act == O.ACT_RELU:
                best = min(best, float(np.abs(pre).min()))
            x = O.act_fwd(pre, l.act)
        return x
    nb = 2 * len(net.base)
    xb = chain(net.base, ps[:nb], np.asarray(s, np.float64))
    if net.dueling:
        nv = 2 * len(net.val)
        chain(net.val, ps[nb:nb + nv], xb); chain(net.adv, ps[nb + nv:], xb)
    return best


def _act(x, act):
    return {O.ACT_IDENTITY: lambda v: v, O.ACT_RELU: torch.relu, O.ACT_TANH: torch.tanh, O.ACT_SIGMOID: torch.sigmoid}[act](x)


def _chain(layers, ps, x):
    for i, l in enumerate(layers):
        W, b = ps[2 * i], ps[2 * i + 1]
        if l.kind == "dense":
            x = _act(x.reshape(x.shape[0], -1) @ W + b, l.act)
        else:       # true convolution: cross-correlation with the flipped kernel; W is (cout, cin, kh, kw)
            x = _act(F.conv2d(x, W.flip(2, 3), b, stride=(l.sh, l.sw)), l.act)
    return x


def _q(net, ps, x):
    nb = 2 * len(net.base)
    xb = _chain(net.base, ps[:nb], x)
    if not net.dueling:
        return xb
    nv = 2 * len(net.val)
    v, a = _chain(net.val, ps[nb:nb + nv], xb), _chain(net.adv, ps[nb + nv:], xb)
    return v + a - a.mean(dim=1, keepdim=True)      # src/dueling.jl:10


def step_torch(net, p_on, p_tg, batch, gamma, double_q):
    s, a, r, sp, done, w = batch
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    s, sp, r, done, w = t(s), t(sp), t(r), t(done), t(w)
    a = torch.tensor(np.asarray(a, np.int64))
    B = s.shape[0]
    pon = [t(p).requires_grad_(True) for p in net.unflatten(np.asarray(p_on, np.float64))]
    ptg = [t(p) for p in net.unflatten(np.asarray(p_tg, np.float64))]
    with torch.no_grad():       # the targets are constants of the loss (src/solver.jl:209-217)
        q_tg_sp = _q(net, ptg, sp)
        q_on_sp = _q(net, pon, sp) if double_q else q_tg_sp
        src = q_on_sp if double_q else q_tg_sp      # first-max tie rule of Julia's argmax: the smallest index among the maxima
        best = (src == src.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)
        y = r + (1.0 - done) * float(gamma) * q_tg_sp[torch.arange(B), best]
    q = _q(net, pon, s)
    td = q[torch.arange(B), a] - y
    x = w * td
    ab = x.abs(); qd = torch.clamp(ab, max=1.0)
    loss = (0.5 * qd * qd + (ab - qd)).sum() / B        # src/helpers.jl:14-19, src/solver.jl:223-224
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
