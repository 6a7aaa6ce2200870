"""fp64 reference of ONE batch_train! for networks that carry any of the ELEVEN activations (TEST INFRASTRUCTURE), feed-forward (src/solver.jl:191-236) and recurrent
(src/solver.jl:239-287), over the package's nn descriptors: Dense, Conv (pad included), MaxPool / MeanPool, LayerNorm, Dropout and LSTM layers, plain or dueling.

The law (include/dqn_mi355x.h; NNlib's definitions with their DEFAULT parameters, recalled, not executed): identity, relu, tanh, sigmoid, and
    leakyrelu  x > 0 ? x : 0.01 x                    elu       x >= 0 ? x : expm1(x)             selu      L (x > 0 ? x : A expm1(x))
    softplus   log1p(exp(-|x|)) + max(x, 0)          softsign  x / (1 + |x|)                     relu6     min(max(x, 0), 6)            hardtanh  max(-1, min(1, x))
The codes are restated here as plain integers (the header's DQN_ACT_* values): the reference does not read them from the package it checks.

Two legs that share no activation code:
  * "torch"  torch float64 autograd over torch.nn.functional's own functions (F.leaky_relu, F.elu, F.selu, F.softplus, F.softsign, F.relu6, F.hardtanh);
  * "numpy"  the closed forms above in NumPy and, for the backward, the derivative written as a function of the OUTPUT y alone -- the column the engine runs, which keeps
             only y (dact_np) -- entered into the graph as a torch.autograd.Function.
Five WRONG engines (WRONG) are legs of their own name, each the numpy leg with one law replaced: tests/test_activations_cpu.py shows every one of them apart from the law.
A leg overrides the entry "act" (the fused activation) of step_reference's table of laws; everything that is no activation is step_reference's: the walker, the step, every
other layer's law, the gradient blocks and their check; Adam, the parameter check and the constants are imported as before.  feedforward_reference._act is neither edited nor patched.

Data rules, beside the argmax gap (GAP) of the feed-forward tables:
  * MARGIN: every fp64 pre-activation on s stays RELU_MARGIN away from each kink of its activation (KINKS: relu, leakyrelu, selu 0; relu6 0 and 6; hardtanh -1 and 1;
    elu -- alpha = 1 makes it C1 --, softplus and softsign have none): across a kink the derivative jumps, and no tolerance covers a unit that sits on different sides in
    the two precisions.
  * OCCUPANCY: each piece of each piecewise activation (PIECES) holds at least 1 / 20 of that layer's units on s -- a relu6 layer that never saturates tests relu.
The parameters are glorot draws, rescaled layer by layer (calibrate) so that the reference alone satisfies both on the case's rows: the glorot scale leaves relu6's upper
piece and most of hardtanh's empty.  This is MORE than the one `pscale` factor of the LayerNorm and Dropout tables, on purpose: one factor for the whole network cannot hold
three pieces of a relu6 occupied in two stacked layers (the second layer's inputs lie in [0, 6], and a factor that fills the first layer's upper piece empties the second
layer's middle one), and a saturating activation on the output layer needs per-action means, or two saturated actions tie the argmax exactly.  The price: a relu6 layer
always sees pre-activations of standard deviation 4 around 3, so the absolute Q errors of those cases are larger than the other tables' (docs/history/activations.md).
Seeds are fixed in the table and were found on the CPU with this module alone (find_seed); no case is skipped at run time."""


import numpy as np
import torch
import torch.nn.functional as F

import dqn_oracle as O
import dropout_reference as DR
import layernorm_reference as LR
import recurrent_reference as R
import step_reference as S
from feedforward_edges_common import GAP, TOL_GN, TOL_LOSS, TOL_Q, TOL_TD      # noqa: F401  (one set of constants, with the meaning they have there)
from feedforward_reference import GRAD_C, GRAD_RTOL, RELU_MARGIN, Adam, check_params      # noqa: F401
from step_reference import blocks, check_grads, legs_agree      # noqa: F401

nn = LR.nn
F64 = torch.float64
LRATE = LR.LR
I, RELU, TANH, SIG, LEAKYRELU, ELU, SELU, SOFTPLUS, SOFTSIGN, RELU6, HARDTANH = range(11)      # DQN_ACT_*
NAMES = ("identity", "relu", "tanh", "sigmoid", "leakyrelu", "elu", "selu", "softplus", "softsign", "relu6", "hardtanh")
NEW = (LEAKYRELU, ELU, SELU, SOFTPLUS, SOFTSIGN, RELU6, HARDTANH)
LAMBDA, ALPHA, LAMBDA_ALPHA = 1.0507009873554805, 1.6732632423543772, 1.7580993408473766
KINKS = {RELU: (0.0,), LEAKYRELU: (0.0,), SELU: (0.0,), RELU6: (0.0, 6.0), HARDTANH: (-1.0, 1.0)}
PIECES = {LEAKYRELU: (0.0,), ELU: (0.0,), SELU: (0.0,), RELU6: (0.0, 6.0), HARDTANH: (-1.0, 1.0)}      # the cuts between the pieces the occupancy rule counts
OCCUPANCY = 1.0 / 20.0


# ------------------------------------------------------------------ the two legs of an activation
def act_torch(x, a):
    return {I: lambda v: v, RELU: torch.relu, TANH: torch.tanh, SIG: torch.sigmoid, LEAKYRELU: F.leaky_relu, ELU: F.elu, SELU: F.selu,
            SOFTPLUS: lambda v: F.softplus(v, threshold=700.0),      # the default threshold = 20 returns x above it: 2e-9 off the law at x = 20
            SOFTSIGN: F.softsign, RELU6: F.relu6, HARDTANH: F.hardtanh}[a](x)


def act_np(x, a, wrong=None):
    """the closed forms, fp64"""
    x = np.asarray(x, np.float64); neg = np.minimum(x, 0.0)
    if a == I:
        return x
    if a == RELU or (a == RELU6 and wrong == "relu6_no_upper_kink"):
        return np.where(x > 0, x, 0.0)
    if a == TANH:
        return np.tanh(x)
    if a == SIG:
        return 1.0 / (1.0 + np.exp(-x))
    if a == LEAKYRELU:
        return np.where(x > 0, x, (0.1 if wrong == "leakyrelu_slope_0.1" else 0.01) * x)
    if a == ELU:
        return np.where(x >= 0, x, np.expm1(neg))
    if a == SELU:
        return (1.0 if wrong == "selu_without_lambda" else LAMBDA) * np.where(x > 0, x, ALPHA * np.expm1(neg))
    if a == SOFTPLUS:
        return np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0.0)
    if a == SOFTSIGN:
        return x / (1.0 + np.abs(x))
    if a == RELU6:
        return np.minimum(np.maximum(x, 0.0), 6.0)
    assert a == HARDTANH, a
    return np.maximum(-1.0, np.minimum(1.0, x))


def dact_np(dy, y, a, wrong=None):
    """dL/dx from dL/dy and the OUTPUT y alone (the engine keeps nothing else)"""
    if a == I:
        return dy
    if a == RELU or (a == RELU6 and wrong == "relu6_no_upper_kink") or (a == ELU and wrong == "elu_differentiated_as_relu"):
        return np.where(y > 0, dy, 0.0)
    if a == TANH:
        return dy * (1.0 - y * y)
    if a == SIG:
        return dy * (y * (1.0 - y))
    if a == LEAKYRELU:
        return np.where(y > 0, dy, (0.1 if wrong == "leakyrelu_slope_0.1" else 0.01) * dy)
    if a == ELU:
        return np.where(y >= 0, dy, dy * (y + 1.0))
    if a == SELU:
        return np.where(y > 0, dy, dy * (y + ALPHA)) if wrong == "selu_without_lambda" else np.where(y > 0, LAMBDA * dy, dy * (y + LAMBDA_ALPHA))
    if a == SOFTPLUS:
        return dy * (y * (1.0 - y)) if wrong == "softplus_differentiated_as_y(1-y)" else dy * -np.expm1(-y)      # sigmoid(x) = 1 - exp(-y)
    if a == SOFTSIGN:
        return dy * (1.0 - np.abs(y)) ** 2
    if a == RELU6:
        return np.where((y > 0) & (y < 6), dy, 0.0)
    assert a == HARDTANH, a
    return np.where((y > -1) & (y < 1), dy, 0.0)


WRONG = {"leakyrelu_slope_0.1": LEAKYRELU, "elu_differentiated_as_relu": ELU, "selu_without_lambda": SELU, "softplus_differentiated_as_y(1-y)": SOFTPLUS,
         "relu6_no_upper_kink": RELU6}      # the wrong engine -> the activation whose cases must show it


class _ActNumpy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, wrong):
        y = act_np(x.detach().numpy(), a, wrong)
        ctx.y, ctx.a, ctx.wrong = y, a, wrong
        return torch.tensor(y, dtype=F64)

    @staticmethod
    def backward(ctx, dy):
        return torch.tensor(dact_np(dy.numpy(), ctx.y, ctx.a, ctx.wrong)), None, None


def _numpy(wrong=None):
    return {"act": S.act_law(lambda x, a: _ActNumpy.apply(x, a, wrong))}


LEGS = {"torch": {}, "numpy": _numpy()} | {w: _numpy(w) for w in WRONG}      # a wrong engine is a leg of its own name


def _see_pre(probe, l, pre, cx):
    probe["pre"].setdefault(cx.k, []).append(pre.detach().numpy().copy())


OBSERVERS = {"pre": _see_pre, "sigma": LR.OBSERVERS["sigma"]}      # {"pre": {layer index: [fp64 pre-activations seen]}, "sigma": the smallest LayerNorm sigma}


def new_probe():
    return S.Probe(OBSERVERS, pre={}, sigma=np.inf)


# masks None: Dropout inactive (every pass but the online one on s)
q_values = S.bound(S.q_values, LEGS, "masks")
ff_step, rec_step = S.bound(S.ff_step, LEGS, "masks"), S.bound(S.rec_step, LEGS, "masks")


def has_dropout(net):
    return any(l.kind == "dropout" for l in nn.all_layers(net))


def masks_of(net, k, B, T=0):
    """the engine's Dropout masks of train step k (dropout_reference.masks_for), None for a network without the layer"""
    return DR.masks_for(net, k, B, T) if has_dropout(net) else None


def distance(a, b):
    """step_reference.distance, plus grad_norm and the gradients as ONE block: a lower bound of check_grads' own measure (block scale <= max |g|)"""
    out = S.distance(a, b)
    out["grad_norm"] = abs(a["grad_norm"] - b["grad_norm"]) / (TOL_GN["rtol"] * abs(b["grad_norm"]))
    ga, gb = a["grads"], b["grads"]; gmax = np.abs(gb).max()
    out["grads"] = float((np.abs(ga - gb) / (GRAD_C * max(gmax, 1e-300) + GRAD_RTOL * np.abs(gb))).max())
    return out


# ------------------------------------------------------------------ the case table
def case(name, act, mk, B, family, **kw):
    c = LR.case(name, mk, B, **kw)
    c.act, c.family = act, family
    return c


def _mlp(*dims, hact=I):
    return lambda a: nn.Chain(*[nn.Dense(dims[k], dims[k + 1], a if k + 2 < len(dims) else hact) for k in range(len(dims) - 1)])


def _before(a):
    """another new activation (the Dense layer's in front of the LayerNorm, in the ln_do family): the previous one of the seven.  The case's own activation sits on the
    LayerNorm: behind a Dense layer the normalisation would cancel selu's lambda, and no test could tell an engine without it"""
    return NEW[(NEW.index(a) - 1) % len(NEW)]


# family -> (a -> network, B, case options).  Shapes: feedforward_edges_common.BOUNDARY's smallest at each epilogue family (tests/test_activations_gpu.py asserts the
# launch class with its facts() / launches()); prio = 0 keeps the small networks off the single-launch step, which has a family of its own
FAMILIES = {
    "lds": (_mlp(32, 32, 32, 4), 32, dict(obs=(32,))),                                                    # fwd_k32: the LDS-tiled forward and dW
    "dx_wide": (_mlp(32, 32, 32, 4), 128, dict(obs=(32,))),                                               # B % 128 == 0: the 128-sample dX body (dx_mode 2) and its in-line derivative
    "valu": (_mlp(33, 32, 32, 4), 5, dict(obs=(33,))),                                                    # fwd_k33 at B = 5: the VALU forward and dW
    "mfma_u8": (_mlp(36, 32, 32, 4), 32, dict(obs=(36,), u8=1)),                                          # fwd_k36: the direct MFMA forward
    "split_k": (_mlp(1028, 32, 32, 4), 32, dict(obs=(1028,), prio=1)),                                    # fwd_k1028_b32: three split-K slabs
    "red_head": (_mlp(1028, 32, 4), 32, dict(obs=(1028,), prio=1)),                                       # ... under the head: k_red_head<TRANS>
    "head_cols4": (_mlp(64, 128, 4), 32, dict(obs=(64,))),                                                # head_k128
    "head_td": (_mlp(64, 127, 4), 32, dict(obs=(64,))),                                                   # head_k127
    "tiny": (_mlp(12, 24, 20, 4), 8, dict(obs=(12,), prio=1)),                                            # the single-launch step (and its DQN_NO_TINY twin schedule)
    "conv": (lambda a: nn.Chain(nn.Conv(3, 1, 4, a, pad=1), nn.MeanPool(2), nn.Conv(3, 4, 8, a), nn.flattenbatch, nn.Dense(32, 16, a), nn.Dense(16, 4)), 32, dict(obs=(1, 8, 8))),
    "ln_do": (lambda a: nn.Chain(nn.Dense(6, 16, _before(a)), nn.LayerNorm(16, a), nn.Dropout(0.1), nn.Dense(16, 4)), 32, dict()),
    "dueling": (lambda a: nn.create_dueling_network(_mlp(12, 24, 20, 4)(a)), 32, dict(obs=(12,), dueling=True)),       # activated hidden layers in both streams
    "hact": (lambda a: _mlp(64, 128, 4, hact=a)(TANH), 32, dict(obs=(64,))),                              # the activation on the OUTPUT layer, in k_head_cols4
    "hact_dueling": (lambda a: nn.create_dueling_network(_mlp(6, 16, 4, hact=a)(TANH)), 32, dict(dueling=True)),      # ... of the advantage stream, in head_td (the value head is Dense(16, 1))
    "lstm": (lambda a: nn.Chain(nn.LSTM(6, 8), nn.Dense(8, 12, a), nn.Dense(12, 3)), 4, dict(nA=3, T=3, pscale=3.0)),
}
SEEDS = {("dx_wide", "softsign"): 2, ("valu", "relu6"): 2, ("mfma_u8", "leakyrelu"): 3, ("head_cols4", "hardtanh"): 2, ("conv", "leakyrelu"): 2, ("hact", "hardtanh"): 3, ("hact_dueling", "relu6"): 4,
         ("hact_dueling", "hardtanh"): 5}      # (family, activation name) -> seed, where 1 does not keep twice the rules (find_seed)


def _case(fam, a):
    mk, B, kw = FAMILIES[fam]
    return case(f"{fam}_{NAMES[a]}", a, (lambda: mk(a)), B, fam, **({"prio": 0} | kw | {"seed": SEEDS.get((fam, NAMES[a]), 1)}))


CASES = [_case(fam, a) for fam in FAMILIES if fam != "lstm" for a in NEW]
REC_CASES = [_case("lstm", a) for a in NEW]
ALL = CASES + REC_CASES
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)
STEPS = 3


# ------------------------------------------------------------------ data: glorot draws, calibrated to the rules
TARGET = {RELU6: (3.0, 4.0), HARDTANH: (0.0, 1.2)}      # (mean, standard deviation) of a hidden layer's pre-activations on the case's rows; every other activation (0, 1.5)
# a SATURATING activation on the output layer: two actions saturated in one column are an exact tie of the argmax.  So the per-action means are spread: action 0 alone reaches
# the upper piece, the last action alone the lower one
TARGET_OUT = {RELU6: (lambda n: np.linspace(5.6, 0.4, n), 1.0), HARDTANH: (lambda n: np.linspace(0.85, -0.85, n), 0.4)}


def _is_output(net, k):
    ls = nn.all_layers(net)
    if isinstance(net, nn.DuelingNetwork):
        nb, nv = len(net.base.layers), len(net.val.layers)
        return k in (nb + nv - 1, len(ls) - 1)
    return k == len(ls) - 1


def calibrate(net, p, rows):
    """rescales, layer by layer in forward order, every Dense / Conv / LayerNorm layer's weights (a LayerNorm's scale) and resets its bias so that the fp64 pre-activations
    on `rows` (feed-forward: (n, ...); recurrent: (T, n, ...)) have the layer's target mean per unit and standard deviation around it (TARGET; an output layer: mean 0,
    deviation 1, or TARGET_OUT).  Deterministic; uses the reference's forward alone"""
    p = np.asarray(p, np.float64).copy(); blks = dict(blocks(net)); ls = nn.all_layers(net)
    for k, l in enumerate(ls):
        if l.kind not in ("dense", "conv", "layernorm"):
            continue
        nm = f"{'ln' if l.kind == 'layernorm' else l.kind}{k}"
        wsl, bsl = blks[nm + (".scale" if l.kind == "layernorm" else ".W")], blks[nm + (".bias" if l.kind == "layernorm" else ".b")]
        nunit = bsl.stop - bsl.start
        if _is_output(net, k):
            mean, std = (TARGET_OUT[l.act][0](nunit), TARGET_OUT[l.act][1]) if l.act in TARGET_OUT else (np.zeros(nunit), 1.0)
        else:
            m, std = TARGET.get(l.act, (0.0, 1.5)); mean = np.full(nunit, m)
        noise = p[bsl].copy(); p[bsl] = 0.0      # (the draw's bias noise comes back on top of the target mean)
        probe = new_probe(); q_values(net, p, rows, probe=probe)
        lin = np.concatenate([x.reshape((x.shape[0], nunit, -1)) for x in probe["pre"][k]])      # (rows, unit, positions)
        mu = lin.mean(axis=(0, 2)); dev = (lin - mu[None, :, None]).std()
        g = std / dev
        p[wsl] *= g; p[bsl] = mean - g * mu + noise
    return p


def _finish(c, D, rows, seed):
    rng = np.random.default_rng((c.seed if seed is None else seed) + 7919)
    D.p_on = calibrate(D.net, D.p_on, rows).astype(np.float32)
    D.p_tg = (D.p_on + 0.05 * rng.standard_normal(D.p_on.size)).astype(np.float32)
    return D


_DATA = {}


def data(c, seed=None):
    """the case's network, rows (or episodes), calibrated parameters and step indices (or draws): deterministic from the seed"""
    key = (c.name, c.seed if seed is None else seed)
    if key not in _DATA:
        if c.T:
            D = LR.rec_data(c, seed)
            _DATA[key] = _finish(c, D, _episode_rows(D, c), seed)
        else:
            D = LR.ff_data(c, seed)
            _DATA[key] = _finish(c, D, LR.ff_batch(c, D, np.arange(len(D.a)))[0], seed)
    return _DATA[key]


def _episode_rows(D, c):
    """(T, episodes, obs): the first T observations of every episode of the ring, through the sampler itself"""
    idx = np.arange(len([e for e in D.ring if e is not None]), dtype=np.int64)
    return R.sample_batch(D.ring, idx, np.zeros(len(idx), np.int32), c.T, c.obs)[0].astype(np.float64)


def step(c, D, p_on, batch, k, **kw):
    """the reference's result of train step k (k steps completed before: the Dropout mask's counter) at the parameters p_on on the given batch"""
    masks = masks_of(D.net, k, c.B, c.T)
    return (rec_step if c.T else ff_step)(D.net, p_on, D.p_tg, batch, float(np.float32(c.gamma)), bool(c.dq), masks, **kw)


def trajectory(c, D=None, steps=STEPS, seed=None, **kw):
    """the case's steps with the reference alone (fp64 Adam; fp64 priorities where the case updates them): yields (k, parameters before the step, batch, result)"""
    D = data(c, seed) if D is None else D
    p = D.p_on.astype(np.float64); adam = Adam(p.size, lr=LRATE)
    prio = None if c.T else O.priority_from_td(np.abs(D.r), np.float32(1e-3), np.float32(0.6)).astype(np.float64)
    for k in range(steps):
        if c.T:
            idx, start = D.draws[k]; batch = R.sample_batch(D.ring, idx, start, c.T, c.obs)
        else:
            ix = D.idx[k]; f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
            batch = (f(D.s[ix]), D.a[ix], D.r[ix], f(D.sp[ix]), D.d[ix].astype(np.float64), O.is_weights(prio[ix], prio, 0.4, np.float64))
        o = step(c, D, p, batch, k, **kw)
        yield k, p, batch, o
        if c.prio and not c.T:
            prio[D.idx[k]] = O.priority_from_td(np.abs(o["td"]), np.float32(1e-3), np.float32(0.6), np.float64)
        p = adam.step(p, o["grads"])


# ------------------------------------------------------------------ the rules
def rules(net, p_on, s, masks=None, mask=None):
    """(margin, occupancy, sigma_min) of the online network on the s columns in fp64.  margin: the smallest distance of a pre-activation from a kink of its activation
    (inf without kinks); occupancy: the smallest share of a layer's units that a piece of its piecewise activation holds (1 without such a layer); mask (recurrent):
    (T, B) -- the columns the loss keeps (a padded column carries no gradient)"""
    probe = new_probe(); q_values(net, p_on, s, masks, probe=probe)
    keep = None if mask is None else np.asarray(mask).reshape(-1) > 0
    margin, occ = np.inf, 1.0; ls = nn.all_layers(net)
    for k, pres in probe["pre"].items():
        a = ls[k].act; x = np.concatenate([v.reshape(v.shape[0], -1) for v in pres])      # (T * B, units), time-major as the mask
        if keep is not None:
            x = x[keep]
        for kink in KINKS.get(a, ()):
            margin = min(margin, float(np.abs(x - kink).min()))
        if a in PIECES:
            cuts = (-np.inf,) + PIECES[a] + (np.inf,)
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                occ = min(occ, float(((x > lo) & (x < hi)).mean()))
    return margin, occ, probe["sigma"]


def case_rules(c, seed=None, steps=STEPS):
    """the worst (margin, occupancy, sigma_min, argmax gap) along the fp64 trajectory of the case's steps"""
    D = data(c, seed); out = [np.inf, 1.0, np.inf, np.inf]
    for k, p, batch, o in trajectory(c, D, steps):
        m, occ, sg = rules(D.net, p, batch[0], masks_of(D.net, k, c.B, c.T), batch[5] if c.T else None)
        qsel = o["q_on_sp"] if c.dq else o["q_tg_sp"]
        out = [min(out[0], m), min(out[1], occ), min(out[2], sg), min(out[3], LR._gap(np.concatenate(qsel) if c.T else qsel))]
    return tuple(out)


def rules_ok(c, seed=None, k=2.0):
    m, occ, sg, gap = case_rules(c, seed)
    return m > k * RELU_MARGIN and occ >= OCCUPANCY and sg >= k * LR.SIGMA_MIN and gap > k * GAP


find_seed = lambda c, cap=200: S.find_seed(c, rules_ok, cap)


TELL = 100.0      # a wrong engine must move some compared quantity by this many of its tolerances


def tell_distance(c, wrong, seed=None):
    """what the wrong engine is off by on the case's first step, in tolerances: the largest over the compared quantities"""
    D = data(c, seed)
    for k, p, batch, o in trajectory(c, D, 1, leg="numpy"):
        return max(distance(step(c, D, p, batch, k, leg=wrong), o).values())
