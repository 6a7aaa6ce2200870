"""
Host-side description of solver.qnetwork: the Flux vocabulary the reference's users write
(README.md:26-46: Chain(Dense(2,32), Dense(32,n))) mirrored as plain Python descriptors, plus
create_dueling_network (src/dueling.jl:36-58).  No arithmetic happens here: descriptors are lowered to
dqn_layer_desc records and handed to the HIP engine.
"""
from __future__ import annotations

import operator

import numpy as np

from . import _abi

identity, relu, tanh, sigmoid = _abi.ACT_IDENTITY, _abi.ACT_RELU, _abi.ACT_TANH, _abi.ACT_SIGMOID
# NNlib's default parameters only: leakyrelu(x) = leakyrelu(x, 0.01), elu(x) = elu(x, 1) (include/dqn_mi355x.h has the table of all eleven)
leakyrelu, elu, selu, softplus, softsign, relu6, hardtanh = (_abi.ACT_LEAKYRELU, _abi.ACT_ELU, _abi.ACT_SELU, _abi.ACT_SOFTPLUS, _abi.ACT_SOFTSIGN, _abi.ACT_RELU6,
                                                             _abi.ACT_HARDTANH)
ACT_NAMES = ("identity", "relu", "tanh", "sigmoid", "leakyrelu", "elu", "selu", "softplus", "softsign", "relu6", "hardtanh")      # index = DQN_ACT_* code


class _UnsupportedActivation:
    """a name Flux users write that the engine cannot run: a sentinel `lower` refuses with the reason"""

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return self.name


# not monotone: the derivative is no function of the output y, and the engine keeps only y (every backward epilogue differentiates from it)
# ... as the fused activation of a Dense / Conv / LayerNorm / GroupNorm, that is.  A standalone Activation(σ) layer reads the stored output of the layer in front, so x is there:
# the four are its codes 11..14 (LAYER_ACT_NAMES), taken by their .name
gelu, swish, mish, hardswish = (_UnsupportedActivation(n) for n in ("gelu", "swish", "mish", "hardswish"))
LAYER_ACT_NAMES = ACT_NAMES + ("gelu", "swish", "mish", "hardswish")      # index = the DQN_ACT_* code on an Activation layer (kind 14), the only kind that takes 11..14


def _act_code(l):
    """the DQN_ACT_* code of a layer's activation, or the DeepQLearningError that names what is supported"""
    a = l.act
    supported = " / ".join(ACT_NAMES)
    if isinstance(a, _UnsupportedActivation):
        raise _abi.DQNError(f"DeepQLearningError: unsupported activation {a.name} on {l!r}: {a.name} is not monotone, so its derivative needs the pre-activation, and the "
                            f"MI355X engine keeps only each layer's output y and differentiates from it (supported: {supported})")
    if isinstance(a, (int, np.integer)) and not isinstance(a, bool) and 0 <= int(a) < len(ACT_NAMES):
        return int(a)
    raise _abi.DQNError(f"DeepQLearningError: unsupported activation {a!r} on {l!r} (supported: {supported}, with NNlib's default parameters only)")


class flattenbatch:  # src/helpers.jl:6-8 -- a no-op marker: the engine flattens between Conv and Dense
    kind = "flatten"


class Dense:
    """Flux Dense(in, out, act)."""
    kind = "dense"

    def __init__(self, n_in, n_out, act=identity):
        self.n_in, self.n_out, self.act = int(n_in), int(n_out), act

    def __repr__(self):
        return f"Dense({self.n_in}, {self.n_out}, act={self.act})"

    def shapes(self):  # host array shapes in Julia memory order: weight (out,in) == C (in,out); bias (out,)
        return [(self.n_in, self.n_out), (self.n_out,)]

    def fans(self):
        return self.n_in, self.n_out


class SamePad:
    """Flux SamePad(): output size = input size ÷ stride.  For an odd kernel that is the symmetric pad (k - 1) ÷ 2 per axis; for an even kernel Flux pads one more element
    on the high side than on the low side, an asymmetric pad the engine does not run."""

    def __repr__(self):
        return "SamePad()"


def _pair(v, name, what):
    """an int or a 2-tuple in this mirror's (H, W) order -> (h, w)"""
    if np.isscalar(v):
        return int(v), int(v)
    t = tuple(int(x) for x in v)
    if len(t) != 2:
        raise _abi.DQNError(f"DeepQLearningError: {name}: {what} must be an int or a pair")
    return t


def _resolve_pad(pad, kh, kw, dh=1, dw=1):
    """Flux's pad argument -> symmetric (ph, pw): an int, a 2-tuple (per axis), a 4-tuple (lo, hi per axis: W axis first, as Flux stores it) or SamePad().  With a dilation
    the kernel's extent per axis is (k - 1) * d + 1: SamePad() resolves to (k - 1) * d / 2, and the pad may reach the extent minus one."""
    dil = "" if dh == dw == 1 else f", dilation=({dh}, {dw})"
    name = f"Conv(({kh}, {kw}), ...; pad={pad!r}{dil})"
    eh, ew = (kh - 1) * dh, (kw - 1) * dw      # the (dilated) extent minus one
    if isinstance(pad, SamePad) or pad is SamePad:
        if eh % 2 or ew % 2:
            raise _abi.DQNError(f"DeepQLearningError: {name}: SamePad() on an even kernel is an asymmetric pad (lo != hi); the MI355X engine supports symmetric zero padding only")
        return eh // 2, ew // 2
    if np.isscalar(pad):
        ph = pw = int(pad)
    else:
        t = tuple(int(v) for v in pad)
        if len(t) == 2:
            ph, pw = t
        elif len(t) == 4:      # Flux: (w_lo, w_hi, h_lo, h_hi) -- the first pair belongs to the W axis, as stride[1] does
            if t[0] != t[1] or t[2] != t[3]:
                raise _abi.DQNError(f"DeepQLearningError: {name}: asymmetric pad (lo != hi on an axis); the MI355X engine supports symmetric zero padding only")
            pw, ph = t[0], t[2]
        else:
            raise _abi.DQNError(f"DeepQLearningError: {name}: pad must be an int, a 2-tuple, a symmetric 4-tuple or SamePad()")
    if ph < 0 or pw < 0:
        raise _abi.DQNError(f"DeepQLearningError: {name}: pad ({ph}, {pw}) must not be negative")
    if ph > eh or pw > ew:
        raise _abi.DQNError(f"DeepQLearningError: {name}: pad ({ph}, {pw}) is larger than " + ("kernel - 1" if dh == dw == 1 else "the dilated kernel extent - 1") + f" = ({eh}, {ew})")
    return ph, pw


class Conv:
    """Flux Conv((kh,kw), cin=>cout, act; stride, pad, dilation, groups) -- true convolution; pad = symmetric zero padding per axis (an int, (ph, pw), a symmetric Flux 4-tuple
    or SamePad()), 0 <= pad <= (kernel - 1) * dilation.  Output map (H + 2 ph - (kh - 1) dh - 1) ÷ sh + 1 by (W + 2 pw - (kw - 1) dw - 1) ÷ sw + 1.  dilation: an int or
    (dh, dw) in this mirror's (H, W) order (Flux writes (W, H), as for stride).  groups = g divides cin and cout: output channels [j cout/g, (j+1) cout/g) read input channels
    [j cin/g, (j+1) cin/g); the weight is (kw, kh, cin ÷ g, cout) and the glorot fans are nfan of that size.  dilation = 1 and groups = 1 is the Conv it always was (layer
    kind 1); anything else is layer kind 15 (csrc/conv_own.hip): base chain only, not inside a SkipConnection."""
    kind = "conv"

    def __init__(self, k, cin, cout, act=identity, stride=1, pad=0, dilation=1, groups=1):
        self.kh, self.kw = (k, k) if np.isscalar(k) else (int(k[0]), int(k[1]))
        self.sh, self.sw = (stride, stride) if np.isscalar(stride) else (int(stride[0]), int(stride[1]))
        self.cin, self.cout, self.act = int(cin), int(cout), act
        name = f"{type(self).__name__}(({self.kh}, {self.kw}), {self.cin} => {self.cout}; dilation={dilation!r}, groups={groups!r})"
        self.dh, self.dw = _pair(dilation, name, "dilation")
        self.groups = int(groups)
        if self.dh < 1 or self.dw < 1:
            raise _abi.DQNError(f"DeepQLearningError: {name}: dilation must be at least 1 per axis")
        if self.dh > 255 or self.dw > 255 or self.groups > 32767:
            raise _abi.DQNError(f"DeepQLearningError: {name}: the MI355X engine takes dilation <= 255 and groups <= 32767")
        if self.groups < 1 or self.cin % self.groups or self.cout % self.groups:
            raise _abi.DQNError(f"DeepQLearningError: {name}: groups must be >= 1 and divide cin = {self.cin} and cout = {self.cout}")
        self.ph, self.pw = _resolve_pad(pad, self.kh, self.kw, self.dh, self.dw)

    @property
    def general(self):
        """dilation != 1 or groups != 1: the layer lowers to kind 15 (LAYER_CONV_DG)"""
        return (self.dh, self.dw, self.groups) != (1, 1, 1)

    def __repr__(self):
        dg = f", dilation=({self.dh}, {self.dw}), groups={self.groups}" if self.general else ""
        return f"Conv(({self.kh}, {self.kw}), {self.cin} => {self.cout}, act={self.act}, stride=({self.sh}, {self.sw}), pad=({self.ph}, {self.pw}){dg})"

    def shapes(self):  # weight (kw,kh,cin÷g,cout) == C (cout,cin÷g,kh,kw)
        return [(self.cout, self.cin // self.groups, self.kh, self.kw), (self.cout,)]

    def fans(self):    # Flux nfan(kw, kh, cin ÷ g, cout)
        return self.kh * self.kw * (self.cin // self.groups), self.kh * self.kw * self.cout


class DepthwiseConv(Conv):
    """Flux DepthwiseConv((kh,kw), cin=>cout, act; stride, pad, dilation) = Conv(...; groups = cin), cout a multiple of cin"""

    def __init__(self, k, cin, cout, act=identity, stride=1, pad=0, dilation=1):
        if int(cin) < 1 or int(cout) % int(cin):
            raise _abi.DQNError(f"DeepQLearningError: DepthwiseConv({k!r}, {cin} => {cout}): groups = cin must divide cout (cout is a multiple of cin)")
        super().__init__(k, cin, cout, act, stride, pad, dilation, groups=int(cin))


class _Pool:
    """Flux MaxPool / MeanPool((kh, kw); pad = 0, stride = (kh, kw)): per channel on a (C, H, W) map, output (C, (H-kh)÷sh+1, (W-kw)÷sw+1); trailing rows / columns that
    no window covers are dropped.  No parameters, no activation."""

    def __init__(self, k, stride=None, pad=0):
        self.kh, self.kw = (int(k), int(k)) if np.isscalar(k) else (int(k[0]), int(k[1]))
        stride = (self.kh, self.kw) if stride is None else stride      # Flux: stride defaults to the window
        self.sh, self.sw = (int(stride), int(stride)) if np.isscalar(stride) else (int(stride[0]), int(stride[1]))
        if np.any(np.asarray(pad) != 0):
            raise _abi.DQNError(f"DeepQLearningError: the MI355X engine supports {type(self).__name__} with pad=0 only (got pad={pad!r})")
        self.act = identity

    def shapes(self):   # Flux.params holds nothing for a pool layer
        return []

    def __repr__(self):
        return f"{type(self).__name__}(({self.kh}, {self.kw}), stride=({self.sh}, {self.sw}))"


class MaxPool(_Pool):
    kind = "maxpool"


class MeanPool(_Pool):
    kind = "meanpool"


class _AdaptivePool:
    """Flux 0.14 AdaptiveMaxPool / AdaptiveMeanPool(out) over NNlib (recalled, not executed here): per channel on a (C, H, W) map, output (C, oh, ow) with 1 <= out <= in per
    axis.  Flux's rule per axis: stride = in ÷ out, k = in - (out - 1) * stride, pad = 0, then maxpool / meanpool with that geometry -- NOT torch's adaptive windows (5 -> 3:
    Flux takes [0..2] [1..3] [2..4], torch [0,2) [1,4) [3,5)).  The map size is the engine's to know: it resolves the window (build_layers).  `out` is an integer or (oh, ow)
    in this mirror's (H, W) order; Flux writes (ow, oh).  No parameters, no activation.  Placement is a pool's."""

    def __init__(self, out):
        if np.isscalar(out):
            self.oh = self.ow = int(out)
        else:
            t = tuple(int(v) for v in out)
            if len(t) != 2:
                raise _abi.DQNError(f"DeepQLearningError: {type(self).__name__}({out!r}): the output size must be an integer or a pair (oh, ow)")
            self.oh, self.ow = t
        if self.oh < 1 or self.ow < 1:
            raise _abi.DQNError(f"DeepQLearningError: {type(self).__name__}(({self.oh}, {self.ow})): the output size must be at least (1, 1)")
        self.act = identity

    def shapes(self):   # Flux.params holds nothing for a pool layer
        return []

    def __repr__(self):
        return f"{type(self).__name__}(({self.ow}, {self.oh}))"      # Flux's order: (W, H)


class AdaptiveMaxPool(_AdaptivePool):
    kind = "adaptivemaxpool"


class AdaptiveMeanPool(_AdaptivePool):
    kind = "adaptivemeanpool"


class GlobalMaxPool(_AdaptivePool):
    """Flux 0.14 GlobalMaxPool(): maxpool with window = the whole (h, w) map, output (1, 1, c, batch) -- AdaptiveMaxPool((1, 1)) exactly, and lowered as it"""
    kind = "adaptivemaxpool"

    def __init__(self):
        super().__init__(1)

    def __repr__(self):
        return "GlobalMaxPool()"


class GlobalMeanPool(_AdaptivePool):
    """Flux 0.14 GlobalMeanPool(): meanpool with window = the whole (h, w) map, output (1, 1, c, batch) -- AdaptiveMeanPool((1, 1)) exactly, and lowered as it"""
    kind = "adaptivemeanpool"

    def __init__(self):
        super().__init__(1)

    def __repr__(self):
        return "GlobalMeanPool()"


POOL_KINDS = ("maxpool", "meanpool", "adaptivemaxpool", "adaptivemeanpool")      # parameter-free layers on a (c, h, w) map whose output is a map


class LayerNorm:
    """Flux 0.14 LayerNorm(n, λ = identity; affine = true, eps = 1f-5) on a feature vector of length n, per batch column (Flux's `normalise`; recalled, not executed here):
    μ = mean(x), σ = sqrt(mean((x - μ)²)) (uncorrected), y = λ.(scale .* (x - μ) / (σ + eps) .+ bias) -- eps is added to σ OUTSIDE the root, which is not torch's
    sqrt(var + eps).  Flux.params: diag.scale (n, ones), diag.bias (n, zeros).  Directly behind a Dense or recurrent layer (or the Dropout that follows one), base chain only."""
    kind = "layernorm"

    def __init__(self, n, act=identity, eps=1e-5, affine=True):
        if isinstance(n, (tuple, list)):
            raise _abi.DQNError(f"DeepQLearningError: LayerNorm(size={tuple(n)!r}): a tuple size (normalisation over several dimensions) is not supported; the MI355X engine "
                                "normalises a feature vector, LayerNorm(n) with an integer n")
        if not affine:
            raise _abi.DQNError(f"DeepQLearningError: LayerNorm({n}; affine=false) is not supported; the MI355X engine runs the layer with its scale and bias (affine=true)")
        self.n, self.act, self.eps = int(n), act, float(eps)
        if self.n < 2:
            raise _abi.DQNError(f"DeepQLearningError: LayerNorm({self.n}): n must be >= 2 (over one feature σ is identically 0 and the gradient is NaN)")
        with np.errstate(over="ignore"):
            e32 = np.float32(self.eps)
        if not (np.isfinite(e32) and e32 > 0):
            raise _abi.DQNError(f"DeepQLearningError: LayerNorm({self.n}; eps={eps!r}): eps must be finite and > 0 in Float32")
        self.n_in = self.n_out = self.n      # what a following Dense / the dueling split reads

    def __repr__(self):
        return f"LayerNorm({self.n}, act={self.act}, eps={self.eps!r})"

    def shapes(self):   # Flux.params order: diag.scale, diag.bias
        return [(self.n,), (self.n,)]


class GroupNorm:
    """Flux 0.14 GroupNorm(chs, G, λ = identity; affine = true, track_stats = false, eps = 1f-5) on a (w, h, chs, batch) map (Flux's `_norm_layer_forward`; recalled, not
    executed here): the channels form G contiguous groups of chs / G; per sample and group μ = mean(x), σ² = mean((x - μ)²) (uncorrected),
    y = λ.(γ_ch .* (x - μ) / sqrt(σ² + eps) .+ β_ch) -- eps INSIDE the root (torch's law, not LayerNorm's σ + eps).  Flux.params: β (chs, zeros), THEN γ (chs, ones).
    Directly behind a Conv, a MaxPool / MeanPool, a convolutional SkipConnection or another GroupNorm; base chain only, never the first or the output layer."""
    kind = "groupnorm"

    def __init__(self, chs, G, act=identity, eps=1e-5, affine=True, track_stats=False):
        if not affine:
            raise _abi.DQNError(f"DeepQLearningError: GroupNorm({chs}, {G}; affine=false) is not supported; the MI355X engine runs the layer with its γ and β (affine=true)")
        if track_stats:
            raise _abi.DQNError(f"DeepQLearningError: GroupNorm({chs}, {G}; track_stats=true) is not supported; the MI355X engine keeps no running statistics "
                                "(every pass normalises with the statistics of its own input: track_stats=false, Flux 0.14's default)")
        self.chs, self.G, self.act, self.eps = int(chs), int(G), act, float(eps)
        if self.G < 1 or self.chs < 1 or self.chs % self.G:
            raise _abi.DQNError(f"DeepQLearningError: GroupNorm({self.chs}, {self.G}): the number of groups G must be >= 1 and divide the channel count")
        with np.errstate(over="ignore"):
            e32 = np.float32(self.eps)
        if not (np.isfinite(e32) and e32 > 0):
            raise _abi.DQNError(f"DeepQLearningError: GroupNorm({self.chs}, {self.G}; eps={eps!r}): eps must be finite and > 0 in Float32")

    def __repr__(self):
        return f"GroupNorm({self.chs}, {self.G}, act={self.act}, eps={self.eps!r})"

    def shapes(self):   # Flux.params order: β, γ
        return [(self.chs,), (self.chs,)]


class BatchNorm:
    """Flux BatchNorm: named so that the refusal can name it; the MI355X engine does not run it."""
    kind = "batchnorm"

    def __init__(self, *args, **kwargs):
        raise _abi.DQNError("DeepQLearningError: BatchNorm is not supported: it keeps running statistics, so the online pass on s, the pass on s', the target pass and the acting "
                            "pass would compute different functions; of Flux's normalisation layers the MI355X engine runs LayerNorm(n) and GroupNorm(chs, G) (GroupNorm(chs, 1) "
                            "normalises the whole map)")


class InstanceNorm:
    """Flux InstanceNorm: named so that the refusal can name it; the MI355X engine does not run it."""
    kind = "instancenorm"

    def __init__(self, *args, **kwargs):
        raise _abi.DQNError("DeepQLearningError: InstanceNorm is not supported: its default is affine = false (no γ, β), which the MI355X engine does not run; "
                            "GroupNorm(chs, chs) is instance normalisation with a per-channel affine")


class Dropout:
    """Flux 0.14 Dropout(p; dims = :) on a feature vector, per batch column, in Flux's automatic mode (recalled, not executed here): active only under Flux.gradient --
    in the train step's online forward on s, y = keep ? x * Float32(1 / (1 - p)) : 0 -- and the identity in every other pass (online on s', target, acting, evaluation,
    after restore_best_model).  The mask is the engine's own counter-based law, not Julia's RNG.  No parameters: Flux.params skips the layer.
    Directly behind a Dense, recurrent or LayerNorm layer, base chain only, never the first or the output layer."""
    kind = "dropout"

    def __init__(self, p, dims=None):
        if dims is not None and dims != ":":
            raise _abi.DQNError(f"DeepQLearningError: Dropout({p!r}; dims={dims!r}) is not supported; the MI355X engine drops single elements (dims = :)")
        self.p, self.act = float(p), identity
        if not (np.isfinite(self.p) and 0.0 <= self.p < 1.0):
            raise _abi.DQNError(f"DeepQLearningError: Dropout({p!r}): p must be finite with 0 <= p < 1" + (" (p = 1 drops every feature: Q would be constant)" if self.p == 1.0 else ""))

    def __repr__(self):
        return f"Dropout({self.p!r})"

    def shapes(self):   # Flux.params holds nothing for a Dropout layer
        return []


class Activation:
    """A standalone activation layer: Julia's Base.Broadcast.BroadcastFunction(σ) in a Chain (BroadcastFunction(σ)(x) == σ.(x); recalled, not executed here).  y = σ.(x) on
    whatever the layer in front yields -- a feature vector or a (c, h, w) map, kept.  σ is any of the eleven codes or of nn.gelu / nn.swish / nn.mish / nn.hardswish (NNlib's
    tanh-form gelu).  No parameters: Flux.params skips the layer.  Base chain only, never the first or the output layer (the last base layer of a dueling network is fine), not
    inside a SkipConnection; a LayerNorm or Dropout may not directly follow it.  What it is for: the post-add relu of a ResNet-v1 block, and the four activations a fused layer
    cannot run (DESIGN.md section 4 "Activation layers")."""
    kind = "activation"

    def __init__(self, sigma):
        if isinstance(sigma, _UnsupportedActivation) and sigma.name in LAYER_ACT_NAMES:
            self.code = LAYER_ACT_NAMES.index(sigma.name)
        elif isinstance(sigma, (int, np.integer)) and not isinstance(sigma, bool) and 0 <= int(sigma) < len(LAYER_ACT_NAMES):
            self.code = int(sigma)
        else:
            raise _abi.DQNError(f"DeepQLearningError: unsupported activation {sigma!r} on Activation (supported: {' / '.join(LAYER_ACT_NAMES)}, with NNlib's default parameters only; "
                                "a closure cannot be inspected)")
        self.act = identity      # the layer has no fused activation: σ is the layer (lowered into dqn_layer_desc.act from .code)

    def __repr__(self):
        return f"Activation({LAYER_ACT_NAMES[self.code]})"

    def shapes(self):   # Flux.params holds nothing for the layer
        return []


class LSTM:
    """Flux LSTM(in, out) = Recur(LSTMCell): params Wi (4out,in), Wh (4out,out), b (4out, forget gate bias 1), state0 (h0, c0)."""
    kind = "lstm"

    def __init__(self, n_in, n_out):
        self.n_in, self.n_out, self.act = int(n_in), int(n_out), identity

    def shapes(self):   # Julia memory order: Wi (4out,in) == C (in,4out), Wh (4out,out) == C (out,4out), b, h0, c0
        h = self.n_out
        return [(self.n_in, 4 * h), (h, 4 * h), (4 * h,), (h,), (h,)]


class GRU:
    """Flux GRU(in, out) = Recur(GRUCell), gates r, z, n: params Wi (3out,in), Wh (3out,out), b (3out, zero), state0 h0 (out,1, zero)."""
    kind = "gru"

    def __init__(self, n_in, n_out):
        self.n_in, self.n_out, self.act = int(n_in), int(n_out), identity

    def shapes(self):   # Julia memory order: Wi (3out,in) == C (in,3out), Wh (3out,out) == C (out,3out), b, h0
        h = self.n_out
        return [(self.n_in, 3 * h), (h, 3 * h), (3 * h,), (h,)]

    def fans(self):     # glorot fans of Wi and Wh
        h = self.n_out
        return [(self.n_in, 3 * h), (h, 3 * h)]


class RNN:
    """Flux RNN(in, out, σ = tanh) = Recur(RNNCell): h' = σ.(Wi*x .+ Wh*h .+ b); params Wi (out,in), Wh (out,out), b (out, zero), state0 h0 (out,1, zero)."""
    kind = "rnn"

    def __init__(self, n_in, n_out, act=tanh):
        self.n_in, self.n_out, self.act = int(n_in), int(n_out), act     # act: the CELL's σ (lowered into dqn_layer_desc.act)

    def shapes(self):   # Julia memory order: Wi (out,in) == C (in,out), Wh (out,out) == C (out,out), b, h0
        h = self.n_out
        return [(self.n_in, h), (h, h), (h,), (h,)]

    def fans(self):     # glorot fans of Wi and Wh
        h = self.n_out
        return [(self.n_in, h), (h, h)]


class Chain:
    def __init__(self, *layers):
        self.layers = [l for l in layers if getattr(l, "kind", None) != "flatten" and l is not flattenbatch]

    def __iter__(self):
        return iter(self.layers)

    def __len__(self):
        return len(self.layers)


class SkipConnection:
    """Flux 0.14 SkipConnection(layers, +) on a feature vector (recalled, not executed here): y = layers(x) .+ x.  No parameters and no activation of its own: Flux.params
    yields the inner layers' parameters in order.  `layers` is a Chain (or one layer) of Dense, LayerNorm and Dropout layers that maps n -> n; the connection is `+` only
    ("+" or operator.add).  The block stands in the base chain behind a Dense, recurrent, LayerNorm or Dropout layer or another block: never first, never behind a
    Conv / pool, never the output layer (DESIGN.md section 4 "Skip connections").  create_dueling_network treats it as a non-Dense layer.

    On a (c, h, w) map -- behind a Conv, a MaxPool / MeanPool or another such block -- `layers` is a Chain (or one layer) of Conv layers with pad != 0 that maps
    (c, h, w) -> (c, h, w): the residual convolutional block x + Conv(Conv(x)) (DESIGN.md section 4 "Convolutional skip blocks")."""
    kind = "skip"

    def __init__(self, layers, connection):
        if not (connection == "+" or connection is operator.add):
            name = connection if isinstance(connection, str) else getattr(connection, "__name__", None) or repr(connection)
            raise _abi.DQNError(f"DeepQLearningError: SkipConnection(layers, {name}) is not supported; the MI355X engine runs SkipConnection with the connection + only "
                                "(vcat, *, closures and Parallel are not supported)")
        self.layers = layers if isinstance(layers, Chain) else Chain(layers)
        self.connection, self.act = "+", identity
        if len(self.layers) < 1:
            raise _abi.DQNError("DeepQLearningError: SkipConnection(Chain(), +) holds no layer; the MI355X engine needs at least one inner layer")

    def __repr__(self):
        return f"SkipConnection(Chain({', '.join(repr(l) for l in self.layers)}), +)"

    def shapes(self):   # Flux.params holds nothing for the block itself: the inner layers' arrays come from all_layers
        return []


class Parallel:
    """Flux Parallel(connection, layers...): named so that the refusal can name it; the MI355X engine does not run it."""
    kind = "parallel"

    def __init__(self, connection, *layers):
        self.connection, self.layers = connection, layers

    def __repr__(self):
        return "Parallel(...)"


class DuelingNetwork:
    """src/dueling.jl:1-6: base, val, adv chains; Flux.params order = base, val, adv."""

    def __init__(self, base, val, adv):
        self.base, self.val, self.adv = base, val, adv


def create_dueling_network(m: Chain) -> DuelingNetwork:
    """src/dueling.jl:36-58: split the trailing run of Dense layers into value / advantage streams; the value stream
    gets a fresh Dense(in_of_last, 1).  Throws the reference's error string if there is no trailing Dense."""
    layers = m.layers
    n = len(layers)
    duel_layer = -1
    for i in range(1, n + 1):
        if getattr(layers[n - i], "kind", None) != "dense":
            duel_layer = n - i + 1
            break
        elif i == n:
            duel_layer = 0
    if duel_layer == -1:
        raise _abi.DQNError("DeepQLearningError: the qnetwork provided is incompatible with dueling")
    trailing = layers[duel_layer:]
    if not trailing:      # the chain does not end in a Dense layer: nothing to split into value / advantage streams
        raise _abi.DQNError("DeepQLearningError: the qnetwork provided is incompatible with dueling")
    last = trailing[-1]
    val = Chain(*[Dense(l.n_in, l.n_out, l.act) for l in trailing[:-1]], Dense(last.n_in, 1))
    adv = Chain(*[Dense(l.n_in, l.n_out, l.act) for l in trailing])
    return DuelingNetwork(Chain(*layers[:duel_layer]), val, adv)


def lower(net):
    """Chain | DuelingNetwork -> (list[LayerDesc], dueling flag)."""
    out = []
    chan = [0]      # channels of the map the next layer reads (0 in front of the first Conv: the engine takes the observation's)
    map_join = [False]      # the last block lowered was a convolutional one: what follows it stands on a map
    top = None if isinstance(net, DuelingNetwork) else net      # the chain whose last layer is the network's output layer (a dueling base chain's is not)

    def add_skip(blk, stream, first, prev_kind, is_last, front=None):
        # SkipConnection(Chain(inner...), +): the inner layers' descriptors, then ONE join descriptor (kind SKIPADD, cin = m the number of inner layers, n_in = n_out = 0: the
        # engine fills in the feature count).  The placement rules are stated here by name; the engine's build_layers holds them again for C callers
        if stream != _abi.STREAM_BASE:
            raise _abi.DQNError(f"DeepQLearningError: {blk!r} is supported in the base chain only (not in a value / advantage stream)")
        if first:
            raise _abi.DQNError(f"DeepQLearningError: {blk!r} cannot be the first layer: a skip block's input is never the observation (it must follow a Dense, recurrent, LayerNorm or Dropout layer or another skip block)")
        if any(getattr(l, "kind", None) == "activation" for l in blk.layers):
            raise _abi.DQNError(f"DeepQLearningError: an Activation layer inside a SkipConnection is not supported (a standalone activation stands in the base chain, in front of or behind the block; inside, use the fused activation of Dense / Conv): {blk!r}")
        if any(getattr(l, "kind", None) == "groupnorm" for l in blk.layers):
            raise _abi.DQNError(f"DeepQLearningError: a GroupNorm layer inside a SkipConnection is not supported (GroupNorm stands in the base chain, in front of or behind the block): {blk!r}")
        if any(getattr(l, "kind", None) == "conv" and l.general for l in blk.layers):
            raise _abi.DQNError(f"DeepQLearningError: a Conv with dilation != 1 or groups != 1 (DepthwiseConv included) inside a SkipConnection is not supported (dilated and grouped residual blocks are not supported; the layer stands in the base chain, in front of or behind the block): {blk!r}")
        on_map = prev_kind in ("conv", "groupnorm") + POOL_KINDS or (prev_kind == "skip" and map_join[0])
        if on_map and not first and all(getattr(l, "kind", None) in ("conv",) + POOL_KINDS for l in blk.layers):
            return add_skip_map(blk, stream, is_last)
        if on_map:
            raise _abi.DQNError(f"DeepQLearningError: {blk!r} cannot follow a Conv / MaxPool / MeanPool layer: a skip block stands on a feature vector (convolutional residual blocks are not supported)")
        if is_last:
            raise _abi.DQNError(f"DeepQLearningError: {blk!r} cannot be the network's output layer")
        n_first = n_last = None
        for l in blk.layers:
            k = getattr(l, "kind", None)
            if k == "skip":
                raise _abi.DQNError(f"DeepQLearningError: a SkipConnection inside a SkipConnection is not supported (nested skip blocks): {blk!r}")
            if k in ("lstm", "gru", "rnn"):
                raise _abi.DQNError(f"DeepQLearningError: a recurrent layer inside a SkipConnection is not supported (its inner layers are Dense, LayerNorm and Dropout layers only): {blk!r}")
            if k in ("conv",) + POOL_KINDS:
                raise _abi.DQNError(f"DeepQLearningError: a Conv / MaxPool / MeanPool layer inside a SkipConnection is not supported (its inner layers are Dense, LayerNorm and Dropout layers only; convolutional residual blocks are not supported): {blk!r}")
            if k not in ("dense", "layernorm", "dropout"):
                raise _abi.DQNError(f"DeepQLearningError: unsupported layer {l!r} inside a SkipConnection (Dense / LayerNorm / Dropout only)")
            if k != "dropout":
                n_first = l.n_in if n_first is None else n_first
                n_last = l.n_out
        if n_first is not None and n_first != n_last:
            raise _abi.DQNError(f"DeepQLearningError: {blk!r} maps {n_first} features to {n_last}; SkipConnection(layers, +) needs layers: n -> n")
        inner0 = blk.layers.layers[0]      # the block's first inner layer reads the layer in front of the block: the rule of add() below holds across the block's edge (the engine refuses it by index)
        if getattr(front, "kind", None) == "activation" and inner0.kind in ("layernorm", "dropout"):
            raise _abi.DQNError(f"DeepQLearningError: {inner0!r} cannot directly follow {front!r}: a {type(inner0).__name__} directly behind a standalone Activation layer is not supported, "
                                "as the first inner layer of a SkipConnection neither (it must directly follow a Dense, recurrent" + (" or LayerNorm" if inner0.kind == "dropout" else "") + " layer)")
        if inner0.kind in ("layernorm", "dropout") and getattr(front, "kind", None) == inner0.kind:
            raise _abi.DQNError(f"DeepQLearningError: {inner0!r} cannot directly follow {front!r}: two {type(inner0).__name__} layers in a row are not supported, "
                                "as the first inner layer of a SkipConnection neither (it must directly follow a Dense, recurrent" + (" or LayerNorm" if inner0.kind == "dropout" else "") + " layer)")
        add(blk.layers, stream)
        d = _abi.LayerDesc()
        d.kind, d.act, d.stream, d.cin = _abi.LAYER_SKIPADD, _abi.ACT_IDENTITY, stream, len(blk.layers)
        out.append(d)
        map_join[0] = False

    def add_skip_map(blk, stream, is_last):
        # the block stands on a (c, h, w) map and holds Conv / pool layers only: the convolutional block, kind SKIPADD_MAP -- the same descriptor shape.  Its inner layers are
        # Convs with pad != 0 and keep the channel count; that they keep (h, w) is the engine's check (it knows the map)
        if is_last:
            raise _abi.DQNError(f"DeepQLearningError: {blk!r} cannot be the network's output layer")
        for l in blk.layers:
            if l.kind in POOL_KINDS:
                raise _abi.DQNError(f"DeepQLearningError: a MaxPool / MeanPool layer inside a convolutional SkipConnection is not supported (its inner layers are Conv layers with pad != 0 only): {blk!r}")
            if l.ph == 0 and l.pw == 0:
                raise _abi.DQNError(f"DeepQLearningError: a Conv with pad 0 inside a convolutional SkipConnection is not supported (its inner layers are Conv layers with pad != 0 only; 1x1 and unpadded inner convolutions are not supported): {blk!r}")
        cin, cout = blk.layers.layers[0].cin, blk.layers.layers[-1].cout
        if cin != cout:
            raise _abi.DQNError(f"DeepQLearningError: {blk!r} maps {cin} channels to {cout}; SkipConnection(layers, +) needs layers: (c, h, w) -> (c, h, w)")
        add(blk.layers, stream)
        d = _abi.LayerDesc()
        d.kind, d.act, d.stream, d.cin = _abi.LAYER_SKIPADD_MAP, _abi.ACT_IDENTITY, stream, len(blk.layers)
        out.append(d)
        map_join[0] = True

    def shape_kind(layers, i):
        # the kind of the layer whose output shape layer i reads: the layer in front, looking through Activation layers (they keep the shape AND the kind of shape)
        j = i - 1
        while j >= 0 and getattr(layers[j], "kind", None) == "activation":
            j -= 1
        return getattr(layers[j], "kind", None) if j >= 0 else None

    NEVER_FIRST = {"activation": "its input is the stored output of the layer in front (an activation on the observation is not supported)",
                   "groupnorm": "normalising the observation is not supported (it must follow a Conv, MaxPool / MeanPool or GroupNorm layer or a convolutional SkipConnection)"}

    def placed(l, stream, is_last):
        # the placement of an own-level kind, by name: never the first layer (the kinds of NEVER_FIRST), base chain only, never the output layer (every kind but a Conv)
        if l.kind in NEVER_FIRST and not out:
            raise _abi.DQNError(f"DeepQLearningError: {l!r} cannot be the first layer: {NEVER_FIRST[l.kind]}")
        if stream != _abi.STREAM_BASE:
            raise _abi.DQNError(f"DeepQLearningError: {l!r} is supported in the base chain only (not in a value / advantage stream)")
        if is_last and l.kind != "conv":
            raise _abi.DQNError(f"DeepQLearningError: {l!r} cannot be the network's output layer")

    def add(chain, stream):
        layers = list(chain)
        for i, l in enumerate(layers):
            d = _abi.LayerDesc()
            is_last = i + 1 == len(layers) and chain is top
            if getattr(l, "kind", None) == "parallel":
                raise _abi.DQNError("DeepQLearningError: Parallel is not supported; of Flux's branching layers the MI355X engine runs SkipConnection(layers, +) only")
            if getattr(l, "kind", None) == "skip":
                add_skip(l, stream, not out, shape_kind(layers, i), is_last, layers[i - 1] if i > 0 else None)
                continue
            if getattr(l, "kind", None) == "activation":      # act = σ (0..14); n_in == n_out == 0: the engine fills in the incoming feature count and keeps the incoming shape
                placed(l, stream, is_last)
                d.kind, d.act, d.stream = _abi.LAYER_ACTIVATION, l.code, stream
                out.append(d)
                continue
            if callable(l) and getattr(l, "kind", None) is None and not isinstance(l, type):
                raise _abi.DQNError(f"DeepQLearningError: unsupported layer {l!r}: a closure cannot be inspected; write a standalone activation as Activation(relu) "
                                    "(Julia: Base.BroadcastFunction(relu)), not as x -> relu.(x)")
            if getattr(l, "kind", None) not in ("dense", "dropout", "lstm", "gru", "rnn", "conv", "groupnorm", "layernorm") + POOL_KINDS:
                raise _abi.DQNError(f"DeepQLearningError: unsupported layer {l!r} (supported: GlobalMaxPool / GlobalMeanPool / AdaptiveMaxPool / AdaptiveMeanPool, and (SkipConnection(+) / Conv / MaxPool / MeanPool / GroupNorm / Dense / Dropout / LSTM / GRU / RNN / LayerNorm / flattenbatch only); a standalone activation is Activation(σ))")
            if l.kind in ("layernorm", "dropout") and i > 0 and getattr(layers[i - 1], "kind", None) == "activation":
                raise _abi.DQNError(f"DeepQLearningError: {l!r} cannot directly follow {layers[i - 1]!r}: a {type(l).__name__} directly behind a standalone Activation layer is not supported "
                                    "(it must directly follow a Dense, recurrent" + (" or LayerNorm" if l.kind == "dropout" else "") + " layer)")
            if l.kind in ("layernorm", "dropout") and i > 0 and getattr(layers[i - 1], "kind", None) == l.kind:      # (the engine refuses it by index: build_layers)
                raise _abi.DQNError(f"DeepQLearningError: {l!r} cannot directly follow {layers[i - 1]!r}: two {type(l).__name__} layers in a row are not supported "
                                    "(it must directly follow a Dense, recurrent" + (" or LayerNorm" if l.kind == "dropout" else "") + " layer)")
            d.act, d.stream = _act_code(l), stream
            if l.kind == "dense":
                d.kind, d.n_in, d.n_out = _abi.LAYER_DENSE, l.n_in, l.n_out
            elif l.kind == "lstm":
                d.kind, d.n_in, d.n_out = _abi.LAYER_LSTM, l.n_in, l.n_out
            elif l.kind == "gru":
                d.kind, d.n_in, d.n_out = _abi.LAYER_GRU, l.n_in, l.n_out
            elif l.kind == "rnn":       # act carries the cell's σ
                d.kind, d.n_in, d.n_out = _abi.LAYER_RNN, l.n_in, l.n_out
            elif l.kind == "layernorm":      # n in both size slots; the fp32 bit pattern of eps rides in cin (as a Conv's pad rides in n_in / n_out)
                d.kind, d.n_in, d.n_out = _abi.LAYER_LAYERNORM, l.n, l.n
                d.cin = int(np.float32(l.eps).view(np.int32))
            elif l.kind == "groupnorm":      # cin == cout == chs, kh = G, the fp32 bit pattern of eps in kw; n_in == n_out == 0: the engine fills in c * h * w
                placed(l, stream, is_last)
                d.kind, d.cin, d.cout, d.kh = _abi.LAYER_GROUPNORM, l.chs, l.chs, l.G
                d.kw = int(np.float32(l.eps).view(np.int32))
            elif l.kind == "dropout":      # n_in == n_out == 0: the engine fills in the incoming feature count; p crosses as its Float64 bit pattern, low word in cin, high in cout
                bits = int(np.float64(l.p).view(np.uint64))
                d.kind = _abi.LAYER_DROPOUT
                d.cin, d.cout = int(np.uint32(bits & 0xFFFFFFFF).view(np.int32)), int(np.uint32(bits >> 32).view(np.int32))
            elif l.kind in ("adaptivemaxpool", "adaptivemeanpool"):      # kh, kw = the OUTPUT size (oh, ow); sh = sw = n_in = n_out = 0: the engine resolves the window from the map
                placed(l, stream, is_last)
                d.kind = _abi.LAYER_ADAPTIVEMAXPOOL if l.kind == "adaptivemaxpool" else _abi.LAYER_ADAPTIVEMEANPOOL
                d.cin = d.cout = chan[0]
                d.kh, d.kw = l.oh, l.ow
            elif l.kind in ("maxpool", "meanpool"):      # cin == cout == channels of the incoming map
                d.kind = _abi.LAYER_MAXPOOL if l.kind == "maxpool" else _abi.LAYER_MEANPOOL
                d.cin = d.cout = chan[0]
                d.kh, d.kw, d.sh, d.sw = l.kh, l.kw, l.sh, l.sw
            else:
                d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = l.cin, l.cout, l.kh, l.kw, l.sh, l.sw
                if l.general:      # dilation != 1 or groups != 1: kind 15; the five small integers ride packed, pad_h | pad_w << 16 in n_in, dh | dw << 8 | g << 16 in n_out
                    placed(l, stream, is_last)
                    d.kind = _abi.LAYER_CONV_DG
                    d.n_in, d.n_out = l.ph | (l.pw << 16), l.dh | (l.dw << 8) | (l.groups << 16)
                else:
                    d.kind = _abi.LAYER_CONV
                    d.n_in, d.n_out = l.ph, l.pw      # the pad rides in the slots a Conv leaves unused (0, 0 for every unpadded layer)
                chan[0] = l.cout
            out.append(d)

    if isinstance(net, DuelingNetwork):
        add(net.base, _abi.STREAM_BASE)
        add(net.val, _abi.STREAM_VAL)
        add(net.adv, _abi.STREAM_ADV)
        return out, True
    add(net, _abi.STREAM_BASE)
    return out, False


def isrecurrent(m):
    """src/helpers.jl:25-32."""
    return any(getattr(l, "kind", None) in ("lstm", "gru", "rnn") for l in all_layers(m))


def all_layers(net):
    """the layers in Flux.params order; a SkipConnection block contributes its inner layers (the join has no parameters)."""
    def flat(chain):
        out = []
        for l in chain:
            out += flat(l.layers) if getattr(l, "kind", None) == "skip" else [l]
        return out
    return flat(net.base) + flat(net.val) + flat(net.adv) if isinstance(net, DuelingNetwork) else flat(net)


def glorot_params(net, seed=1):
    """Flux default init: glorot_uniform weights ((rand - 0.5) * sqrt(24/(fan_in+fan_out))), zero biases, as one flat
    fp32 vector in Flux.params order.  (NumPy's RNG stream, not Julia's.)"""
    rng = np.random.default_rng(seed)
    parts = []
    for l in all_layers(net):
        if l.kind in POOL_KINDS + ("dropout", "activation"):      # no parameters
            continue
        if l.kind == "groupnorm":      # β = zeros, then γ = ones
            parts += [np.zeros(l.chs, np.float32), np.ones(l.chs, np.float32)]
            continue
        if l.kind == "layernorm":      # Flux Scale(n): scale = ones, bias = zeros
            parts += [np.ones(l.n, np.float32), np.zeros(l.n, np.float32)]
            continue
        if l.kind == "lstm":
            h = l.n_out
            for shp, fi, fo in (((l.n_in, 4 * h), l.n_in, 4 * h), ((h, 4 * h), h, 4 * h)):
                parts.append(((rng.random(shp, dtype=np.float32) - np.float32(0.5)) * np.sqrt(np.float32(24.0) / np.float32(fi + fo))).astype(np.float32).reshape(-1))
            b = np.zeros(4 * h, np.float32)
            b[h:2 * h] = 1.0        # Flux LSTMCell: forget-gate bias initialised to 1
            parts += [b, np.zeros(h, np.float32), np.zeros(h, np.float32)]
            continue
        if l.kind in ("gru", "rnn"):      # Flux GRUCell / RNNCell: glorot Wi, Wh; zero b (no forget-gate bias); zero state0
            for shp, (fi, fo) in zip(l.shapes()[:2], l.fans()):
                parts.append(((rng.random(shp, dtype=np.float32) - np.float32(0.5)) * np.sqrt(np.float32(24.0) / np.float32(fi + fo))).astype(np.float32).reshape(-1))
            parts += [np.zeros(l.shapes()[2], np.float32), np.zeros(l.n_out, np.float32)]
            continue
        wshape, bshape = l.shapes()
        fi, fo = l.fans()
        parts.append(((rng.random(wshape, dtype=np.float32) - np.float32(0.5)) * np.sqrt(np.float32(24.0) / np.float32(fi + fo))).astype(np.float32).reshape(-1))
        parts.append(np.zeros(bshape, np.float32))
    return np.concatenate(parts)


def nature_dqn(n_actions=4, in_channels=4):
    """BASELINE config 2: Chain(Conv((8,8),4=>32,relu;stride=4), Conv((4,4),32=>64,relu;stride=2),
    Conv((3,3),64=>64,relu), flattenbatch, Dense(3136,512,relu), Dense(512,nA)) for 84x84 inputs."""
    return Chain(Conv(8, in_channels, 32, relu, 4), Conv(4, 32, 64, relu, 2), Conv(3, 64, 64, relu, 1), flattenbatch,
                 Dense(3136, 512, relu), Dense(512, n_actions))
