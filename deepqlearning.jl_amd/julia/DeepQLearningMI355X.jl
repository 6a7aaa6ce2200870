# DeepQLearningMI355X.jl -- thin `ccall` shim that plugs libdqn_mi355x.so (include/dqn_mi355x.h) into
# DeepQLearning.jl v0.7.1 WITHOUT touching the package: it adds one replay type and one policy type and lets Julia's
# multiple dispatch route the hot path to the GPU:
#
#   batch_train!(solver, env, policy, optimizer, target_q, replay::HIPReplayBuffer)   <- src/solver.jl:191-198 seam
#   add_exp!, sample, get_batch, update_priorities!, populate_replay_buffer!            <- src/prioritized_experience_replay.jl:61-134
#   AbstractNNPolicy interface: getnetwork, resetstate!, actionmap, action, actionvalues, value  <- src/policy.jl:1-76
#
#   solve(MI355XSolver(solver), mdp)  /  initialize_replay_buffer(solver, env, action_indices, engine)  /  dqn_train!(solver, env, ::HIPNNPolicy, replay)
#                                                                                        <- src/solver.jl:30-57, :59-178, :180-189
#
# NOT EXECUTED IN THIS BUILD: neither the build container nor the GPU box has a `julia` binary (SURVEY.md), so this file
# ships as reviewed source.  Every call below goes through exactly the C entry points that tests/ exercise from Python
# (ctypes) with the same buffers, so its behaviour is pinned by the same fixtures.
module DeepQLearningMI355X

using DeepQLearning, Flux, POMDPs, POMDPTools, Random, Printf, Statistics, BSON
import DeepQLearning: batch_train!, add_exp!, update_priorities!, get_batch, populate_replay_buffer!, is_full, max_size,
                      getnetwork, resetstate!, actionmap, initialize_replay_buffer, dqn_train!,
                      AbstractNNPolicy, DQExperience, DeepQLearningSolver
import CommonRLInterface: AbstractEnv, observe, actions, act!, reset!, terminated
import TensorBoardLogger: TBLogger, log_value
import StatsBase
import POMDPModels      # the problem types of envs_create_control! (MountainCar, InvertedPendulum)
export MI355XSolver, HIPReplayBuffer, HIPEpisodeReplayBuffer, HIPNNPolicy, train_steps!, EngineGroup, close!, group_info, rollout_info

const LIB = get(ENV, "DQN_MI355X_LIB", "libdqn_mi355x.so")

# ---- C structs (must match include/dqn_mi355x.h field for field)
struct LayerDesc
    kind::Int32; act::Int32; stream::Int32
    n_in::Int32; n_out::Int32
    cin::Int32; cout::Int32; kh::Int32; kw::Int32; sh::Int32; sw::Int32
end
mutable struct HParams
    batch_size::Int32; n_actions::Int32
    obs_c::Int32; obs_h::Int32; obs_w::Int32; obs_dtype::Int32
    learning_rate::Float32
    adam_beta1::Float64; adam_beta2::Float64; adam_eps::Float64
    adam_f64_scalars::Int32
    gamma::Float32
    double_q::Int32; dueling::Int32; prioritized_replay::Int32
    buffer_size::Int64
    prio_alpha::Float32; prio_beta::Float32; prio_eps::Float32
    seed::UInt64
    use_graph::Int32; use_mfma::Int32
    recurrence::Int32; trace_length::Int32
    sample_distinct::Int32
    reserved::NTuple{3,Int32}
    HParams() = new()
end

check(rc) = rc == 0 ? nothing : throw(unsafe_string(ccall((:dqn_last_error, LIB), Cstring, ())))  # reference errors are thrown Strings

# DQN_ACT_* (include/dqn_mi355x.h has the table of the eleven laws).  NNlib's default parameters only: leakyrelu(x) = leakyrelu(x, 0.01), elu(x) = elu(x, 1)
const ACT = Dict(identity => 0, relu => 1, tanh => 2, sigmoid => 3, leakyrelu => 4, elu => 5, selu => 6, softplus => 7, softsign => 8, relu6 => 9, hardtanh => 10)
const ACT_SUPPORTED = "identity / relu / tanh / sigmoid / leakyrelu / elu / selu / softplus / softsign / relu6 / hardtanh"
const ACT_NEEDS_X = (gelu, swish, mish, hardswish)      # not monotone: the derivative is no function of the output
# the activation a layer carries: σ of a Dense / Conv / RNN cell, λ of a LayerNorm / GroupNorm; nothing for the layers without one
layer_act(l) = (l isa Dense || l isa Conv) ? l.σ : (l isa Flux.LayerNorm || l isa Flux.GroupNorm) ? l.λ : (l isa Flux.Recur && l.cell isa Flux.RNNCell) ? l.cell.σ : nothing
# the one check of a layer's activation: lower_layer calls it first, so that every ACT[...] lookup below it is a hit (a bare lookup died on a KeyError with no explanation).
# Throws the DeepQLearningError that names what is supported, and why the rest is not
function check_act(l)
    f = layer_act(l)
    (f === nothing || haskey(ACT, f)) && return nothing
    any(g -> f === g, ACT_NEEDS_X) && throw("DeepQLearningError: unsupported activation $(f) on $(typeof(l)): it is not monotone, so its derivative needs the pre-activation, and the MI355X engine keeps only each layer's output and differentiates from it (supported: $(ACT_SUPPORTED))")
    throw("DeepQLearningError: unsupported activation $(f) on $(typeof(l)) (supported: $(ACT_SUPPORTED)); default parameters only: a closure such as x -> leakyrelu(x, 0.2f0) or x -> elu(x, 2f0) has no code")
end

function lower_layer(l, stream)::LayerDesc
    check_act(l)
    if l isa Dense
        return LayerDesc(0, ACT[l.σ], stream, size(l.weight, 2), size(l.weight, 1), 0, 0, 0, 0, 0, 0)
    elseif l isa Conv
        kw, kh, cin, cout = size(l.weight)
        # l.pad is NTuple{4}: (lo, hi) of the W axis, then of the H axis -- the first pair belongs to the W axis, as l.stride[1] does.  Symmetric zero padding only
        # (SamePad() on an even kernel yields lo != hi); the engine checks 0 <= pad <= kernel - 1.  (pad_h, pad_w) ride in the n_in, n_out slots a Conv leaves unused
        p = length(l.pad) == 4 ? l.pad : (l.pad[1], l.pad[1], l.pad[2], l.pad[2])
        (p[1] == p[2] && p[3] == p[4]) || throw("DeepQLearningError: the MI355X engine supports Conv with symmetric pad only (lo == hi on each axis), got asymmetric pad=$(l.pad)")
        # l.dilation is NTuple{2} in (W, H) order, like l.stride; l.groups an Int; with groups the weight is (kw, kh, cin ÷ groups, cout), so size(l.weight, 3) is the channels PER GROUP.
        # dilation = 1 and groups = 1 stays kind 1, the descriptor it always was; anything else (DepthwiseConv included: Flux builds it as Conv(...; groups = cin)) is kind 15 with
        # the FULL channel counts and the five small integers packed: pad_h | pad_w << 16 in n_in, dh | dw << 8 | groups << 16 in n_out (include/dqn_mi355x.h)
        dil = l.dilation; g = l.groups
        if any(!=(1), dil) || g != 1
            all(>=(1), dil) || throw("DeepQLearningError: Conv with dilation=$(dil): the dilation must be at least 1 per axis")
            (all(<=(255), dil) && g <= 32767) || throw("DeepQLearningError: Conv with dilation=$(dil), groups=$(g): the MI355X engine takes dilation <= 255 and groups <= 32767")
            (g >= 1 && cout % g == 0) || throw("DeepQLearningError: Conv with groups=$(g): groups must be >= 1 and divide cin = $(cin * g) and cout = $(cout)")
            (p[3] <= (kh - 1) * dil[2] && p[1] <= (kw - 1) * dil[1]) || throw("DeepQLearningError: Conv pad ($(p[3]), $(p[1])) is larger than the dilated kernel extent - 1 = ($((kh - 1) * dil[2]), $((kw - 1) * dil[1]))")
            stream == 0 || throw("DeepQLearningError: a Conv with dilation=$(dil) / groups=$(g) is supported in the base chain only (not in a value / advantage stream)")
            return LayerDesc(15, ACT[l.σ], stream, p[3] | (p[1] << 16), dil[2] | (dil[1] << 8) | (g << 16), cin * g, cout, kh, kw, l.stride[2], l.stride[1])
        end
        return LayerDesc(1, ACT[l.σ], stream, p[3], p[1], cin, cout, kh, kw, l.stride[2], l.stride[1])
    elseif l isa Flux.MaxPool      # fields k, pad, stride; no parameters; cin = cout = 0: the engine takes the channels of the incoming map
        any(!=(0), l.pad) && throw("DeepQLearningError: the MI355X engine supports MaxPool with pad=0 only")
        return LayerDesc(5, 0, stream, 0, 0, 0, 0, l.k[2], l.k[1], l.stride[2], l.stride[1])
    elseif l isa Flux.MeanPool
        any(!=(0), l.pad) && throw("DeepQLearningError: the MI355X engine supports MeanPool with pad=0 only")
        return LayerDesc(6, 0, stream, 0, 0, 0, 0, l.k[2], l.k[1], l.stride[2], l.stride[1])
    elseif l isa Flux.GlobalMaxPool || l isa Flux.GlobalMeanPool      # no fields; maxpool / meanpool with window = the whole (w, h) map, output (1, 1, c, batch): the adaptive kinds with output (1, 1)
        return LayerDesc(l isa Flux.GlobalMaxPool ? 12 : 13, 0, stream, 0, 0, 0, 0, 1, 1, 0, 0)
    elseif l isa Flux.AdaptiveMaxPool || l isa Flux.AdaptiveMeanPool      # field out, in Julia's (W, H) order; no parameters.  Flux's PoolDims rule per axis -- stride = in ÷ out,
        # k = in - (out - 1) * stride, pad 0 -- needs the map size, which the engine knows: kh, kw carry the OUTPUT size (oh, ow), sh = sw = 0, and the engine resolves the window
        return LayerDesc(l isa Flux.AdaptiveMaxPool ? 12 : 13, 0, stream, 0, 0, 0, 0, l.out[2], l.out[1], 0, 0)
    elseif l isa Flux.LayerNorm      # Flux 0.14 fields λ, diag, ϵ, size, affine; Flux.params order diag.scale, diag.bias == the ABI's LayerNorm block
        # normalise(x; dims, ϵ) = (x .- μ) ./ (σ .+ ϵ) with the uncorrected σ: ϵ is added OUTSIDE the root -- the engine runs this law, not torch's sqrt(var + eps).
        # n in both size slots, the Float32 bit pattern of ϵ in cin (as a Conv's pad rides in n_in / n_out)
        length(l.size) == 1 || throw("DeepQLearningError: the MI355X engine supports LayerNorm(n) with an integer n only, got size=$(l.size)")
        (l.affine && l.diag isa Flux.Scale) || throw("DeepQLearningError: the MI355X engine supports LayerNorm with affine=true only")
        return LayerDesc(7, ACT[l.λ], stream, l.size[1], l.size[1], reinterpret(Int32, Float32(l.ϵ)), 0, 0, 0, 0, 0)
    elseif l isa Flux.GroupNorm      # Flux 0.14 fields G, λ, β, γ, μ, σ², ϵ, momentum, chs, affine, track_stats, active; Flux.params order β, γ (bias FIRST) == the ABI's GroupNorm block
        # _norm_layer_forward: (x .- μ) ./ sqrt.(σ² .+ ϵ) with the uncorrected σ² per sample and group of chs / G contiguous channels: ϵ INSIDE the root (not LayerNorm's σ + ϵ).
        # cin = cout = chs, kh = G, the Float32 bit pattern of ϵ in kw; n_in = n_out = 0: the engine takes the feature count of the incoming map
        l.affine || throw("DeepQLearningError: the MI355X engine supports GroupNorm with affine=true only")
        l.track_stats && throw("DeepQLearningError: the MI355X engine supports GroupNorm with track_stats=false only (it keeps no running statistics: every pass normalises with the statistics of its own input)")
        return LayerDesc(11, ACT[l.λ], stream, 0, 0, l.chs, l.chs, l.G, reinterpret(Int32, Float32(l.ϵ)), 0, 0)
    elseif l isa Flux.Dropout      # Flux 0.14 fields p, dims, active, rng; no parameters (Flux.params skips the layer)
        # automatic mode (active === nothing): the layer is active only under Flux.gradient -- the engine masks the online forward on s and nothing else.  A forced mode
        # (trainmode! / testmode!) is not the reference's behaviour.  p crosses as its Float64 bit pattern, low word in cin, high word in cout (Float32(0.1) would move
        # 1 / (1 - p) off Flux's value); n_in = n_out = 0: the engine takes the incoming feature count.  The mask is the engine's own counter-based law, not l.rng
        l.dims === Colon() || throw("DeepQLearningError: the MI355X engine supports Dropout with dims = : only, got dims=$(l.dims)")
        l.active === nothing || throw("DeepQLearningError: the MI355X engine supports Dropout in Flux's automatic mode only (active = nothing), got active=$(l.active): a forced train / test mode is not the reference's behaviour")
        bits = reinterpret(UInt64, Float64(l.p))
        return LayerDesc(8, 0, stream, 0, 0, reinterpret(Int32, UInt32(bits & 0xffffffff)), reinterpret(Int32, UInt32(bits >> 32)), 0, 0, 0, 0)
    elseif l isa Flux.Recur && l.cell isa Flux.LSTMCell     # Flux.params order Wi, Wh, b, state0 (h0, c0) == the ABI's LSTM block
        return LayerDesc(2, 0, stream, size(l.cell.Wi, 2), size(l.cell.Wh, 2), 0, 0, 0, 0, 0, 0)
    elseif l isa Flux.Recur && l.cell isa Flux.GRUCell      # Flux.params order Wi, Wh, b, state0 (h0) == the ABI's GRU block (Flux's GRUv3 has another block: unsupported)
        return LayerDesc(3, 0, stream, size(l.cell.Wi, 2), size(l.cell.Wh, 2), 0, 0, 0, 0, 0, 0)
    elseif l isa Flux.Recur && l.cell isa Flux.RNNCell      # Flux.params order Wi, Wh, b, state0 (h0) == the ABI's RNN block; act = the cell's σ (the engine accepts the first four codes there)
        return LayerDesc(4, ACT[l.cell.σ], stream, size(l.cell.Wi, 2), size(l.cell.Wh, 2), 0, 0, 0, 0, 0, 0)
    end
    if l isa Base.Broadcast.BroadcastFunction      # Julia's own callable struct (>= 1.6; field f, recalled): BroadcastFunction(σ)(x) == σ.(x) -- the standalone activation layer, kind 14.
        # No parameters (Flux.params finds nothing in it).  act = σ's code: the eleven of ACT, then ACT_NEEDS_X in order = 11..14 (gelu, swish, mish, hardswish: the layer reads the
        # stored output of the layer in front, so the pre-activation their derivative needs is there).  n_in = n_out = 0: the engine takes the incoming feature count and shape
        i = findfirst(g -> l.f === g, ACT_NEEDS_X)
        code = haskey(ACT, l.f) ? ACT[l.f] : i === nothing ? -1 : 10 + i
        code >= 0 || throw("DeepQLearningError: unsupported activation $(l.f) in Base.BroadcastFunction (supported: $(ACT_SUPPORTED) / gelu / swish / mish / hardswish); default parameters only: a closure such as x -> leakyrelu(x, 0.2f0) has no code")
        return LayerDesc(14, code, stream, 0, 0, 0, 0, 0, 0, 0, 0)
    end
    l isa Flux.BatchNorm && throw("DeepQLearningError: BatchNorm is not supported: it keeps running statistics, so the online pass on s, the pass on s', the target pass and the acting pass would compute different functions; of Flux's normalisation layers the MI355X engine runs LayerNorm(n) and GroupNorm(chs, G)")
    l isa Flux.InstanceNorm && throw("DeepQLearningError: InstanceNorm is not supported: its default is affine = false, which the MI355X engine does not run; GroupNorm(chs, chs) is instance normalisation with a per-channel affine")
    l isa Flux.Parallel && throw("DeepQLearningError: Parallel is not supported; of Flux's branching layers the MI355X engine runs SkipConnection(layers, +) only")
    throw("DeepQLearningError: unsupported layer $(typeof(l)) (supported: GlobalMaxPool / GlobalMeanPool / AdaptiveMaxPool / AdaptiveMeanPool, and (SkipConnection(+) / Conv / MaxPool / MeanPool / GroupNorm / Dense / Dropout / LSTM / GRU / RNN / LayerNorm / flattenbatch only); a standalone activation is written Base.BroadcastFunction(relu): an anonymous closure such as x -> relu.(x) cannot be inspected and is skipped as glue, like x -> flattenbatch(x))")
end
# What a Chain may hold beside layers.  ORDER MATTERS: Julia declares `struct BroadcastFunction{F} <: Function` (recalled), so the standalone activation layer IS a Function and
# must be recognised BEFORE anything is taken for glue -- asked second, Base.BroadcastFunction(gelu) would be dropped and the network would train without its activations.
#   is_act_layer   Base.BroadcastFunction(σ): a layer (kind 14), never glue
#   glue           identity, flattenbatch and EVERY other function, named or anonymous, as before: no descriptor, the engine flattens between a map and a Dense by itself.
#                  The reference's own models write the flatten as a closure -- Chain(x -> flattenbatch(x), Dense(...), ...) in its tests and benchmarks -- and a closure
#                  cannot be inspected, so it cannot be told from x -> relu.(x).  THE LIMITATION: an activation written as a closure is skipped like any glue and the
#                  network trains without it; a standalone activation must be written Base.BroadcastFunction(relu) (README, DESIGN section 4 "Activation layers")
is_act_layer(l) = l isa Base.Broadcast.BroadcastFunction
is_glue(l) = !is_act_layer(l) && (l === identity || l === flattenbatch || l isa Function)
# the placement of the standalone activation layers, by name (the engine's build_layers holds the same rules by layer index for C callers): never the first layer, never the
# network's output layer (the last base layer of a dueling network is fine), base chain only, no LayerNorm / Dropout directly behind it -- the NEXT DESCRIPTOR, whatever it
# belongs to: a LayerNorm / Dropout that is the first inner layer of a SkipConnection directly behind the Activation reads the Activation's output and is refused too, as the engine refuses it
const ACT_LAYER_NAMES = ("identity", "relu", "tanh", "sigmoid", "leakyrelu", "elu", "selu", "softplus", "softsign", "relu6", "hardtanh", "gelu", "swish", "mish", "hardswish")
function check_act_layers(descs, dueling)
    for (i, d) in enumerate(descs)
        d.kind == 14 || continue
        nm = "Base.BroadcastFunction($(ACT_LAYER_NAMES[d.act + 1]))"
        i == 1 && throw("DeepQLearningError: $(nm) cannot be the first layer: its input is the stored output of the layer in front (an activation on the observation is not supported)")
        d.stream == 0 || throw("DeepQLearningError: $(nm) is supported in the base chain only (not in a value / advantage stream)")
        (!dueling && i == length(descs)) && throw("DeepQLearningError: $(nm) cannot be the network's output layer")
        if i < length(descs) && descs[i + 1].stream == 0 && (descs[i + 1].kind == 7 || descs[i + 1].kind == 8)
            throw("DeepQLearningError: $(descs[i + 1].kind == 7 ? "LayerNorm" : "Dropout") cannot directly follow $(nm): a LayerNorm / Dropout directly behind a standalone activation layer is not supported")
        end
    end
    descs
end
# Flux 0.14 SkipConnection(layers, connection), fields layers, connection: layers(x) .+ x for connection === +.  No parameters of its own (Flux.params yields the inner
# layers' in order, which flatparams below follows) and no activation.  Lowered as the inner layers' descriptors, then ONE join descriptor of kind 9 directly behind them:
# cin = m, the number of inner descriptors; n_in = n_out = 0: the engine takes the feature count.  The engine checks the placement (base chain, on a feature vector, never
# first or last, n -> n); what it cannot see is refused here by name: another connection (vcat, *, a closure), a nested block, an inner layer that is not Dense / LayerNorm / Dropout
#
# The CONVOLUTIONAL block, x + Conv(Conv(x)): where the descriptor in front is a Conv, a pool or the join of another such block (kinds 1, 5, 6, 10) and every inner layer
# is a Conv or a pool, the join is of kind 10 -- the same descriptor shape.  Its inner layers are Convs with pad != 0 that keep the channel count; a pool, a pad-0 Conv and
# a channel change are refused here by name, that the block keeps (h, w) is the engine's check
is_map_desc(d) = d.kind == 1 || d.kind == 5 || d.kind == 6 || d.kind == 10 || d.kind == 11 || d.kind == 12 || d.kind == 13 || d.kind == 15      # (11: a GroupNorm keeps the incoming map; 12, 13: the adaptive / global pools; 15: a dilated / grouped Conv)
is_general_conv(x) = x isa Conv && (any(!=(1), x.dilation) || x.groups != 1)      # kind 15: never inside a SkipConnection, so lower_skip_map! must not take it for a padded Conv
is_map_layer(x) = x isa Conv || x isa Flux.MaxPool || x isa Flux.MeanPool || x isa Flux.AdaptiveMaxPool || x isa Flux.AdaptiveMeanPool || x isa Flux.GlobalMaxPool || x isa Flux.GlobalMeanPool
function lower_skip_map!(descs, l, stream, inner)
    m = 0; c_in = 0; c_out = 0
    for x in inner
        is_glue(x) && continue
        x isa Conv || throw("DeepQLearningError: a MaxPool / MeanPool layer inside a convolutional SkipConnection is not supported (its inner layers are Conv layers with pad != 0 only)")
        all(==(0), x.pad) && throw("DeepQLearningError: a Conv with pad 0 inside a convolutional SkipConnection is not supported (its inner layers are Conv layers with pad != 0 only; 1x1 and unpadded inner convolutions are not supported)")
        m == 0 && (c_in = size(x.weight, 3)); c_out = size(x.weight, 4)
        push!(descs, lower_layer(x, stream)); m += 1
    end
    c_in == c_out || throw("DeepQLearningError: the convolutional SkipConnection maps $(c_in) channels to $(c_out); SkipConnection(layers, +) needs layers: (c, h, w) -> (c, h, w)")
    push!(descs, LayerDesc(10, 0, stream, 0, 0, m, 0, 0, 0, 0, 0))
end
function lower_skip!(descs, l, stream)
    l.connection === (+) || throw("DeepQLearningError: SkipConnection(layers, $(l.connection)) is not supported; the MI355X engine runs SkipConnection with the connection + only (vcat, *, closures and Parallel are not supported)")
    inner = l.layers isa Flux.Chain ? collect(l.layers.layers) : Any[l.layers]
    any(is_act_layer, inner) && throw("DeepQLearningError: an Activation layer (Base.BroadcastFunction) inside a SkipConnection is not supported (a standalone activation stands in the base chain, in front of or behind the block; inside, use the fused activation of Dense / Conv)")      # asked BEFORE the glue filter: the layer is a Function
    real = filter(!is_glue, inner)
    any(is_general_conv, real) && throw("DeepQLearningError: a Conv with dilation != 1 or groups != 1 (DepthwiseConv included) inside a SkipConnection is not supported (dilated and grouped residual blocks are not supported; the layer stands in the base chain, in front of or behind the block)")
    any(x -> x isa Flux.GroupNorm, real) && throw("DeepQLearningError: a GroupNorm layer inside a SkipConnection is not supported (GroupNorm stands in the base chain, in front of or behind the block)")
    if !isempty(descs) && is_map_desc(descs[end]) && !isempty(real) && all(is_map_layer, real)
        return lower_skip_map!(descs, l, stream, inner)
    end
    k = length(descs); while k >= 1 && descs[k].kind == 14; k -= 1; end      # a standalone activation keeps its input's shape AND kind of shape: look through it
    if 1 <= k < length(descs) && is_map_desc(descs[k]) && !isempty(real) && all(is_map_layer, real)
        return lower_skip_map!(descs, l, stream, inner)
    end
    m = 0
    for x in inner
        is_glue(x) && continue
        x isa Flux.SkipConnection && throw("DeepQLearningError: a SkipConnection inside a SkipConnection is not supported (nested skip blocks)")
        (x isa Dense || x isa Flux.LayerNorm || x isa Flux.Dropout) || throw("DeepQLearningError: unsupported layer $(typeof(x)) inside a SkipConnection (its inner layers are Dense, LayerNorm and Dropout layers only)")
        push!(descs, lower_layer(x, stream)); m += 1
    end
    m >= 1 || throw("DeepQLearningError: SkipConnection(Chain(), +) holds no layer; the MI355X engine needs at least one inner layer")
    push!(descs, LayerDesc(9, 0, stream, 0, 0, m, 0, 0, 0, 0, 0))
end
lower_into!(descs, l, stream) = is_glue(l) ? descs : l isa Flux.SkipConnection ? lower_skip!(descs, l, stream) : push!(descs, lower_layer(l, stream))
function lower(q)
    descs = LayerDesc[]
    if q isa DeepQLearning.DuelingNetwork
        for (chain, s) in ((q.base, 0), (q.val, 1), (q.adv, 2)), l in chain.layers
            lower_into!(descs, l, Int32(s))
        end
    else
        for l in q.layers; lower_into!(descs, l, Int32(0)); end
    end
    check_act_layers(descs, q isa DeepQLearning.DuelingNetwork)
end
flatparams(q) = reduce(vcat, [vec(Float32.(w)) for w in Flux.params(q)])   # Flux.params order, Julia memory order: exactly the ABI layout

# ---- engine handle
mutable struct Engine
    h::Ptr{Cvoid}
    B::Int; nA::Int; obs_dims::Tuple
    obs_u8::Bool      # replay rows are BYTES (hp.obs_dtype = DQN_OBS_U8): training reads byte / 255f0 (test/test_env.jl:59)
end
# observation rows in the replay's storage type.  dqn_replay_add reads the void* as bytes for a u8 replay: a Float32 buffer there
# would be cut to its first E bytes, so only UInt8 arrays are accepted (the Python mirror's _obs_rows does the same).  The EPISODE replay
# always stores Float32 rows (dqn_episode_add copies E*4 bytes per observation): dqn_engine_create refuses recurrence with obs_u8, so
# obs_rows never returns bytes for a HIPEpisodeReplayBuffer.
function obs_rows(e::Engine, x, what)
    e.obs_u8 || return Float32.(vec(x))
    eltype(x) == UInt8 || error("$what: this replay stores UInt8 observations (obs_u8 = true); got $(eltype(x)) -- pass the raw bytes")
    return collect(vec(x))
end
# what the POLICY must see for such a replay: the scale training uses
policy_obs(e::Engine, o) = (e.obs_u8 && eltype(o) == UInt8) ? Float32.(vec(o)) ./ 255f0 : Float32.(vec(o))
function Engine(solver::DeepQLearningSolver, env::AbstractEnv, q; device=0, obs_u8=false)
    o = observe(env); dims = size(o)
    c, h, w = length(dims) == 3 ? (dims[3], dims[2], dims[1]) : (prod(dims), 1, 1)   # Julia (W,H,C) -> C [C][H][W]
    hp = HParams(); check(ccall((:dqn_hparams_default, LIB), Cint, (Ref{HParams},), hp))
    hp.batch_size = solver.batch_size; hp.n_actions = length(actions(env))
    hp.obs_c, hp.obs_h, hp.obs_w, hp.obs_dtype = c, h, w, obs_u8 ? 1 : 0
    hp.learning_rate = solver.learning_rate; hp.gamma = Float32(DeepQLearning.default_discount(env))
    hp.double_q = solver.double_q; hp.dueling = q isa DeepQLearning.DuelingNetwork; hp.prioritized_replay = solver.prioritized_replay
    hp.buffer_size = solver.buffer_size
    hp.recurrence = solver.recurrence; hp.trace_length = solver.trace_length
    descs = lower(q); out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dqn_engine_create, LIB), Cint, (Ptr{LayerDesc}, Cint, Ref{HParams}, Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}),
                descs, length(descs), hp, C_NULL, device, out))
    e = Engine(out[], solver.batch_size, length(actions(env)), dims, obs_u8)
    finalizer(x -> ccall((:dqn_engine_destroy, LIB), Cint, (Ptr{Cvoid},), x.h), e)
    p = flatparams(q)
    check(ccall((:dqn_set_params, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Csize_t), e.h, 0, p, length(p)))
    check(ccall((:dqn_sync_target, LIB), Cint, (Ptr{Cvoid},), e.h))
    e
end

# ---- replay protocol (src/prioritized_experience_replay.jl)
mutable struct HIPReplayBuffer
    e::Engine
    rng::AbstractRNG
end
max_size(r::HIPReplayBuffer) = (cap = Ref{Int64}(); ccall((:dqn_replay_size, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ref{Int64}), r.e.h, C_NULL, cap); cap[])
cur_size(r::HIPReplayBuffer) = (cur = Ref{Int64}(); ccall((:dqn_replay_size, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}), r.e.h, cur, C_NULL); cur[])
is_full(r::HIPReplayBuffer) = cur_size(r) == max_size(r)

function add_exp!(r::HIPReplayBuffer, expe::DQExperience, td_err=abs(expe.r))      # :65-74
    s = obs_rows(r.e, expe.s, "add_exp!"); sp = obs_rows(r.e, expe.sp, "add_exp!")
    check(ccall((:dqn_replay_add, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int32}, Ref{Float32}, Ptr{Cvoid}, Ref{UInt8}, Ref{Float32}, Cint),
                r.e.h, s, Int32(expe.a - 1), Float32(expe.r), sp, UInt8(expe.done), Float32(td_err), 1))   # 1-based -> 0-based action
end
function update_priorities!(r::HIPReplayBuffer, indices::Vector{Int64}, td_errors)  # :76-80
    check(ccall((:dqn_update_priorities, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float32}, Cint), r.e.h, indices .- 1, Float32.(td_errors), length(indices)))
end
function get_batch(r::HIPReplayBuffer, idx::Vector{Int64})                           # :89-104
    B = r.e.B
    s = zeros(Float32, r.e.obs_dims..., B); sp = similar(s)
    a = zeros(Int32, B); rew = zeros(Float32, B); done = zeros(Float32, B); w = zeros(Float32, B)
    check(ccall((:dqn_replay_get_batch, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float32}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                r.e.h, idx .- 1, s, a, rew, sp, done, w))
    return s, [CartesianIndex(Int(a[i]) + 1, i) for i in 1:B], rew, sp, done, idx, w
end
function StatsBase.sample(r::HIPReplayBuffer)                                        # :82-87 (sum-tree on the device)
    idx = zeros(Int64, r.e.B)
    check(ccall((:dqn_replay_sample, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), r.e.h, idx))
    get_batch(r, idx .+ 1)
end

# populate_replay_buffer!(replay, env, action_indices; max_pop, max_steps, policy) (:106-134): the package's method is typed on
# PrioritizedReplayBuffer and reads replay._curr_size, so the HIP replay gets its own: a random (or given) policy fills the ring with
# priority |r|, episodes are cut at max_steps
function populate_replay_buffer!(replay::HIPReplayBuffer, env::AbstractEnv, action_indices;
                                 max_pop::Int64 = max_size(replay), max_steps::Int64 = 100,
                                 policy::Policy = FunctionPolicy(o -> rand(actions(env))))
    reset!(env); o = observe(env); step = 0
    for _ in 1:(max_pop - cur_size(replay))
        a = action(policy, o)
        rew = Float32(act!(env, a)); op = observe(env); done = terminated(env)
        add_exp!(replay, DQExperience(o, action_indices[a], rew, op, done), abs(rew))    # "assume initial td error is r" (:122)
        o = op; step += 1
        if done || step >= max_steps
            reset!(env); o = observe(env); step = 0
        end
    end
    cur_size(replay) >= replay.e.B || throw(AssertionError("replay._curr_size >= replay.batch_size"))    # :133
    replay
end

# ---- the hot path: ONE ccall per batch_train!  (src/solver.jl:191-236)
function batch_train!(solver::DeepQLearningSolver, env::AbstractEnv, policy::AbstractNNPolicy, optimizer, target_q,
                      replay::HIPReplayBuffer; discount=DeepQLearning.default_discount(env))
    loss = Ref{Float32}(0); gn = Ref{Float32}(0)
    check(ccall((:dqn_train_step, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ref{Float32}, Ref{Float32}, Ptr{Float32}), replay.e.h, C_NULL, loss, gn, C_NULL))
    return loss[], gn[]
end

# The same step WITHOUT waiting for it (feed-forward engines): returns once the step is enqueued; the ticket names the (loss, grad_norm) record the
# step's last launch publishes into a mapped host ring.  The reference looks at batch_train!'s return values only every log_freq env steps
# (src/solver.jl:154-167), so the shim's dqn_train! loop below trains with this call and fetches the scalars of the newest step when it logs.
function batch_train_async!(replay::HIPReplayBuffer)
    ticket = Ref{UInt64}(0)
    check(ccall((:dqn_train_step_async, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ref{UInt64}), replay.e.h, C_NULL, ticket))
    return ticket[]
end
function step_scalars(e::Engine, ticket::UInt64; wait::Bool = true)
    loss = Ref{Float32}(0); gn = Ref{Float32}(0); pub = Ref{UInt64}(0)
    check(ccall((:dqn_step_scalars, LIB), Cint, (Ptr{Cvoid}, UInt64, Cint, Ref{Float32}, Ref{Float32}, Ref{UInt64}), e.h, ticket, wait ? 1 : 0, loss, gn, pub))
    return pub[] == ticket ? (loss[], gn[]) : nothing
end

# n sampled batch_train! steps back to back with nothing in between (no reference equivalent: offline / catch-up training on a filled replay).
# Bit-identical to n batch_train! calls; inside the call step i's last launch already gathers step i+1's batch (dqn_train_steps).
function train_steps!(e::Engine, n::Integer)
    loss = Ref{Float32}(0); gn = Ref{Float32}(0)
    check(ccall((:dqn_train_steps, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{Float32}, Ref{Float32}), e.h, n, loss, gn))
    return loss[], gn[]
end

# ---- engine groups (no reference equivalent): K small engines -- seeds, a learning-rate sweep, an ensemble -- stepped by ONE launch of K workgroups.  After
# train_steps!(g, n) every member is bit for bit what train_steps!(e, n) would have left (include/dqn_mi355x.h, engine groups).  The group keeps its members
# reachable; close!(g) before a member is finalized (dqn_engine_destroy refuses a member of a live group).
mutable struct GroupInfo
    n_members::Int32; max_lds_bytes::UInt32; launches_per_step::Int32; reserved::Int32
    GroupInfo() = new(0, 0, 0, 0)
end
mutable struct EngineGroup
    h::Ptr{Cvoid}
    members::Vector{Engine}
end
function EngineGroup(members::Vector{Engine})
    hs = Ptr{Cvoid}[e.h for e in members]; out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:dqn_group_create, LIB), Cint, (Ptr{Ptr{Cvoid}}, Cint, Ref{Ptr{Cvoid}}), hs, length(hs), out))
    g = EngineGroup(out[], members)
    finalizer(close!, g)
    g
end
function close!(g::EngineGroup)
    g.h == C_NULL && return nothing
    ccall((:dqn_group_destroy, LIB), Cint, (Ptr{Cvoid},), g.h); g.h = C_NULL
    nothing
end
function train_steps!(g::EngineGroup, n::Integer)      # -> (loss[K], grad_norm[K]) of the last step
    K = length(g.members); loss = zeros(Float32, K); gn = zeros(Float32, K)
    check(ccall((:dqn_group_train_steps, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{Float32}), g.h, n, loss, gn))
    return loss, gn
end
function group_info(g::EngineGroup)
    gi = GroupInfo()
    check(ccall((:dqn_group_info, LIB), Cint, (Ptr{Cvoid}, Ref{GroupInfo}), g.h, gi))
    return (n_members = Int(gi.n_members), max_lds_bytes = Int(gi.max_lds_bytes), launches_per_step = Int(gi.launches_per_step))
end

# ---- DRQN: EpisodeReplayBuffer protocol (src/episode_replay.jl) and the recurrent batch_train! (src/solver.jl:239-287)
mutable struct HIPEpisodeReplayBuffer
    e::Engine
    rng::AbstractRNG
end
function add_exp!(r::HIPEpisodeReplayBuffer, expe::DQExperience)                      # :46-52 (the engine stores the episode when done)
    check(ccall((:dqn_episode_add, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int32}, Ref{Float32}, Ptr{Cvoid}, Ref{UInt8}, Cint),
                r.e.h, obs_rows(r.e, expe.s, "add_exp!"), Int32(expe.a - 1), Float32(expe.r), obs_rows(r.e, expe.sp, "add_exp!"), UInt8(expe.done), 1))
end
add_episode!(r::HIPEpisodeReplayBuffer) = check(ccall((:dqn_episode_commit, LIB), Cint, (Ptr{Cvoid},), r.e.h))   # :54-60, after generate_episode
ep_count(r::HIPEpisodeReplayBuffer) = (cur = Ref{Int64}(); ccall((:dqn_episode_count, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}), r.e.h, cur, C_NULL); cur[])
max_size(r::HIPEpisodeReplayBuffer) = (cap = Ref{Int64}(); ccall((:dqn_episode_count, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ref{Int64}), r.e.h, C_NULL, cap); cap[])
is_full(r::HIPEpisodeReplayBuffer) = ep_count(r) == max_size(r)
# populate_replay_buffer!(r::EpisodeReplayBuffer, env, action_indices; max_pop, max_steps) (src/episode_replay.jl:97-130): random rollouts of
# fewer than max_steps steps, each stored as one episode whether or not it terminated
function populate_replay_buffer!(r::HIPEpisodeReplayBuffer, env::AbstractEnv, action_indices; max_pop::Int64 = max_size(r), max_steps::Int64 = 100)
    for _ in 1:(max_pop - ep_count(r))
        reset!(env); o = observe(env); done = false; step = 1
        while !done && step < max_steps
            a = rand(actions(env)); rew = Float32(act!(env, a)); op = observe(env); done = terminated(env)
            add_exp!(r, DQExperience(o, action_indices[a], rew, op, done))     # a terminal transition stores the episode (add_exp!, :46-52)
            o = op; step += 1
        end
        done || add_episode!(r)                                                 # cut at max_steps: add_episode!(r, ep), :100-101
    end
    ep_count(r) >= r.e.B || throw(AssertionError("r._curr_size >= r.batch_size"))
    r
end
function batch_train!(solver::DeepQLearningSolver, env::AbstractEnv, policy::AbstractNNPolicy, optimizer, target_q,
                      replay::HIPEpisodeReplayBuffer; discount=DeepQLearning.default_discount(env))
    loss = Ref{Float32}(0); gn = Ref{Float32}(0)
    check(ccall((:dqn_train_step_drqn, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ref{Float32}, Ref{Float32}), replay.e.h, C_NULL, C_NULL, loss, gn))
    return loss[], gn[]
end

# ---- policy (src/policy.jl)
struct HIPNNPolicy{P,A} <: AbstractNNPolicy
    problem::P
    e::Engine
    qnetwork::Any            # the Flux model, refreshed on demand by getnetwork
    action_map::Vector{A}
    n_input_dims::Int64
end
function getnetwork(p::HIPNNPolicy)                    # Flux.params(active_q) <- engine (BSON save path keeps working, src/solver.jl:292)
    ps = Flux.params(p.qnetwork); n = sum(length, ps); flat = zeros(Float32, n)
    check(ccall((:dqn_get_params, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Csize_t), p.e.h, 0, flat, n))
    off = 0; for w in ps; copyto!(w, reshape(flat[off+1:off+length(w)], size(w))); off += length(w); end
    p.qnetwork
end
resetstate!(p::HIPNNPolicy) = check(ccall((:dqn_reset_state, LIB), Cint, (Ptr{Cvoid},), p.e.h))   # Flux.reset!: Recur state <- state0
# hiddenstates(m) / sethiddenstates!(m, hs) (src/helpers.jl:61-79) for the policy's Recur state, which lives in the engine: flat Float32 vector, per
# recurrent layer in chain order: an LSTM layer's h then c, a GRU or RNN layer's h.  The engine keeps it apart from the train step's sequences, so the save / restore the reference does around batch_train! (:137-139) is a no-op
# here; these exist for callers that checkpoint or transplant the state themselves.
function hiddenstates(p::HIPNNPolicy)
    n = sum(Int[(l.cell isa Flux.LSTMCell ? 2 : 1) * size(l.cell.Wh, 2) for l in filter(l -> l isa Flux.Recur, collect(p.qnetwork))])      # Wh: (4h, h) / (3h, h) / (h, h)
    hc = zeros(Float32, n)
    check(ccall((:dqn_get_hidden, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), p.e.h, hc, n))
    hc
end
sethiddenstates!(p::HIPNNPolicy, hc::Vector{Float32}) = check(ccall((:dqn_set_hidden, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), p.e.h, hc, length(hc)))
actionmap(p::HIPNNPolicy) = p.action_map
function _q(p::HIPNNPolicy, o)
    ndims(o) == p.n_input_dims || throw("NNPolicyError: was expecting an array with $(p.n_input_dims) dimensions, got $(ndims(o))")
    q = zeros(Float32, p.e.nA)
    check(ccall((:dqn_forward, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Cint, Ptr{Float32}), p.e.h, 0, policy_obs(p.e, o), 1, q))
    q
end
POMDPs.action(p::HIPNNPolicy, o::AbstractArray) = p.action_map[argmax(_q(p, o))]
POMDPTools.actionvalues(p::HIPNNPolicy, o::AbstractArray) = _q(p, o)
POMDPs.value(p::HIPNNPolicy, o::AbstractArray) = maximum(_q(p, o))
sync_target!(p::HIPNNPolicy) = check(ccall((:dqn_sync_target, LIB), Cint, (Ptr{Cvoid},), p.e.h))   # replaces Flux.loadparams! at src/solver.jl:142-145
function setnetwork!(p::HIPNNPolicy, weights)          # Flux.loadparams!(getnetwork(policy), weights) -> engine (restore_best_model, src/solver.jl:172-174,314-315)
    Flux.loadparams!(p.qnetwork, weights)
    flat = flatparams(p.qnetwork)
    check(ccall((:dqn_set_params, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Csize_t), p.e.h, 0, flat, length(flat)))
    p
end

# ---- solve / initialize_replay_buffer / dqn_train! routes (src/solver.jl:30-57, :180-189, :59-178): ZERO edits to the package.
# `solve(MI355XSolver(solver), mdp)` is the one-line change in user code; everything behind it dispatches on the HIP types.
struct MI355XSolver <: POMDPs.Solver
    solver::DeepQLearningSolver
    device::Int
    obs_u8::Bool
end
MI355XSolver(solver::DeepQLearningSolver; device = 0, obs_u8 = false) = MI355XSolver(solver, device, obs_u8)
POMDPs.solve(s::MI355XSolver, problem::MDP) = solve(s, MDPCommonRLEnv{AbstractArray{Float32}}(problem))       # :30-33
POMDPs.solve(s::MI355XSolver, problem::POMDP) = solve(s, POMDPCommonRLEnv{AbstractArray{Float32}}(problem))   # :35-38
function POMDPs.solve(s::MI355XSolver, env::AbstractEnv)                                                       # :40-57
    solver = s.solver
    action_map = collect(actions(env))
    action_indices = Dict(a => i for (i, a) in enumerate(action_map))
    DeepQLearning.isrecurrent(solver.qnetwork) && !solver.recurrence &&
        throw("DeepQLearningError: you passed in a recurrent model but recurrence is set to false")
    active_q = solver.dueling ? DeepQLearning.create_dueling_network(solver.qnetwork) : solver.qnetwork
    engine = Engine(solver, env, active_q; device = s.device, obs_u8 = s.obs_u8)
    replay = initialize_replay_buffer(solver, env, action_indices, engine)
    policy = HIPNNPolicy(env, engine, active_q, action_map, length(DeepQLearning.obs_dimensions(env)))
    dqn_train!(solver, env, policy, replay)
end
HIPNNPolicy(env::MDPCommonRLEnv, e::Engine, q, action_map::Vector, n::Int) = HIPNNPolicy(convert(MDP, env), e, q, action_map, n)       # src/policy.jl:24
HIPNNPolicy(env::POMDPCommonRLEnv, e::Engine, q, action_map::Vector, n::Int) = HIPNNPolicy(convert(POMDP, env), e, q, action_map, n)   # :25

function initialize_replay_buffer(solver::DeepQLearningSolver, env::AbstractEnv, action_indices, engine::Engine)   # :180-189
    replay = solver.recurrence ? HIPEpisodeReplayBuffer(engine, solver.rng) : HIPReplayBuffer(engine, solver.rng)
    populate_replay_buffer!(replay, env, action_indices, max_pop = solver.train_start)
    replay
end

# dqn_train! is dispatchable on the policy type (src/solver.jl:59).  The generic method would keep a Flux deepcopy as target network and
# refresh THAT every target_update_freq steps (:65, :142-145) -- the engine's own target net would never be synced -- so the HIP policy
# gets its own driver: same cadence (train / target / eval / save / log), same logged scalars, the optimizer, the target network and the
# hidden-state save/restore around batch_train! (:137-139: the engine keeps the policy's Recur state apart from the train step) inside the engine.
function dqn_train!(solver::DeepQLearningSolver, env::AbstractEnv, policy::HIPNNPolicy, replay)
    logger = nothing
    if solver.logdir !== nothing
        logger = TBLogger(solver.logdir); solver.logdir = logger.logdir
    end
    sync_target!(policy)                                   # target_q = deepcopy(active_q), :65
    resetstate!(policy); reset!(env); obs = observe(env)
    action_indices = Dict(a => i for (i, a) in enumerate(actionmap(policy)))
    ep_rewards = Float64[0.0]; ep_steps = Int64[]; step = 0
    best_eval = -Inf; scores_eval = -Inf; model_saved = false; eval_next = false; save_next = false
    loss_val = NaN32; grad_val = NaN32; ticket = UInt64(0)
    for t in 1:solver.max_steps
        act = action(solver.exploration_policy, policy, t, obs)
        rew = act!(env, act); op = observe(env); done = terminated(env)
        expe = DQExperience(obs, action_indices[act], Float32(rew), op, done)
        if solver.recurrence
            add_exp!(replay, expe)
        else
            add_exp!(replay, expe, solver.prioritized_replay ? abs(expe.r) : 0f0)     # :91-94
        end
        obs = op; step += 1; ep_rewards[end] += rew
        if done || step >= solver.max_episode_length
            if eval_next                                   # evaluation waits for the episode to end, :101-122
                scores_eval, steps_eval, info_eval = DeepQLearning.evaluation(solver.evaluation_policy, policy, env, solver.num_ep_eval,
                                                                              solver.max_episode_length, solver.verbose)
                eval_next = false
                if save_next                               # only right after an evaluation
                    model_saved, best_eval = DeepQLearning.save_model(solver, getnetwork(policy), scores_eval, best_eval, model_saved)   # qnetwork.bson, :290-300
                    save_next = false
                end
                if logger !== nothing
                    log_value(logger, "eval_reward", scores_eval, step = t); log_value(logger, "eval_steps", steps_eval, step = t)
                    for (k, v) in info_eval; log_value(logger, k, v, step = t); end
                end
            end
            reset!(env); obs = observe(env); resetstate!(policy)
            push!(ep_steps, step); push!(ep_rewards, 0.0); step = 0
        end
        if t % solver.train_freq == 0                                                            # ONE ccall, :136-140
            if replay isa HIPReplayBuffer
                ticket = batch_train_async!(replay)          # returns once enqueued: the env loop runs on while the GPU trains
            else
                loss_val, grad_val = batch_train!(solver, env, policy, nothing, nothing, replay)
            end
        end
        t % solver.target_update_freq == 0 && sync_target!(policy)                             # :142-145 inside the engine
        t % solver.eval_freq == 0 && (eval_next = true)
        t % solver.save_freq == 0 && (save_next = true)
        if t % solver.log_freq == 0 && logger !== nothing
            nt = POMDPTools.loginfo(solver.exploration_policy, t)
            for (k, v) in pairs(nt); log_value(logger, String(k), v, step = t); end
            avg100 = mean(ep_rewards[max(1, length(ep_rewards) - 101):end])
            ticket != 0 && ((loss_val, grad_val) = step_scalars(policy.e, ticket))      # (loss, grad_norm) of the newest train step: the values :154-167 print
            solver.verbose && @printf("%5d / %5d eps %0.3f |  avgR %1.3f | Loss %2.3e | Grad %2.3e | EvalR %1.3f \n",
                                      t, solver.max_steps, nt[1], avg100, loss_val, grad_val, scores_eval)
            log_value(logger, "avg_reward", avg100, step = t); log_value(logger, "loss", loss_val, step = t); log_value(logger, "grad_val", grad_val, step = t)
        end
    end
    if model_saved && solver.verbose                       # quirk kept: the best weights come back only if verbose, :170-176
        @printf("Restore model with eval reward %1.3f \n", best_eval)
        setnetwork!(policy, BSON.load(joinpath(solver.logdir, "qnetwork.bson"))[:qnetwork])
    else
        getnetwork(policy)                                 # leave the Flux model in step with the engine for the caller
    end
    policy
end

# ---- device-resident vectorised environments (dqn_env_spec / dqn_rollout_cfg / dqn_rollout_stats, include/dqn_mi355x.h)
# the env loop of dqn_train! (src/solver.jl:82-145) for n copies of a built-in MDP without observations crossing PCIe
struct EnvSpec
    kind::Int32; n_envs::Int32; max_episode_length::Int32; seed::UInt64
    o_stack::Int32; max_time::Int32; images::Ptr{UInt8}                       # TestMDP: UInt8[H*W, 3] (bad, normal, good)
    size_x::Int32; size_y::Int32; tprob::Float32; n_reward_cells::Int32
    reward_xy::NTuple{16,Int32}; reward_val::NTuple{8,Float32}                # SimpleGridWorld reward cells (x1,y1,x2,y2,...)
end
struct RolloutCfg
    train_freq::Int32; target_update_freq::Int32; eps_start::Float32; eps_stop::Float32; eps_steps::Float32; cadence_env_steps::Int32; t0::Int64
end
mutable struct RolloutStats
    episodes::Int64; reward_sum::Float64; train_steps::Int64; last_loss::Float32; last_grad_norm::Float32
    RolloutStats() = new(0, 0.0, 0, 0f0, 0f0)
end
function envs_create_gridworld!(e::Engine, mdp; n_envs, max_episode_length = 100, seed = 0)      # mdp::POMDPModels.SimpleGridWorld
    cells = collect(mdp.rewards); xy = zeros(Int32, 16); rv = zeros(Float32, 8)
    for (k, (pos, r)) in enumerate(cells); xy[2k-1] = pos[1]; xy[2k] = pos[2]; rv[k] = r; end
    spec = EnvSpec(1, n_envs, max_episode_length, seed, 0, 0, C_NULL, mdp.size[1], mdp.size[2], mdp.tprob, length(cells), Tuple(xy), Tuple(rv))
    check(ccall((:dqn_envs_create, LIB), Cint, (Ptr{Cvoid}, Ref{EnvSpec}), e.h, spec))
end
function envs_create_testmdp!(e::Engine, images::Matrix{UInt8}, o_stack, max_time; n_envs, max_episode_length = 100, seed = 0)
    GC.@preserve images begin
        spec = EnvSpec(0, n_envs, max_episode_length, seed, o_stack, max_time, pointer(images), 0, 0, 0f0, 0, ntuple(_ -> Int32(0), 16), ntuple(_ -> 0f0, 8))
        check(ccall((:dqn_envs_create, LIB), Cint, (Ptr{Cvoid}, Ref{EnvSpec}), e.h, spec))
    end
end
# ---- tabular environments (dqn_tabular_env): any discrete POMDPs.jl problem as its matrices, so that it runs on the device loop.  Julia arrays are column-major:
# an array indexed [sp, a, s] IS the header's row-major [S][A][S]
struct TabularEnv
    n_envs::Int32; max_episode_length::Int32; seed::UInt64
    n_states::Int32; n_obs::Int32
    T::Ptr{Float32}; Z::Ptr{Float32}; Z0::Ptr{Float32}; R::Ptr{Float32}; terminal::Ptr{UInt8}; b0::Ptr{Float32}; features::Ptr{Float32}
end
function tabulate(problem::Union{MDP,POMDP})
    ss = ordered_states(problem); as = ordered_actions(problem); S = length(ss); A = length(as)
    ispomdp = problem isa POMDP
    os = ispomdp ? ordered_observations(problem) : ss; O = ispomdp ? length(os) : 0
    T = zeros(Float32, S, A, S); R = zeros(Float32, S, A, S); term = zeros(UInt8, S); b0 = zeros(Float32, S)
    Z = zeros(Float32, max(O, 1), S, A); Z0 = zeros(Float32, max(O, 1), S)
    for (si, s) in enumerate(ss)
        term[si] = isterminal(problem, s) ? 1 : 0
        b0[si] = pdf(initialstate(problem), s)
        for (ai, a) in enumerate(as)
            term[si] == 1 && continue                     # rows of terminal states are exempt from the row-sum check
            d = transition(problem, s, a)
            for (spi, sp) in enumerate(ss)
                T[spi, ai, si] = pdf(d, sp)
                R[spi, ai, si] = reward(problem, s, a, sp)
            end
        end
    end
    if ispomdp
        for (ai, a) in enumerate(as), (spi, sp) in enumerate(ss), (oi, o) in enumerate(os)
            Z[oi, spi, ai] = pdf(observation(problem, a, sp), o)
        end
        # the observation after a reset: POMDPCommonRLEnv draws it from initialobs where the model defines one.  tabulate does not ask for initialobs: it APPROXIMATES
        # Z0[s] by the first ordered action's observation model (exact for TigerPOMDP, whose first action is listen; DESIGN 6.2.2)
        for (si, s) in enumerate(ss), (oi, o) in enumerate(os)
            Z0[oi, si] = Z[oi, si, 1]
        end
    end
    feat = ispomdp ? reduce(hcat, [vec(convert_o(Vector{Float32}, o, problem)) for o in os]) : reduce(hcat, [vec(convert_s(Vector{Float32}, s, problem)) for s in ss])
    (T = T, Z = Z, Z0 = Z0, R = R, terminal = term, b0 = b0, features = Matrix{Float32}(feat), n_states = S, n_obs = O)
end
function envs_create_tabular!(e::Engine, problem::Union{MDP,POMDP}; n_envs, max_episode_length = 100, seed = 0)
    t = tabulate(problem)
    GC.@preserve t begin
        pz = t.n_obs > 0 ? pointer(t.Z) : Ptr{Float32}(C_NULL); pz0 = t.n_obs > 0 ? pointer(t.Z0) : Ptr{Float32}(C_NULL)
        spec = TabularEnv(n_envs, max_episode_length, seed, t.n_states, t.n_obs, pointer(t.T), pz, pz0, pointer(t.R), pointer(t.terminal), pointer(t.b0), pointer(t.features))
        check(ccall((:dqn_envs_create_tabular, LIB), Cint, (Ptr{Cvoid}, Ref{TabularEnv}), e.h, spec))
    end
end
# ---- continuous-state control problems (dqn_control_env): POMDPModels' MountainCar and InvertedPendulum on the device loop.  Fields the problem carries itself
# (MountainCar: cost, jackpot; InvertedPendulum: g, m, l, M, alpha, dt, cost) come from it, the rest are the header's defaults (recalled from POMDPModels 0.4)
struct ControlEnv
    kind::Int32; n_envs::Int32; max_episode_length::Int32; seed::UInt64
    force::Float64; freq::Float64; gravity::Float64; v_max::Float64; x_min::Float64; goal::Float64; cost::Float64; jackpot::Float64; x0::Float64; v0::Float64
    g::Float64; m::Float64; l::Float64; M::Float64; alpha::Float64; dt::Float64; u_max::Float64; noise::Float64; theta_max::Float64; init_half::Float64
end
const ENV_MOUNTAINCAR = Int32(3)
const ENV_PENDULUM = Int32(4)
control_spec(mdp::POMDPModels.MountainCar, n_envs, max_episode_length, seed) =
    ControlEnv(ENV_MOUNTAINCAR, n_envs, max_episode_length, seed, 0.001, 3.0, 0.0025, 0.07, -1.2, 0.5, mdp.cost, mdp.jackpot, -0.5, 0.0,
               9.81, 2.0, 8.0, 8.0, 1 / (2.0 + 8.0), 0.1, 50.0, 20.0, pi / 2, 0.1)
control_spec(mdp::POMDPModels.InvertedPendulum, n_envs, max_episode_length, seed) =
    ControlEnv(ENV_PENDULUM, n_envs, max_episode_length, seed, 0.001, 3.0, 0.0025, 0.07, -1.2, 0.5, mdp.cost, 100.0, -0.5, 0.0,
               mdp.g, mdp.m, mdp.l, mdp.M, mdp.alpha, mdp.dt, 50.0, 20.0, pi / 2, 0.1)
function envs_create_control!(e::Engine, mdp::Union{POMDPModels.MountainCar,POMDPModels.InvertedPendulum}; n_envs, max_episode_length = 100, seed = 0)
    check(ccall((:dqn_envs_create_control, LIB), Cint, (Ptr{Cvoid}, Ref{ControlEnv}), e.h, control_spec(mdp, n_envs, max_episode_length, seed)))
end
# inspection: the Float64 states (2 x n_envs) of the control copies as they stand, and the states they held before their last step
function envs_peek_state(e::Engine, n_envs)
    s = zeros(Float64, 2, n_envs); p = zeros(Float64, 2, n_envs)
    check(ccall((:dqn_envs_peek_state, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), e.h, s, p))
    s, p
end
function evaluate(e::Engine, n_eval, max_episode_length; seed = 0)                   # basic_evaluation (src/evaluation_policy.jl:17-42) on the device
    r = Ref{Float64}(0); st = Ref{Float64}(0)
    check(ccall((:dqn_evaluate, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, UInt64, Ref{Float64}, Ref{Float64}), e.h, n_eval, max_episode_length, seed, r, st))
    r[], st[]
end
# inspection: the Q columns (n_actions x n_envs) and the greedy actions (1-based) of the last vector step's acting forward; read-only, nothing is launched.  Throws before
# the set's first vector step and after another forward used the policy workspace (a host-side action / value call, evaluate)
function envs_peek_q(e::Engine, n_envs)
    q = zeros(Float32, e.nA, n_envs); a = zeros(Int32, n_envs)
    check(ccall((:dqn_envs_peek_q, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int32}), e.h, q, a))
    q, a .+ Int32(1)
end
# ---- exploration on the device loop (dqn_exploration / dqn_rollout_explore): POMDPTools' EpsGreedyPolicy and SoftmaxPolicy with any schedule.  The schedule is
# evaluated HERE, per vector step, and rounded to Float32; the device only reads the table.  A LinearDecaySchedule (or a constant eps) stays on dqn_rollout's own fp32
# law, so existing trajectories do not move
struct Exploration
    kind::Int32; n_values::Int32; values::Ptr{Float32}
end
const EXPLORE_EPS_GREEDY = Int32(0)
const EXPLORE_SOFTMAX = Int32(1)
# (kind, values) for vector steps t0 .. t0 + n - 1, or `nothing` where dqn_rollout's linear law serves the policy
exploration_table(p::POMDPTools.SoftmaxPolicy, t0, n) = (EXPLORE_SOFTMAX, Float32[p.temperature(t) for t in t0:t0+n-1])
function exploration_table(p::POMDPTools.EpsGreedyPolicy, t0, n)
    p.eps isa POMDPTools.LinearDecaySchedule && return nothing
    (EXPLORE_EPS_GREEDY, Float32[p.eps(t) for t in t0:t0+n-1])
end
linear_eps(p::POMDPTools.EpsGreedyPolicy) = p.eps isa POMDPTools.LinearDecaySchedule ? (Float32(p.eps.start), Float32(p.eps.stop), Float32(p.eps.steps)) : (1f0, 0.01f0, 5000f0)
linear_eps(p) = (1f0, 0.01f0, 5000f0)
# env_step_cadence = true: train_freq / target_update_freq count ENV steps as dqn_train! does (src/solver.jl:136-145) -- n / train_freq train steps per vector step
# explore = an exploration policy: its eps / temperature schedule drives the call (eps is then ignored unless the policy's schedule is a LinearDecaySchedule)
function rollout!(e::Engine, n_steps; t0 = 1, train_freq = 4, target_update_freq = 500, eps = (1f0, 0.01f0, 5000f0), env_step_cadence = false, explore = nothing)
    st = RolloutStats()
    tab = explore === nothing ? nothing : exploration_table(explore, t0, n_steps)
    explore === nothing || tab !== nothing || (eps = linear_eps(explore))
    cfg = RolloutCfg(train_freq, target_update_freq, eps[1], eps[2], eps[3], env_step_cadence ? 1 : 0, t0)
    if tab === nothing
        check(ccall((:dqn_rollout, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{RolloutCfg}, Ref{RolloutStats}), e.h, n_steps, cfg, st))
    else
        kind, vals = tab
        GC.@preserve vals begin
            x = Exploration(kind, length(vals), pointer(vals))
            check(ccall((:dqn_rollout_explore, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{RolloutCfg}, Ref{Exploration}, Ref{RolloutStats}), e.h, n_steps, cfg, x, st))
        end
    end
    st
end
# ---- grouped acting (dqn_rollout_many): n_steps vector steps of EVERY member's device loop, one launch of K workgroups per vector step, the group train step and the
# target syncs inside the call.  eps: one (start, stop, steps) for all members or a vector of K; explore: nothing, or a vector of K exploration policies (an entry
# `nothing`: that member's linear law).  Returns K records; member k ends bit for bit where rollout!(g.members[k], ...) would have left it
struct RolloutStatsRec      # the isbits form of RolloutStats: an array of K of them is what the call fills
    episodes::Int64; reward_sum::Float64; train_steps::Int64; last_loss::Float32; last_grad_norm::Float32
end
function rollout!(g::EngineGroup, n_steps; t0 = 1, train_freq = 4, target_update_freq = 500, eps = (1f0, 0.01f0, 5000f0), explore = nothing)
    K = length(g.members)
    epsk = eps isa AbstractVector ? collect(eps) : fill(eps, K)
    pols = explore === nothing ? fill(nothing, K) : collect(explore)
    tabs = Any[p === nothing ? nothing : exploration_table(p, t0, n_steps) for p in pols]
    cfgs = Vector{RolloutCfg}(undef, K); xs = Vector{Exploration}(undef, K); ptrs = fill(Ptr{Exploration}(C_NULL), K)
    vals = Vector{Vector{Float32}}(undef, K)
    for k in 1:K
        e3 = (pols[k] === nothing || tabs[k] !== nothing) ? epsk[k] : linear_eps(pols[k])
        cfgs[k] = RolloutCfg(train_freq, target_update_freq, e3[1], e3[2], e3[3], 0, t0)
        vals[k] = tabs[k] === nothing ? Float32[] : tabs[k][2]
    end
    st = Vector{RolloutStatsRec}(undef, K)
    GC.@preserve vals xs ptrs begin
        for k in 1:K
            tabs[k] === nothing && continue
            xs[k] = Exploration(tabs[k][1], length(vals[k]), pointer(vals[k]))
            ptrs[k] = pointer(xs, k)
        end
        check(ccall((:dqn_rollout_many, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{RolloutCfg}, Ptr{Ptr{Exploration}}, Ptr{RolloutStatsRec}),
                    g.h, n_steps, cfgs, explore === nothing ? Ptr{Ptr{Exploration}}(C_NULL) : pointer(ptrs), st))
    end
    st
end
function rollout_info(g::EngineGroup)      # (launches per vector step, dynamic LDS bytes of the acting launch); throws with the member and the reason where one is declined
    n = Ref{Cint}(0); lds = Ref{Cuint}(0)
    check(ccall((:dqn_rollout_many_info, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cuint}), g.h, n, lds))
    Int(n[]), Int(lds[])
end
# ---- grouped evaluation (dqn_evaluate_many): basic_evaluation of EVERY member, n_eval greedy episodes each, the whole episode loop inside the kernel.  seeds: one per
# member.  Returns K (avg_reward, avg_steps) pairs; member k's is bit for bit what evaluate(g.members[k], n_eval, max_episode_length; seed = seeds[k]) returns
function evaluate(g::EngineGroup, n_eval, max_episode_length; seeds)
    K = length(g.members)
    length(seeds) == K || error("evaluate: $(length(seeds)) seeds were given for $K members (one per member)")
    sd = UInt64[UInt64(s) for s in seeds]; r = Vector{Float64}(undef, K); st = Vector{Float64}(undef, K)
    check(ccall((:dqn_evaluate_many, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt64}, Ptr{Float64}, Ptr{Float64}), g.h, n_eval, max_episode_length, sd, r, st))
    [(r[k], st[k]) for k in 1:K]
end
function evaluate_info(g::EngineGroup, n_eval, max_episode_length)      # (launches per call, vector steps per launch at most, dynamic LDS bytes); throws with the member and the reason where one is declined
    n = Ref{Cint}(0); b = Ref{Cint}(0); lds = Ref{Cuint}(0)
    check(ccall((:dqn_evaluate_many_info, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{Cint}, Ref{Cint}, Ref{Cuint}), g.h, n_eval, max_episode_length, n, b, lds))
    Int(n[]), Int(b[]), Int(lds[])
end

end # module
