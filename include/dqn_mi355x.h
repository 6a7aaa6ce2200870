/*
 * dqn_mi355x.h -- C ABI of libdqn_mi355x.so, the MI355X-native (gfx950) engine for
 * the DeepQLearning.jl hot path: PrioritizedReplayBuffer + batch_train!.
 *
 * The reference (JuliaPOMDP/DeepQLearning.jl v0.7.1) has NO FFI: its extension
 * mechanism is Julia multiple dispatch.  Each entry point below replaces one
 * dispatch seam of the reference; the `ccall` stubs a maintainer adds are in
 * INTEGRATION.md and deepqlearning.jl_amd/julia/DeepQLearningMI355X.jl.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error; dqn_last_error() gives the
 *    message (thread-local).  Reference errors are thrown Strings
 *    ("DeepQLearningError: ...", src/solver.jl:46, src/dueling.jl:47) and @assert
 *    (src/prioritized_experience_replay.jl:66,78,83-84,90); the shim re-throws.
 *  - host arrays are taken AS JULIA LAYS THEM OUT (column-major, batch last):
 *      obs (W,H,C)  == C float[C][H][W];    batch (W,H,C,B) == float[B][C][H][W]
 *      Dense weight (out,in) == float[in][out];  Conv weight (kw,kh,cin,cout) ==
 *      float[cout][cin][kh][kw], UN-flipped (the engine applies NNlib's true
 *      convolution itself);  Q-values (nA,B) == float[B][nA].
 *  - flat parameter vectors are in Flux.params order: base, val, adv streams
 *    (src/dueling.jl:2-6,13), per layer weight then bias.
 *  - action indices are 0-BASED at the ABI (the Julia shim subtracts 1 from the
 *    reference's 1-based index, src/solver.jl:84).
 *  - the caller owns every host pointer and may free it when the call returns.
 *  - an engine is NOT thread-safe (the reference is strictly sequential); distinct
 *    engines (one per GPU) are independent.
 *  - no torch / HIP types appear in any signature.
 */
#ifndef DQN_MI355X_H
#define DQN_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden: only these entry points are exported */
#endif

typedef struct dqn_engine dqn_engine_t;

enum { DQN_LAYER_DENSE = 0, DQN_LAYER_CONV = 1, DQN_LAYER_LSTM = 2, DQN_LAYER_GRU = 3, DQN_LAYER_RNN = 4, DQN_LAYER_MAXPOOL = 5, DQN_LAYER_MEANPOOL = 6, DQN_LAYER_LAYERNORM = 7, DQN_LAYER_DROPOUT = 8, DQN_LAYER_SKIPADD = 9, DQN_LAYER_SKIPADD_MAP = 10, DQN_LAYER_GROUPNORM = 11, DQN_LAYER_ADAPTIVEMAXPOOL = 12, DQN_LAYER_ADAPTIVEMEANPOOL = 13, DQN_LAYER_ACTIVATION = 14, DQN_LAYER_CONV_DG = 15 };
/* Activations of Dense, Conv and LayerNorm layers (NNlib's DEFAULT parameters only: leakyrelu a = 0.01, elu alpha = 1).  x: the fp32 pre-activation, y: the stored fp32
 * output.  The engine keeps only y and differentiates from it, as NNlib's own rules do (deriv_elu(y), deriv_selu(y), (1 - abs(y))^2, ...).  The forwards with a
 * transcendental or a division go through Float64 and round once.  L = 1.0507009873554805, A = 1.6732632423543772, LA = L * A = 1.7580993408473766.
 *   code          forward                                                        dx from (dy, y), fp32
 *   IDENTITY   0  x                                                              dy
 *   RELU       1  x > 0 ? x : 0                                                  y > 0 ? dy : 0
 *   TANH       2  (float)tanh((double)x)                                         dy * (1 - y * y)
 *   SIGMOID    3  (float)(1 / (1 + exp(-(double)x)))                             dy * (y * (1 - y))
 *   LEAKYRELU  4  x > 0 ? x : 0.01f * x                                          y > 0 ? dy : 0.01f * dy
 *   ELU        5  x >= 0 ? x : (float)expm1((double)x)                           y >= 0 ? dy : dy * (y + 1)
 *   SELU       6  (float)(L * (x > 0 ? x : A * expm1((double)x)))                y > 0 ? (float)L * dy : dy * (y + (float)LA)
 *   SOFTPLUS   7  (float)(log1p(exp(-fabs((double)x))) + max((double)x, 0))      dy * (float)(-expm1(-(double)y))        (sigmoid(x) = 1 - exp(-y))
 *   SOFTSIGN   8  (float)((double)x / (1 + fabs((double)x)))                     dy * ((1 - |y|) * (1 - |y|))
 *   RELU6      9  min(max(x, 0), 6)                                              (y > 0 && y < 6) ? dy : 0
 *   HARDTANH  10  max(-1, min(1, x))                                             (y > -1 && y < 1) ? dy : 0
 * A Dense, Conv or LayerNorm layer takes any of the eleven; any other code is refused at dqn_plan_default / dqn_engine_create by layer index and code.  An RNN layer's
 * cell activation stays one of the first four (IDENTITY .. SIGMOID): the cell states its arithmetic on its own.  gelu, swish, mish and hardswish are not monotone: their
 * derivative needs the pre-activation, which the engine does not keep; parametrised forms (leakyrelu(x, 0.2), elu(x, 2)) have no code.  NNlib's definitions are recalled,
 * not executed: elu's x >= 0, selu's x > 0 and leakyrelu's derivative taken at x > 0 are what only a maintainer with Julia can pin. */
enum { DQN_ACT_IDENTITY = 0, DQN_ACT_RELU = 1, DQN_ACT_TANH = 2, DQN_ACT_SIGMOID = 3, DQN_ACT_LEAKYRELU = 4, DQN_ACT_ELU = 5, DQN_ACT_SELU = 6, DQN_ACT_SOFTPLUS = 7,
       DQN_ACT_SOFTSIGN = 8, DQN_ACT_RELU6 = 9, DQN_ACT_HARDTANH = 10 };
#define DQN_ACT_LAST DQN_ACT_HARDTANH
/* Four more codes, valid on DQN_LAYER_ACTIVATION ONLY (every other kind keeps refusing codes above DQN_ACT_LAST): the standalone activation layer's input is the stored
 * output of the layer in front, so x is there and the derivative is taken from it.  Float64, rounded once; the backward is ONE fp32 multiply dy * (float)sigma'(x).
 *   code          forward                                                                    sigma'(x), Float64
 *   GELU      11  0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))   (NNlib's tanh form)         0.5 (1 + t) + 0.5 x (1 - t^2) sqrt(2/pi) (1 + 3 * 0.044715 x^2)
 *   SWISH     12  x s,  s = 1 / (1 + exp(-x))                                                  s (1 + x (1 - s))
 *   MISH      13  x t,  t = tanh(softplus(x))  (softplus as code 7)                             t + x (1 - t^2) s
 *   HARDSWISH 14  x clamp((x + 3) / 6, 0, 1)                                                   x < -3 ? 0 : x > 3 ? 1 : (2x + 3) / 6
 * On that layer the eleven codes above run the table's forward on the stored input and the table's derivative from the layer's own output: Dense(n, m) -> Activation(sigma)
 * trains with the bits of Dense(n, m, sigma).  Which value the kinks take is NNlib's rule and unpinned. */
enum { DQN_ACT_GELU = 11, DQN_ACT_SWISH = 12, DQN_ACT_MISH = 13, DQN_ACT_HARDSWISH = 14 };
#define DQN_ACT_LAYER_LAST DQN_ACT_HARDSWISH
enum { DQN_STREAM_BASE = 0, DQN_STREAM_VAL = 1, DQN_STREAM_ADV = 2 };
enum { DQN_OBS_F32 = 0, DQN_OBS_U8 = 1 }; /* u8: stored byte, consumed as (float)byte/255f0 (test/test_env.jl:59) */
enum { DQN_NET_ONLINE = 0, DQN_NET_TARGET = 1 };

/* One layer of solver.qnetwork (a Flux.Chain of Conv / Dense, src/solver.jl:2,
 * README.md:64-70) AFTER create_dueling_network (src/dueling.jl:36-58) has split
 * it: the shim passes base layers, then val layers, then adv layers.
 * flattenbatch (src/helpers.jl:6-8) is implicit between a Conv and a Dense. */
typedef struct {
    int32_t kind;   /* DQN_LAYER_* */
    int32_t act;    /* DQN_ACT_* (Dense, Conv, LayerNorm: any of the eleven); for an RNN layer the cell's activation, one of the first four */
    int32_t stream; /* DQN_STREAM_*; all BASE when dueling == 0 */
    int32_t n_in, n_out;               /* Dense(in,out); LSTM(in,out) = Flux Recur(LSTMCell): params Wi (4out,in), Wh (4out,out), b (4out), state0 h0, c0;
                                          GRU(in,out) = Flux Recur(GRUCell): params Wi (3out,in), Wh (3out,out), b (3out), state0 h0;
                                          RNN(in,out,act) = Flux Recur(RNNCell): params Wi (out,in), Wh (out,out), b (out), state0 h0 (out,1),
                                          in C order Wi[in][out], Wh[out][out], b, h0; act carries the cell's activation (default tanh) */
    int32_t cin, cout, kh, kw, sh, sw; /* Conv((kh,kw), cin=>cout; stride=(sh,sw), pad=(pad_h,pad_w)): for DQN_LAYER_CONV the slots n_in / n_out carry pad_h / pad_w,
                                          symmetric zero padding per axis, 0 <= pad_h <= kh - 1, 0 <= pad_w <= kw - 1 (0, 0 = no padding); output map
                                          (H + 2 pad_h - kh) / sh + 1 by (W + 2 pad_w - kw) / sw + 1; a padded Conv is base chain only and single GPU only;
                                          CONV_DG (kind 15): Conv((kh,kw), cin=>cout, act; stride, pad, dilation=(dh,dw), groups=g) and DepthwiseConv (g = cin) -- Flux 0.14, recalled, not
                                          executed.  cin, cout = the FULL channel counts, kh, kw, sh, sw as for Conv.  The five small integers ride packed: n_in = pad_h | pad_w << 16
                                          (each 0..65535), n_out = dh | dw << 8 | g << 16 (dh, dw 1..255, g 1..32767); a negative slot or a field outside its range is refused.  g divides
                                          cin and cout; output channels [j cout/g, (j+1) cout/g) read input channels [j cin/g, (j+1) cin/g).  Tap (ky, kx) of output (oy, ox) reads
                                          iy = oy sh + ky dh - pad_h, ix = ox sw + kx dw - pad_w; 0 <= pad_h <= (kh-1) dh, likewise w; output map (H + 2 pad_h - (kh-1) dh - 1) / sh + 1 by
                                          (W + 2 pad_w - (kw-1) dw - 1) / sw + 1.  Parameters: weight (cout, cin/g, kh, kw) (Julia (kw, kh, cin/g, cout)), bias (cout).  The plan entry
                                          means what a Conv's means, on K = (cin/g) kh kw and N = cout.  Base chain only (first layer included), never inside a skip block, single GPU
                                          only.  dh = dw = g = 1 is valid here and gives the bits of DQN_LAYER_CONV; the shim and the Python mirror lower such a Conv to DQN_LAYER_CONV;
                                          MaxPool((kh,kw); stride=(sh,sw)) / MeanPool(...), pad 0: cin == cout == channels of the incoming map (or both 0: the engine fills them in), act = IDENTITY,
                                          no parameters (Flux.params skips the layer); base chain only, first or behind a Conv / pool; its plan entry is ignored;
                                          AdaptiveMaxPool((ow, oh)) / AdaptiveMeanPool(...) (kinds 12 / 13; Flux 0.14 over NNlib, recalled, not executed) and GlobalMaxPool() / GlobalMeanPool()
                                          (the same kinds with output (1, 1)): kh, kw = the OUTPUT size (oh, ow), 1 <= oh <= h, 1 <= ow <= w of the incoming (c, h, w) map; sh = sw = 0,
                                          n_in = n_out = 0, cin == cout == channels (or both 0), act = IDENTITY, stream = BASE; its plan entry is all zeros and ignored.  The engine
                                          resolves the window per axis by FLUX's rule, stride = in / out (integer division), k = in - (out - 1) * stride, pad 0 -- NOT torch's adaptive
                                          windows (5 -> 3: Flux [0..2] [1..3] [2..4], torch [0,2) [1,4) [3,5)) -- and the layer is then MaxPool / MeanPool with that geometry in every
                                          respect (placement, tie rule, divisor f32(kh * kw), backward, single GPU only).  Output (1, 1) -- the window is the whole map, the
                                          (1, 1, c, batch) output of the Global layers -- runs the whole-map reduction kernels (pool_global.hip); every other output runs the pool kernels;
                                          LayerNorm(n, act; affine = true, eps) (Flux 0.14 `normalise`, recalled, not executed): n_in == n_out == n >= 2 == the incoming feature count, act = the
                                          layer's activation, stream = BASE, cin = the fp32 BIT PATTERN of eps (0 = the default 1f-5; finite and > 0), every other slot 0.  Per batch column
                                          mu = mean(x), sigma = sqrt(mean((x - mu)^2)), y = act(scale * (x - mu) / (sigma + eps) + bias): eps is added to sigma OUTSIDE the root (not torch's
                                          sqrt(var + eps)).  Parameters in Flux.params order: scale (n), bias (n).  Directly behind a Dense or recurrent layer (or the Dropout layer that follows one), base chain only, never the
                                          output layer, single GPU only; its plan entry is ignored.  A column with sigma = 0 has a finite forward (x_hat = 0); its backward is undefined;
                                          GroupNorm(chs, G, act; affine = true, track_stats = false, eps) (Flux 0.14 `_norm_layer_forward`, recalled, not executed) on the incoming
                                          (c, h, w) map: cin == cout == chs == c (or both 0: the engine fills them in), kh = G >= 1 with c % G == 0 and (c / G) * h * w >= 2, kw = the fp32
                                          BIT PATTERN of eps (0 = the default 1f-5; finite and > 0), n_in == n_out == c * h * w (or both 0), act = the layer's activation (any of the eleven),
                                          stream = BASE, sh = sw = 0.  Per batch column and group of c / G contiguous channels: mu = mean(x), var = mean((x - mu)^2),
                                          y = act(gamma_ch * (x - mu) / sqrt(var + eps) + beta_ch): eps INSIDE the root (torch's law, not LayerNorm's).  Parameters in Flux.params order:
                                          beta (c, zeros), gamma (c, ones) -- bias FIRST.  Directly behind a Conv, a MaxPool / MeanPool, a convolutional skip block or another GroupNorm; base
                                          chain only, never the first or the output layer, not inside a skip block, single GPU only; its plan entry is all zeros and ignored;
                                          Activation (kind 14; Julia's Base.Broadcast.BroadcastFunction(sigma) in a Chain, recalled, not executed): y = sigma(x) per element on the incoming
                                          feature vector or (c, h, w) map, whose shape and kind of shape it keeps.  act = any of the fifteen codes 0..14, stream = BASE, n_in == n_out == the
                                          incoming feature count (or both 0: the engine fills them in), every other slot 0.  No parameters (Flux.params skips the layer); its plan entry is
                                          all zeros and ignored.  Base chain only, never the first or the output layer (the last base layer of a dueling network is fine), not inside a skip
                                          block, single GPU only; a LayerNorm or Dropout may not directly follow it;
                                          Dropout(p), dims = : (Flux 0.14 automatic mode, recalled, not executed): n_in == n_out == the incoming feature count (or both 0: the engine fills them
                                          in), act = IDENTITY, stream = BASE, p as its Float64 BIT PATTERN, low word in cin, high word in cout (finite, 0 <= p < 1), every other slot 0.
                                          No parameters (Flux.params skips the layer); its plan entry is all zeros and ignored.  ACTIVE only in the online network's pass on the s columns
                                          of a train step (the forward Flux.gradient differentiates): y = keep ? x * Float32(1 / (1 - p)) : +0, dX = keep ? dY * scale : +0 with the same
                                          mask regenerated; the IDENTITY, at no cost, in every other pass (online on s', target, dqn_forward, dqn_greedy_action, the device loops,
                                          dqn_evaluate).  The mask is the engine's own law (Julia's RNG is not matched): Philox4x32-10 keyed by hparams.seed on the counter
                                          {k lo, k hi, q, 0x44520000 | layer index}, k = train steps completed before this one, q = f * ceil(C / 4) + col / 4 over the C active columns
                                          (col = t * B + b in a recurrent step), the four output words for columns 4 (col / 4) + 0..3, u = (word >> 8) * 2^-24, keep <=> (double)u >= p.
                                          Directly behind a Dense, recurrent or LayerNorm layer (a LayerNorm may follow it), base chain only, never the first or the output layer,
                                          single GPU only;
                                          SKIPADD, the join of a SkipConnection(layers, +) block (Flux 0.14, recalled, not executed): layers(x) .+ x.  ONE descriptor placed directly
                                          AFTER the descriptors of the block's inner layers: cin = m >= 1, the number of inner layers (the m descriptors immediately before it, same
                                          stream); n_in == n_out == the feature count n (or both 0: the engine fills them in), act = IDENTITY, stream = BASE, every other slot 0.
                                          No parameters (Flux.params yields the inner layers' in order); its plan entry is all zeros and ignored.  In EVERY pass
                                          y = y_K + y_P, one fp32 add per element: y_K the stored output of the last inner layer K (after K's activation), y_P the stored output of
                                          the producer P that the first inner layer F reads (after P's; a Dropout's masked output in its active pass, its producer's elsewhere).
                                          Backward: dact[K] = dY .* act_K'(y_K); F's input gradient dF is taken raw and dact[P] = (dF + dY) .* act_P'(y_P) -- P's derivative once,
                                          after the sum.  The inner layers are Dense, LayerNorm and Dropout layers (no recurrent layer, Conv, pool or nested block) and map n -> n;
                                          P is a Dense, recurrent, LayerNorm or Dropout layer or the join of a preceding block: never the observation (the block is never the first
                                          layer), never a Conv / pool map (a convolutional residual block is the next kind, SKIPADD_MAP; under this kind it is refused); the block is never the output layer.  LayerNorm and
                                          Dropout may be the first inner layer and may directly follow a join.  Base chain only, single GPU only;
                                          SKIPADD_MAP, the join of a CONVOLUTIONAL SkipConnection(layers, +) block, x + Conv(Conv(x)) on a (c, h, w) map: the descriptor has the shape
                                          of SKIPADD's -- ONE descriptor directly after the m inner descriptors, cin = m >= 1, n_in == n_out == c * h * w (or both 0), act = IDENTITY,
                                          stream = BASE, every other slot 0, an all-zero plan entry -- and the law is SKIPADD's, element for element of the map X[(ci, iy, ix)][column].
                                          The inner layers are Convs with pad != 0 on at least one axis (no pad-0 Conv, pool, Dense, LayerNorm, Dropout, recurrent layer or nested
                                          block) and map (c, h, w) -> (c, h, w); P is a Conv (padded or not, any activation), a MaxPool / MeanPool or the join of a preceding
                                          SKIPADD_MAP block: never the observation, never a feature vector, never a SKIPADD join.  The join's output is a (c, h, w) map for whatever
                                          follows (a Conv, a pool, another block, or a Dense / recurrent layer on c * h * w features).  Where K has no activation the add runs in the
                                          epilogue of K's forward launch, and the + dY of the entry in the epilogue of F's input-gradient launch (conv_own.hip): the same bits as the
                                          separate launches.  Base chain only, never the output layer, single GPU only */
} dqn_layer_desc;

/* Summation-order plan of one layer: the K dimension of each contraction is cut
 * into chunks of `*_kc` elements; inside a chunk products are accumulated as ONE
 * k-ascending fp32 fma chain starting at +0 (== gfx950 fp32 MFMA numerics), and
 * chunk sums are added in ascending chunk order.  0 = no split.  The plan only
 * fixes rounding order; DESIGN.md section 4 states it. */
typedef struct {
    int32_t fwd_kc; /* forward:  K = n_in            | cin*kh*kw           */
    int32_t dx_kc;  /* dX:       K = n_out           | conv: RAW kernel taps (ky*kw + kx ascending) per chunk; each chunk chains its VALID taps, co innermost */
    int32_t dw_kc;  /* dW, db:   K = batch           | out_positions*batch (position-major, sample-minor); conv: a multiple of batch_size, or -- when batch_size % 32 == 0 -- of 32 */
} dqn_layer_plan;

/* DeepQLearningSolver fields that reach the hot path (src/solver.jl:1-28) plus the
 * PrioritizedReplayBuffer constructor defaults (src/prioritized_experience_replay.jl:39-45;
 * NB the reference never forwards the solver's alpha/beta/epsilon, src/solver.jl:185). */
typedef struct {
    int32_t batch_size;        /* solver.batch_size (32) */
    int32_t n_actions;         /* length(actions(env)) */
    int32_t obs_c, obs_h, obs_w; /* obs as float[C][H][W]; vector obs of length n: (n,1,1) */
    int32_t obs_dtype;         /* DQN_OBS_* replay storage type */
    float   learning_rate;     /* solver.learning_rate (1f-4) -> Adam eta */
    double  adam_beta1, adam_beta2, adam_eps; /* Flux Adam defaults 0.9, 0.999, 1e-8 */
    int32_t adam_f64_scalars;  /* 1: Flux 0.14 semantics (Float64 eta/beta/eps, evaluate in f64, round on store) */
    float   gamma;             /* discount (src/solver.jl:208, helpers.jl:83-85) */
    int32_t double_q;          /* solver.double_q */
    int32_t dueling;           /* solver.dueling */
    int32_t prioritized_replay;/* solver.prioritized_replay: 0 => priorities are not updated (src/solver.jl:231) */
    int64_t buffer_size;       /* solver.buffer_size */
    float   prio_alpha, prio_beta, prio_eps; /* 0.6, 0.4, 1e-3 */
    uint64_t seed;             /* sampler key (Philox4x32-10 counter RNG) */
    int32_t use_graph;         /* 1: replay the train step from a captured hipGraph */
    int32_t use_mfma;          /* 1: fp32 MFMA kernels where shapes allow (bit-identical to the VALU path) */
    int32_t recurrence;        /* solver.recurrence: DRQN on an EpisodeReplayBuffer (src/solver.jl:12,182-183,239-287) */
    int32_t trace_length;      /* solver.trace_length (40) */
    int32_t sample_distinct;   /* 0 (default): stratified sum-tree draws, duplicates possible within a batch.  1: B DISTINCT indices like the reference's
                                * sample(rng, 1:n, Weights(p), B, replace=false) (...replay.jl:85): after the stratified draws, every later duplicate is redrawn
                                * from the tree with the mass of all taken leaves removed (successive sampling on the residual priorities) */
    int32_t reserved[3];
} dqn_hparams;

const char* dqn_last_error(void);
int dqn_version(void);

/* Fill `hp` with the reference defaults (src/solver.jl:3-27, ...replay.jl:42-45). */
int dqn_hparams_default(dqn_hparams* hp);

/* Host-only (no GPU needed): the default summation-order plan the engine would use
 * for this network, one entry per layer. */
/* Version of the plan SEMANTICS (what a dqn_layer_plan value means for the rounding order) and of dqn_plan_default's choices.  Results are bit-identical only
 * between builds of the same version under the same plan; a checkpoint records both and a resume across versions is refused.
 *   1  rounds 1-2      2  round 3: conv dx_kc = RAW taps per chunk, conv dw_kc may be sample-granular      3  round 4: dw_kc < 0 = column-group chunks
 *   (recurrent networks; the default for the networks the fused recurrent step covers) */
#define DQN_PLAN_VERSION 3
int dqn_plan_version(void);
int dqn_plan_default(const dqn_layer_desc* layers, int n_layers, const dqn_hparams* hp,
                     dqn_layer_plan* plan_out);

/* solve(): src/solver.jl:40-57 builds replay + (dueling) network + policy; the
 * engine owns their device state.  plan_or_null overrides the default plan. */
int dqn_engine_create(const dqn_layer_desc* layers, int n_layers, const dqn_hparams* hp,
                      const dqn_layer_plan* plan_or_null, int device, dqn_engine_t** out);
int dqn_engine_destroy(dqn_engine_t* e);
int dqn_engine_get_plan(dqn_engine_t* e, dqn_layer_plan* plan_out /* n_layers entries */);
int dqn_n_params(dqn_engine_t* e, size_t* n);
/* bytes per element of the batch arena the train step gathers into: 4 (fp32 X0[f][2B]) or 1 (byte arena: u8 replay whose first layer converts
 * byte/255 inside its tile loads).  Decided when the step program is built (first train call); measurement tools price the gather with it. */
int dqn_batch_arena_elem_bytes(dqn_engine_t* e, int* bytes);

/* Flux.params(active_q) / Flux.loadparams! (src/solver.jl:143-144, :292, :314-315). */
int dqn_set_params(dqn_engine_t* e, int which, const float* flat, size_t n);
int dqn_get_params(dqn_engine_t* e, int which, float* flat, size_t n);
/* target_q <- active_q every target_update_freq steps (src/solver.jl:142-145). */
int dqn_sync_target(dqn_engine_t* e);
/* Adam state (no reference equivalent: the reference cannot resume an optimizer). */
int dqn_get_adam_state(dqn_engine_t* e, float* m, float* v, double* beta_pow /*[2]*/, size_t n);
int dqn_set_adam_state(dqn_engine_t* e, const float* m, const float* v, const double* beta_pow, size_t n);

/* add_exp!(r, DQExperience(s,a,r,sp,done), td_err) for n transitions
 * (src/prioritized_experience_replay.jl:65-74; n > 1 serves vectorised envs).
 * s, sp: n rows of obs in the replay storage dtype; td_err may be NULL => |r| (:65). */
int dqn_replay_add(dqn_engine_t* e, const void* s, const int32_t* a, const float* r,
                   const void* sp, const uint8_t* done, const float* td_err, int n);
int dqn_replay_size(dqn_engine_t* e, int64_t* cur, int64_t* cap); /* _curr_size, max_size (:61-63) */
int dqn_replay_get_priorities(dqn_engine_t* e, float* prio, int64_t n); /* r._priorities[1:n] */

/* StatsBase.sample(r) (:82-87).  The reference draws B distinct indices with
 * probability proportional to priority (StatsBase A-ExpJ, O(n)); the engine uses a
 * stratified sum-tree descent (O(B log n)); parity is defined on GIVEN indices via
 * the two calls below.  idx_out (host, B int64, 0-based) may be NULL. */
int dqn_replay_sample(dqn_engine_t* e, int64_t* idx_out);
/* get_batch(r, idx) (:89-104): the deterministic seam.  Any output may be NULL.
 * s, sp: float[B][C][H][W]; a: int32[B]; r, done, w: float[B]. */
int dqn_replay_get_batch(dqn_engine_t* e, const int64_t* idx, float* s, int32_t* a, float* r,
                         float* sp, float* done, float* w);
/* update_priorities!(r, idx, td) (:76-80). */
int dqn_update_priorities(dqn_engine_t* e, const int64_t* idx, const float* td, int n);

/* batch_train!(solver, env, policy, optimizer, target_q, replay) (src/solver.jl:191-236):
 * sample (or use idx) -> gather + IS weights -> double-Q Bellman target -> Huber(w*td)/B ->
 * backward -> max-abs grad norm -> Adam -> priority update.  Returns (loss_val, grad_norm)
 * like the reference (:235).  All outputs optional; with every output NULL the call only
 * enqueues work on the engine's stream (no host sync). */
int dqn_train_step(dqn_engine_t* e, const int64_t* idx_or_null, float* loss, float* grad_norm,
                   float* td_out /* B */);
/* The same step without waiting for it: returns as soon as the step is enqueued on the engine's stream.  *ticket names the (loss, grad_norm) record the step's
 * last launch publishes into a mapped pinned host ring (no fold launch, no D2H copy, no stream synchronize).  The reference reads batch_train!'s return values
 * only every log_freq env steps (src/solver.jl:154-167); the shim's dqn_train! loop fetches them there.  dqn_train_step(e, idx, &loss, &gn, NULL) itself is
 * this call followed by dqn_step_scalars(e, ticket, 1, ...).  Single-device feed-forward engines. */
int dqn_train_step_async(dqn_engine_t* e, const int64_t* idx_or_null, uint64_t* ticket);
/* (loss, grad_norm) of the step that returned `ticket` -- one of the 64 newest.  wait != 0: blocks (host spin on the record, stream synchronize as a fallback)
 * until it has arrived.  wait == 0: returns at once; *published = ticket and the outputs are written if the record was there, *published = 0 otherwise.
 * Device-side assertion failures of that step (AssertionError: all(new_priorities .> 0f0)) are reported here. */
int dqn_step_scalars(dqn_engine_t* e, uint64_t ticket, int wait, float* loss, float* grad_norm, uint64_t* published);
/* run `n_steps` sampled train steps back to back; returns the last step's scalars.  Bit-identical to n_steps calls of dqn_train_step(e, NULL, ...)
 * (tests/test_gpu_parity.py::test_train_steps_pipelined_gather_bit_exact), but inside the call nothing else can touch the replay, so step i's last
 * launch already gathers step i+1's batch and steps 2..n run without a sample / gather launch (prioritized replay; f32 observations, or u8
 * observations on the byte arena; any batch size; replicas too -- the gather is rank-local). */
int dqn_train_steps(dqn_engine_t* e, int n_steps, float* loss, float* grad_norm);

/* Results of the last train step (parity checks; not on the hot path). */
int dqn_get_last_q(dqn_engine_t* e, float* q_on_s, float* q_on_sp, float* q_tg_sp /* each [B][nA] */,
                   int32_t* best_a /* B */, float* q_targets /* B */);
int dqn_get_last_indices(dqn_engine_t* e, int64_t* idx /* B */);
int dqn_get_last_td(dqn_engine_t* e, float* td /* B, unweighted: Q(s, a) - y */, float* is_weights /* B */); /* feed-forward engines; either may be NULL */
int dqn_get_grads(dqn_engine_t* e, float* flat, size_t n); /* Flux.params order/layout */

/* ---- DRQN (solver.recurrence = true): EpisodeReplayBuffer (src/episode_replay.jl) and batch_train!(..., ::EpisodeReplayBuffer)
 * (src/solver.jl:239-287).  buffer_size counts EPISODES.  Only the first trace_length transitions of an episode are ever
 * read by the reference's sampler (episode_replay.jl:82-92 copies the episode PREFIX), so only those are kept. */
/* add_exp!(r::EpisodeReplayBuffer, exp) (:46-52): append n transitions to the open episode; an episode is stored when done. */
int dqn_episode_add(dqn_engine_t* e, const void* s, const int32_t* a, const float* r, const void* sp, const uint8_t* done, int n);
/* add_episode!(r, ep) (:54-60) for populate_replay_buffer!/generate_episode (:97-130): store the open episode now. */
int dqn_episode_commit(dqn_engine_t* e);
int dqn_episode_count(dqn_engine_t* e, int64_t* cur, int64_t* cap);
/* sample(r::EpisodeReplayBuffer) (:71-95) for GIVEN draws: ep_idx[B] distinct episodes (0-based), ep_start[B] in [0,len).
 * Outputs (all optional): s, sp: float[T][B][C][H][W]; a: int32[T][B] (0-based); r, done: float[T][B]; mask: int32[T][B]. */
int dqn_episode_get_batch(dqn_engine_t* e, const int64_t* ep_idx, const int32_t* ep_start, float* s, int32_t* a, float* r,
                          float* sp, float* done, int32_t* mask);
/* recurrent batch_train! (src/solver.jl:239-287): targets with hidden state carried over sp[1..T] for both nets, BPTT over
 * s[1..T] of the masked Huber loss / B / T, max-abs grad norm, Adam; no IS weights, no priority update.
 * ep_idx/ep_start NULL => the engine draws them (uniform without replacement; start uniform in [0,len)). */
int dqn_train_step_drqn(dqn_engine_t* e, const int64_t* ep_idx, const int32_t* ep_start, float* loss, float* grad_norm);
/* Recur state of the POLICY network (src/policy.jl:32-34 resetstate!, src/helpers.jl:61-79 hiddenstates/sethiddenstates!):
 * dqn_forward / dqn_greedy_action advance it for recurrent networks (n streams, one per observation row). */
int dqn_reset_state(dqn_engine_t* e);
/* Flat layout, per recurrent layer in chain order: an LSTM layer writes h then c, a GRU layer writes h; each is [out][streams]
 * (streams = observations per dqn_forward call, 1 before the first).  An RNN layer writes h only, [out][streams], as a GRU layer does.
 * n = sum over LSTM layers of 2 x out x streams + sum over GRU and RNN layers of out x streams floats. */
int dqn_get_hidden(dqn_engine_t* e, float* hc, size_t n);
int dqn_set_hidden(dqn_engine_t* e, const float* hc, size_t n);

/* NNPolicy: actionvalues / action / value (src/policy.jl:38-64) for n observations
 * (n = 1 in the reference; n > 1 serves vectorised envs).  obs: float[n][C][H][W]. */
int dqn_forward(dqn_engine_t* e, int which, const float* obs, int n, float* q_out /* [n][nA] */);
int dqn_greedy_action(dqn_engine_t* e, const float* obs, int n, int32_t* a_out /* first-max tie rule */);

/* ---- vectorised environments on the device (north star: "vectorised parallel environments (SimpleGridWorld /
 * image-obs MDPs)").  n lock-stepped copies of a built-in MDP live in HBM; one vector step is one iteration of the dqn_train!
 * loop (src/solver.jl:82-145) for all copies: eps-greedy action from the online net (POMDPTools EpsGreedyPolicy:
 * rand < eps ? random action : greedy), act!, observe, add_exp!(replay, exp, |r|) straight into the replay ring, episode
 * bookkeeping (reset on done or max_episode_length), every train_freq vector steps one batch_train!, every
 * target_update_freq a target sync.  No observation crosses PCIe.  Randomness: Philox4x32-10 keyed by seed, counter =
 * (global vector step, env, purpose), so the CPU twin reproduces every trajectory bit for bit.
 *
 * RECURRENT engines (hparams.recurrence = 1; single device: refused on an engine with a communicator or under DQN_SIM_WORLD, and dqn_comm_init is refused once
 * such an env set exists).  1 <= n_envs <= 1024; buffer_size counts episodes, the transition-ring capacity does not apply.
 *  - Policy state.  The training copies' Recur state IS the engine's policy state with n_envs streams: dqn_get_hidden (streams = n_envs) reads it, dqn_set_hidden
 *    writes it, dqn_reset_state resets it -- resetstate!(policy) acts on the one policy.  The evaluation copies own a private state of n_eval streams.
 *  - State advance.  every vector step advances every copy's state, exploring or not (this project's host loop also computes the greedy action on every step;
 *    what POMDPTools' EpsGreedyPolicy does to a recurrent policy on the exploring branch is third-party: recalled, not executed here).
 *  - resetstate! per copy.  A copy whose episode ended (done, or max_episode_length steps) gets, before the first recurrent layer of its next acting step, state0
 *    of the ONLINE net as it is then (h0 / c0 are trainable); other copies' columns are untouched.  The acting forward of a copy equals, bit for bit,
 *    dqn_forward on a stream that was reset at the same points and fed the same observations.
 *  - add_exp!.  Nothing is written to the prioritized ring or the sum-tree.  Each copy has an open episode; a transition is kept only while the open length is below
 *    trace_length (the prefix is all a sample can read), the length counts on.  Truncation at max_episode_length resets the env and the Recur state but does NOT
 *    close the open episode (the reference stores an episode only on done, src/episode_replay.jl:46-52; dqn_episode_add behaves the same).  On done the
 *    staged prefix, with the episode's true length, is committed to ring slot (ep_widx + k) % capacity, where k is the rank of the copy among the copies that
 *    finished in this vector step in ascending copy index; cursor and count advance by the number of finishers.  (The reference has one copy: the order among
 *    copies is this project's definition.)  dqn_envs_create on an engine that has an env set discards the open episodes and keeps the committed ones.
 *  - One collector at a time.  dqn_envs_create and dqn_rollout are refused while the host-side open episode (dqn_episode_add) is non-empty; dqn_episode_add and
 *    dqn_episode_commit are refused on an engine that has an env set.
 *  - Training.  Where a train step is due and the ring holds batch_size episodes, dqn_rollout runs the sampled recurrent step (dqn_train_step_drqn with NULL
 *    draws: the same host sampler, the same draw counter), after refreshing the host's view of the ring from the device.  The train step leaves the policy's
 *    Recur state as it found it (src/solver.jl:137-139).  dqn_episode_export / dqn_get_counters after a rollout describe the committed ring; open episodes
 *    are not part of a checkpoint.
 *  - dqn_evaluate leaves the training copies, the policy state, the ring, the open episodes and the counters exactly as they were. */
enum { DQN_ENV_TESTMDP = 0, DQN_ENV_GRIDWORLD = 1, DQN_ENV_TABULAR = 2 };      /* DQN_ENV_TABULAR has its own spec and entry point, dqn_envs_create_tabular below */
typedef struct {
    int32_t kind;               /* DQN_ENV_* */
    int32_t n_envs;
    int32_t max_episode_length; /* solver.max_episode_length (100) */
    uint64_t seed;
    /* TestMDP (test/test_env.jl:10-87): obs = stack of o_stack of three fixed H x W integer images / 255, chosen by the last
     * actions; rewards [-0.1, 0, 0.1][sp[end]] x (-10 if s[end] == 2); terminal at t >= max_time; 4 actions */
    int32_t o_stack, max_time;
    const uint8_t* images;      /* uint8[3][H*W]: bad, normal, good; H, W from hparams.obs_h/obs_w; obs_c == o_stack */
    /* SimpleGridWorld (POMDPModels defaults, third-party; recalled): size_x x size_y grid, 4 actions up/down/left/right,
     * reward cells are terminal, intended move with probability tprob, obs = Float32[x, y] */
    int32_t size_x, size_y; float tprob; int32_t n_reward_cells; int32_t reward_xy[8][2]; float reward_val[8];
} dqn_env_spec;
typedef struct {
    int32_t train_freq, target_update_freq;     /* solver.train_freq (4), solver.target_update_freq (500); 0 = never */
    float eps_start, eps_stop, eps_steps;       /* LinearDecaySchedule(start, stop, steps) of the exploration policy */
    int32_t cadence_env_steps;                  /* (r05; occupies what was padding: offsets and size unchanged)  0: train_freq / target_update_freq count VECTOR steps -- one
                                                 * train step per train_freq steps of all n copies.  1: they count ENV steps as the reference's loop does (src/solver.jl:136-145):
                                                 * after vector step t, floor(t*n / train_freq) - floor((t-1)*n / train_freq) train steps run back to back (8 per vector step
                                                 * for 32 copies at train_freq = 4) and the target network is synced whenever a multiple of target_update_freq env steps
                                                 * was crossed.  The n transitions of a vector step are added BEFORE its train steps (the reference interleaves them). */
    int64_t t0;                                 /* global index of the first vector step of this call (t counts from 1) */
} dqn_rollout_cfg;
typedef struct { int64_t episodes; double reward_sum; int64_t train_steps; float last_loss, last_grad_norm; } dqn_rollout_stats;
int dqn_envs_create(dqn_engine_t* e, const dqn_env_spec* spec);
/* ---- tabular environments: any discrete MDP / POMDP given as its matrices (TigerPOMDP, BabyPOMDP, SimpleGridWorld, the POMDPModels zoo) on the device loop.
 * The tables are copied to HBM at creation (the caller's pointers are not kept); afterwards the set behaves exactly as one made by dqn_envs_create: dqn_rollout,
 * dqn_evaluate, dqn_envs_reset, dqn_envs_peek, dqn_envs_info and the lifecycle rules above apply unchanged, on feed-forward and recurrent engines.  The acting step
 * takes the general four-launch tail (dqn_envs_info: fused_tail = 0).
 *
 * One step of copy i at vector step t (POMDPTools' MDPCommonRLEnv / POMDPCommonRLEnv; third-party, recalled): sp ~ T[s][a]; o ~ Z[a][sp] (an MDP: o = sp);
 * r = R[s][a][sp]; done = terminal[sp].  The observation of the transition's s is the feature row of the observation index held before the step, that of sp the
 * feature row of o.  Reset: s ~ b0, then o ~ Z0[s] (an MDP: o = s).
 *
 * THE SAMPLING LAW.  At creation the host turns every distribution row (T[s][a][:], Z[a][sp][:], Z0[s][:], b0[:]) into a cumulative row with a plain fp32 loop in
 * ascending index order (acc = acc + p; no contraction, no device kernel).  A draw is u = u01(philox(seed, t, i, purpose)) with the counter layout and u01 of the
 * built-in kinds ((r >> 8) * 2^-24).  The pick is the first j with u < cdf[j].  If no j qualifies (the row's fp32 sum lies at or below u) the pick is the last j
 * with cdf[j] > cdf[j - 1] (cdf[0] > 0 for j = 0) -- so an entry of probability zero is never picked.  (A row without any positive entry -- possible only for T at
 * a terminal state, reachable only if b0 puts mass there -- picks index 0.)  The device finds j by binary search over the cumulative row; a cumulative row of
 * non-negative fp32 terms is non-decreasing, so this is the j of the linear scan that defines the law.  Purposes 1-6 belong to the built-in kinds (1 explore or not,
 * 2 random action, 3-4 SimpleGridWorld move, 5-6 SimpleGridWorld reset); the tabular kind draws with the four below.
 *
 * Refused, each with a message naming the offending value: n_states outside 1..1024, n_obs outside 0..1024; n_envs outside what the engine kind allows (above);
 * a missing table, or Z / Z0 given with n_obs == 0; a negative or non-finite probability; a row whose sum, taken in double, is further than 1e-3 from 1 (rows of T at
 * terminal states are exempt); a non-finite reward or feature; an engine with a u8 replay (feature rows are floats); an engine with a communicator or created under
 * DQN_SIM_WORLD -- and dqn_comm_init once such a set exists (no exchange path has run with it). */
enum { DQN_ENV_RAND_TAB_NEXT = 7, DQN_ENV_RAND_TAB_OBS = 8, DQN_ENV_RAND_TAB_INIT = 9, DQN_ENV_RAND_TAB_INIT_OBS = 10 };      /* next state, observation, initial state, initial observation */
typedef struct {
    int32_t n_envs, max_episode_length; uint64_t seed;
    int32_t n_states, n_obs;      /* S; O = 0: an MDP, the observation index IS the state index */
    const float*   T;             /* [S][A][S]  P(sp | s, a),  A = hparams.n_actions */
    const float*   Z;             /* [A][S][O]  P(o | a, sp);  NULL iff O == 0 */
    const float*   Z0;            /* [S][O]     P(o | s) of the observation after a reset; NULL iff O == 0 */
    const float*   R;             /* [S][A][S]  reward(s, a, sp) */
    const uint8_t* terminal;      /* [S] */
    const float*   b0;            /* [S] initial-state distribution */
    const float*   features;      /* [O ? O : S][E]  convert_o / convert_s row per index, E = obs_c*obs_h*obs_w */
} dqn_tabular_env;
int dqn_envs_create_tabular(dqn_engine_t* e, const dqn_tabular_env* spec);
/* ---- continuous-state control problems: POMDPModels' MountainCar and InvertedPendulum on the device loop.  The state of a copy is two Float64 values, carried from
 * step to step as the reference's MDPCommonRLEnv carries it; the observation is Float32[state[1], state[2]] (convert_s); there are three actions.  After creation the
 * set behaves exactly as one made by dqn_envs_create: dqn_rollout, dqn_rollout_explore (both kinds), dqn_evaluate, dqn_envs_reset, dqn_envs_peek, dqn_envs_peek_q,
 * dqn_envs_info and the lifecycle rules above apply unchanged, on feed-forward and recurrent engines, and as a member of an engine group.  The acting step takes the
 * general four-launch tail (dqn_envs_info: fused_tail = 0).  dqn_envs_create answers "unknown environment kind" for these kinds, as it does for DQN_ENV_TABULAR.
 *
 * THE LAWS are those of POMDPModels 0.4 (third-party): RECALLED, NOT EXECUTED here.  Every constant is a field of the spec, so a different recollection is a
 * different spec, not a different build.  Both laws are plain IEEE double arithmetic in the written order, left to right, without fused multiply-add; cos / sin are
 * the device library's double versions (no fast intrinsic).  a = the action index 0, 1, 2.
 *
 * MOUNTAINCAR, state (x, v), push = a - 1:
 *     v' = v + push * force + cos(freq * x) * (-gravity);   v' = max(min(v_max, v'), -v_max);   x' = x + v';   if x' < x_min: x' = x_min, v' = 0
 *     done = x' >= goal;   r = cost + (done ? jackpot : 0).   Reset: (x0, v0), no draw.
 * INVERTEDPENDULUM (Lagoudakis & Parr), state (theta, omega), explicit Euler from the pre-step state:
 *     u = (a - 1) * u_max + noise * (U12 - 0.5)
 *     acc = (g * sin(theta) - alpha * m * l * omega * omega * sin(2 * theta) * 0.5 - alpha * cos(theta) * u) / ((4 / 3) * l - alpha * m * l * cos(theta) * cos(theta))
 *     theta' = theta + omega * dt;   omega' = omega + acc * dt;   done = |theta'| > theta_max;   r = done ? cost : 0
 *     Reset: theta = (U13 - 0.5) * 2 * init_half,  omega = (U14 - 0.5) * 2 * init_half.
 * A draw is U = (double)u01(philox(seed, t, i, purpose)) with the counter layout and the 24-bit u01 of the other kinds; U12 is drawn at the vector step of the
 * transition, U13 / U14 at the step whose reset they serve (0 for dqn_envs_reset), as the other kinds' reset draws are.  The transition's s is the Float32
 * observation of the pre-step state, sp that of the post-step state; the reward goes to the replay as (float)r.  Episode bookkeeping, truncation, pending resets,
 * priorities and the open-episode rules of a recurrent engine are the loop's: nothing in them depends on the kind.
 *
 * Refused before the engine's current env set is touched, each with a message naming the field and the value: an unknown kind; n_envs outside what the engine
 * kind allows (above); a constant that is not finite; dt <= 0; v_max <= 0; l <= 0; x_min >= goal; a pendulum whose denominator can reach 0 (4/3 <= alpha * m); an
 * engine whose observation is not 2 floats or whose network has not 3 outputs; an engine with a u8 replay; an engine with a communicator or created under
 * DQN_SIM_WORLD -- and dqn_comm_init once such a set exists (single GPU only). */
enum { DQN_ENV_MOUNTAINCAR = 3, DQN_ENV_PENDULUM = 4 };
enum { DQN_ENV_RAND_PEND_NOISE = 12, DQN_ENV_RAND_PEND_THETA0 = 13, DQN_ENV_RAND_PEND_OMEGA0 = 14 };      /* the pendulum's action noise, its reset of theta and of omega; 1-11 are taken */
typedef struct {
    int32_t kind;               /* DQN_ENV_MOUNTAINCAR or DQN_ENV_PENDULUM; the other member's constants are checked for finiteness only */
    int32_t n_envs;
    int32_t max_episode_length;
    uint64_t seed;
    /* MountainCar.  POMDPModels defaults: force 0.001, freq 3, gravity 0.0025, v_max 0.07, x_min -1.2, goal 0.5, cost -1, jackpot 100, x0 -0.5, v0 0 (discount 0.99) */
    double force, freq, gravity, v_max, x_min, goal;
    double cost;                /* both members: MountainCar's reward per step, the pendulum's reward on falling.  Default -1 for either */
    double jackpot, x0, v0;
    /* InvertedPendulum.  POMDPModels defaults: g 9.81, m 2, l 8, M 8, alpha 1 / (m + M), dt 0.1, u_max 50, noise 20, theta_max pi / 2, init_half 0.1 (discount 0.99).
     * M enters the law through alpha only */
    double g, m, l, M, alpha, dt, u_max, noise, theta_max, init_half;
} dqn_control_env;
int dqn_envs_create_control(dqn_engine_t* e, const dqn_control_env* spec);
/* inspection (parity tests): the Float64 state of the training copies as it stands, and the state each copy held before its last step (what the last transition's s
 * is the observation of; zero before the set's first step).  Either pointer may be NULL.  Refused on an env set of another kind. */
int dqn_envs_peek_state(dqn_engine_t* e, double* state /* [n_envs][2] */, double* prev /* [n_envs][2] or NULL */);
int dqn_envs_reset(dqn_engine_t* e);
int dqn_rollout(dqn_engine_t* e, int n_vector_steps, const dqn_rollout_cfg* cfg, dqn_rollout_stats* stats_or_null);
/* ---- exploration by table: POMDPTools' two exploration policies, EpsGreedyPolicy and SoftmaxPolicy, each with any schedule (a number, a LinearDecaySchedule, any
 * function of the step).  The HOST evaluates the schedule and rounds it to fp32; the device only reads the table: values[j] is eps (DQN_EXPLORE_EPS_GREEDY) or the
 * temperature tau (DQN_EXPLORE_SOFTMAX) of vector step cfg->t0 + j; n_values is n_vector_steps, or 1 for a constant.  x == NULL is exactly dqn_rollout; with x given
 * cfg->eps_* are ignored.  Feed-forward and recurrent engines, the three env kinds, both cadences, every graph mode; dqn_evaluate stays greedy.  A rollout with a
 * table takes the general four-launch tail (the fused tail, act_head.hip, serves the linear law only); dqn_envs_info keeps reporting what dqn_rollout uses.
 *
 * EPS TABLE.  rand < eps ? random action : greedy stays as it is (purposes 1 and 2, u01(...) < eps); only eps changes, to values[t - t0].  eps = 1 always
 * explores (u01 < 1), eps = 0 never does.
 *
 * SOFTMAX (POMDPTools' SoftmaxPolicy.action: vals ./ tau, subtract the maximum, exp, normalise, weighted sample -- third-party, recalled and not executed here).  In
 * fp32, on the Q column q_0 .. q_{nA-1} the step computes anyway (what dqn_envs_peek's actions are the argmax of when nothing explores):
 *     z_k = q_k / tau (IEEE division);  m = max_k z_k;  w_k = expf(z_k - m) (the device library's expf, no fast intrinsic);  c_k = c_{k-1} + w_k in ascending k (c_{-1} = 0);
 *     target = u * c_{nA-1},  u = u01(philox(seed, t, i, DQN_ENV_RAND_SOFTMAX)).
 * The pick is the first k with target < c_k.  If none qualifies, the last k with c_k > c_{k-1} -- so an action whose weight underflowed to zero is never picked (the
 * rule of the tabular kind's draws).  On a recurrent engine nothing else changes: every vector step advances every copy's Recur state.
 *
 * Refused before anything is enqueued, each with a message naming the offending value and its index: an unknown kind; n_values neither 1 nor n_vector_steps; NULL
 * values; eps outside [0, 1] or NaN; tau <= 0 or not finite.  A refused call leaves the env set as it was. */
enum { DQN_EXPLORE_EPS_GREEDY = 0, DQN_EXPLORE_SOFTMAX = 1 };
enum { DQN_ENV_RAND_SOFTMAX = 11 };            /* Philox purpose of the softmax draw; 1-10 are taken */
typedef struct { int32_t kind; int32_t n_values; const float* values; } dqn_exploration;
int dqn_rollout_explore(dqn_engine_t* e, int n_vector_steps, const dqn_rollout_cfg* cfg, const dqn_exploration* x, dqn_rollout_stats* stats_or_null);
/* basic_evaluation (src/evaluation_policy.jl:17-42; cadence src/solver.jl:101-122) batched on the device: n_eval
 * further copies of the MDP given to dqn_envs_create each run ONE greedy episode (while !done && step <= max_episode_length); returns
 * the average undiscounted return (Float64 sum of the Float32 rewards, as r_tot) and the average step count. */
int dqn_evaluate(dqn_engine_t* e, int n_eval, int max_episode_length, uint64_t seed, double* avg_reward, double* avg_steps);
/* inspection (parity tests): current observations float[n][C][H][W], last actions int32[n], last rewards float[n], last dones uint8[n] */
int dqn_envs_peek(dqn_engine_t* e, float* obs, int32_t* actions, float* rewards, uint8_t* dones);
/* inspection (parity tests): what the acting forward of the LAST vector step of the training env set computed, read-only -- the stream is synchronised and two buffers
 * are copied; nothing is launched and nothing is rewritten (dqn_envs_peek re-observes the env states for its obs; this does not).  q[i] is the Q column of copy i's
 * policy input at that step, after the dueling join ((v + a) - mean(a)); greedy[i] is its first-max argmax.  dqn_envs_peek's actions[i] is greedy[i] unless copy i
 * explored.  Every schedule of the acting step writes them (the four-launch tail, the fused tail, the recurrent tail, the single-workgroup step of an engine group).
 * Either pointer may be NULL.  Refused, with a message: no device environments; the set has not taken a vector step since it was created (dqn_rollout,
 * dqn_rollout_explore or dqn_rollout_many with n_vector_steps >= 1); the policy workspace that holds the columns was used by another forward since that step
 * (dqn_forward, dqn_greedy_action, dqn_evaluate, or a reallocation for more columns). */
int dqn_envs_peek_q(dqn_engine_t* e, float* q /* [n_envs][n_actions] */, int32_t* greedy /* [n_envs] */);
/* inspection (parity tests, which must know WHICH schedule they compared): n_envs of the training set; fused_tail = 1 when the acting step of that set runs its tail as one
 * launch (act_head.hip: reduce + heads + Q / argmax + eps-greedy + act! + add_exp!'s per-experience part), 0 for the general four-launch tail.  Builds the acting program
 * (as dqn_rollout would) if it does not exist yet. */
int dqn_envs_info(dqn_engine_t* e, int* n_envs, int* fused_tail);

/* ---- checkpoint / resume (absent in the reference, which only saves the best network: src/solver.jl:290-318).
 * Together with dqn_get/set_params, dqn_get/set_adam_state these make a run resumable bit for bit: the replay in its storage type
 * (rows `first .. first+n-1` of the ring, slot order), stored priorities, ring cursor, and the sampler / optimizer counters. */
typedef struct { int64_t size, widx; uint64_t sample_ctr, train_steps; } dqn_counters;
int dqn_replay_export(dqn_engine_t* e, int64_t first, int64_t n, void* s, void* sp, int32_t* a, float* r, uint8_t* done, float* priorities);
/* replaces the whole replay: n <= capacity transitions go to slots 0..n-1 with the given priorities (NOT td errors); the sum-tree is rebuilt */
int dqn_replay_import(dqn_engine_t* e, int64_t n, const void* s, const void* sp, const int32_t* a, const float* r, const uint8_t* done, const float* priorities);
/* ... and for the episode replay of a recurrent engine (src/episode_replay.jl; config 4): episodes first..first+n-1 in slot order, rows
 * [n][trace_length][obs] float (only the first trace_length transitions of an episode can ever be sampled, :82-92, so only they are stored),
 * a / r / done [n][trace_length], len[n] = the episode's true length.  dqn_get/set_counters then mean: size = episodes, widx = ring cursor,
 * sample_ctr = the host sampler's draw counter.  An episode still being collected is not part of a checkpoint. */
int dqn_episode_export(dqn_engine_t* e, int64_t first, int64_t n, float* s, float* sp, int32_t* a, float* r, uint8_t* done, int32_t* len);
int dqn_episode_import(dqn_engine_t* e, int64_t n, const float* s, const float* sp, const int32_t* a, const float* r, const uint8_t* done, const int32_t* len);
int dqn_get_counters(dqn_engine_t* e, dqn_counters* out);
int dqn_set_counters(dqn_engine_t* e, const dqn_counters* in);   /* size must equal the imported n; widx < capacity */

/* data-parallel replicas (no reference equivalent): after dqn_comm_init every train step exchanges gradients between backward and Adam
 * with ONE collective over RCCL (dlopen'ed librccl) on the engine's stream -- an all-gather of the wide dense layers' operands and of the
 * small gradients, or an all-reduce of the flat gradient (no qualifying layer, recurrent engines, DQN_DP_ALLREDUCE=1);
 * Adam then applies the sum * 1/world, identically on every rank.  unique_id: 128 bytes from dqn_comm_unique_id on rank 0.
 * Every rank must issue the same sequence of train steps. */
int dqn_comm_unique_id(void* id128);
int dqn_comm_init(dqn_engine_t* e, const void* id128, int rank, int world);
/* what the communicator ITSELF reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice) next to what the engine was told: a bench line can prove how
 * many ranks RCCL saw.  No communicator: rccl_nranks = 0, rccl_rank = rccl_device = -1.  exchange: 0 none, 1 all-gather of the wide dense layers' operands +
 * small gradients, 2 all-reduce of the flat gradient, -1 not decided yet (the step program is built at the first train step). */
typedef struct dqn_comm_info_t { int32_t rccl_nranks, rccl_rank, rccl_device, engine_world, engine_rank, sim_world, exchange, dp_overlap; } dqn_comm_info_t;
int dqn_comm_info(dqn_engine_t* e, dqn_comm_info_t* out);
/* bytes ONE rank contributes to the step's collective (the packed block of the all-gather: X | dpre of the wide dense layers + every other gradient range; or the flat
 * gradient of the all-reduce); 0 without a communicator / before the step program exists (it is built by the first train step) */
int dqn_comm_exchange_bytes(dqn_engine_t* e, int64_t* bytes_per_rank);

/* TEST HOOK for the exchange above on ONE GPU: an engine created with the environment variable DQN_SIM_WORLD=k plays k ranks; this call runs
 * one data-parallel step with k DISTINCT batches idx[k][B] (rank r's packed block lands in slot r of the gathered buffer, as ncclAllGather
 * would deliver it).  loss[k]: per-rank losses; td_out[k][B].  Equivalent single-device step: the concatenated batch of k*B samples. */
int dqn_sim_ranks_step(dqn_engine_t* e, const int64_t* idx, float* loss, float* grad_norm, float* td_out);

/* raw access for harnesses that time kernels on the engine's own stream. */
int dqn_stream_sync(dqn_engine_t* e);
int dqn_stream_handle(dqn_engine_t* e, void** hip_stream);
/* per-kernel timing of the last dqn_profile_step call: names (static strings) and
 * milliseconds measured with HIP events on the engine stream. */
int dqn_profile_step(dqn_engine_t* e, int max_entries, const char** names, float* ms, int* n_entries);
/* as dqn_profile_step, but TWO train steps run and the second is timed as a MIDDLE step of dqn_train_steps(n): inside that call step i's last
 * launch (Adam) already gathers step i+1's batch, so a middle step has no gather launch of its own (where dqn_train_steps pipelines it;
 * otherwise both steps are plain ones).  Results of dqn_train_steps(n) are bit-identical to n dqn_train_step calls either way. */
int dqn_profile_steady_step(dqn_engine_t* e, int max_entries, const char** names, float* ms, int* n_entries);

/* ---- engine groups: many small Q-networks trained at once (seeds, learning-rate sweeps, bootstrapped ensembles; no reference equivalent).
 * A network that fits in one workgroup's LDS trains as ONE launch of ONE workgroup per step (dqn_train_step on such an engine occupies one compute unit of the
 * device).  A group steps K such engines with ONE launch of K workgroups per step: workgroup k runs member k's step on member k's own parameters, Adam state,
 * sum-tree, replay rows and counters.  Members share nothing; there is no traffic between workgroups.
 *
 * THE LAW.  After dqn_group_train_steps(g, n, ...) every member is indistinguishable from an engine on which dqn_train_steps(e, n, ...) was called: parameters of
 * both networks, gradients, Adam m / v / beta powers, the sum-tree and priorities, the counters, dqn_get_last_indices, dqn_get_last_q, the TD errors and IS weights,
 * the returned loss and grad norm, and the bytes of a checkpoint are bit for bit the same.  Members may differ in everything an engine is created with: network
 * (any network that takes the single-workgroup step), batch size, obs_dtype, seed, learning rate, gamma, Adam constants, double_q, dueling, sample_distinct, replay
 * contents and replay size.
 *
 * STREAM ORDER.  The group owns a stream.  On entry that stream waits for everything enqueued so far on every member's stream; on exit every member's stream waits
 * for the group's steps.  A member's own calls (dqn_replay_add, dqn_train_step, dqn_sync_target, dqn_rollout, the getters) can therefore be interleaved freely with
 * group calls, with no host synchronise in between.  The n steps are n back-to-back launches.
 *
 * ERRORS.  A member's device-side assertion (AssertionError: all(new_priorities .> 0f0)) is reported by the group call in the standalone call's words, prefixed by
 * "member <index>:"; the other members' steps stand and their entries of loss / grad_norm are written.
 *
 * REFUSED, each with a message naming the member index and the reason: a null or duplicate member; n_members outside 1..4096; a member on another device than
 * member 0; a member that does not take the single-workgroup step -- recurrent, a layer that is not Dense, batch_size > 64, no prioritized replay, too many
 * parameters, a plan that cuts a layer's dX sum into chunks (the default plan does for Dense layers 128 or more wide: create such an engine with dx_kc = 0), DQN_NO_TINY,
 * data-parallel replicas (a communicator or DQN_SIM_WORLD),; at train time a member holding fewer than batch_size transitions (AssertionError: r._curr_size >=
 * r.batch_size) and n < 1.  dqn_engine_destroy and dqn_comm_init of a member of a live group are refused (the latter would rebuild the member's step program under the group): destroy the group first.  dqn_group_create builds each member's step program.
 * (Trace builds only: the timing probe DQN_TINY_STOP, which ends a standalone step early, is not honoured by a group: it always runs whole steps.) */
typedef struct dqn_group dqn_group_t;
typedef struct { int32_t n_members; uint32_t max_lds_bytes /* the launch's dynamic LDS: the largest member's */; int32_t launches_per_step /* 1 */; int32_t reserved; } dqn_group_info_t;
int dqn_group_create(dqn_engine_t* const* members, int n_members, dqn_group_t** out);
int dqn_group_train_steps(dqn_group_t* g, int n, float* loss_or_null /* [n_members] */, float* grad_norm_or_null /* [n_members] */);
int dqn_group_info(dqn_group_t* g, dqn_group_info_t* out);
int dqn_group_destroy(dqn_group_t* g);

/* ---- grouped acting: the device environment loop of all K members, ONE launch per vector step (tiny_act.hip).
 * A member of a group is a Dense-only network whose parameters fit in LDS, so one vector step of its env loop -- policy forward on its n copies, Q, argmax,
 * exploration, act!, add_exp! with its sum-tree ancestors, the ring rows and the next policy input -- runs as ONE workgroup.  dqn_rollout_many steps every member with
 * one launch of K workgroups per vector step, one group train launch at t % train_freq == 0 and one target-sync launch at t % target_update_freq == 0.
 *
 * THE LAW.  After dqn_rollout_many(g, n, cfgs, xs, out) every member k is bit for bit what dqn_rollout_explore(member_k, n, &cfgs[k], xs ? xs[k] : NULL, &out[k])
 * leaves: environment state and episode statistics (what dqn_envs_peek returns; its obs is re-observed from the env state, which the next policy input pol_x equals),
 * the last step's Q columns and greedy actions pol_q / pol_a (what dqn_envs_peek_q returns), replay rows, metadata, priorities and tree, the counters,
 * and -- after the interleaved train steps and target syncs -- parameters, Adam state, last loss / grad norm / indices / TD, and the bytes of a checkpoint.
 *
 * Vector-step cadence only.  Members may differ in everything an engine or an env set is created with (network, n_envs, env kind, obs_dtype, seed, eps schedule,
 * table); train_freq, target_update_freq and t0 must be equal across cfgs and cadence_env_steps must be 0.  explore is NULL, or K pointers of which a NULL entry
 * means that member's linear law.  The standalone loop trains a member only once its replay holds a batch and a group launch cannot skip a member: for every due
 * step of the call the host decides beforehand whether each member would train, and members that disagree are refused.
 *
 * STREAM ORDER and ERRORS are the group's (above): events in from every member's stream, events out on the error paths too, one synchronise at the end; a member's
 * device-side assertion is reported with its index, the other members' steps stand.  The flag is consumed by the call whether or not it trained.
 *
 * REFUSED before anything is enqueued, naming the member and the reason: a null handle, n_steps < 1, NULL cfgs, t0 < 1, unequal train_freq / target_update_freq /
 * t0, cadence_env_steps != 0, an invalid table (dqn_rollout_explore's words), members that disagree on a due train step, and a member that does not take the
 * single-workgroup acting step: no device environments, recurrent, a layer that is not Dense, parameters x n_envs > 262144, or more than 144 KB of LDS for its
 * parameters, the policy input, the activations of its n copies and the step's tail.  The per-call work does not grow with K in launches or copies: one H2D copy of
 * the K RolloutDev records, one of all tables, one launch that folds statistics, scalars and flags, one D2H copy -- and the 2 K event operations. */
int dqn_rollout_many(dqn_group_t* g, int n_vector_steps, const dqn_rollout_cfg* cfgs /* [K] */, const dqn_exploration* const* explore /* NULL or [K] with NULL entries */,
                     dqn_rollout_stats* out /* NULL or [K] */);
int dqn_rollout_many_info(dqn_group_t* g, int* launches_per_vector_step /* 1 */, unsigned* max_lds_bytes /* the acting launch's dynamic LDS: the largest member's */);

/* ---- grouped evaluation: basic_evaluation of all K members, the whole greedy episode loop inside the kernel (tiny_eval.hip).
 * In evaluation mode there is no replay, no tree and no exploration, and every copy is independent of every other, so nothing forces one launch per vector step: a
 * workgroup holds its member's parameters in LDS, resets the member's n_eval evaluation copies and repeats observe -> forward -> act! until every copy's one episode
 * is over.  The forward runs on one TILE of copies at a time (as many columns as fit in LDS beside the parameters); a column's values depend on that column alone, so
 * the tiling cannot change a bit.  One launch runs at most `steps_per_launch` vector steps (a compile-time bound: a caller's max_episode_length does not set a
 * kernel's duration); a call is ceil((max_episode_length + 1) / steps_per_launch) back-to-back launches of K workgroups, whatever K is.
 *
 * THE LAW.  After dqn_evaluate_many(g, n_eval, L, seeds, r, s), r[k] and s[k] are bit for bit the doubles dqn_evaluate(member_k, n_eval, L, seeds[k], ...) returns:
 * per copy the Float64 sum of its Float32 rewards, summed over the copies in ascending order in Float64, divided by n_eval; likewise the episode lengths.  Member k
 * is left as that call leaves it: training copies, open episodes, replay, tree, counters, parameters, Adam state and the bytes of a checkpoint are unchanged, and
 * dqn_envs_peek_q is refused until the training set steps again (the evaluation copies' forward used the policy workspace).
 *
 * STREAM ORDER and ERRORS are the group's (above): events in from every member's stream, events out on every path, one synchronise at the end.
 *
 * REFUSED before anything is enqueued or changed, naming the value (and the member): a null handle, n_eval outside 1..1024, max_episode_length < 1, NULL seeds, both
 * outputs NULL, and a member that does not take the single-workgroup evaluation: no device environments (of any of the three kinds), or a network whose parameters
 * and a tile of four copies do not fit the LDS of one workgroup (with P at its limit of 16 384 that is E + sum of layer widths > 1600).  The rule does not depend on
 * the number of training copies nor on n_eval.  The per-call work does not grow with K in launches or copies: one H2D copy of the K records, the launches, one D2H
 * copy of the K sums -- and the 2 K event operations.  Out of scope: softmax or eps in evaluation, recurrent members, caller-defined evaluation policies. */
int dqn_evaluate_many(dqn_group_t* g, int n_eval, int max_episode_length, const uint64_t* seeds /* [K] */, double* avg_reward /* NULL or [K] */, double* avg_steps /* NULL or [K] */);
int dqn_evaluate_many_info(dqn_group_t* g, int n_eval, int max_episode_length, int* launches /* per call -- independent of K */, int* steps_per_launch,
                           unsigned* max_lds_bytes /* the evaluation launch's dynamic LDS: the largest member's */);

/* ---- debug entries.
 * dqn_debug_devmem: the device and pinned host memory the library holds at this moment, process-wide (no handle): live blocks and their bytes, over every engine and
 * group.  Exact counters of the library's own allocations -- not what the device reports, which includes other processes.  After every handle is destroyed, and
 * after a refused dqn_engine_create, both are what they were before.  Either pointer may be NULL. */
int dqn_debug_devmem(size_t* blocks, size_t* bytes);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DQN_MI355X_H */
