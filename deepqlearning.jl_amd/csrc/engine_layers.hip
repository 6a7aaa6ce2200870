// engine_layers.hip -- host only: build_layers, the ONE gate every network passes before a kernel decodes a layer on trust (dqn_plan_default and dqn_engine_create call it).
// Per layer the driver resolves what the layer reads (LayerCtx), one function per layer family validates the descriptor and fills the geometry, lay_out_params places the
// parameters.  A rule that several families hold is stated once, as a helper that takes the words that differ; a helper returns 0 or -1 with the refusal recorded (fail).
// Refusals are pinned byte for byte, the order of the checks inside a family included (tests/test_build_layers_cpu.py; docs/history/build_layers.md).
#include "engine.h"

namespace {
// layer i = l = L[i] reads layer prev (-1: the observation): a (c, h, w) map, or a feature vector as (c, 1, 1)
struct LayerCtx { const dqn_layer_desc& d; int i; const dqn_hparams* hp; LayerDev* L; LayerDev& l; int prev, c, h, w; };
#define CHECK(rule) do { if (rule) return -1; } while (0)

// ---------------------------------------------------------------- the rules several families hold
// what the refusals call layer p, whose output is a feature vector; inner_noun: an inner layer no convolutional skip block may hold (KindTraits::a_noun has the own-level kinds)
const char* inner_noun(const LayerDev& p) { return is_recurrent(p.kind) ? "a recurrent layer" : kind_traits(p).a_noun ? kind_traits(p).a_noun : "a Dense layer"; }
const char* vec_noun(const LayerDev& p) {
    return is_actl(p.kind) ? "an Activation layer on a feature vector" : p.kind == DQN_LAYER_SKIPADD ? "the join of a skip block on a feature vector" : inner_noun(p);
}
// fmt: the subject with its verb ("MaxPool layers are")
__attribute__((format(printf, 3, 4))) int base_only(const LayerCtx& x, bool says_stream, const char* fmt, ...) {
    if (x.l.stream == DQN_STREAM_BASE) return 0;
    char subject[96], stream[32] = ""; va_list ap; va_start(ap, fmt); vsnprintf(subject, sizeof subject, fmt, ap); va_end(ap);
    if (says_stream) snprintf(stream, sizeof stream, "; stream = %d", x.l.stream);
    return fail("layer %d: %s supported in the base chain only (not in a value / advantage stream%s)", x.i, subject, stream);
}
int not_first(const LayerCtx& x, const char* noun, const char* why) { return x.prev < 0 ? fail("layer %d: %s cannot be the first layer (%s)", x.i, noun, why) : 0; }
// every kernel decodes the code on trust: an unknown one would train with some other law
int act_code(const LayerCtx& x, const char* noun, int last, const char* word = "activation", bool says_range = true) {
    if (x.d.act >= DQN_ACT_IDENTITY && x.d.act <= last) return 0;
    return says_range ? fail("layer %d: %s %s %d is not one of DQN_ACT_* (0..%d)", x.i, noun, word, x.d.act, last) : fail("layer %d: %s %s %d is not one of DQN_ACT_*", x.i, noun, word, x.d.act);
}
int no_act(const LayerCtx& x, const char* subject) {
    return x.d.act != DQN_ACT_IDENTITY ? fail("layer %d: %s has no activation (act must be DQN_ACT_IDENTITY, got %d)", x.i, subject, x.d.act) : 0;
}
// cin / cout: both 0 (taken from the incoming map) or both the incoming channel count
int channels(const LayerCtx& x, const char* noun) {
    if (!(x.d.cin || x.d.cout) || (x.d.cin == x.c && x.d.cout == x.c)) return 0;
    return fail(is_gn(x.l.kind) ? "layer %d: %s chs (cin %d / cout %d) != incoming channels %d" : "layer %d: %s cin %d / cout %d != incoming channels %d", x.i, noun, x.d.cin, x.d.cout, x.c);
}
int n_in_is_features(const LayerCtx& x, const char* noun) { return x.d.n_in != x.l.in_feat ? fail("layer %d: %s n_in %d != incoming features %d", x.i, noun, x.d.n_in, x.l.in_feat) : 0; }
int n_slots_equal(const LayerCtx& x, const char* noun, const char* carry) {
    return x.d.n_in != x.d.n_out ? fail("layer %d: %s n_in %d != n_out %d (both carry %s)", x.i, noun, x.d.n_in, x.d.n_out, carry) : 0;
}
int n_is_features(const LayerCtx& x, const char* noun, const char* whose, bool map) {
    if (x.d.n_in == x.l.in_feat) return 0;
    return map ? fail("layer %d: %s size n = %d != %s features %d * %d * %d = %d", x.i, noun, x.d.n_in, whose, x.c, x.h, x.w, x.l.in_feat)
               : fail("layer %d: %s size n = %d != %s features %d", x.i, noun, x.d.n_in, whose, x.l.in_feat);
}
// n_in == n_out == the feature count (map: spelt c * h * w), or both 0
int feature_slots(const LayerCtx& x, const char* noun, const char* whose, bool map) {
    CHECK(n_slots_equal(x, noun, map ? "the feature count c * h * w, or both 0" : "the feature count n, or both 0"));
    return x.d.n_in != 0 ? n_is_features(x, noun, whose, map) : 0;
}
enum { S_CIN = 1, S_COUT = 2, S_KH = 4, S_KW = 8, S_SH = 16, S_SW = 32, S_N_IN = 64, S_N_OUT = 128 };      // the descriptor's slots, in the order in which the refusals list them
int unused_slots(const LayerCtx& x, const char* subject, const char* uses, int unused) {
    const struct { const char* name; int v; } s[] = {{"cin", x.d.cin}, {"cout", x.d.cout}, {"kh", x.d.kh}, {"kw", x.d.kw}, {"sh", x.d.sh}, {"sw", x.d.sw}, {"n_in", x.d.n_in}, {"n_out", x.d.n_out}};
    char names[64] = "", vals[128] = ""; bool any = false;
    for (int k = 0; k < 8; k++) if ((unused >> k) & 1) {
        const char* sep = names[0] ? " / " : "";
        snprintf(names + strlen(names), sizeof names - strlen(names), "%s%s", sep, s[k].name); snprintf(vals + strlen(vals), sizeof vals - strlen(vals), "%s%d", sep, s[k].v); any = any || s[k].v;
    }
    return any ? fail("layer %d: %s uses %s only; %s = %s must be 0", x.i, subject, uses, names, vals) : 0;
}
// LayerNorm / Dropout: prev is a Dense or recurrent layer (allowed: or ...), not a standalone activation, a map or another layer of the kind
int directly_follows(const LayerCtx& x, const char* noun, const char* allowed) {
    const int p = x.L[x.prev].kind; char is[160];
    if (is_actl(p)) snprintf(is, sizeof is, "an Activation layer; a %s directly behind a standalone activation is not supported", noun);
    else if (has_map(p)) snprintf(is, sizeof is, "a %s layer, whose output is a (%d, %d, %d) map", is_gn(p) ? "GroupNorm" : "Conv / MaxPool / MeanPool", x.c, x.h, x.w);
    else if (p == x.l.kind) snprintf(is, sizeof is, "a %s layer", noun);
    else return 0;
    return fail("layer %d: %s must directly follow a %s layer (layer %d is %s)", x.i, noun, allowed, x.prev, is);
}
int eps_ok(const LayerCtx& x, const char* noun, float eps, int bits) {      // bits: the descriptor slot, 0 = the default 1f-5 (ln_eps, gn_eps)
    return (!(eps > 0.0f) || !(eps <= 3.402823466e38f)) ? fail("layer %d: %s eps = %g (bit pattern 0x%08x) must be finite and > 0", x.i, noun, (double)eps, (unsigned)bits) : 0;
}
// a parameterless layer that keeps the incoming shape (behind a feature vector h = w = 1); cin / cout are the family's
void keeps_shape(const LayerCtx& x) { LayerDev& l = x.l; l.K = l.N = 0; l.npos = 1; l.out_feat = l.in_feat; l.ih = l.oh = x.h; l.iw = l.ow = x.w; }

// ---------------------------------------------------------------- one function per layer family
// Conv: pad = (ph, pw) rides in the n_in / n_out slots (zero in every pad-0 descriptor): symmetric zero padding, at most kernel - 1 per axis (conv_own.hip)
int conv_checks(const LayerCtx& x) {
    LayerDev& l = x.l; const int i = x.i, h = x.h, w = x.w;
    CHECK(act_code(x, "Conv", DQN_ACT_LAST));
    if (l.cin != x.c) return fail("layer %d: conv cin %d != incoming channels %d", i, l.cin, x.c);
    l.ph = x.d.n_in; l.pw = x.d.n_out;
    if (l.ph < 0 || l.pw < 0) return fail("layer %d: Conv pad (%d, %d) must not be negative", i, l.ph, l.pw);
    if ((l.ph || l.pw) && (l.kh < 1 || l.kw < 1 || l.ph > l.kh - 1 || l.pw > l.kw - 1))
        return fail("layer %d: Conv pad (%d, %d) is larger than kernel - 1 = (%d, %d): a window would lie in the padding alone", i, l.ph, l.pw, l.kh - 1, l.kw - 1);
    if (l.ph || l.pw) CHECK(base_only(x, false, "Conv with pad (%d, %d) is", l.ph, l.pw));
    if ((l.ph || l.pw) && (l.sh < 1 || l.sw < 1 || l.kh > h + 2 * l.ph || l.kw > w + 2 * l.pw))
        return fail("layer %d: Conv kernel (%d, %d) / stride (%d, %d) does not fit the %dx%d input map extended by pad (%d, %d)", i, l.kh, l.kw, l.sh, l.sw, h, w, l.ph, l.pw);
    if (l.kh > h + 2 * l.ph || l.kw > w + 2 * l.pw || l.sh < 1 || l.sw < 1) return fail("layer %d: conv kernel/stride does not fit the %dx%d input", i, h, w);
    return 0;
}
// Flux Conv(...; dilation, groups) / DepthwiseConv (conv_own.hip): pad_h | pad_w << 16 rides in n_in, dh | dw << 8 | g << 16 in n_out (include/dqn_mi355x.h)
int cdg_checks(const LayerCtx& x) {
    LayerDev& l = x.l; const dqn_layer_desc& d = x.d; const int i = x.i;
    CHECK(act_code(x, "dilated / grouped Conv", DQN_ACT_LAST));
    if (d.n_in < 0 || d.n_out < 0)
        return fail("layer %d: dilated / grouped Conv: the packed slots n_in = %d (pad_h | pad_w << 16) and n_out = %d (dh | dw << 8 | groups << 16) must not be negative", i, d.n_in, d.n_out);
    l.ph = d.n_in & 0xffff; l.pw = d.n_in >> 16; l.dh = d.n_out & 0xff; l.dw = (d.n_out >> 8) & 0xff; l.groups = d.n_out >> 16;
    CHECK(base_only(x, false, "a Conv with dilation (%d, %d) / groups %d is", l.dh, l.dw, l.groups));
    if (l.dh < 1 || l.dw < 1) return fail("layer %d: Conv dilation (%d, %d) must be at least 1 per axis", i, l.dh, l.dw);
    if (l.kh < 1 || l.kw < 1 || l.sh < 1 || l.sw < 1) return fail("layer %d: dilated / grouped Conv kernel (%d, %d) / stride (%d, %d) must be positive", i, l.kh, l.kw, l.sh, l.sw);
    if (l.cin < 1 || l.cout < 1 || l.groups < 1 || l.cin % l.groups || l.cout % l.groups) return fail("layer %d: Conv groups = %d must be >= 1 and divide cin = %d and cout = %d", i, l.groups, l.cin, l.cout);
    if (l.cin != x.c) return fail("layer %d: dilated / grouped Conv cin %d != incoming channels %d", i, l.cin, x.c);
    const long long eh = (long long)(l.kh - 1) * l.dh, ew = (long long)(l.kw - 1) * l.dw;      // the dilated extent minus one, per axis
    if (l.ph > eh || l.pw > ew)
        return fail("layer %d: Conv pad (%d, %d) is larger than the dilated kernel extent - 1 = (%lld, %lld): a window would lie in the padding alone", i, l.ph, l.pw, eh, ew);
    if (eh + 1 > x.h + 2 * l.ph || ew + 1 > x.w + 2 * l.pw)
        return fail("layer %d: Conv kernel (%d, %d) with dilation (%d, %d) spans (%lld, %lld) and does not fit the %dx%d input map extended by pad (%d, %d)", i, l.kh, l.kw, l.dh, l.dw, eh + 1, ew + 1, x.h, x.w, l.ph, l.pw);
    return 0;
}
int conv_layer(const LayerCtx& x) {
    LayerDev& l = x.l; const dqn_layer_desc& d = x.d; const bool dg = is_cdg(l.kind);
    l.cin = d.cin; l.cout = d.cout; l.kh = d.kh; l.kw = d.kw; l.sh = d.sh; l.sw = d.sw;
    CHECK(dg ? cdg_checks(x) : conv_checks(x));
    // ONE geometry: a Conv is the case dilation 1, groups 1 (its dh, dw, groups stay 0).  Trailing rows / columns of the extended map no window covers are dropped
    const long long eh = (long long)(l.kh - 1) * (dg ? l.dh : 1), ew = (long long)(l.kw - 1) * (dg ? l.dw : 1);
    l.ih = x.h; l.iw = x.w; l.oh = (int)((x.h + 2 * l.ph - eh - 1) / l.sh) + 1; l.ow = (int)((x.w + 2 * l.pw - ew - 1) / l.sw) + 1;
    l.K = (l.cin / (dg ? l.groups : 1)) * l.kh * l.kw; l.N = l.cout; l.npos = l.oh * l.ow; l.out_feat = l.cout * l.npos;
    return 0;
}
// Flux MaxPool / MeanPool, pad 0 (pool.hip): per channel on the incoming (c, h, w) map; no parameters (K = N = 0), no activation.  AdaptiveMaxPool / AdaptiveMeanPool((ow, oh)),
// GlobalMaxPool / GlobalMeanPool (output (1, 1)): kh, kw carry the OUTPUT size, resolved here into a pool's window
int pool_layer(const LayerCtx& x) {
    LayerDev& l = x.l; const dqn_layer_desc& d = x.d; const int i = x.i, h = x.h, w = x.w; const bool adaptive = is_adaptive_pool(l.kind);
    const char* nm = adaptive ? (is_mean_pool(l.kind) ? "AdaptiveMeanPool" : "AdaptiveMaxPool") : is_mean_pool(l.kind) ? "MeanPool" : "MaxPool";
    CHECK(base_only(x, adaptive, "%s layers are", nm));
    if (x.prev >= 0 && !out_is_map(x.L, x.prev)) {
        if (adaptive) return fail("layer %d: %s must be the first layer or follow a layer whose output is a (c, h, w) map (layer %d is %s, whose output is a feature vector of %d)",
                                  i, nm, x.prev, vec_noun(x.L[x.prev]), x.L[x.prev].out_feat);
        return fail("layer %d: %s must be the first layer or follow a Conv / MaxPool / MeanPool layer (it follows a Dense or recurrent layer, whose output is no (c, h, w) map)", i, nm);
    }
    CHECK(no_act(x, nm));
    CHECK(channels(x, nm));
    if (adaptive) {
        CHECK(unused_slots(x, nm, "cin, cout, kh and kw (the OUTPUT size (oh, ow))", S_SH | S_SW | S_N_IN | S_N_OUT));
        if (d.kh < 1 || d.kw < 1) return fail("layer %d: %s output size (%d, %d) must be at least (1, 1)", i, nm, d.kh, d.kw);
        if (d.kh > h || d.kw > w) return fail("layer %d: %s output size (%d, %d) is larger than the %dx%d input map (the adaptive rule needs 1 <= out <= in per axis)", i, nm, d.kh, d.kw, h, w);
        // Flux's rule per axis (NOT torch's adaptive windows): stride = in / out, k = in - (out - 1) * stride, pad 0; then (in - k) / stride + 1 == out
        l.sh = h / d.kh; l.sw = w / d.kw; l.kh = h - (d.kh - 1) * l.sh; l.kw = w - (d.kw - 1) * l.sw;
    } else {
        if (d.sh < 1 || d.sw < 1) return fail("layer %d: %s stride (%d, %d) must be positive", i, nm, d.sh, d.sw);
        if (d.kh < 1 || d.kw < 1 || d.kh > h || d.kw > w) return fail("layer %d: %s window (%d, %d) does not fit the %dx%d input map", i, nm, d.kh, d.kw, h, w);
        l.kh = d.kh; l.kw = d.kw; l.sh = d.sh; l.sw = d.sw;
    }
    l.cin = l.cout = x.c; l.ih = h; l.iw = w; l.oh = (h - l.kh) / l.sh + 1; l.ow = (w - l.kw) / l.sw + 1;      // trailing rows / columns no window covers are dropped
    l.K = 0; l.N = 0; l.npos = l.oh * l.ow; l.out_feat = l.cout * l.npos;
    return 0;
}
// Flux LayerNorm(n, act; affine = true, eps) (layernorm.hip): per column over the n incoming features; K = N = n, parameters scale (n), bias (n)
int layernorm_layer(const LayerCtx& x) {
    LayerDev& l = x.l; const dqn_layer_desc& d = x.d;
    CHECK(not_first(x, "LayerNorm", "it must directly follow a Dense or recurrent layer"));
    CHECK(base_only(x, true, "LayerNorm layers are"));
    CHECK(directly_follows(x, "LayerNorm", "Dense or recurrent"));
    CHECK(n_slots_equal(x, "LayerNorm", "the size n"));
    if (d.n_out < 2) return fail("layer %d: LayerNorm size n = %d must be >= 2 (over one feature sigma is identically 0 and the gradient is NaN)", x.i, d.n_out);
    CHECK(n_is_features(x, "LayerNorm", "incoming", false));
    CHECK(act_code(x, "LayerNorm", DQN_ACT_LAST));
    CHECK(unused_slots(x, "LayerNorm", "n_in, n_out, act and cin (the bit pattern of eps)", S_COUT | S_KH | S_KW | S_SH | S_SW));
    l.cin = d.cin;      // the fp32 bit pattern of eps
    CHECK(eps_ok(x, "LayerNorm", ln_eps(l), d.cin));
    l.K = l.N = d.n_out; l.npos = 1; l.out_feat = l.N; l.ih = l.iw = l.oh = l.ow = 1;
    return 0;
}
// Flux GroupNorm(chs, G, act; eps) (groupnorm.hip): per column and group of c / G contiguous channels of the incoming (c, h, w) map, which it keeps; K = N = c, parameters beta (c), gamma (c)
int groupnorm_layer(const LayerCtx& x) {
    LayerDev& l = x.l; const dqn_layer_desc& d = x.d; const int i = x.i, c = x.c, h = x.h, w = x.w;
    CHECK(not_first(x, "GroupNorm", "normalising the observation is not supported; it must directly follow a Conv, MaxPool / MeanPool or GroupNorm layer or a convolutional skip block"));
    CHECK(base_only(x, true, "GroupNorm layers are"));
    if (!out_is_map(x.L, x.prev))
        return fail("layer %d: GroupNorm must directly follow a Conv, MaxPool / MeanPool or GroupNorm layer or a convolutional skip block (layer %d is %s, whose output is no (c, h, w) map)",
                    i, x.prev, vec_noun(x.L[x.prev]));
    CHECK(act_code(x, "GroupNorm", DQN_ACT_LAST));
    CHECK(channels(x, "GroupNorm"));
    CHECK(feature_slots(x, "GroupNorm", "incoming", true));
    CHECK(unused_slots(x, "GroupNorm", "cin, cout, kh (the group count G), kw (the bit pattern of eps), n_in, n_out and act", S_SH | S_SW));
    if (d.kh < 1 || c % d.kh) return fail("layer %d: GroupNorm G = %d must be >= 1 and divide the channel count %d", i, d.kh, c);
    if ((long long)(c / d.kh) * h * w < 2)
        return fail("layer %d: GroupNorm(%d, %d) on a (%d, %d, %d) map normalises over n_g = %d element (n_g must be >= 2: over one element the variance is identically 0 and the output is constant)",
                    i, c, d.kh, c, h, w, (c / d.kh) * h * w);
    l.cin = l.cout = c; l.kh = d.kh; l.kw = d.kw;      // G, and the fp32 bit pattern of eps
    CHECK(eps_ok(x, "GroupNorm", gn_eps(l), d.kw));
    l.ih = l.oh = h; l.iw = l.ow = w; l.K = l.N = c; l.npos = h * w; l.out_feat = l.in_feat;
    return 0;
}
// Flux Dropout(p), dims = : (dropout.hip): per element of the n incoming features; no parameters, p's Float64 bits in (cin, cout)
int dropout_layer(const LayerCtx& x) {
    LayerDev& l = x.l; const dqn_layer_desc& d = x.d;
    CHECK(not_first(x, "Dropout", "it must directly follow a Dense, recurrent or LayerNorm layer; dropout on the observation is not supported"));
    CHECK(base_only(x, true, "Dropout layers are"));
    CHECK(directly_follows(x, "Dropout", "Dense, recurrent or LayerNorm"));
    CHECK(no_act(x, "Dropout"));
    CHECK(feature_slots(x, "Dropout", "incoming", false));
    CHECK(unused_slots(x, "Dropout", "n_in, n_out, cin and cout (the Float64 bit pattern of p)", S_KH | S_KW | S_SH | S_SW));
    l.cin = d.cin; l.cout = d.cout;      // the Float64 bit pattern of p, low word then high word (do_p)
    const double p = do_p(l);
    if (!(p >= 0.0) || !(p < 1.0))
        return fail("layer %d: Dropout p = %g (bit pattern 0x%08x%08x) must be finite with 0 <= p < 1%s", x.i, p, (unsigned)d.cout, (unsigned)d.cin, p == 1.0 ? " (p = 1 drops every feature: Q would be constant)" : "");
    keeps_shape(x);
    return 0;
}
// inner layer j of a skip block (bs: what the refusals call the block): a map block holds Convs with pad != 0 only, a block on a feature vector Dense, LayerNorm and Dropout layers
int skip_inner(const LayerCtx& x, int j, bool map, const char* bs, int m) {
    const LayerDev& in = x.L[j]; const int k = in.kind, i = x.i;
    if (in.stream != DQN_STREAM_BASE) return fail("layer %d: the %s's inner layer %d is not in the base chain (stream = %d)", i, bs, j, in.stream);
    if (is_skip(k)) return fail("layer %d: the %s's %d inner layers reach across the join of another skip block (layer %d); nested skip blocks are not supported", i, bs, m, j);
    char holds[80] = "", more[40] = ""; const char *only = map ? "Conv layers with pad != 0" : "Dense, LayerNorm and Dropout layers", *note = "";
    if (is_actl(k)) { snprintf(holds, sizeof holds, "an Activation layer"); note = " (a standalone activation inside a skip block is not supported)"; }
    else if (is_cdg(k)) {
        snprintf(holds, sizeof holds, "a Conv with dilation (%d, %d) / groups %d", in.dh, in.dw, in.groups); note = " (dilated and grouped residual blocks are not supported)";
        if (map) only = "Conv layers with pad != 0, dilation 1 and groups 1";
    } else if (map) {
        if (is_pool(k)) snprintf(holds, sizeof holds, "a MaxPool / MeanPool layer");
        else if (k != DQN_LAYER_CONV) snprintf(holds, sizeof holds, "%s", inner_noun(in));
        else if (!is_padded(in)) { snprintf(holds, sizeof holds, "a Conv with pad 0"); snprintf(more, sizeof more, ", kernel (%d, %d)", in.kh, in.kw); }
    } else if (is_recurrent(k)) snprintf(holds, sizeof holds, "a recurrent layer");
    else if (is_gn(k)) { snprintf(holds, sizeof holds, "a GroupNorm layer"); note = " (GroupNorm inside a skip block is not supported)"; }
    else if (has_map(k)) { snprintf(holds, sizeof holds, "a Conv / MaxPool / MeanPool layer"); note = " (convolutional residual blocks are not supported)"; }
    return holds[0] ? fail("layer %d: the %s holds %s (layer %d%s); its inner layers are %s only%s", i, bs, holds, j, more, only, note) : 0;
}
// the join of a Flux SkipConnection(layers, +) block (skip.hip): y = y_K + y_P; cin = m, the number of inner layers (the m descriptors in front); src = K, src2 = P.
// map: the join of a CONVOLUTIONAL block, the same law on a (c, h, w) map; entry = a Conv / pool / map join
int skip_layer(const LayerCtx& x) {
    LayerDev& l = x.l; const dqn_layer_desc& d = x.d; LayerDev* L = x.L; const int i = x.i, m = d.cin, prev = x.prev; const bool map = is_skip_map(l.kind);
    const char* bs = map ? "convolutional skip block" : "skip block"; char join[48]; snprintf(join, sizeof join, "a %s's join", bs);
    CHECK(base_only(x, true, "a %s is", bs));
    CHECK(no_act(x, join));
    if (m < 1) return fail("layer %d: a %s holds at least one inner layer (cin = m = %d must be >= 1)", i, bs, m);
    CHECK(unused_slots(x, join, "n_in, n_out and cin (the number of inner layers)", S_COUT | S_KH | S_KW | S_SH | S_SW));
    if (m > i) return fail("layer %d: the %s's %d inner layers would start before the first layer (the block cannot be the first layer: its input is never the observation)", i, bs, m);
    for (int j = i - m; j < i; j++) CHECK(skip_inner(x, j, map, bs, m));
    const int pp = L[i - m].src;      // the block's entry P: what the first inner layer reads
    if (pp < 0) return fail("layer %d: the %s's first inner layer (layer %d) reads the observation; a skip block cannot be the first layer (its input must be %s)", i, bs, i - m,
                            map ? "the map of a Conv, MaxPool or MeanPool layer or of another convolutional skip block" : "the output of a Dense, recurrent, LayerNorm or Dropout layer or of another skip block");
    if (map) {
        if (!out_is_map(L, pp))
            return fail("layer %d: the convolutional skip block's input is the feature vector of layer %d (%s); a convolutional skip block stands on the (c, h, w) map of a Conv, MaxPool or MeanPool layer or of another convolutional skip block",
                        i, pp, vec_noun(L[pp]));
        if (L[prev].cout != L[pp].cout || L[prev].oh != L[pp].oh || L[prev].ow != L[pp].ow)
            return fail("layer %d: the convolutional skip block maps a (%d, %d, %d) map to a (%d, %d, %d) map; SkipConnection(layers, +) needs layers: (c, h, w) -> (c, h, w)", i, L[pp].cout, L[pp].oh, L[pp].ow, L[prev].cout, L[prev].oh, L[prev].ow);
    } else {
        if (is_gn(L[pp].kind)) return fail("layer %d: the skip block's input is the (c, h, w) map of layer %d (a GroupNorm layer); a skip block stands on a feature vector", i, pp);
        if (out_is_map(L, pp))
            return fail("layer %d: the skip block's input is the (c, h, w) map of layer %d (a Conv / MaxPool / MeanPool layer); a skip block stands on a feature vector (convolutional residual blocks are not supported)", i, pp);
        if (L[prev].out_feat != L[pp].out_feat) return fail("layer %d: the skip block maps %d features to %d; SkipConnection(layers, +) needs layers: n -> n", i, L[pp].out_feat, L[prev].out_feat);
    }
    CHECK(feature_slots(x, bs, "the block's", map));
    l.cin = m; l.src2 = pp; if (map) l.cout = x.c;      // (cin is m, NOT the channel count: the layer behind a map join reads cout, oh, ow)
    keeps_shape(x);
    return 0;
}
// the standalone activation layer (act_layer.hip): y = σ(x) per element on whatever the layer in front yields -- a feature vector or a (c, h, w) map, kept; no parameters
int activation_layer(const LayerCtx& x) {
    LayerDev& l = x.l;
    CHECK(not_first(x, "an Activation layer", "its input is the stored output of the layer in front; an activation on the observation is not supported"));
    CHECK(base_only(x, true, "Activation layers are"));
    CHECK(act_code(x, "Activation", DQN_ACT_LAYER_LAST, "code"));
    CHECK(feature_slots(x, "Activation", "incoming", false));
    CHECK(unused_slots(x, "Activation", "act, n_in and n_out", S_CIN | S_COUT | S_KH | S_KW | S_SH | S_SW));
    l.cell_act = x.d.act; l.act = DQN_ACT_IDENTITY;      // σ, and what the generic epilogues read (common.h)
    l.cin = l.cout = x.c;      // behind a map: the map, for the layer behind it (out_is_map); behind a feature vector: (n, 1, 1)
    keeps_shape(x);
    return 0;
}
int dense_layer(const LayerCtx& x) {
    LayerDev& l = x.l;
    CHECK(act_code(x, "Dense", DQN_ACT_LAST));
    CHECK(n_in_is_features(x, "dense"));
    l.K = x.d.n_in; l.N = x.d.n_out; l.npos = 1; l.out_feat = l.N; l.ih = l.iw = l.oh = l.ow = 1;
    return 0;
}
// the cell's activation (CellOps::has_act) goes to cell_act, never to act (the cell's kernels apply it); an RNN cell's σ is one of the first four codes: cell.h states the
// cell's arithmetic on its own, and the codes above DQN_ACT_SIGMOID are Dense / Conv / LayerNorm epilogues only
int recurrent_layer(const LayerCtx& x) {
    LayerDev& l = x.l; const CellOps* C = cell_ops(l.kind);
    if (!x.hp->recurrence) return fail("DeepQLearningError: you passed in a recurrent model but recurrence is set to false");   // src/solver.jl:45-47
    if (l.stream != DQN_STREAM_BASE) return fail("%s layers are supported in the base chain only", C->display);      // (no layer index: not base_only's sentence)
    CHECK(n_in_is_features(x, C->display));
    if (C->has_act) CHECK(act_code(x, C->display, DQN_ACT_SIGMOID, "activation", false));
    l.H = x.d.n_out; l.K = x.d.n_in; l.N = C->ngates * l.H; l.npos = 1; l.out_feat = l.H; if (C->has_act) l.cell_act = x.d.act; l.act = DQN_ACT_IDENTITY; l.ih = l.iw = l.oh = l.ow = 1;
    return 0;
}
int layer_family(const LayerCtx& x) {
    const int k = x.l.kind;
    return is_conv_kind(k) ? conv_layer(x) : is_pool(k) ? pool_layer(x) : is_ln(k) ? layernorm_layer(x) : is_gn(k) ? groupnorm_layer(x) : is_do(k) ? dropout_layer(x) : is_skip(k) ? skip_layer(x)
         : is_actl(k) ? activation_layer(x) : k == DQN_LAYER_DENSE ? dense_layer(x) : is_recurrent(k) ? recurrent_layer(x) : fail("layer %d: unknown kind %d", x.i, k);
}
// where the layer's parameters lie in the external (Flux.params order) and the internal (16-B aligned arrays) vector
void lay_out_params(LayerDev& l, size_t& off, size_t& eoff) {
    if (is_recurrent(l.kind)) {      // Flux.params Wi, Wh, b, h0(, c0) -> internal [Wi][b][Wh][junk][h0]([c0])[zeros]
        const bool has_c = cell_ops(l.kind)->has_c;
        const size_t kn = (size_t)l.K * l.N, hn = (size_t)l.H * l.N;
        l.ew_off = eoff; eoff += kn; l.ewh_off = eoff; eoff += hn; l.eb_off = eoff; eoff += l.N; l.eh0_off = eoff; eoff += l.H; if (has_c) { l.ec0_off = eoff; eoff += l.H; }
        off = (off + 3) / 4 * 4; l.w_off = off; off += kn; l.b_off = off; off += l.N; l.wh_off = off; off += hn; off += l.N /* junk bias row of the Wh dW pass */;
        l.h0_off = off; off += l.H; if (has_c) { l.c0_off = off; off += l.H; } off = (off + 3) / 4 * 4; l.z_off = off; off += l.N;
    } else {
        const size_t wn = layer_wn(l);      // K * N weights; a LayerNorm's scale vector (N)
        if (is_gn(l.kind)) { l.eb_off = eoff; eoff += l.N; l.ew_off = eoff; eoff += wn; }      // Flux.params of a GroupNorm: beta, THEN gamma
        else { l.ew_off = eoff; eoff += wn; l.eb_off = eoff; eoff += l.N; }
        off = (off + 3) / 4 * 4; l.w_off = off; off += wn; l.b_off = off; off += l.N;
    }
}
// the network's ends against the hyperparameters: a dueling network has both streams, 1 value and n_actions advantages
int check_ends(const dqn_hparams* hp, const LayerDev* L, int lb, int lv, int la) {
    if (hp->dueling) {
        if (lv < 0 || la < 0 || L[lv].out_feat != 1 || L[la].out_feat != hp->n_actions) return fail("DeepQLearningError: the qnetwork provided is incompatible with dueling");   // src/dueling.jl:47
    } else if (lb < 0 || L[lb].out_feat != hp->n_actions) return fail("network output size != n_actions");
    if (!hp->dueling && !kind_traits(L[lb]).output_ok) return fail("layer %d: %s cannot be the network's output layer", lb, kind_traits(L[lb]).a_noun);
    if (hp->n_actions > DQN_MAX_ACTIONS) return fail("n_actions > %d unsupported", DQN_MAX_ACTIONS);
    return 0;
}
}      // namespace

int build_layers(const dqn_layer_desc* d, int n, const dqn_hparams* hp, LayerDev* L, int* lb, int* lv, int* la, size_t* P, size_t* Pint) {
    if (n <= 0 || n > DQN_MAX_LAYERS) return fail("bad layer count %d", n);
    *lb = *lv = *la = -1; size_t off = 0, eoff = 0;
    for (int i = 0; i < n; i++) {
        LayerDev& l = L[i]; memset(&l, 0, sizeof l);
        l.kind = d[i].kind; l.act = d[i].act; l.stream = d[i].stream; l.src2 = -1;
        int* const last = l.stream == DQN_STREAM_BASE ? lb : l.stream == DQN_STREAM_VAL ? lv : la;      // the last layer of this layer's stream so far; a stream starts on the base chain
        const int prev = *last >= 0 ? *last : *lb;
        l.src = prev;
        int c, h, w;
        if (prev < 0) { c = hp->obs_c; h = hp->obs_h; w = hp->obs_w; }
        else if (out_is_map(L, prev)) { c = L[prev].cout; h = L[prev].oh; w = L[prev].ow; }
        else { c = L[prev].out_feat; h = 1; w = 1; }
        l.in_feat = c * h * w;
        CHECK(layer_family({d[i], i, hp, L, l, prev, c, h, w}));
        lay_out_params(l, off, eoff);
        *last = i;
    }
    *P = eoff; *Pint = (off + 3) / 4 * 4;
    return check_ends(hp, L, *lb, *lv, *la);
}
