// conv_own.hip -- the convolutions launched alone on their level: Conv((kh, kw), cin => cout, act; stride, pad = (ph, pw)) with SYMMETRIC ZERO PADDING (layer kind 1 with
// pad != 0; template parameter DG = 0) and Conv(...; dilation = (dh, dw), groups = g) / DepthwiseConv (groups = cin) (layer kind DQN_LAYER_CONV_DG; DG = 1).  Forward, dX and
// dW / db as implicit GEMMs whose operand loads carry the border as a predicate: the tap
//     iy = oy * sh + ky * dh - ph,   ix = ox * sw + kx * dw - pw     in [0, ih) x [0, iw), else the operand is an exact 0
// -- no zero-bordered scratch map, no crop -- and a per-group K range: output channel n belongs to group j = n / (cout / g) and reads input channels [j * cin/g, (j + 1) * cin/g).
// The CONV_* macros below state these three expressions (tap, channel base, group width) ONCE; DG = 0 makes them the literals 1, 0 and the full channel counts and reads none
// of LayerDev's dh / dw / groups, which are 0 on a kind-1 layer.  One body per contraction serves both kinds.
//
// Canonical order ("Padded convolutions" and "Dilated and grouped convolutions"): a padded conv IS the pad-0 conv of nn_valu.hip / nn_mfma.hip /
// nn_gemm.hip on the zero-extended map, under the same dqn_layer_plan; a kind-15 layer IS that padded conv with the layer's own kernel zero-stuffed to
// ((kh - 1) dh + 1, (kw - 1) dw + 1) and zero outside the group's diagonal block, of which only the LIVE terms are chained:
//   forward   per plan chunk (fwd_kc, on the layer's own K = (cin/g) kh kw) one k = (ci within the group, ky, kx)-ascending fmaf chain from +0; chunk sums added in ascending
//             order, + bias, activation
//   dW / db   per live weight and plan chunk (dw_kc) one (position, sample)-ascending chain; oh*ow is the layer's own; slabs [S][(K+1)][N] are summed by the step's reduce /
//             Adam launch
//   dX        per input element, per chunk of RAW taps (dx_kc) one chain over the VALID taps -- (iy + ph - ky * dh) divisible by sh with quotient in [0, oh), likewise x: the
//             interior crop of the extended map's dX -- with co (within the group) innermost; then the producing layer's activation derivative
// The VALU and thin kernels SKIP an out-of-range tap, the MFMA kernels multiply by the exact zero: the same bits, because a skipped term == the term times an exact zero -- a
// chain that starts at +0 never holds -0 under round-to-nearest, so fma(0, w, acc) == acc for every finite w.  For the same reason a kind-15 layer equals the kind-1 network on
// the expanded kernel bit for bit under unsplit plan entries (tests/test_conv_dg_gpu.py).
//
// Forms of each contraction, bit-identical:
//   MFMA   fp32 v_mfma_f32_16x16x4_f32, one wave = one register tile, operands straight from L2 as in nn_mfma.hip: where cout/g (forward, dW), cin/g (dX) and the columns
//          tile by 16
//   thin   kind 15 only, cin/g == 1 (depthwise) or K < 16: NOT an implicit GEMM padded to tiles -- pool.hip's work split, a thread owns (one output feature [forward] or input
//          feature [dX], four adjacent columns); one 16-byte access where leading dimension, column offset and count are multiples of 4, one column at a time otherwise.  No
//          LDS, no atomics, plain vector stores; the dX is a gather per input element over its valid taps; dW / db one thread per (chunk, weight), the rows of a channel in
//          neighbouring lanes.  Taken whatever use_mfma says
//   VALU   one thread per output element: every other shape
// A first-layer conv may read the BYTE arena of a u8 replay (xu8): value = u8_unit(byte), and a zero byte is an exact 0.
//
// Residual epilogues (the join of a convolutional skip block, DQN_LAYER_SKIPADD_MAP; DESIGN.md section 4 "Convolutional skip blocks"), template parameter RES / ADD, DG = 0
// only (build_layers refuses a dilated / grouped conv inside a block):
//   forward   Y = act(tot + bias) + R        R = the stored output of the block's entry P on this pass's columns ([out_feat][ldr], window rcol0): the block's LAST inner
//                                            layer writes the JOIN's activation; one fp32 add behind the activation, the add skip.hip's k_skip_fwd makes in a launch of its own
//   dX        out = dact(acc + dY, y_P, act_P)   dY = dact[join] ([in_feat][B]): the block's FIRST inner layer writes dact[P]; the add and the derivative k_skip_bwd_entry makes
// The same operands in the same order as the separate launches, hence the same bits.  The addend comes straight from global memory (no LDS, no atomics); its loads are issued
// together, before the first use: in front of the contraction where that costs one register (VALU forms), at the head of the epilogue where it would cost a register tile
// held across the whole MFMA loop (MT x NT x 4 VGPRs).  RES = ADD = 0 compiles to the kernels without the operand: a conv outside a block keeps its code and its bits.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// The geometry of the two kinds, stated once (dg: the compile-time DG).  tap_y / tap_x: the row / column offset of tap ky / kx; the group width in output and in input
// channels; the first input channel of output channel n's group; the group of input channel ci.  Macros, not functions: only the live arm of `dg ? :` is compiled, so a
// DG = 0 kernel holds no load of dh / dw / groups and no division -- and a helper that took L by reference would keep the kernel's LayerDev in memory through the
// compiler's first scalar-replacement pass, which moves the dW and dX kernels' code (docs/history/conv_own.md)
#define CONV_TAP_Y(dg, L, ky) ((dg) ? (ky) * (L).dh : (ky))
#define CONV_TAP_X(dg, L, kx) ((dg) ? (kx) * (L).dw : (kx))
#define CONV_OUTS_PER_GROUP(dg, L) ((dg) ? (L).N / (L).groups : (L).N)
#define CONV_INS_PER_GROUP(dg, L) ((dg) ? (L).cin / (L).groups : (L).cin)
#define CONV_CHAN_BASE_OF_OUT(dg, L, n) ((dg) ? ((n) / CONV_OUTS_PER_GROUP(dg, L)) * CONV_INS_PER_GROUP(dg, L) : 0)
#define CONV_GROUP_OF_IN(dg, L, ci) ((dg) ? (ci) / CONV_INS_PER_GROUP(dg, L) : 0)

// the operand X[(ci, iy, ix)][col] of the UNPADDED map, float or byte arena
template <int U8> __device__ __forceinline__ float ld_x(const void* __restrict__ X, size_t i) {
    if (U8) return u8_unit(reinterpret_cast<const unsigned char*>(X)[i]);
    return reinterpret_cast<const float*>(X)[i];
}

// ------------------------------------------------------------------ VALU: one thread per output element
template <int U8, int RES, int DG>
__global__ __launch_bounds__(256) void k_conv_fwd(LayerDev L, const float* __restrict__ P, const void* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y,
                                                  const float* __restrict__ R, int ldr, int rcol0) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)L.N * L.npos * ncols) return;
    const int col = (int)(t % ncols); const int pos = (int)((t / ncols) % L.npos); const int n = (int)(t / ((size_t)ncols * L.npos));
    const int oy = pos / L.ow, ox = pos % L.ow; const int y0 = oy * L.sh - L.ph, x0 = ox * L.sw - L.pw;
    const int cb = CONV_CHAN_BASE_OF_OUT(DG, L, n);
    const float* W = P + L.w_off;
    const int S = dqn_nchunks(L.K, L.fwd_kc), kc = dqn_chunk_len(L.K, L.fwd_kc), khw = L.kh * L.kw;
    float res = 0.0f; if (RES) res = R[((size_t)n * L.npos + pos) * ldr + rcol0 + col];      // in flight under the contraction
    float tot = 0.0f;
    for (int s = 0; s < S; s++) {
        const int k0 = s * kc, k1 = min(L.K, k0 + kc);
        int ci = k0 / khw, ky = (k0 / L.kw) % L.kh, kx = k0 % L.kw;
        float acc = 0.0f;
        for (int k = k0; k < k1; k++) {
            const int iy = y0 + CONV_TAP_Y(DG, L, ky), ix = x0 + CONV_TAP_X(DG, L, kx);
            if (iy >= 0 && iy < L.ih && ix >= 0 && ix < L.iw)
                acc = fmaf(ld_x<U8>(X, (size_t)(((cb + ci) * L.ih + iy) * L.iw + ix) * ldx + col0 + col), W[(size_t)k * L.N + n], acc);
            if (++kx == L.kw) { kx = 0; if (++ky == L.kh) { ky = 0; ++ci; } }
        }
        tot = s == 0 ? acc : tot + acc;
    }
    const float y = act_f(tot + P[L.b_off + n], L.act);
    Y[t] = RES ? y + res : y;
}

// thread = (chunk, k, n) for k < K, plus the virtual row k == K of the bias gradient; out = slabs [S][(K+1)][N] (S == 1: the gradient block itself)
template <int U8, int DG>
__global__ __launch_bounds__(256) void k_conv_dw(LayerDev L, const void* __restrict__ X, int ldx, const float* __restrict__ dpre, int B, int S, int kc, float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per_s = (size_t)(L.K + 1) * L.N;
    if (t >= per_s * S) return;
    const int s = (int)(t / per_s); const size_t e = t % per_s;
    const int n = (int)(e % L.N), k = (int)(e / L.N);
    const int KK = L.npos * B, j0 = s * kc, j1 = min(KK, j0 + kc);
    const int khw = L.kh * L.kw; const int ci = CONV_CHAN_BASE_OF_OUT(DG, L, n) + k / khw, ky = (k / L.kw) % L.kh, kx = k % L.kw;      // (unused for the bias row)
    float acc = 0.0f;
    int pos = j0 / B, b = j0 % B;
    for (int j = j0; j < j1; j++) {
        const float d = dpre[((size_t)n * L.npos + pos) * B + b];
        if (k < L.K) {
            const int oy = pos / L.ow, ox = pos % L.ow; const int iy = oy * L.sh + CONV_TAP_Y(DG, L, ky) - L.ph, ix = ox * L.sw + CONV_TAP_X(DG, L, kx) - L.pw;
            if (iy >= 0 && iy < L.ih && ix >= 0 && ix < L.iw) acc = fmaf(ld_x<U8>(X, (size_t)((ci * L.ih + iy) * L.iw + ix) * ldx + b), d, acc);
        } else acc = acc + d;
        if (++b == B) { b = 0; ++pos; }
    }
    out[(size_t)s * per_s + e] = acc;
}

// the co loop runs over the outs_per_group output channels of the input channel's group.  ADD: dY is the join's gradient.  With a single inner layer it IS the buffer dpre
// points at: both are only read, which __restrict__ allows
template <int ADD, int DG>
__global__ __launch_bounds__(256) void k_conv_dx(LayerDev L, const float* __restrict__ P, const float* __restrict__ dpre, int B, float* __restrict__ out,
                                                 const float* __restrict__ ysrc, int ldy, int act_src, const float* __restrict__ dY) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)L.in_feat * B) return;
    float add = 0.0f; if (ADD) add = dY[e];      // in flight under the contraction
    const int b = (int)(e % B); const int feat = (int)(e / B);
    const float* W = P + L.w_off;
    const int hw = L.ih * L.iw; const int ci = feat / hw, iy = (feat % hw) / L.iw, ix = feat % L.iw;
    const int cg = CONV_INS_PER_GROUP(DG, L), ng = CONV_OUTS_PER_GROUP(DG, L); const int j = CONV_GROUP_OF_IN(DG, L, ci), cil = ci - j * cg, co0 = j * ng;      // the group's first output channel
    const int tc = DQN_CONV_TAP_CHUNK(L); int cur = -1; bool have = false; float tot = 0.0f, acc = 0.0f;
    for (int ky = 0; ky < L.kh; ky++) {
        const int ty = iy + L.ph - CONV_TAP_Y(DG, L, ky); if (ty < 0 || ty % L.sh) continue; const int oy = ty / L.sh; if (oy >= L.oh) continue;
        for (int kx = 0; kx < L.kw; kx++) {
            const int tx = ix + L.pw - CONV_TAP_X(DG, L, kx); if (tx < 0 || tx % L.sw) continue; const int ox = tx / L.sw; if (ox >= L.ow) continue;
            const int cid = (ky * L.kw + kx) / tc;
            if (cid != cur) { if (cur >= 0) { tot = have ? tot + acc : acc; have = true; acc = 0.0f; } cur = cid; }
            const float* wr = W + (size_t)((cil * L.kh + ky) * L.kw + kx) * L.N + co0; const int pos = oy * L.ow + ox;
            for (int co = 0; co < ng; co++) acc = fmaf(dpre[((size_t)(co0 + co) * L.npos + pos) * B + b], wr[co], acc);
        }
    }
    if (have) acc = tot + acc;
    if (ADD) acc = acc + add;
    if (ysrc) acc = dact_f(acc, ysrc[(size_t)feat * ldy + b], act_src);
    out[e] = acc;
}

// ------------------------------------------------------------------ thin groups (kind 15 only): a thread owns (feature, four adjacent columns); VEC: the four columns are one 16-byte access
template <int U8, int VEC>
__global__ __launch_bounds__(256) void k_cdg_thin_fwd(LayerDev L, const float* __restrict__ P, const void* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y) {
    const int nq = (ncols + 3) >> 2;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t f = t / nq; const int c0 = (int)(t - f * nq) * 4;
    if (f >= (size_t)L.N * L.npos) return;
    const int n = (int)(f / L.npos), pos = (int)(f - (size_t)n * L.npos);
    const int oy = pos / L.ow, ox = pos - oy * L.ow; const int y0 = oy * L.sh - L.ph, x0 = ox * L.sw - L.pw;
    const int cb = CONV_CHAN_BASE_OF_OUT(1, L, n);
    const float* W = P + L.w_off + n;
    const int nj = VEC ? 4 : min(4, ncols - c0);
    const int S = dqn_nchunks(L.K, L.fwd_kc), kc = dqn_chunk_len(L.K, L.fwd_kc), khw = L.kh * L.kw;
    float tot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = 0; s < S; s++) {
        const int k0 = s * kc, k1 = min(L.K, k0 + kc);
        int ci = k0 / khw, ky = (k0 / L.kw) % L.kh, kx = k0 % L.kw;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = k0; k < k1; k++) {
            const int iy = y0 + CONV_TAP_Y(1, L, ky), ix = x0 + CONV_TAP_X(1, L, kx);
            if (iy >= 0 && iy < L.ih && ix >= 0 && ix < L.iw) {
                const float w = W[(size_t)k * L.N];
                const size_t xi = (size_t)(((cb + ci) * L.ih + iy) * L.iw + ix) * ldx + col0 + c0;
                if (VEC) {
                    float x[4];
                    if (U8) { const uchar4 v = *reinterpret_cast<const uchar4*>(reinterpret_cast<const unsigned char*>(X) + xi); x[0] = u8_unit(v.x); x[1] = u8_unit(v.y); x[2] = u8_unit(v.z); x[3] = u8_unit(v.w); }
                    else { const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(X) + xi); x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[j] = fmaf(x[j], w, acc[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) if (j < nj) acc[j] = fmaf(ld_x<U8>(X, xi + j), w, acc[j]);
                }
            }
            if (++kx == L.kw) { kx = 0; if (++ky == L.kh) { ky = 0; ++ci; } }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) tot[j] = s == 0 ? acc[j] : tot[j] + acc[j];
    }
    const float bias = P[L.b_off + n];
    float* yb = Y + f * ncols + c0;
    if (VEC) { float4 v; v.x = act_f(tot[0] + bias, L.act); v.y = act_f(tot[1] + bias, L.act); v.z = act_f(tot[2] + bias, L.act); v.w = act_f(tot[3] + bias, L.act); *reinterpret_cast<float4*>(yb) = v; }
    else {
#pragma unroll
        for (int j = 0; j < 4; j++) if (j < nj) yb[j] = act_f(tot[j] + bias, L.act);
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void k_cdg_thin_dx(LayerDev L, const float* __restrict__ P, const float* __restrict__ dpre, int B, float* __restrict__ out,
                                                     const float* __restrict__ ysrc, int ldy, int act_src) {
    const int nq = (B + 3) >> 2;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t feat = t / nq; const int c0 = (int)(t - feat * nq) * 4;
    if (feat >= (size_t)L.in_feat) return;
    const int hw = L.ih * L.iw; const int ci = (int)(feat / hw), ip = (int)(feat - (size_t)ci * hw), iy = ip / L.iw, ix = ip - iy * L.iw;
    const int cg = CONV_INS_PER_GROUP(1, L), ng = CONV_OUTS_PER_GROUP(1, L); const int j = CONV_GROUP_OF_IN(1, L, ci), cil = ci - j * cg;
    const float* W = P + L.w_off + (size_t)j * ng;
    const float* dp = dpre + (size_t)j * ng * L.npos * B + c0;
    const int nj = VEC ? 4 : min(4, B - c0);
    const int tc = DQN_CONV_TAP_CHUNK(L); int cur = -1; bool have = false;
    float tot[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ky = 0; ky < L.kh; ky++) {
        const int ty = iy + L.ph - CONV_TAP_Y(1, L, ky); if (ty < 0 || ty % L.sh) continue; const int oy = ty / L.sh; if (oy >= L.oh) continue;
        for (int kx = 0; kx < L.kw; kx++) {
            const int tx = ix + L.pw - CONV_TAP_X(1, L, kx); if (tx < 0 || tx % L.sw) continue; const int ox = tx / L.sw; if (ox >= L.ow) continue;
            const int cid = (ky * L.kw + kx) / tc;
            if (cid != cur) {
                if (cur >= 0) {
#pragma unroll
                    for (int q = 0; q < 4; q++) { tot[q] = have ? tot[q] + acc[q] : acc[q]; acc[q] = 0.0f; }
                    have = true;
                }
                cur = cid;
            }
            const float* wr = W + (size_t)((cil * L.kh + ky) * L.kw + kx) * L.N; const int pos = oy * L.ow + ox;
            for (int co = 0; co < ng; co++) {
                const float w = wr[co]; const float* d = dp + ((size_t)co * L.npos + pos) * B;
                if (VEC) { const float4 v = *reinterpret_cast<const float4*>(d); acc[0] = fmaf(v.x, w, acc[0]); acc[1] = fmaf(v.y, w, acc[1]); acc[2] = fmaf(v.z, w, acc[2]); acc[3] = fmaf(v.w, w, acc[3]); }
                else {
#pragma unroll
                    for (int q = 0; q < 4; q++) if (q < nj) acc[q] = fmaf(d[q], w, acc[q]);
                }
            }
        }
    }
    if (have) {
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = tot[q] + acc[q];
    }
    float* ob = out + feat * B + c0;
    if (VEC) {
        float4 v; v.x = acc[0]; v.y = acc[1]; v.z = acc[2]; v.w = acc[3];
        if (ysrc) { const float4 y = *reinterpret_cast<const float4*>(ysrc + feat * ldy + c0); v.x = dact_f(v.x, y.x, act_src); v.y = dact_f(v.y, y.y, act_src); v.z = dact_f(v.z, y.z, act_src); v.w = dact_f(v.w, y.w, act_src); }
        *reinterpret_cast<float4*>(ob) = v;
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++) if (q < nj) ob[q] = ysrc ? dact_f(acc[q], ysrc[feat * ldy + c0 + q], act_src) : acc[q];
    }
}

// dW / db of a thin layer: thread = (chunk, n, k) with k FASTEST -- the K + 1 rows of one output channel sit in neighbouring lanes and read the same dpre row --, the tap's
// validity taken once per position, the samples of a position walked four at a time where VEC (the chain itself stays one sample after the other, in k_conv_dw's order)
template <int U8, int VEC>
__global__ __launch_bounds__(256) void k_cdg_thin_dw(LayerDev L, const void* __restrict__ X, int ldx, const float* __restrict__ dpre, int B, int S, int kc, float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int K1 = L.K + 1; const size_t per_s = (size_t)K1 * L.N;
    if (t >= per_s * S) return;
    const int s = (int)(t / per_s); const int e = (int)(t % per_s);
    const int k = e % K1, n = e / K1;
    const int KK = L.npos * B, j0 = s * kc, j1 = min(KK, j0 + kc);
    const int khw = L.kh * L.kw; const int ci = CONV_CHAN_BASE_OF_OUT(1, L, n) + k / khw, ky = (k / L.kw) % L.kh, kx = k % L.kw;      // (unused for the bias row)
    float acc = 0.0f;
    for (int pos = j0 / B; pos * B < j1; pos++) {
        const int b0 = max(j0, pos * B) - pos * B, b1 = min(j1, (pos + 1) * B) - pos * B;
        const float* d = dpre + ((size_t)n * L.npos + pos) * B;
        if (k == L.K) {
            if (VEC) for (int b = b0; b < b1; b += 4) { const float4 v = *reinterpret_cast<const float4*>(d + b); acc = acc + v.x; acc = acc + v.y; acc = acc + v.z; acc = acc + v.w; }
            else for (int b = b0; b < b1; b++) acc = acc + d[b];
            continue;
        }
        const int oy = pos / L.ow, ox = pos - oy * L.ow; const int iy = oy * L.sh + CONV_TAP_Y(1, L, ky) - L.ph, ix = ox * L.sw + CONV_TAP_X(1, L, kx) - L.pw;
        if (iy < 0 || iy >= L.ih || ix < 0 || ix >= L.iw) continue;
        const size_t xr = (size_t)((ci * L.ih + iy) * L.iw + ix) * ldx;
        if (VEC) {
            for (int b = b0; b < b1; b += 4) {
                const float4 v = *reinterpret_cast<const float4*>(d + b); float x[4];
                if (U8) { const uchar4 u = *reinterpret_cast<const uchar4*>(reinterpret_cast<const unsigned char*>(X) + xr + b); x[0] = u8_unit(u.x); x[1] = u8_unit(u.y); x[2] = u8_unit(u.z); x[3] = u8_unit(u.w); }
                else { const float4 u = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(X) + xr + b); x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w; }
                acc = fmaf(x[0], v.x, acc); acc = fmaf(x[1], v.y, acc); acc = fmaf(x[2], v.z, acc); acc = fmaf(x[3], v.w, acc);
            }
        } else for (int b = b0; b < b1; b++) acc = fmaf(ld_x<U8>(X, xr + b), d[b], acc);
    }
    out[(size_t)s * per_s + (size_t)k * L.N + n] = acc;
}

// ------------------------------------------------------------------ MFMA: one wave = one register tile (operand layouts: nn_mfma.hip)
// forward: task = (channel tile, column group, position); a channel tile lies inside ONE group (16 NT divides cout/g), so the wave's K range is that group's.  The wave walks
// the plan chunks itself and adds the chunk sums in ascending order
template <int MT, int NT, int U8, int RES, int DG>
__global__ __launch_bounds__(256) void k_conv_mfma_fwd(LayerDev L, const float* __restrict__ P, const void* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y, int ntasks,
                                                       const float* __restrict__ R, int ldr, int rcol0) {
    extern __shared__ int tap_lds[];      // k -> (ci within the group << 16 | ky << 8 | kx)
    {
        const int khw = L.kh * L.kw;
        for (int k = threadIdx.x; k < L.K; k += 256) { const int ci = k / khw, ky = (k / L.kw) % L.kh, kx = k % L.kw; tap_lds[k] = (ci << 16) | (ky << 8) | kx; }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    int task = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6));
    if (task >= ntasks) return;
    const int ngroups = L.N / (16 * NT), mgroups = ncols / (16 * MT);
    const int ng = task % ngroups; task /= ngroups;
    const int mg = task % mgroups; const int pos = task / mgroups;
    const int n0 = ng * 16 * NT, c0 = mg * 16 * MT;
    const int cb = CONV_CHAN_BASE_OF_OUT(DG, L, n0);
    const int oy = pos / L.ow, ox = pos % L.ow; const int y0 = oy * L.sh - L.ph, x0 = ox * L.sw - L.pw;
    const float* Wp = P + L.w_off + n0 + l15;
    const size_t xcol = (size_t)col0 + c0 + l15;
    const int S = dqn_nchunks(L.K, L.fwd_kc), kc = dqn_chunk_len(L.K, L.fwd_kc);
    auto lda = [&](int k, float (&a)[MT]) {      // the A operand of MFMA step k: 16 columns of one input element, or zeros beyond the border
        const int tp = tap_lds[k]; const int ci = cb + (tp >> 16), iy = y0 + CONV_TAP_Y(DG, L, (tp >> 8) & 255), ix = x0 + CONV_TAP_X(DG, L, tp & 255);
        const bool in = iy >= 0 && iy < L.ih && ix >= 0 && ix < L.iw;
        const size_t row = in ? (size_t)((ci * L.ih + iy) * L.iw + ix) * ldx + xcol : 0;
#pragma unroll
        for (int m = 0; m < MT; m++) a[m] = in ? ld_x<U8>(X, row + 16 * m) : 0.0f;
    };
    f32x4 acc[MT][NT], tot[MT][NT];
    for (int s = 0; s < S; s++) {
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int t = 0; t < NT; t++) acc[m][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int k0 = s * kc, k1 = min(L.K, k0 + kc);
        constexpr int U = 8;
        int k = k0 + kq;
        for (; k + 4 * (U - 1) < k1; k += 4 * U) {      // U steps of operands in flight; the chain stays k-ascending
            float a[U][MT], b[U][NT];
#pragma unroll
            for (int u = 0; u < U; u++) {
                lda(k + 4 * u, a[u]);
#pragma unroll
                for (int t = 0; t < NT; t++) b[u][t] = Wp[(size_t)(k + 4 * u) * L.N + 16 * t];
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int m = 0; m < MT; m++)
#pragma unroll
                    for (int t = 0; t < NT; t++) acc[m][t] = MFMA(a[u][m], b[u][t], acc[m][t]);
        }
        for (; k < k1; k += 4) {
            float a[MT], b[NT];
            lda(k, a);
#pragma unroll
            for (int t = 0; t < NT; t++) b[t] = Wp[(size_t)k * L.N + 16 * t];
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int t = 0; t < NT; t++) acc[m][t] = MFMA(a[m], b[t], acc[m][t]);
        }
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int t = 0; t < NT; t++) {
                if (s == 0) tot[m][t] = acc[m][t];
                else { tot[m][t].x = tot[m][t].x + acc[m][t].x; tot[m][t].y = tot[m][t].y + acc[m][t].y; tot[m][t].z = tot[m][t].z + acc[m][t].z; tot[m][t].w = tot[m][t].w + acc[m][t].w; }
            }
    }
    f32x4 res[RES ? MT : 1][RES ? NT : 1];
    if (RES) {      // every load of the addend tile before the first use
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int m = 0; m < MT; m++) res[RES ? m : 0][RES ? t : 0] = *reinterpret_cast<const f32x4*>(R + ((size_t)(n0 + 16 * t + l15) * L.npos + pos) * ldr + rcol0 + c0 + 16 * m + 4 * kq);
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int n = n0 + 16 * t + l15;
        const float bias = P[L.b_off + n];
#pragma unroll
        for (int m = 0; m < MT; m++) {
            f32x4 v = tot[m][t];
            act_v4(v, bias, L.act);
            if (RES) { const f32x4 r = res[RES ? m : 0][RES ? t : 0]; v.x = v.x + r.x; v.y = v.y + r.y; v.z = v.z + r.z; v.w = v.w + r.w; }
            *reinterpret_cast<f32x4*>(Y + ((size_t)n * L.npos + pos) * ncols + c0 + 16 * m + 4 * kq) = v;
        }
    }
}

// dX: task = (column group, 16 input channels of ONE group, input position); the co loop runs over that group's cout/g output channels
template <int MT, int ADD, int DG>
__global__ __launch_bounds__(256) void k_conv_mfma_dx(LayerDev L, const float* __restrict__ P, const float* __restrict__ dpre, int B, float* __restrict__ out,
                                                      const float* __restrict__ ysrc, int ldy, int act_src, int ntasks, const float* __restrict__ dY) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    int task = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6));
    if (task >= ntasks) return;
    const int mgroups = B / (16 * MT);
    const int mg = task % mgroups; task /= mgroups;
    const int b0 = mg * 16 * MT;
    const float* W = P + L.w_off;
    const int ctiles = L.cin / 16; const int ct = task % ctiles; const int ip = task / ctiles;
    const int iy = ip / L.iw, ix = ip % L.iw; const int ci = ct * 16 + l15;
    const int cg = CONV_INS_PER_GROUP(DG, L), ng = CONV_OUTS_PER_GROUP(DG, L); const int j = CONV_GROUP_OF_IN(DG, L, ct * 16), cil = ci - j * cg, co0 = j * ng;      // the group's first output channel
    const size_t feat = (size_t)ci * L.ih * L.iw + ip;
    f32x4 acc[MT], tot[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) { acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; tot[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    const int tc = DQN_CONV_TAP_CHUNK(L); int cur = -1; bool have = false;
    const unsigned cstride = (unsigned)L.npos * (unsigned)B;
    for (int ky = 0; ky < L.kh; ky++) {
        const int ty = iy + L.ph - CONV_TAP_Y(DG, L, ky); if (ty < 0 || ty % L.sh) continue; const int oy = ty / L.sh; if (oy >= L.oh) continue;
        for (int kx = 0; kx < L.kw; kx++) {
            const int tx = ix + L.pw - CONV_TAP_X(DG, L, kx); if (tx < 0 || tx % L.sw) continue; const int ox = tx / L.sw; if (ox >= L.ow) continue;
            const int cid = (ky * L.kw + kx) / tc;
            if (cid != cur) {
                if (cur >= 0) {
#pragma unroll
                    for (int m = 0; m < MT; m++) { if (have) { tot[m].x = tot[m].x + acc[m].x; tot[m].y = tot[m].y + acc[m].y; tot[m].z = tot[m].z + acc[m].z; tot[m].w = tot[m].w + acc[m].w; } else tot[m] = acc[m]; acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
                    have = true;
                }
                cur = cid;
            }
            const float* wr = W + (size_t)((cil * L.kh + ky) * L.kw + kx) * L.N + co0;
            const float* dp = dpre + (size_t)co0 * cstride + (size_t)(oy * L.ow + ox) * B + b0 + l15;
            constexpr int U = 8;
            int co = kq;
            for (; co + 4 * (U - 1) < ng; co += 4 * U) {
                float av[U][MT], bv[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    bv[u] = wr[co + 4 * u];
#pragma unroll
                    for (int m = 0; m < MT; m++) av[u][m] = dp[(size_t)(co + 4 * u) * cstride + 16 * m];
                }
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int m = 0; m < MT; m++) acc[m] = MFMA(av[u][m], bv[u], acc[m]);
            }
            for (; co < ng; co += 4) {
                const float b = wr[co];
#pragma unroll
                for (int m = 0; m < MT; m++) acc[m] = MFMA(dp[(size_t)co * cstride + 16 * m], b, acc[m]);
            }
        }
    }
    f32x4 add[MT];
    if (ADD) {      // every load of the addend before the first use
#pragma unroll
        for (int m = 0; m < MT; m++) add[m] = *reinterpret_cast<const f32x4*>(dY + feat * B + b0 + 16 * m + 4 * kq);
    }
#pragma unroll
    for (int m = 0; m < MT; m++) {
        f32x4 v = acc[m];
        if (have) { v.x = tot[m].x + v.x; v.y = tot[m].y + v.y; v.z = tot[m].z + v.z; v.w = tot[m].w + v.w; }
        const int bcol = b0 + 16 * m + 4 * kq;
        if (ADD) { v.x = v.x + add[m].x; v.y = v.y + add[m].y; v.z = v.z + add[m].z; v.w = v.w + add[m].w; }
        if (ysrc) { const f32x4 y = *reinterpret_cast<const f32x4*>(ysrc + feat * ldy + bcol); dact_v4(v, y, act_src); }
        *reinterpret_cast<f32x4*>(out + feat * B + bcol) = v;
    }
}

// dW / db: task = (channel tile inside ONE group, 16 rows of the (K+1) x N block, plan chunk); row K is the bias gradient (A operand 1: fma(1, d, acc) == acc + d).  Chunks cover whole positions or are cut in samples (multiples of 4)
template <int NT, int U8, int DG>
__global__ __launch_bounds__(256) void k_conv_mfma_dw(LayerDev L, const void* __restrict__ X, int ldx, const float* __restrict__ dpre, int B, int S, int kc, float* __restrict__ out, int ntasks) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    int task = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6));
    if (task >= ntasks) return;
    const int ngroups = L.N / (16 * NT), mtiles = (L.K + 1 + 15) / 16;
    const int ng = task % ngroups; task /= ngroups;
    const int mt = task % mtiles; const int s = task / mtiles;
    const int n0 = ng * 16 * NT;
    const int cb = CONV_CHAN_BASE_OF_OUT(DG, L, n0);
    const int krow = mt * 16 + l15;                       // this lane's A row
    const bool real = krow < L.K; const float aconst = krow == L.K ? 1.0f : 0.0f;
    int ci = 0, ky = 0, kx = 0;
    if (real) { const int khw = L.kh * L.kw; ci = cb + krow / khw; ky = (krow / L.kw) % L.kh; kx = krow % L.kw; }
    const int KK = L.npos * B, j0 = s * kc, j1 = min(KK, j0 + kc);
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const unsigned nstride = 16u * (unsigned)L.npos * (unsigned)B;
    for (int pos = j0 / B; pos * B < j1; pos++) {
        // the chunk's samples of this position, in MFMA steps of 4 (chunk bounds and B are multiples of 4: a step never straddles a position or a chunk)
        const int bsteps = (min(j1, (pos + 1) * B) - pos * B) / 4; int bs = (max(j0, pos * B) - pos * B) / 4;
        const int oy = pos / L.ow, ox = pos % L.ow; const int iy = oy * L.sh + CONV_TAP_Y(DG, L, ky) - L.ph, ix = ox * L.sw + CONV_TAP_X(DG, L, kx) - L.pw;
        const bool in = real && iy >= 0 && iy < L.ih && ix >= 0 && ix < L.iw;
        const size_t xr = in ? (size_t)((ci * L.ih + iy) * L.iw + ix) * ldx + kq : 0;
        const float afix = real ? 0.0f : aconst;           // a tap beyond the border: an exact 0
        const float* dr = dpre + ((size_t)(n0 + l15) * L.npos + pos) * B + kq;
        constexpr int U = 8;
        for (; bs + U <= bsteps; bs += U) {
            float av[U], bv[U][NT];
#pragma unroll
            for (int u = 0; u < U; u++) {
                av[u] = in ? ld_x<U8>(X, xr + 4 * (bs + u)) : afix;
#pragma unroll
                for (int t = 0; t < NT; t++) bv[u][t] = dr[t * nstride + 4 * (bs + u)];
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int t = 0; t < NT; t++) acc[t] = MFMA(av[u], bv[u][t], acc[t]);
        }
        for (; bs < bsteps; bs++) {
            const float a = in ? ld_x<U8>(X, xr + 4 * bs) : afix;
#pragma unroll
            for (int t = 0; t < NT; t++) acc[t] = MFMA(a, dr[(size_t)t * nstride + 4 * bs], acc[t]);
        }
    }
    const size_t per_s = (size_t)(L.K + 1) * L.N;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int n = n0 + 16 * t + l15;
        const float v[4] = {acc[t].x, acc[t].y, acc[t].z, acc[t].w};
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int k = mt * 16 + 4 * kq + r;
            if (k <= L.K) out[(size_t)s * per_s + (size_t)k * L.N + n] = v[r];
        }
    }
}

// ------------------------------------------------------------------ launchers (mf: hp.use_mfma).  Kind 15: thin first.  Then the MFMA form where the shape tiles, else the VALU form -- the same bits.
// One dispatch helper per contraction turns the run-time tile counts / arena type into template arguments; V is the residual variant (RES / ADD), a compile-time choice of the caller
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
template <int DG> static bool conv_thin(const LayerDev& L) { return DG && (L.cin == L.groups || L.K < 16); }      // depthwise, or a contraction shorter than one MFMA tile row
template <int U8, int V, int DG, class... A> static void mfma_fwd_tiles(int MT, int NT, dim3 g, size_t lds, hipStream_t st, A... a) {
    const dim3 b(256);
    if (MT == 2 && NT == 2) hipLaunchKernelGGL((k_conv_mfma_fwd<2, 2, U8, V, DG>), g, b, lds, st, a...);
    else if (MT == 2) hipLaunchKernelGGL((k_conv_mfma_fwd<2, 1, U8, V, DG>), g, b, lds, st, a...);
    else if (NT == 2) hipLaunchKernelGGL((k_conv_mfma_fwd<1, 2, U8, V, DG>), g, b, lds, st, a...);
    else hipLaunchKernelGGL((k_conv_mfma_fwd<1, 1, U8, V, DG>), g, b, lds, st, a...);
}
template <int DG, class... A> static void mfma_dw_tiles(int NT, int xu8, dim3 g, hipStream_t st, A... a) {
    const dim3 b(256);
    if (xu8) { if (NT == 2) hipLaunchKernelGGL((k_conv_mfma_dw<2, 1, DG>), g, b, 0, st, a...); else hipLaunchKernelGGL((k_conv_mfma_dw<1, 1, DG>), g, b, 0, st, a...); }
    else     { if (NT == 2) hipLaunchKernelGGL((k_conv_mfma_dw<2, 0, DG>), g, b, 0, st, a...); else hipLaunchKernelGGL((k_conv_mfma_dw<1, 0, DG>), g, b, 0, st, a...); }
}
template <int V, int DG, class... A> static void mfma_dx_tiles(int MT, dim3 g, hipStream_t st, A... a) {
    const dim3 b(256);
    if (MT == 2) hipLaunchKernelGGL((k_conv_mfma_dx<2, V, DG>), g, b, 0, st, a...); else hipLaunchKernelGGL((k_conv_mfma_dx<1, V, DG>), g, b, 0, st, a...);
}

// R: the fused join of a map block, kind 1 only (an inner layer never reads the observation: no byte arena); the addend tile is read 16 bytes per lane where its rows allow it, else the VALU form
template <int DG> static void conv_own_fwd(hipStream_t st, const LayerDev& L, const float* P, const void* X, int ldx, int col0, int ncols, float* Y, int mf, int xu8, const float* R, int ldr, int rcol0) {
    if constexpr (DG) if (conv_thin<DG>(L)) {
        const bool vec = !(ldx % 4 || col0 % 4 || ncols % 4) && al16(Y) && (xu8 ? ((uintptr_t)X & 3) == 0 : al16(X));
        const size_t tot = (size_t)L.N * L.npos * ((ncols + 3) / 4); const dim3 g((unsigned)((tot + 255) / 256)), b(256);
        if (xu8) { if (vec) hipLaunchKernelGGL((k_cdg_thin_fwd<1, 1>), g, b, 0, st, L, P, X, ldx, col0, ncols, Y); else hipLaunchKernelGGL((k_cdg_thin_fwd<1, 0>), g, b, 0, st, L, P, X, ldx, col0, ncols, Y); }
        else     { if (vec) hipLaunchKernelGGL((k_cdg_thin_fwd<0, 1>), g, b, 0, st, L, P, X, ldx, col0, ncols, Y); else hipLaunchKernelGGL((k_cdg_thin_fwd<0, 0>), g, b, 0, st, L, P, X, ldx, col0, ncols, Y); }
        return;
    }
    const int ng = CONV_OUTS_PER_GROUP(DG, L);
    const int S = dqn_nchunks(L.K, L.fwd_kc), kc = dqn_chunk_len(L.K, L.fwd_kc);
    if (mf && !(ng % 16 || ncols % 16 || L.K % 4 || (S > 1 && kc % 4) || L.K > 16384 || L.kh > 255 || L.kw > 255 || L.cin > 32767) && al16(Y) && !(R && (ldr % 4 || rcol0 % 4 || !al16(R)))) {
        const int MT = (ncols % 32 == 0 && (long)(ncols / 32) * (L.N / 16) * L.npos >= 1024) ? 2 : 1, NT = ng % 32 == 0 ? 2 : 1;
        const int ntasks = (L.N / (16 * NT)) * (ncols / (16 * MT)) * L.npos; const size_t lds = (size_t)L.K * sizeof(int); const dim3 g((ntasks + 3) / 4);
        if (R) { if constexpr (!DG) mfma_fwd_tiles<0, 1, DG>(MT, NT, g, lds, st, L, P, X, ldx, col0, ncols, Y, ntasks, R, ldr, rcol0); }
        else if (xu8) mfma_fwd_tiles<1, 0, DG>(MT, NT, g, lds, st, L, P, X, ldx, col0, ncols, Y, ntasks, R, ldr, rcol0);
        else mfma_fwd_tiles<0, 0, DG>(MT, NT, g, lds, st, L, P, X, ldx, col0, ncols, Y, ntasks, R, ldr, rcol0);
        return;
    }
    const size_t tot = (size_t)L.N * L.npos * ncols; const dim3 g((unsigned)((tot + 255) / 256)), b(256);
    if (R) { if constexpr (!DG) hipLaunchKernelGGL((k_conv_fwd<0, 1, DG>), g, b, 0, st, L, P, X, ldx, col0, ncols, Y, R, ldr, rcol0); }
    else if (xu8) hipLaunchKernelGGL((k_conv_fwd<1, 0, DG>), g, b, 0, st, L, P, X, ldx, col0, ncols, Y, R, ldr, rcol0);
    else hipLaunchKernelGGL((k_conv_fwd<0, 0, DG>), g, b, 0, st, L, P, X, ldx, col0, ncols, Y, R, ldr, rcol0);
}
// dst: the layer's (K+1) x N gradient block, or S = dqn_nchunks(npos*B, dw_kc) slabs of it.  A thin layer's weights are few: one thread per (chunk, weight) whatever mf says (k_cdg_thin_dw)
template <int DG> static void conv_own_dw(hipStream_t st, const LayerDev& L, const void* X, int ldx, const float* dpre, int B, float* dst, int mf, int xu8) {
    const int KK = L.npos * B, S = dqn_nchunks(KK, L.dw_kc), kc = dqn_chunk_len(KK, L.dw_kc); const int ng = CONV_OUTS_PER_GROUP(DG, L);
    const size_t tot = (size_t)(L.K + 1) * L.N * S; const dim3 gv((unsigned)((tot + 255) / 256)), b(256);
    if constexpr (DG) if (conv_thin<DG>(L)) {
        const bool vec = !(B % 4 || ldx % 4 || (S > 1 && kc % 4)) && al16(dpre) && (xu8 ? ((uintptr_t)X & 3) == 0 : al16(X));
        if (xu8) { if (vec) hipLaunchKernelGGL((k_cdg_thin_dw<1, 1>), gv, b, 0, st, L, X, ldx, dpre, B, S, kc, dst); else hipLaunchKernelGGL((k_cdg_thin_dw<1, 0>), gv, b, 0, st, L, X, ldx, dpre, B, S, kc, dst); }
        else     { if (vec) hipLaunchKernelGGL((k_cdg_thin_dw<0, 1>), gv, b, 0, st, L, X, ldx, dpre, B, S, kc, dst); else hipLaunchKernelGGL((k_cdg_thin_dw<0, 0>), gv, b, 0, st, L, X, ldx, dpre, B, S, kc, dst); }
        return;
    }
    if (mf && !(ng % 16 || B % 4 || (S > 1 && kc % 4))) {      // whole positions per chunk, or chunks cut in samples (large batches): multiples of 4 either way
        const int NT = ng % 32 == 0 ? 2 : 1; const int ntasks = (L.N / (16 * NT)) * ((L.K + 1 + 15) / 16) * S;
        mfma_dw_tiles<DG>(NT, xu8, dim3((ntasks + 3) / 4), st, L, X, ldx, dpre, B, S, kc, dst, ntasks);
        return;
    }
    if (xu8) hipLaunchKernelGGL((k_conv_dw<1, DG>), gv, b, 0, st, L, X, ldx, dpre, B, S, kc, dst);
    else hipLaunchKernelGGL((k_conv_dw<0, DG>), gv, b, 0, st, L, X, ldx, dpre, B, S, kc, dst);
}
// dY: the fused entry add of a map block, kind 1 only
template <int DG> static void conv_own_dx(hipStream_t st, const LayerDev& L, const float* P, const float* dpre, int B, float* out, const float* ysrc, int ldy, int act_src, int mf, const float* dY) {
    if constexpr (DG) if (conv_thin<DG>(L)) {
        const bool vec = !(B % 4 || ldy % 4) && al16(out) && al16(ysrc) && al16(dpre);
        const size_t tot = (size_t)L.in_feat * ((B + 3) / 4); const dim3 g((unsigned)((tot + 255) / 256)), b(256);
        if (vec) hipLaunchKernelGGL(k_cdg_thin_dx<1>, g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src);
        else hipLaunchKernelGGL(k_cdg_thin_dx<0>, g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src);
        return;
    }
    const int cg = CONV_INS_PER_GROUP(DG, L), ng = CONV_OUTS_PER_GROUP(DG, L);
    if (mf && !(B % 16 || ng % 4 || cg % 16 || ldy % 4) && al16(out) && al16(ysrc) && al16(dY)) {
        const int MT = (B % 32 == 0 && (long)(B / 32) * (L.cin / 16) * L.ih * L.iw >= 1024) ? 2 : 1;
        const int ntasks = (B / (16 * MT)) * (L.cin / 16) * L.ih * L.iw; const dim3 g((ntasks + 3) / 4);
        if (dY) { if constexpr (!DG) mfma_dx_tiles<1, DG>(MT, g, st, L, P, dpre, B, out, ysrc, ldy, act_src, ntasks, dY); }
        else mfma_dx_tiles<0, DG>(MT, g, st, L, P, dpre, B, out, ysrc, ldy, act_src, ntasks, dY);
        return;
    }
    const size_t tot = (size_t)L.in_feat * B; const dim3 g((unsigned)((tot + 255) / 256)), b(256);
    if (dY) { if constexpr (!DG) hipLaunchKernelGGL((k_conv_dx<1, DG>), g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src, dY); }
    else hipLaunchKernelGGL((k_conv_dx<0, DG>), g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src, dY);
}

// the layer's kind picks the geometry; a kind-15 layer carries no residual operand (build_layers refuses it inside a skip block)
void launch_conv_own_fwd(hipStream_t st, const LayerDev& L, const float* P, const void* X, int ldx, int col0, int ncols, float* Y, int mf, int xu8, const float* R, int ldr, int rcol0) {
    if (is_cdg(L.kind)) conv_own_fwd<1>(st, L, P, X, ldx, col0, ncols, Y, mf, xu8, nullptr, 0, 0);
    else conv_own_fwd<0>(st, L, P, X, ldx, col0, ncols, Y, mf, xu8, R, ldr, rcol0);
}
void launch_conv_own_dw(hipStream_t st, const LayerDev& L, const void* X, int ldx, const float* dpre, int B, float* dst, int mf, int xu8) {
    if (is_cdg(L.kind)) conv_own_dw<1>(st, L, X, ldx, dpre, B, dst, mf, xu8);
    else conv_own_dw<0>(st, L, X, ldx, dpre, B, dst, mf, xu8);
}
void launch_conv_own_dx(hipStream_t st, const LayerDev& L, const float* P, const float* dpre, int B, float* out, const float* ysrc, int ldy, int act_src, int mf, const float* dY) {
    if (is_cdg(L.kind)) conv_own_dx<1>(st, L, P, dpre, B, out, ysrc, ldy, act_src, mf, nullptr);
    else conv_own_dx<0>(st, L, P, dpre, B, out, ysrc, ldy, act_src, mf, dY);
}
