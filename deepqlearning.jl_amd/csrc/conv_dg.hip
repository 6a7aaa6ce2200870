// conv_dg.hip -- Conv((kh, kw), cin => cout, act; stride, pad, dilation = (dh, dw), groups = g) and DepthwiseConv (groups = cin): layer kind DQN_LAYER_CONV_DG.  The sibling of
// conv_pad.hip: forward, dX and dW / db as implicit GEMMs whose operand loads carry the border as a predicate, with the tap geometry
//     iy = oy * sh + ky * dh - ph,   ix = ox * sw + kx * dw - pw
// and a per-group K range: output channel n belongs to group j = n / (cout / g) and reads input channels [j * cin/g, (j + 1) * cin/g).
//
// Canonical order ("Dilated and grouped convolutions"): the layer IS the groups = 1, dilation = 1 conv of conv_pad.hip on the same zero-extended map whose
// kernel is the layer's own, zero-stuffed to ((kh - 1) dh + 1, (kw - 1) dw + 1) and zero outside the group's diagonal block; only the LIVE terms are chained:
//   forward   per plan chunk (fwd_kc, on the layer's own K = (cin/g) kh kw) one k = (ci within the group, ky, kx)-ascending fmaf chain from +0; chunk sums added in ascending
//             order, + bias, activation
//   dW / db   per live weight and plan chunk (dw_kc) one (position, sample)-ascending chain; slabs [S][(K+1)][N]
//   dX        per input element, per chunk of RAW taps (dx_kc) one chain over the VALID taps -- (iy + ph - ky * dh) divisible by sh with quotient in [0, oh), likewise x -- with co
//             (within the group) innermost; then the producing layer's activation derivative
// A skipped term and a term multiplied by an exact zero give the same bits (a chain that starts at +0 never holds -0), so the layer equals the kind-1 network on the expanded
// kernel bit for bit under unsplit plan entries (tests/test_conv_dg_gpu.py).
//
// Three forms of each contraction, bit-identical:
//   MFMA   fp32 v_mfma_f32_16x16x4_f32, one wave = one register tile, operands straight from L2 (conv_pad.hip's kernels with the group's channel base and the dilated tap):
//          where cout/g (forward, dW), cin/g (dX) and the columns tile by 16
//   thin   cin/g == 1 (depthwise) or K < 16: NOT an implicit GEMM padded to tiles -- pool.hip's work split, a thread owns (one output feature [forward] or input feature [dX],
//          four adjacent columns); one 16-byte access where leading dimension, column offset and count are multiples of 4, one column at a time otherwise.  No LDS, no atomics,
//          plain vector stores; the dX is a gather per input element over its valid taps; dW / db one thread per (chunk, weight), the rows of a channel in neighbouring lanes.  Taken whatever use_mfma says
//   VALU   one thread per output element: every other shape
// A first-layer conv may read the BYTE arena of a u8 replay (xu8): value = u8_unit(byte).
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

template <int U8> __device__ __forceinline__ float ld_xg(const void* __restrict__ X, size_t i) {
    if (U8) return u8_unit(reinterpret_cast<const unsigned char*>(X)[i]);
    return reinterpret_cast<const float*>(X)[i];
}

// ------------------------------------------------------------------ VALU: one thread per output element
template <int U8>
__global__ __launch_bounds__(256) void k_cdg_fwd(LayerDev L, const float* __restrict__ P, const void* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)L.N * L.npos * ncols) return;
    const int col = (int)(t % ncols); const int pos = (int)((t / ncols) % L.npos); const int n = (int)(t / ((size_t)ncols * L.npos));
    const int oy = pos / L.ow, ox = pos % L.ow; const int y0 = oy * L.sh - L.ph, x0 = ox * L.sw - L.pw;
    const int cb = (n / (L.N / L.groups)) * (L.cin / L.groups);      // the group's first input channel
    const float* W = P + L.w_off;
    const int S = dqn_nchunks(L.K, L.fwd_kc), kc = dqn_chunk_len(L.K, L.fwd_kc), khw = L.kh * L.kw;
    float tot = 0.0f;
    for (int s = 0; s < S; s++) {
        const int k0 = s * kc, k1 = min(L.K, k0 + kc);
        int ci = k0 / khw, ky = (k0 / L.kw) % L.kh, kx = k0 % L.kw;
        float acc = 0.0f;
        for (int k = k0; k < k1; k++) {
            const int iy = y0 + ky * L.dh, ix = x0 + kx * L.dw;
            if (iy >= 0 && iy < L.ih && ix >= 0 && ix < L.iw)
                acc = fmaf(ld_xg<U8>(X, (size_t)(((cb + ci) * L.ih + iy) * L.iw + ix) * ldx + col0 + col), W[(size_t)k * L.N + n], acc);
            if (++kx == L.kw) { kx = 0; if (++ky == L.kh) { ky = 0; ++ci; } }
        }
        tot = s == 0 ? acc : tot + acc;
    }
    Y[t] = act_f(tot + P[L.b_off + n], L.act);
}

// thread = (chunk, k, n) for k < K, plus the virtual row k == K of the bias gradient; out = slabs [S][(K+1)][N] (S == 1: the gradient block itself)
template <int U8>
__global__ __launch_bounds__(256) void k_cdg_dw(LayerDev L, const void* __restrict__ X, int ldx, const float* __restrict__ dpre, int B, int S, int kc, float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per_s = (size_t)(L.K + 1) * L.N;
    if (t >= per_s * S) return;
    const int s = (int)(t / per_s); const size_t e = t % per_s;
    const int n = (int)(e % L.N), k = (int)(e / L.N);
    const int KK = L.npos * B, j0 = s * kc, j1 = min(KK, j0 + kc);
    const int khw = L.kh * L.kw; const int ci = (n / (L.N / L.groups)) * (L.cin / L.groups) + k / khw, ky = (k / L.kw) % L.kh, kx = k % L.kw;      // (unused for the bias row)
    float acc = 0.0f;
    int pos = j0 / B, b = j0 % B;
    for (int j = j0; j < j1; j++) {
        const float d = dpre[((size_t)n * L.npos + pos) * B + b];
        if (k < L.K) {
            const int oy = pos / L.ow, ox = pos % L.ow; const int iy = oy * L.sh + ky * L.dh - L.ph, ix = ox * L.sw + kx * L.dw - L.pw;
            if (iy >= 0 && iy < L.ih && ix >= 0 && ix < L.iw) acc = fmaf(ld_xg<U8>(X, (size_t)((ci * L.ih + iy) * L.iw + ix) * ldx + b), d, acc);
        } else acc = acc + d;
        if (++b == B) { b = 0; ++pos; }
    }
    out[(size_t)s * per_s + e] = acc;
}

__global__ __launch_bounds__(256) void k_cdg_dx(LayerDev L, const float* __restrict__ P, const float* __restrict__ dpre, int B, float* __restrict__ out,
                                                const float* __restrict__ ysrc, int ldy, int act_src) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)L.in_feat * B) return;
    const int b = (int)(e % B); const int feat = (int)(e / B);
    const int hw = L.ih * L.iw; const int ci = feat / hw, iy = (feat % hw) / L.iw, ix = feat % L.iw;
    const int cg = L.cin / L.groups, ng = L.N / L.groups; const int j = ci / cg, cil = ci - j * cg;
    const float* W = P + L.w_off + (size_t)j * ng;
    const float* dp = dpre + (size_t)j * ng * L.npos * B + b;
    const int tc = DQN_CONV_TAP_CHUNK(L); int cur = -1; bool have = false; float tot = 0.0f, acc = 0.0f;
    for (int ky = 0; ky < L.kh; ky++) {
        const int ty = iy + L.ph - ky * L.dh; if (ty < 0 || ty % L.sh) continue; const int oy = ty / L.sh; if (oy >= L.oh) continue;
        for (int kx = 0; kx < L.kw; kx++) {
            const int tx = ix + L.pw - kx * L.dw; if (tx < 0 || tx % L.sw) continue; const int ox = tx / L.sw; if (ox >= L.ow) continue;
            const int cid = (ky * L.kw + kx) / tc;
            if (cid != cur) { if (cur >= 0) { tot = have ? tot + acc : acc; have = true; acc = 0.0f; } cur = cid; }
            const float* wr = W + (size_t)((cil * L.kh + ky) * L.kw + kx) * L.N; const int pos = oy * L.ow + ox;
            for (int co = 0; co < ng; co++) acc = fmaf(dp[((size_t)co * L.npos + pos) * B], wr[co], acc);
        }
    }
    if (have) acc = tot + acc;
    if (ysrc) acc = dact_f(acc, ysrc[(size_t)feat * ldy + b], act_src);
    out[e] = acc;
}

// ------------------------------------------------------------------ thin groups: a thread owns (feature, four adjacent columns); VEC: the four columns are one 16-byte access
template <int U8, int VEC>
__global__ __launch_bounds__(256) void k_cdg_thin_fwd(LayerDev L, const float* __restrict__ P, const void* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y) {
    const int nq = (ncols + 3) >> 2;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t f = t / nq; const int c0 = (int)(t - f * nq) * 4;
    if (f >= (size_t)L.N * L.npos) return;
    const int n = (int)(f / L.npos), pos = (int)(f - (size_t)n * L.npos);
    const int oy = pos / L.ow, ox = pos - oy * L.ow; const int y0 = oy * L.sh - L.ph, x0 = ox * L.sw - L.pw;
    const int cb = (n / (L.N / L.groups)) * (L.cin / L.groups);
    const float* W = P + L.w_off + n;
    const int nj = VEC ? 4 : min(4, ncols - c0);
    const int S = dqn_nchunks(L.K, L.fwd_kc), kc = dqn_chunk_len(L.K, L.fwd_kc), khw = L.kh * L.kw;
    float tot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = 0; s < S; s++) {
        const int k0 = s * kc, k1 = min(L.K, k0 + kc);
        int ci = k0 / khw, ky = (k0 / L.kw) % L.kh, kx = k0 % L.kw;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = k0; k < k1; k++) {
            const int iy = y0 + ky * L.dh, ix = x0 + kx * L.dw;
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
                    for (int j = 0; j < 4; j++) if (j < nj) acc[j] = fmaf(ld_xg<U8>(X, xi + j), w, acc[j]);
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
    const int cg = L.cin / L.groups, ng = L.N / L.groups; const int j = ci / cg, cil = ci - j * cg;
    const float* W = P + L.w_off + (size_t)j * ng;
    const float* dp = dpre + (size_t)j * ng * L.npos * B + c0;
    const int nj = VEC ? 4 : min(4, B - c0);
    const int tc = DQN_CONV_TAP_CHUNK(L); int cur = -1; bool have = false;
    float tot[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ky = 0; ky < L.kh; ky++) {
        const int ty = iy + L.ph - ky * L.dh; if (ty < 0 || ty % L.sh) continue; const int oy = ty / L.sh; if (oy >= L.oh) continue;
        for (int kx = 0; kx < L.kw; kx++) {
            const int tx = ix + L.pw - kx * L.dw; if (tx < 0 || tx % L.sw) continue; const int ox = tx / L.sw; if (ox >= L.ow) continue;
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
// validity taken once per position, the samples of a position walked four at a time where VEC (the chain itself stays one sample after the other, in k_cdg_dw's order)
template <int U8, int VEC>
__global__ __launch_bounds__(256) void k_cdg_thin_dw(LayerDev L, const void* __restrict__ X, int ldx, const float* __restrict__ dpre, int B, int S, int kc, float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int K1 = L.K + 1; const size_t per_s = (size_t)K1 * L.N;
    if (t >= per_s * S) return;
    const int s = (int)(t / per_s); const int e = (int)(t % per_s);
    const int k = e % K1, n = e / K1;
    const int KK = L.npos * B, j0 = s * kc, j1 = min(KK, j0 + kc);
    const int khw = L.kh * L.kw; const int ci = (n / (L.N / L.groups)) * (L.cin / L.groups) + k / khw, ky = (k / L.kw) % L.kh, kx = k % L.kw;      // (unused for the bias row)
    float acc = 0.0f;
    for (int pos = j0 / B; pos * B < j1; pos++) {
        const int b0 = max(j0, pos * B) - pos * B, b1 = min(j1, (pos + 1) * B) - pos * B;
        const float* d = dpre + ((size_t)n * L.npos + pos) * B;
        if (k == L.K) {
            if (VEC) for (int b = b0; b < b1; b += 4) { const float4 v = *reinterpret_cast<const float4*>(d + b); acc = acc + v.x; acc = acc + v.y; acc = acc + v.z; acc = acc + v.w; }
            else for (int b = b0; b < b1; b++) acc = acc + d[b];
            continue;
        }
        const int oy = pos / L.ow, ox = pos - oy * L.ow; const int iy = oy * L.sh + ky * L.dh - L.ph, ix = ox * L.sw + kx * L.dw - L.pw;
        if (iy < 0 || iy >= L.ih || ix < 0 || ix >= L.iw) continue;
        const size_t xr = (size_t)((ci * L.ih + iy) * L.iw + ix) * ldx;
        if (VEC) {
            for (int b = b0; b < b1; b += 4) {
                const float4 v = *reinterpret_cast<const float4*>(d + b); float x[4];
                if (U8) { const uchar4 u = *reinterpret_cast<const uchar4*>(reinterpret_cast<const unsigned char*>(X) + xr + b); x[0] = u8_unit(u.x); x[1] = u8_unit(u.y); x[2] = u8_unit(u.z); x[3] = u8_unit(u.w); }
                else { const float4 u = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(X) + xr + b); x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w; }
                acc = fmaf(x[0], v.x, acc); acc = fmaf(x[1], v.y, acc); acc = fmaf(x[2], v.z, acc); acc = fmaf(x[3], v.w, acc);
            }
        } else for (int b = b0; b < b1; b++) acc = fmaf(ld_xg<U8>(X, xr + b), d[b], acc);
    }
    out[(size_t)s * per_s + (size_t)k * L.N + n] = acc;
}

// ------------------------------------------------------------------ MFMA: one wave = one register tile (operand layouts: nn_mfma.hip; the kernels of conv_pad.hip with the group's base)
// forward: task = (channel tile, column group, position); a channel tile lies inside ONE group (16 NT divides cout/g), so the wave's K range is that group's
template <int MT, int NT, int U8>
__global__ __launch_bounds__(256) void k_cdg_mfma_fwd(LayerDev L, const float* __restrict__ P, const void* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y, int ntasks) {
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
    const int cb = (n0 / (L.N / L.groups)) * (L.cin / L.groups);
    const int oy = pos / L.ow, ox = pos % L.ow; const int y0 = oy * L.sh - L.ph, x0 = ox * L.sw - L.pw;
    const float* Wp = P + L.w_off + n0 + l15;
    const size_t xcol = (size_t)col0 + c0 + l15;
    const int S = dqn_nchunks(L.K, L.fwd_kc), kc = dqn_chunk_len(L.K, L.fwd_kc);
    auto lda = [&](int k, float (&a)[MT]) {      // the A operand of MFMA step k: 16 columns of one input element, or zeros beyond the border
        const int tp = tap_lds[k]; const int ci = cb + (tp >> 16), iy = y0 + ((tp >> 8) & 255) * L.dh, ix = x0 + (tp & 255) * L.dw;
        const bool in = iy >= 0 && iy < L.ih && ix >= 0 && ix < L.iw;
        const size_t row = in ? (size_t)((ci * L.ih + iy) * L.iw + ix) * ldx + xcol : 0;
#pragma unroll
        for (int m = 0; m < MT; m++) a[m] = in ? ld_xg<U8>(X, row + 16 * m) : 0.0f;
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
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int n = n0 + 16 * t + l15;
        const float bias = P[L.b_off + n];
#pragma unroll
        for (int m = 0; m < MT; m++) {
            f32x4 v = tot[m][t];
            act_v4(v, bias, L.act);
            *reinterpret_cast<f32x4*>(Y + ((size_t)n * L.npos + pos) * ncols + c0 + 16 * m + 4 * kq) = v;
        }
    }
}

// dX: task = (column group, 16 input channels of ONE group, input position); the co loop runs over that group's cout/g output channels
template <int MT>
__global__ __launch_bounds__(256) void k_cdg_mfma_dx(LayerDev L, const float* __restrict__ P, const float* __restrict__ dpre, int B, float* __restrict__ out,
                                                     const float* __restrict__ ysrc, int ldy, int act_src, int ntasks) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    int task = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6));
    if (task >= ntasks) return;
    const int mgroups = B / (16 * MT);
    const int mg = task % mgroups; task /= mgroups;
    const int b0 = mg * 16 * MT;
    const int ctiles = L.cin / 16; const int ct = task % ctiles; const int ip = task / ctiles;
    const int iy = ip / L.iw, ix = ip % L.iw; const int ci = ct * 16 + l15;
    const int cg = L.cin / L.groups, ng = L.N / L.groups; const int j = (ct * 16) / cg, cil = ci - j * cg;
    const float* W = P + L.w_off + (size_t)j * ng;
    const size_t feat = (size_t)ci * L.ih * L.iw + ip;
    f32x4 acc[MT], tot[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) { acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; tot[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    const int tc = DQN_CONV_TAP_CHUNK(L); int cur = -1; bool have = false;
    const unsigned cstride = (unsigned)L.npos * (unsigned)B;
    for (int ky = 0; ky < L.kh; ky++) {
        const int ty = iy + L.ph - ky * L.dh; if (ty < 0 || ty % L.sh) continue; const int oy = ty / L.sh; if (oy >= L.oh) continue;
        for (int kx = 0; kx < L.kw; kx++) {
            const int tx = ix + L.pw - kx * L.dw; if (tx < 0 || tx % L.sw) continue; const int ox = tx / L.sw; if (ox >= L.ow) continue;
            const int cid = (ky * L.kw + kx) / tc;
            if (cid != cur) {
                if (cur >= 0) {
#pragma unroll
                    for (int m = 0; m < MT; m++) { if (have) { tot[m].x = tot[m].x + acc[m].x; tot[m].y = tot[m].y + acc[m].y; tot[m].z = tot[m].z + acc[m].z; tot[m].w = tot[m].w + acc[m].w; } else tot[m] = acc[m]; acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
                    have = true;
                }
                cur = cid;
            }
            const float* wr = W + (size_t)((cil * L.kh + ky) * L.kw + kx) * L.N;
            const float* dp = dpre + (size_t)j * ng * cstride + (size_t)(oy * L.ow + ox) * B + b0 + l15;
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
#pragma unroll
    for (int m = 0; m < MT; m++) {
        f32x4 v = acc[m];
        if (have) { v.x = tot[m].x + v.x; v.y = tot[m].y + v.y; v.z = tot[m].z + v.z; v.w = tot[m].w + v.w; }
        const int bcol = b0 + 16 * m + 4 * kq;
        if (ysrc) { const f32x4 y = *reinterpret_cast<const f32x4*>(ysrc + feat * ldy + bcol); dact_v4(v, y, act_src); }
        *reinterpret_cast<f32x4*>(out + feat * B + bcol) = v;
    }
}

// dW / db: task = (channel tile inside ONE group, 16 rows of the (K+1) x N block, plan chunk); row K is the bias gradient (A operand 1: fma(1, d, acc) == acc + d)
template <int NT, int U8>
__global__ __launch_bounds__(256) void k_cdg_mfma_dw(LayerDev L, const void* __restrict__ X, int ldx, const float* __restrict__ dpre, int B, int S, int kc, float* __restrict__ out, int ntasks) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    int task = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6));
    if (task >= ntasks) return;
    const int ngroups = L.N / (16 * NT), mtiles = (L.K + 1 + 15) / 16;
    const int ng = task % ngroups; task /= ngroups;
    const int mt = task % mtiles; const int s = task / mtiles;
    const int n0 = ng * 16 * NT;
    const int cb = (n0 / (L.N / L.groups)) * (L.cin / L.groups);
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
        const int oy = pos / L.ow, ox = pos % L.ow; const int iy = oy * L.sh + ky * L.dh - L.ph, ix = ox * L.sw + kx * L.dw - L.pw;
        const bool in = real && iy >= 0 && iy < L.ih && ix >= 0 && ix < L.iw;
        const size_t xr = in ? (size_t)((ci * L.ih + iy) * L.iw + ix) * ldx + kq : 0;
        const float afix = real ? 0.0f : aconst;           // a tap beyond the border: an exact 0
        const float* dr = dpre + ((size_t)(n0 + l15) * L.npos + pos) * B + kq;
        constexpr int U = 8;
        for (; bs + U <= bsteps; bs += U) {
            float av[U], bv[U][NT];
#pragma unroll
            for (int u = 0; u < U; u++) {
                av[u] = in ? ld_xg<U8>(X, xr + 4 * (bs + u)) : afix;
#pragma unroll
                for (int t = 0; t < NT; t++) bv[u][t] = dr[t * nstride + 4 * (bs + u)];
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int t = 0; t < NT; t++) acc[t] = MFMA(av[u], bv[u][t], acc[t]);
        }
        for (; bs < bsteps; bs++) {
            const float a = in ? ld_xg<U8>(X, xr + 4 * bs) : afix;
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

// ------------------------------------------------------------------ launchers (mf: hp.use_mfma).  thin first, then the MFMA form where the shape tiles, else the VALU form -- the same bits
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool cdg_thin(const LayerDev& L) { return L.cin == L.groups || L.K < 16; }      // depthwise, or a contraction shorter than one MFMA tile row
void launch_cdg_fwd(hipStream_t st, const LayerDev& L, const float* P, const void* X, int ldx, int col0, int ncols, float* Y, int mf, int xu8) {
    const int ng = L.N / L.groups;
    if (cdg_thin(L)) {
        const bool vec = !(ldx % 4 || col0 % 4 || ncols % 4) && al16(Y) && (xu8 ? ((uintptr_t)X & 3) == 0 : al16(X));
        const size_t tot = (size_t)L.N * L.npos * ((ncols + 3) / 4); const dim3 g((unsigned)((tot + 255) / 256)), b(256);
#define CTF(u, v) hipLaunchKernelGGL((k_cdg_thin_fwd<u, v>), g, b, 0, st, L, P, X, ldx, col0, ncols, Y)
        if (xu8) { if (vec) CTF(1, 1); else CTF(1, 0); } else { if (vec) CTF(0, 1); else CTF(0, 0); }
#undef CTF
        return;
    }
    const int S = dqn_nchunks(L.K, L.fwd_kc), kc = dqn_chunk_len(L.K, L.fwd_kc);
    if (mf && !(ng % 16 || ncols % 16 || L.K % 4 || (S > 1 && kc % 4) || L.K > 16384 || L.kh > 255 || L.kw > 255 || L.cin > 32767) && al16(Y)) {
        const int MT = (ncols % 32 == 0 && (long)(ncols / 32) * (L.N / 16) * L.npos >= 1024) ? 2 : 1, NT = ng % 32 == 0 ? 2 : 1;
        const int ntasks = (L.N / (16 * NT)) * (ncols / (16 * MT)) * L.npos; const size_t lds = (size_t)L.K * sizeof(int); const dim3 g((ntasks + 3) / 4), b(256);
#define CGF(m, n, u) hipLaunchKernelGGL((k_cdg_mfma_fwd<m, n, u>), g, b, lds, st, L, P, X, ldx, col0, ncols, Y, ntasks)
        if (xu8) { if (MT == 2 && NT == 2) CGF(2, 2, 1); else if (MT == 2) CGF(2, 1, 1); else if (NT == 2) CGF(1, 2, 1); else CGF(1, 1, 1); }
        else     { if (MT == 2 && NT == 2) CGF(2, 2, 0); else if (MT == 2) CGF(2, 1, 0); else if (NT == 2) CGF(1, 2, 0); else CGF(1, 1, 0); }
#undef CGF
        return;
    }
    const size_t tot = (size_t)L.N * L.npos * ncols; const dim3 g((unsigned)((tot + 255) / 256)), b(256);
    if (xu8) hipLaunchKernelGGL(k_cdg_fwd<1>, g, b, 0, st, L, P, X, ldx, col0, ncols, Y);
    else hipLaunchKernelGGL(k_cdg_fwd<0>, g, b, 0, st, L, P, X, ldx, col0, ncols, Y);
}
// dst: the layer's (K+1) x N gradient block, or S = dqn_nchunks(npos*B, dw_kc) slabs of it.  A thin layer's weights are few: one thread per (chunk, weight) whatever mf says (k_cdg_thin_dw)
void launch_cdg_dw(hipStream_t st, const LayerDev& L, const void* X, int ldx, const float* dpre, int B, float* dst, int mf, int xu8) {
    const int KK = L.npos * B, S = dqn_nchunks(KK, L.dw_kc), kc = dqn_chunk_len(KK, L.dw_kc); const int ng = L.N / L.groups;
    if (mf && !cdg_thin(L) && !(ng % 16 || B % 4 || (S > 1 && kc % 4))) {      // whole positions per chunk, or chunks cut in samples (large batches): multiples of 4 either way
        const int NT = ng % 32 == 0 ? 2 : 1; const int ntasks = (L.N / (16 * NT)) * ((L.K + 1 + 15) / 16) * S; const dim3 g((ntasks + 3) / 4), b(256);
        if (xu8) { if (NT == 2) hipLaunchKernelGGL((k_cdg_mfma_dw<2, 1>), g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst, ntasks); else hipLaunchKernelGGL((k_cdg_mfma_dw<1, 1>), g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst, ntasks); }
        else     { if (NT == 2) hipLaunchKernelGGL((k_cdg_mfma_dw<2, 0>), g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst, ntasks); else hipLaunchKernelGGL((k_cdg_mfma_dw<1, 0>), g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst, ntasks); }
        return;
    }
    const size_t tot = (size_t)(L.K + 1) * L.N * S; const dim3 g((unsigned)((tot + 255) / 256)), b(256);
    if (cdg_thin(L)) {
        const bool vec = !(B % 4 || ldx % 4 || (S > 1 && kc % 4)) && al16(dpre) && (xu8 ? ((uintptr_t)X & 3) == 0 : al16(X));
#define CTW(u, v) hipLaunchKernelGGL((k_cdg_thin_dw<u, v>), g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst)
        if (xu8) { if (vec) CTW(1, 1); else CTW(1, 0); } else { if (vec) CTW(0, 1); else CTW(0, 0); }
#undef CTW
        return;
    }
    if (xu8) hipLaunchKernelGGL(k_cdg_dw<1>, g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst);
    else hipLaunchKernelGGL(k_cdg_dw<0>, g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst);
}
void launch_cdg_dx(hipStream_t st, const LayerDev& L, const float* P, const float* dpre, int B, float* out, const float* ysrc, int ldy, int act_src, int mf) {
    const int cg = L.cin / L.groups, ng = L.N / L.groups;
    if (cdg_thin(L)) {
        const bool vec = !(B % 4 || ldy % 4) && al16(out) && al16(ysrc) && al16(dpre);
        const size_t tot = (size_t)L.in_feat * ((B + 3) / 4); const dim3 g((unsigned)((tot + 255) / 256)), b(256);
        if (vec) hipLaunchKernelGGL(k_cdg_thin_dx<1>, g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src);
        else hipLaunchKernelGGL(k_cdg_thin_dx<0>, g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src);
        return;
    }
    if (mf && !(B % 16 || ng % 4 || cg % 16 || ldy % 4) && al16(out) && al16(ysrc)) {
        const int MT = (B % 32 == 0 && (long)(B / 32) * (L.cin / 16) * L.ih * L.iw >= 1024) ? 2 : 1;
        const int ntasks = (B / (16 * MT)) * (L.cin / 16) * L.ih * L.iw; const dim3 g((ntasks + 3) / 4), b(256);
        if (MT == 2) hipLaunchKernelGGL(k_cdg_mfma_dx<2>, g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src, ntasks);
        else hipLaunchKernelGGL(k_cdg_mfma_dx<1>, g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src, ntasks);
        return;
    }
    const size_t tot = (size_t)L.in_feat * B; const dim3 g((unsigned)((tot + 255) / 256)), b(256);
    hipLaunchKernelGGL(k_cdg_dx, g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src);
}
