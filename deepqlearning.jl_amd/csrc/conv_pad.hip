// conv_pad.hip -- Conv((kh, kw), cin => cout, act; stride, pad = (ph, pw)) with SYMMETRIC ZERO PADDING: forward, dX and dW / db as implicit GEMMs whose operand
// loads carry the border as a predicate (iy = oy*sh + ky - ph in [0, ih), likewise x; else the operand is an exact 0).  No zero-bordered scratch map, no crop.
//
// Canonical order ("Padded convolutions"): a padded conv IS the pad-0 conv of nn_valu.hip / nn_mfma.hip / nn_gemm.hip on the zero-extended map,
// under the same dqn_layer_plan:
//   forward   per plan chunk (fwd_kc) one k = (ci, ky, kx)-ascending fmaf chain from +0; chunk sums added in ascending order, + bias, activation
//   dW / db   per plan chunk (dw_kc) one (position, sample)-ascending chain; oh*ow is the padded layer's own; slabs [S][(K+1)][N] are summed by the step's reduce / Adam launch
//   dX        per input element, per chunk of RAW taps (dx_kc) one chain over the VALID taps with co innermost: (iy + ph - ky) divisible by sh with quotient in [0, oh),
//             likewise x -- the interior crop of the extended map's dX; then the producing layer's activation derivative
// The VALU kernels SKIP an out-of-range tap, the MFMA kernels multiply by the exact zero: the same bits, because a chain that starts at +0 never holds -0 under
// round-to-nearest, so fma(0, w, acc) == acc for every finite w.
//
// Two forms of each contraction, bit-identical: fp32 MFMA (v_mfma_f32_16x16x4_f32, one wave = one register tile, operands straight from L2 as in nn_mfma.hip) where the
// channel / column counts tile by 16, one thread per output element otherwise.  A first-layer padded conv may read the BYTE arena of a u8 replay (xu8): value = u8_unit(byte),
// and a zero byte is an exact 0.
//
// Residual epilogues (the join of a convolutional skip block, DQN_LAYER_SKIPADD_MAP; DESIGN.md section 4 "Convolutional skip blocks"), template parameter RES / ADD:
//   forward   Y = act(tot + bias) + R        R = the stored output of the block's entry P on this pass's columns ([out_feat][ldr], window rcol0): the block's LAST inner
//                                            layer writes the JOIN's activation; one fp32 add behind the activation, the add skip.hip's k_skip_fwd makes in a launch of its own
//   dX        out = dact(acc + dY, y_P, act_P)   dY = dact[join] ([in_feat][B]): the block's FIRST inner layer writes dact[P]; the add and the derivative k_skip_bwd_entry makes
// The same operands in the same order as the separate launches, hence the same bits.  The addend comes straight from global memory (no LDS, no atomics); its loads are issued
// together, before the first use: in front of the contraction where that costs one register (VALU forms), at the head of the epilogue where it would cost a register tile
// held across the whole MFMA loop (MT x NT x 4 VGPRs).  RES = ADD = 0 compiles to the kernels without the operand: a padded conv outside a block keeps its code and its bits.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// the operand X[(ci, iy, ix)][col] of the UNPADDED map, float or byte arena
template <int U8> __device__ __forceinline__ float ld_x(const void* __restrict__ X, size_t i) {
    if (U8) return u8_unit(reinterpret_cast<const unsigned char*>(X)[i]);
    return reinterpret_cast<const float*>(X)[i];
}

// ------------------------------------------------------------------ VALU: one thread per output element
template <int U8, int RES>
__global__ __launch_bounds__(256) void k_cpad_fwd(LayerDev L, const float* __restrict__ P, const void* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y,
                                                  const float* __restrict__ R, int ldr, int rcol0) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)L.N * L.npos * ncols) return;
    const int col = (int)(t % ncols); const int pos = (int)((t / ncols) % L.npos); const int n = (int)(t / ((size_t)ncols * L.npos));
    const int oy = pos / L.ow, ox = pos % L.ow; const int y0 = oy * L.sh - L.ph, x0 = ox * L.sw - L.pw;
    const float* W = P + L.w_off;
    const int S = dqn_nchunks(L.K, L.fwd_kc), kc = dqn_chunk_len(L.K, L.fwd_kc), khw = L.kh * L.kw;
    float res = 0.0f; if (RES) res = R[((size_t)n * L.npos + pos) * ldr + rcol0 + col];      // in flight under the contraction
    float tot = 0.0f;
    for (int s = 0; s < S; s++) {
        const int k0 = s * kc, k1 = min(L.K, k0 + kc);
        int ci = k0 / khw, ky = (k0 / L.kw) % L.kh, kx = k0 % L.kw;
        float acc = 0.0f;
        for (int k = k0; k < k1; k++) {
            const int iy = y0 + ky, ix = x0 + kx;
            if (iy >= 0 && iy < L.ih && ix >= 0 && ix < L.iw)
                acc = fmaf(ld_x<U8>(X, (size_t)((ci * L.ih + iy) * L.iw + ix) * ldx + col0 + col), W[(size_t)k * L.N + n], acc);
            if (++kx == L.kw) { kx = 0; if (++ky == L.kh) { ky = 0; ++ci; } }
        }
        tot = s == 0 ? acc : tot + acc;
    }
    const float y = act_f(tot + P[L.b_off + n], L.act);
    Y[t] = RES ? y + res : y;
}

// thread = (chunk, k, n) for k < K, plus the virtual row k == K of the bias gradient; out = slabs [S][(K+1)][N] (S == 1: the gradient block itself)
template <int U8>
__global__ __launch_bounds__(256) void k_cpad_dw(LayerDev L, const void* __restrict__ X, int ldx, const float* __restrict__ dpre, int B, int S, int kc, float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per_s = (size_t)(L.K + 1) * L.N;
    if (t >= per_s * S) return;
    const int s = (int)(t / per_s); const size_t e = t % per_s;
    const int n = (int)(e % L.N), k = (int)(e / L.N);
    const int KK = L.npos * B, j0 = s * kc, j1 = min(KK, j0 + kc);
    const int khw = L.kh * L.kw; const int ci = k / khw, ky = (k / L.kw) % L.kh, kx = k % L.kw;      // (unused for the bias row)
    float acc = 0.0f;
    int pos = j0 / B, b = j0 % B;
    for (int j = j0; j < j1; j++) {
        const float d = dpre[((size_t)n * L.npos + pos) * B + b];
        if (k < L.K) {
            const int oy = pos / L.ow, ox = pos % L.ow; const int iy = oy * L.sh + ky - L.ph, ix = ox * L.sw + kx - L.pw;
            if (iy >= 0 && iy < L.ih && ix >= 0 && ix < L.iw) acc = fmaf(ld_x<U8>(X, (size_t)((ci * L.ih + iy) * L.iw + ix) * ldx + b), d, acc);
        } else acc = acc + d;
        if (++b == B) { b = 0; ++pos; }
    }
    out[(size_t)s * per_s + e] = acc;
}

// ADD: dY is the join's gradient.  With a single inner layer it IS the buffer dpre points at: both are only read, which __restrict__ allows
template <int ADD>
__global__ __launch_bounds__(256) void k_cpad_dx(LayerDev L, const float* __restrict__ P, const float* __restrict__ dpre, int B, float* __restrict__ out,
                                                 const float* __restrict__ ysrc, int ldy, int act_src, const float* __restrict__ dY) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)L.in_feat * B) return;
    float add = 0.0f; if (ADD) add = dY[e];      // in flight under the contraction
    const int b = (int)(e % B); const int feat = (int)(e / B);
    const float* W = P + L.w_off;
    const int hw = L.ih * L.iw; const int ci = feat / hw, iy = (feat % hw) / L.iw, ix = feat % L.iw;
    const int tc = DQN_CONV_TAP_CHUNK(L); int cur = -1; bool have = false; float tot = 0.0f, acc = 0.0f;
    for (int ky = 0; ky < L.kh; ky++) {
        const int ty = iy + L.ph - ky; if (ty < 0 || ty % L.sh) continue; const int oy = ty / L.sh; if (oy >= L.oh) continue;
        for (int kx = 0; kx < L.kw; kx++) {
            const int tx = ix + L.pw - kx; if (tx < 0 || tx % L.sw) continue; const int ox = tx / L.sw; if (ox >= L.ow) continue;
            const int cid = (ky * L.kw + kx) / tc;
            if (cid != cur) { if (cur >= 0) { tot = have ? tot + acc : acc; have = true; acc = 0.0f; } cur = cid; }
            const float* wr = W + (size_t)((ci * L.kh + ky) * L.kw + kx) * L.N; const int pos = oy * L.ow + ox;
            for (int co = 0; co < L.N; co++) acc = fmaf(dpre[((size_t)co * L.npos + pos) * B + b], wr[co], acc);
        }
    }
    if (have) acc = tot + acc;
    if (ADD) acc = acc + add;
    if (ysrc) acc = dact_f(acc, ysrc[(size_t)feat * ldy + b], act_src);
    out[e] = acc;
}

// ------------------------------------------------------------------ MFMA: one wave = one register tile (operand layouts: nn_mfma.hip)
// forward: task = (channel group, column group, position); the wave walks the plan chunks itself and adds the chunk sums in ascending order
template <int MT, int NT, int U8, int RES>
__global__ __launch_bounds__(256) void k_cpad_mfma_fwd(LayerDev L, const float* __restrict__ P, const void* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y, int ntasks,
                                                       const float* __restrict__ R, int ldr, int rcol0) {
    extern __shared__ int tap_lds[];      // k -> (ci << 16 | ky << 8 | kx)
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
    const int oy = pos / L.ow, ox = pos % L.ow; const int y0 = oy * L.sh - L.ph, x0 = ox * L.sw - L.pw;
    const float* Wp = P + L.w_off + n0 + l15;
    const size_t xcol = (size_t)col0 + c0 + l15;
    const int S = dqn_nchunks(L.K, L.fwd_kc), kc = dqn_chunk_len(L.K, L.fwd_kc);
    auto lda = [&](int k, float (&a)[MT]) {      // the A operand of MFMA step k: 16 columns of one input element, or zeros beyond the border
        const int tp = tap_lds[k]; const int ci = tp >> 16, iy = y0 + ((tp >> 8) & 255), ix = x0 + (tp & 255);
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

// dX: task = (column group, 16 input channels, input position)
template <int MT, int ADD>
__global__ __launch_bounds__(256) void k_cpad_mfma_dx(LayerDev L, const float* __restrict__ P, const float* __restrict__ dpre, int B, float* __restrict__ out,
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
    const size_t feat = (size_t)ci * L.ih * L.iw + ip;
    f32x4 acc[MT], tot[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) { acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; tot[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    const int tc = DQN_CONV_TAP_CHUNK(L); int cur = -1; bool have = false;
    const unsigned cstride = (unsigned)L.npos * (unsigned)B;
    for (int ky = 0; ky < L.kh; ky++) {
        const int ty = iy + L.ph - ky; if (ty < 0 || ty % L.sh) continue; const int oy = ty / L.sh; if (oy >= L.oh) continue;
        for (int kx = 0; kx < L.kw; kx++) {
            const int tx = ix + L.pw - kx; if (tx < 0 || tx % L.sw) continue; const int ox = tx / L.sw; if (ox >= L.ow) continue;
            const int cid = (ky * L.kw + kx) / tc;
            if (cid != cur) {
                if (cur >= 0) {
#pragma unroll
                    for (int m = 0; m < MT; m++) { if (have) { tot[m].x = tot[m].x + acc[m].x; tot[m].y = tot[m].y + acc[m].y; tot[m].z = tot[m].z + acc[m].z; tot[m].w = tot[m].w + acc[m].w; } else tot[m] = acc[m]; acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
                    have = true;
                }
                cur = cid;
            }
            const float* wr = W + (size_t)((ci * L.kh + ky) * L.kw + kx) * L.N;
            const float* dp = dpre + (size_t)(oy * L.ow + ox) * B + b0 + l15;
            constexpr int U = 8;
            int co = kq;
            for (; co + 4 * (U - 1) < L.N; co += 4 * U) {
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
            for (; co < L.N; co += 4) {
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

// dW / db: task = (channel group, 16 rows of the (K+1) x N block, plan chunk); row K is the bias gradient (A operand 1: fma(1, d, acc) == acc + d).  Chunks cover whole positions or are cut in samples (multiples of 4)
template <int NT, int U8>
__global__ __launch_bounds__(256) void k_cpad_mfma_dw(LayerDev L, const void* __restrict__ X, int ldx, const float* __restrict__ dpre, int B, int S, int kc, float* __restrict__ out, int ntasks) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    int task = __builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6));
    if (task >= ntasks) return;
    const int ngroups = L.N / (16 * NT), mtiles = (L.K + 1 + 15) / 16;
    const int ng = task % ngroups; task /= ngroups;
    const int mt = task % mtiles; const int s = task / mtiles;
    const int n0 = ng * 16 * NT;
    const int krow = mt * 16 + l15;                       // this lane's A row
    const bool real = krow < L.K; const float aconst = krow == L.K ? 1.0f : 0.0f;
    int ci = 0, ky = 0, kx = 0;
    if (real) { const int khw = L.kh * L.kw; ci = krow / khw; ky = (krow / L.kw) % L.kh; kx = krow % L.kw; }
    const int KK = L.npos * B, j0 = s * kc, j1 = min(KK, j0 + kc);
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const unsigned nstride = 16u * (unsigned)L.npos * (unsigned)B;
    for (int pos = j0 / B; pos * B < j1; pos++) {
        // the chunk's samples of this position, in MFMA steps of 4 (chunk bounds and B are multiples of 4: a step never straddles a position or a chunk)
        const int bsteps = (min(j1, (pos + 1) * B) - pos * B) / 4; int bs = (max(j0, pos * B) - pos * B) / 4;
        const int oy = pos / L.ow, ox = pos % L.ow; const int iy = oy * L.sh + ky - L.ph, ix = ox * L.sw + kx - L.pw;
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

// ------------------------------------------------------------------ launchers (mf: hp.use_mfma; the MFMA form where the shape tiles, else the VALU form -- the same bits)
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool cpad_mfma_fwd_ok(const LayerDev& L, int ncols, const float* Y) {
    const int S = dqn_nchunks(L.K, L.fwd_kc), kc = dqn_chunk_len(L.K, L.fwd_kc);
    return !(L.N % 16 || ncols % 16 || L.K % 4 || (S > 1 && kc % 4) || L.K > 16384 || L.kh > 255 || L.kw > 255 || L.cin > 32767) && al16(Y);
}
void launch_cpad_fwd(hipStream_t st, const LayerDev& L, const float* P, const void* X, int ldx, int col0, int ncols, float* Y, int mf, int xu8, const float* R, int ldr, int rcol0) {
    if (R) {      // the fused join of a map block (an inner layer never reads the observation: no byte arena); the addend tile is read 16 bytes per lane where its rows allow it
        if (mf && cpad_mfma_fwd_ok(L, ncols, Y) && !(ldr % 4 || rcol0 % 4) && al16(R)) {
            const int MT = (ncols % 32 == 0 && (long)(ncols / 32) * (L.N / 16) * L.npos >= 1024) ? 2 : 1, NT = L.N % 32 == 0 ? 2 : 1;
            const int ntasks = (L.N / (16 * NT)) * (ncols / (16 * MT)) * L.npos; const size_t lds = (size_t)L.K * sizeof(int); const dim3 g((ntasks + 3) / 4), b(256);
#define CPR(m, n) hipLaunchKernelGGL((k_cpad_mfma_fwd<m, n, 0, 1>), g, b, lds, st, L, P, X, ldx, col0, ncols, Y, ntasks, R, ldr, rcol0)
            if (MT == 2 && NT == 2) CPR(2, 2); else if (MT == 2) CPR(2, 1); else if (NT == 2) CPR(1, 2); else CPR(1, 1);
#undef CPR
            return;
        }
        const size_t tot = (size_t)L.N * L.npos * ncols; const dim3 g((unsigned)((tot + 255) / 256)), b(256);
        hipLaunchKernelGGL((k_cpad_fwd<0, 1>), g, b, 0, st, L, P, X, ldx, col0, ncols, Y, R, ldr, rcol0);
        return;
    }
    if (mf && cpad_mfma_fwd_ok(L, ncols, Y)) {
        const int MT = (ncols % 32 == 0 && (long)(ncols / 32) * (L.N / 16) * L.npos >= 1024) ? 2 : 1, NT = L.N % 32 == 0 ? 2 : 1;
        const int ntasks = (L.N / (16 * NT)) * (ncols / (16 * MT)) * L.npos; const size_t lds = (size_t)L.K * sizeof(int); const dim3 g((ntasks + 3) / 4), b(256);
#define CPF(m, n, u) hipLaunchKernelGGL((k_cpad_mfma_fwd<m, n, u, 0>), g, b, lds, st, L, P, X, ldx, col0, ncols, Y, ntasks, (const float*)nullptr, 0, 0)
        if (xu8) { if (MT == 2 && NT == 2) CPF(2, 2, 1); else if (MT == 2) CPF(2, 1, 1); else if (NT == 2) CPF(1, 2, 1); else CPF(1, 1, 1); }
        else     { if (MT == 2 && NT == 2) CPF(2, 2, 0); else if (MT == 2) CPF(2, 1, 0); else if (NT == 2) CPF(1, 2, 0); else CPF(1, 1, 0); }
#undef CPF
        return;
    }
    const size_t tot = (size_t)L.N * L.npos * ncols; const dim3 g((unsigned)((tot + 255) / 256)), b(256);
    if (xu8) hipLaunchKernelGGL((k_cpad_fwd<1, 0>), g, b, 0, st, L, P, X, ldx, col0, ncols, Y, (const float*)nullptr, 0, 0);
    else hipLaunchKernelGGL((k_cpad_fwd<0, 0>), g, b, 0, st, L, P, X, ldx, col0, ncols, Y, (const float*)nullptr, 0, 0);
}
// dst: the layer's (K+1) x N gradient block, or S = dqn_nchunks(npos*B, dw_kc) slabs of it
void launch_cpad_dw(hipStream_t st, const LayerDev& L, const void* X, int ldx, const float* dpre, int B, float* dst, int mf, int xu8) {
    const int KK = L.npos * B, S = dqn_nchunks(KK, L.dw_kc), kc = dqn_chunk_len(KK, L.dw_kc);
    if (mf && !(L.N % 16 || B % 4 || (S > 1 && kc % 4))) {      // whole positions per chunk, or chunks cut in samples (large batches): multiples of 4 either way
        const int NT = L.N % 32 == 0 ? 2 : 1; const int ntasks = (L.N / (16 * NT)) * ((L.K + 1 + 15) / 16) * S; const dim3 g((ntasks + 3) / 4), b(256);
        if (xu8) { if (NT == 2) hipLaunchKernelGGL((k_cpad_mfma_dw<2, 1>), g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst, ntasks); else hipLaunchKernelGGL((k_cpad_mfma_dw<1, 1>), g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst, ntasks); }
        else     { if (NT == 2) hipLaunchKernelGGL((k_cpad_mfma_dw<2, 0>), g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst, ntasks); else hipLaunchKernelGGL((k_cpad_mfma_dw<1, 0>), g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst, ntasks); }
        return;
    }
    const size_t tot = (size_t)(L.K + 1) * L.N * S; const dim3 g((unsigned)((tot + 255) / 256)), b(256);
    if (xu8) hipLaunchKernelGGL(k_cpad_dw<1>, g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst);
    else hipLaunchKernelGGL(k_cpad_dw<0>, g, b, 0, st, L, X, ldx, dpre, B, S, kc, dst);
}
void launch_cpad_dx(hipStream_t st, const LayerDev& L, const float* P, const float* dpre, int B, float* out, const float* ysrc, int ldy, int act_src, int mf, const float* dY) {
    if (mf && !(B % 16 || L.N % 4 || L.cin % 16 || ldy % 4) && al16(out) && al16(ysrc) && al16(dY)) {
        const int MT = (B % 32 == 0 && (long)(B / 32) * (L.cin / 16) * L.ih * L.iw >= 1024) ? 2 : 1;
        const int ntasks = (B / (16 * MT)) * (L.cin / 16) * L.ih * L.iw; const dim3 g((ntasks + 3) / 4), b(256);
        if (dY) { if (MT == 2) hipLaunchKernelGGL((k_cpad_mfma_dx<2, 1>), g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src, ntasks, dY);
                  else hipLaunchKernelGGL((k_cpad_mfma_dx<1, 1>), g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src, ntasks, dY); }
        else if (MT == 2) hipLaunchKernelGGL((k_cpad_mfma_dx<2, 0>), g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src, ntasks, dY);
        else hipLaunchKernelGGL((k_cpad_mfma_dx<1, 0>), g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src, ntasks, dY);
        return;
    }
    const size_t tot = (size_t)L.in_feat * B; const dim3 g((unsigned)((tot + 255) / 256)), b(256);
    if (dY) hipLaunchKernelGGL(k_cpad_dx<1>, g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src, dY);
    else hipLaunchKernelGGL(k_cpad_dx<0>, g, b, 0, st, L, P, dpre, B, out, ysrc, ldy, act_src, dY);
}
