// layernorm.hip -- Flux LayerNorm(n, act; affine = true, eps) over the batch-innermost Y[feature][column] layout: per batch column
//     mu = mean(x)   sigma = sqrt(mean((x - mu)^2))   x_hat = (x - mu) / (sigma + eps)   y = act(scale * x_hat + bias)
// (Flux 0.14 `normalise`: eps is added to sigma OUTSIDE the root -- not torch's sqrt(var + eps)).  fp32 throughout, two passes for the statistics (the mean, then the
// centred sum of squares).  No contraction, no MFMA: every launch here is bandwidth- and launch-bound.  The reduction runs along the STRIDED axis (features).
//
// Canonical order (DESIGN.md section 4 "LayerNorm layers"):
//   over the features of a column   feature f belongs to slot f mod 16; a slot sums its features in ascending f as one chain from +0 (sum x; fma chain of (x - mu)^2;
//                                   in the backward sum g and the fma chain g * x_hat, g = dpre * scale); the 16 slot sums are added in ascending slot order, slot 0 first.
//                                   mu = sum / f32(n); sigma = sqrt(sumsq / f32(n)); r = 1 / (sigma + eps); x_hat = (x - mu) * r; y = act(fma(scale, x_hat, bias)).
//                                   The order depends on n alone: not on the column count, the column's position, or which of the two work splits below runs.
//   over the columns of a feature   (dscale, dbias) lane l of a wave sums columns l, l + 64, ... ascending as one chain from +0 (dbias: sum dpre; dscale: fma chain dpre * x_hat);
//                                   the 64 lane sums are combined by the butterfly v += v[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.  The order depends on the column count alone.
//   dX                              r * (g - mean(g)) - x_hat * (mean(g * x_hat) / sigma), then the producing layer's activation derivative (dact_f on that layer's output = this
//                                   layer's input), exactly as a pool's backward does.  No float atomics anywhere.
// Work split: a workgroup of 256 threads owns a column tile; thread = (slot = tid / 16, column piece = tid mod 16).  Where every row start is 16-byte aligned (leading dimension,
// column offset and column count all multiples of 4) a piece is four columns as ONE 16-byte access -- 16 lanes cover a 256-byte row piece, a wave four rows -- and the tile is
// 64 columns; otherwise (B = 5: ten columns) a piece is one column and the tile 16 columns.  Slot sums meet in LDS ([16][tile] floats, every thread then reads the 16 sums of
// its own columns: the same address across the slots of a wave is a broadcast, adjacent pieces are adjacent banks).
#include "common.h"

template <int V> struct LnVec { float v[V]; };
template <int V> __device__ __forceinline__ LnVec<V> ln_ld(const float* p);
template <> __device__ __forceinline__ LnVec<1> ln_ld<1>(const float* p) { LnVec<1> r; r.v[0] = *p; return r; }
template <> __device__ __forceinline__ LnVec<4> ln_ld<4>(const float* p) { const float4 q = *reinterpret_cast<const float4*>(p); LnVec<4> r; r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w; return r; }
template <int V> __device__ __forceinline__ void ln_st(float* p, const LnVec<V>& a);
template <> __device__ __forceinline__ void ln_st<1>(float* p, const LnVec<1>& a) { *p = a.v[0]; }
template <> __device__ __forceinline__ void ln_st<4>(float* p, const LnVec<4>& a) { *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]); }

// the 16 slot sums of this thread's columns, slot 0 first (every thread of the tile computes the totals of its own columns)
template <int V> __device__ __forceinline__ LnVec<V> ln_combine(float* red, int slot, int cl, const LnVec<V>& mine) {
    __syncthreads();      // the previous round's readers are done
    ln_st<V>(red + slot * 16 * V + cl, mine);
    __syncthreads();
    LnVec<V> t = ln_ld<V>(red + cl);
#pragma unroll
    for (int s = 1; s < 16; s++) { const LnVec<V> o = ln_ld<V>(red + s * 16 * V + cl);
#pragma unroll
        for (int j = 0; j < V; j++) t.v[j] += o.v[j]; }
    return t;
}

// X[n][ldx] read at columns col0 .. col0 + ncols; Y[n][ncols]; stat (or null): mu at [c], sigma at [ncols + c]
template <int V> __global__ __launch_bounds__(256) void k_ln_fwd(int n, float eps, int act, const float* __restrict__ scale, const float* __restrict__ bias,
                                                                 const float* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y, float* __restrict__ stat) {
    __shared__ __attribute__((aligned(16))) float red[16 * 16 * V];
    const int tid = threadIdx.x, slot = tid >> 4, cl = (tid & 15) * V;
    const int c = blockIdx.x * 16 * V + cl;
    const bool live = c < ncols;      // V == 4: the column count is a multiple of 4, so a live piece is four live columns
    const float* xb = X + col0 + c;
    const float fn = (float)n;
    LnVec<V> s, q, mu, r;
#pragma unroll
    for (int j = 0; j < V; j++) s.v[j] = q.v[j] = 0.0f;
    if (live) {
#pragma unroll 4
        for (int f = slot; f < n; f += 16) { const LnVec<V> x = ln_ld<V>(xb + (size_t)f * ldx);
#pragma unroll
            for (int j = 0; j < V; j++) s.v[j] += x.v[j]; }
    }
    s = ln_combine<V>(red, slot, cl, s);
#pragma unroll
    for (int j = 0; j < V; j++) mu.v[j] = s.v[j] / fn;
    if (live) {
#pragma unroll 4
        for (int f = slot; f < n; f += 16) { const LnVec<V> x = ln_ld<V>(xb + (size_t)f * ldx);
#pragma unroll
            for (int j = 0; j < V; j++) { const float d = x.v[j] - mu.v[j]; q.v[j] = fmaf(d, d, q.v[j]); } }
    }
    q = ln_combine<V>(red, slot, cl, q);
#pragma unroll
    for (int j = 0; j < V; j++) { q.v[j] = sqrtf(q.v[j] / fn); r.v[j] = 1.0f / (q.v[j] + eps); }
    if (!live) return;      // no barrier below
    if (stat && slot == 0) { ln_st<V>(stat + c, mu); ln_st<V>(stat + ncols + c, q); }
#pragma unroll 4
    for (int f = slot; f < n; f += 16) {
        const LnVec<V> x = ln_ld<V>(xb + (size_t)f * ldx); const float sc = scale[f], bi = bias[f]; LnVec<V> y;
#pragma unroll
        for (int j = 0; j < V; j++) { const float xh = (x.v[j] - mu.v[j]) * r.v[j]; y.v[j] = act_f(fmaf(sc, xh, bi), act); }
        ln_st<V>(Y + (size_t)f * ncols + c, y);
    }
}

// dpre[n][B]; X[n][ld] (columns 0 .. B); stat: mu at [c], sigma at [ld_stat + c]; dX[n][B]
template <int V> __global__ __launch_bounds__(256) void k_ln_bwd_dx(int n, float eps, const float* __restrict__ scale, const float* __restrict__ dpre, const float* __restrict__ X, int ld,
                                                                    const float* __restrict__ stat, int ld_stat, int B, float* __restrict__ dX, int act_src) {
    __shared__ __attribute__((aligned(16))) float red[16 * 16 * V];
    const int tid = threadIdx.x, slot = tid >> 4, cl = (tid & 15) * V;
    const int c = blockIdx.x * 16 * V + cl;
    const bool live = c < B;
    const float fn = (float)n;
    LnVec<V> mu, sg, r, a, b;
#pragma unroll
    for (int j = 0; j < V; j++) { mu.v[j] = 0.0f; sg.v[j] = 1.0f; a.v[j] = b.v[j] = 0.0f; }
    if (live) { mu = ln_ld<V>(stat + c); sg = ln_ld<V>(stat + ld_stat + c); }
#pragma unroll
    for (int j = 0; j < V; j++) r.v[j] = 1.0f / (sg.v[j] + eps);
    if (live) {
#pragma unroll 4
        for (int f = slot; f < n; f += 16) {
            const LnVec<V> x = ln_ld<V>(X + (size_t)f * ld + c), d = ln_ld<V>(dpre + (size_t)f * B + c); const float sc = scale[f];
#pragma unroll
            for (int j = 0; j < V; j++) { const float g = d.v[j] * sc, xh = (x.v[j] - mu.v[j]) * r.v[j]; a.v[j] += g; b.v[j] = fmaf(g, xh, b.v[j]); }
        }
    }
    a = ln_combine<V>(red, slot, cl, a);
    b = ln_combine<V>(red, slot, cl, b);
    if (!live) return;      // no barrier below
#pragma unroll
    for (int j = 0; j < V; j++) { a.v[j] = a.v[j] / fn; b.v[j] = (b.v[j] / fn) / sg.v[j]; }
#pragma unroll 4
    for (int f = slot; f < n; f += 16) {
        const LnVec<V> x = ln_ld<V>(X + (size_t)f * ld + c), d = ln_ld<V>(dpre + (size_t)f * B + c); const float sc = scale[f]; LnVec<V> o;
#pragma unroll
        for (int j = 0; j < V; j++) {
            const float g = d.v[j] * sc, xh = (x.v[j] - mu.v[j]) * r.v[j];
            o.v[j] = dact_f(fmaf(-xh, b.v[j], r.v[j] * (g - a.v[j])), x.v[j], act_src);
        }
        ln_st<V>(dX + (size_t)f * B + c, o);
    }
}

// one wave per feature: g_scale[f] = sum over the B columns of dpre * x_hat, g_bias[f] = sum of dpre
__global__ __launch_bounds__(256) void k_ln_bwd_par(int n, float eps, const float* __restrict__ dpre, const float* __restrict__ X, int ld, const float* __restrict__ stat, int ld_stat, int B,
                                                    float* __restrict__ g_scale, float* __restrict__ g_bias) {
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= n) return;      // wave-uniform; no barrier in this kernel
    float ds = 0.0f, db = 0.0f;
    for (int c = lane; c < B; c += 64) {
        const float d = dpre[(size_t)f * B + c], r = 1.0f / (stat[ld_stat + c] + eps), xh = (X[(size_t)f * ld + c] - stat[c]) * r;
        db += d; ds = fmaf(d, xh, ds);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { ds += __shfl_xor(ds, o, 64); db += __shfl_xor(db, o, 64); }
    if (lane == 0) { g_scale[f] = ds; g_bias[f] = db; }
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
void launch_ln_fwd(hipStream_t st, const LayerDev& L, const float* P, const float* X, int ldx, int col0, int ncols, float* Y, float* stat) {
    const int n = L.N; const float eps = ln_eps(L); const float *scale = P + L.w_off, *bias = P + L.b_off;
    const bool vec = ldx % 4 == 0 && col0 % 4 == 0 && ncols % 4 == 0 && al16(X) && al16(Y) && (!stat || al16(stat));
    if (vec) hipLaunchKernelGGL(k_ln_fwd<4>, dim3((unsigned)((ncols + 63) / 64)), dim3(256), 0, st, n, eps, L.act, scale, bias, X, ldx, col0, ncols, Y, stat);
    else hipLaunchKernelGGL(k_ln_fwd<1>, dim3((unsigned)((ncols + 15) / 16)), dim3(256), 0, st, n, eps, L.act, scale, bias, X, ldx, col0, ncols, Y, stat);
}
void launch_ln_bwd(hipStream_t st, const LayerDev& L, const float* P, const float* dpre, const float* X, int ld, const float* stat, int ld_stat, int B, float* dX, int act_src,
                   float* g_scale, float* g_bias) {
    const int n = L.N; const float eps = ln_eps(L); const float* scale = P + L.w_off;
    const bool vec = ld % 4 == 0 && ld_stat % 4 == 0 && B % 4 == 0 && al16(dpre) && al16(X) && al16(stat) && al16(dX);
    if (vec) hipLaunchKernelGGL(k_ln_bwd_dx<4>, dim3((unsigned)((B + 63) / 64)), dim3(256), 0, st, n, eps, scale, dpre, X, ld, stat, ld_stat, B, dX, act_src);
    else hipLaunchKernelGGL(k_ln_bwd_dx<1>, dim3((unsigned)((B + 15) / 16)), dim3(256), 0, st, n, eps, scale, dpre, X, ld, stat, ld_stat, B, dX, act_src);
    hipLaunchKernelGGL(k_ln_bwd_par, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, eps, dpre, X, ld, stat, ld_stat, B, g_scale, g_bias);
}
