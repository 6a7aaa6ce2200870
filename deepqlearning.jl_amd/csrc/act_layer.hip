// act_layer.hip -- the standalone activation layer (DQN_LAYER_ACTIVATION; Flux: Base.Broadcast.BroadcastFunction(σ) in a Chain) over the batch-innermost Y[feature][column]
// layout: y = σ(x) per element, no parameters, the incoming shape kept.  No contraction, no MFMA: both launches are bandwidth- and launch-bound.
//
// The law ("Activation layers"):
//   forward   codes 0..10: act_f(x, σ), the very function the fused epilogues of Dense / Conv / LayerNorm / GroupNorm call -- Dense(n, m) -> Activation(σ) gives the bits of
//             Dense(n, m, σ).  Codes 11..14 (gelu, swish, mish, hardswish) go through Float64 and round once, as tanh / sigmoid do:
//               gelu      0.5 x (1 + tanh(sqrt(2/π) (x + 0.044715 x³)))      NNlib's tanh form, not the erf form
//               swish     x sigm(x)
//               mish      x tanh(softplus(x)),  softplus(x) = log1p(exp(-|x|)) + max(x, 0) as act_slow writes it
//               hardswish x clamp((x + 3) / 6, 0, 1)
//   backward  dX = (dY σ′) then the producing layer's activation derivative on that layer's output (dact_f with act_src: the layer's input IS that output), as a pool's backward.
//             Codes 0..10: dY σ′ = dact_f(dY, y, σ) from the layer's OWN output y -- the arithmetic the fused layer's consumer runs in its dX epilogue, bit for bit.
//             Codes 11..14: σ′ from the INPUT x in Float64, rounded once to fp32, then ONE fp32 multiply dY * σ′:
//               gelu′      0.5 (1 + t) + 0.5 x (1 - t²) sqrt(2/π) (1 + 3 * 0.044715 x²),  t the tanh above
//               swish′     s (1 + x (1 - s)),  s = sigm(x)
//               mish′      t + x (1 - t²) sigm(x),  t = tanh(softplus(x))
//               hardswish′ 0 for x < -3, 1 for x > 3, (2x + 3) / 6 between
//             The bodies of the four live HERE only: inside act_slow / dact_new (common.h) they would sit, as branch targets nobody takes, in every GEMM kernel.
// Work split (pool.hip's): a thread owns (feature, four adjacent columns).  Where leading dimension, column offset and column count are multiples of 4 and the bases are
// 16-byte aligned the four columns are ONE 16-byte access; otherwise (B = 5: ten columns, the target pass starting at column 5) the thread walks its columns one by one.
// Element-wise: nothing depends on the column count, the path, graph or eager.  No LDS, no atomics, plain vector stores.
#include "common.h"

#define ACTL_GELU_C 0.7978845608028654      /* sqrt(2 / pi) */
#define ACTL_GELU_A 0.044715

__device__ __forceinline__ double actl_sigm(double x) { return 1.0 / (1.0 + exp(-x)); }
__device__ __forceinline__ double actl_softplus(double x) { return log1p(exp(-fabs(x))) + (x > 0.0 ? x : 0.0); }

// the forwards of the codes above DQN_ACT_LAST, out of line (one copy per kernel, not four per vector)
__device__ __attribute__((noinline)) static float actl_fwd_x(float xf, int act) {
    const double x = (double)xf;
    switch (act) {
    case DQN_ACT_GELU: return (float)(0.5 * x * (1.0 + tanh(ACTL_GELU_C * (x + ACTL_GELU_A * x * x * x))));
    case DQN_ACT_SWISH: return (float)(x * actl_sigm(x));
    case DQN_ACT_MISH: return (float)(x * tanh(actl_softplus(x)));
    case DQN_ACT_HARDSWISH: { const double h = (x + 3.0) / 6.0; return (float)(x * (h < 0.0 ? 0.0 : h > 1.0 ? 1.0 : h)); }
    default: return xf;
    }
}
// their derivatives from the input, Float64, rounded once
__device__ __attribute__((noinline)) static float actl_der_x(float xf, int act) {
    const double x = (double)xf;
    switch (act) {
    case DQN_ACT_GELU: { const double t = tanh(ACTL_GELU_C * (x + ACTL_GELU_A * x * x * x)); return (float)(0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * ACTL_GELU_C * (1.0 + 3.0 * ACTL_GELU_A * x * x)); }
    case DQN_ACT_SWISH: { const double s = actl_sigm(x); return (float)(s * (1.0 + x * (1.0 - s))); }
    case DQN_ACT_MISH: { const double t = tanh(actl_softplus(x)); return (float)(t + x * (1.0 - t * t) * actl_sigm(x)); }
    case DQN_ACT_HARDSWISH: return x < -3.0 ? 0.0f : x > 3.0 ? 1.0f : (float)((2.0 * x + 3.0) / 6.0);
    default: return 1.0f;
    }
}
__device__ __forceinline__ float actl_f(float x, int act) { return act > DQN_ACT_LAST ? actl_fwd_x(x, act) : act_f(x, act); }
// dY σ′: from the output y for the eleven (dact_f, as every dX epilogue), from the input x for the four
__device__ __forceinline__ float actl_d(float dy, float x, float y, int act) { return act > DQN_ACT_LAST ? dy * actl_der_x(x, act) : dact_f(dy, y, act); }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// X[n][ldx] read at columns col0 .. col0 + ncols; Y[n][ncols]
__global__ __launch_bounds__(256) void k_actl_fwd(int n, const float* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y, int act, int vec) {
    const int ng = (ncols + 3) >> 2;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t f = t / ng; const int c0 = (int)(t - f * ng) * 4;
    if (f >= (size_t)n) return;
    const float* xb = X + f * ldx + col0 + c0;
    float* yb = Y + f * ncols + c0;
    if (vec) {
        float4 v = ld4(xb);
        if (act == DQN_ACT_RELU) { v.x = v.x > 0.0f ? v.x : 0.0f; v.y = v.y > 0.0f ? v.y : 0.0f; v.z = v.z > 0.0f ? v.z : 0.0f; v.w = v.w > 0.0f ? v.w : 0.0f; }
        else if (act != DQN_ACT_IDENTITY) { v.x = actl_f(v.x, act); v.y = actl_f(v.y, act); v.z = actl_f(v.z, act); v.w = actl_f(v.w, act); }
        *reinterpret_cast<float4*>(yb) = v;
        return;
    }
    const int nj = min(4, ncols - c0);
    for (int j = 0; j < nj; j++) yb[j] = actl_f(xb[j], act);
}

// dY[n][B]; X[n][ld] = the layer's input = the producing layer's output, Y[n][ld] = the layer's output (online net, s columns 0 .. B); dX[n][B]
__global__ __launch_bounds__(256) void k_actl_bwd(int n, const float* __restrict__ dY, const float* __restrict__ X, const float* __restrict__ Y, int ld, int B, float* __restrict__ dX,
                                                  int act, int act_src, int vec) {
    const int ng = (B + 3) >> 2;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t f = t / ng; const int c0 = (int)(t - f * ng) * 4;
    if (f >= (size_t)n) return;
    const bool from_x = act > DQN_ACT_LAST;      // wave-uniform: σ′ from the input; else from the output
    if (vec) {
        float4 g = ld4(dY + f * B + c0);
        const float4 x = ld4(X + f * ld + c0);      // both loads in flight before the first use
        if (from_x) { g.x = g.x * actl_der_x(x.x, act); g.y = g.y * actl_der_x(x.y, act); g.z = g.z * actl_der_x(x.z, act); g.w = g.w * actl_der_x(x.w, act); }
        else if (act != DQN_ACT_IDENTITY) { const float4 y = ld4(Y + f * ld + c0); dact_v4(g, y, act); }
        dact_v4(g, x, act_src);
        *reinterpret_cast<float4*>(dX + f * B + c0) = g;
        return;
    }
    const int nj = min(4, B - c0);
    for (int j = 0; j < nj; j++) {
        const float x = X[f * ld + c0 + j], y = Y[f * ld + c0 + j];
        dX[f * B + c0 + j] = dact_f(actl_d(dY[f * B + c0 + j], x, y, act), x, act_src);
    }
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
void launch_actl_fwd(hipStream_t st, int n, int act, const float* X, int ldx, int col0, int ncols, float* Y) {
    const int vec = (ldx % 4 == 0 && col0 % 4 == 0 && ncols % 4 == 0 && al16(X) && al16(Y)) ? 1 : 0;
    const size_t threads = (size_t)n * ((ncols + 3) / 4); const unsigned blocks = (unsigned)((threads + 255) / 256);
    hipLaunchKernelGGL(k_actl_fwd, dim3(blocks), dim3(256), 0, st, n, X, ldx, col0, ncols, Y, act, vec);
}
void launch_actl_bwd(hipStream_t st, int n, int act, const float* dY, const float* X, const float* Y, int ld, int B, float* dX, int act_src) {
    const int vec = (ld % 4 == 0 && B % 4 == 0 && al16(dY) && al16(X) && al16(Y) && al16(dX)) ? 1 : 0;
    const size_t threads = (size_t)n * ((B + 3) / 4); const unsigned blocks = (unsigned)((threads + 255) / 256);
    hipLaunchKernelGGL(k_actl_bwd, dim3(blocks), dim3(256), 0, st, n, dY, X, Y, ld, B, dX, act, act_src, vec);
}
