// cell.h -- what the recurrent cell files (drqn.hip: LSTM, gru.hip, rnn.hip) share beyond common.h's argument structs: the Float64 gate
// activations, the column split of the whole-sequence kernels and the state0 gradient fold.  The cell kernels themselves stay apart: each
// file's header comment states its cell's canonical order.
#pragma once
#include "common.h"

// sigm / tanh through Float64, rounded once (Flux's Float32 activations)
__device__ __forceinline__ float sigm_f(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }
__device__ __forceinline__ float tanh_f(float x) { return (float)tanh((double)x); }

// whole-sequence kernels: batch columns are independent in the recurrence, so a sequence set is split into groups of CB columns (one workgroup each,
// its own LDS copy of Wh); H*CB ~ 256 outputs per step.  CB divides B.
static inline int cell_cb(int H, int B) { int cb = 256 / H; if (cb < 1) cb = 1; if (cb > B) cb = B; while (B % cb) cb--; return cb; }

// trainable state0: the gradient of unit u is the sum over the batch, ascending b, of the [H][B] gradient BPTT leaves behind step 0.
// HAS_C: the LSTM's cell state c beside h (dcn, g_c0; else unused).  A compile-time switch: the loop is one dependent load per iteration on a lone
// wave, and a test of dcn inside it measured 0.4-0.6 us per train step
template <bool HAS_C>
__device__ __forceinline__ void state0_fold(int u, int B, const float* __restrict__ dhn, const float* __restrict__ dcn, float* __restrict__ g_h0, float* __restrict__ g_c0) {
    float sh = 0.0f, sc = 0.0f;
    for (int b = 0; b < B; b++) { sh = sh + dhn[u * B + b]; if (HAS_C) sc = sc + dcn[u * B + b]; }
    g_h0[u] = sh; if (HAS_C) g_c0[u] = sc;
}
// the fold after a whole-sequence BPTT launch (whose workgroups each own a group of columns); dcn, g_c0 null: a cell without c
static __global__ void k_state0_grad(int H, int B, const float* __restrict__ dhn, const float* __restrict__ dcn, float* __restrict__ g_h0, float* __restrict__ g_c0) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= H) return;
    if (dcn) state0_fold<true>(u, B, dhn, dcn, g_h0, g_c0); else state0_fold<false>(u, B, dhn, nullptr, g_h0, nullptr);
}
static inline void launch_state0_grad(hipStream_t st, const CellBwdArgs& a) {
    hipLaunchKernelGGL(k_state0_grad, dim3((a.H + 63) / 64), dim3(64), 0, st, a.H, a.B, a.dhn, a.g_c0 ? a.dh2 : nullptr, a.g_h0, a.g_c0);
}
