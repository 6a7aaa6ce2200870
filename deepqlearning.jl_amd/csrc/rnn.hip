// rnn.hip -- the plain RNN cell of the recurrent path (Flux 0.14 RNN = Recur(RNNCell); third-party, recalled like the LSTM's and the GRU's):
//   gx = Wi*x (H rows, bias-free, by the ordinary dense kernels over all T*B columns), gh = Wh*h_{t-1},  h' = act(gx + gh + b)
//   act = the cell's activation (Flux's sigma, default tanh; any DQN_ACT_*), carried in LayerDev::cell_act -- never in LayerDev::act, which the
//   generic forward / dX epilogues read.  Trainable state0 h0, broadcast over the batch (Flux.reset!).
// Canonical order, used by EVERY form below (step, sequence, policy step) so that they agree bit for bit:
//   gh   = chain_j (+0; j ascending) fma(h_{t-1}[j], Wh[j][u], .)
//   pre  = (gx + gh) + b ;  h' = act_f(pre, act)      (common.h: tanh / sigmoid through Float64, rounded once; relu and identity exact)
// BPTT per step, dh = (head gradient) + (dh_{t-1} of step t+1; +0 at t = T-1):
//   dG = dact_f(dh, h', act)                           (common.h's derivative from the output)
//   dG -> Wi | b dW, Wh dW (X = h_{t-1}) and the input dX (dense contractions over T*B columns).  The Wh | junk pass reads the same dG as
//         Wi | b, so its junk row equals db (as the LSTM's) and never raises max |g|: nothing to clear.
//   dh_{t-1}[j] = chain_n (+0; n ascending over H) fma(dG[n], Wh[j][n], .) ;  dstate0[u] = sum_b (ascending) dh_{-1}[u][b]
#include "cell.h"

// ------------------------------------------------------------------ one time step for up to 3 sequence sets (online s, online sp, target sp)
__global__ void k_rnn_step(CellFwdArgs A, int t) {
    const int per = A.H * A.B;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per * A.nseq) return;
    const CellSeq& S = A.s[i / per];
    const int e = i % per, u = e / A.B, b = e % A.B, H = A.H;
    const int col = S.c0 + t * A.B + b;
    const float* hpb = S.hprev + (size_t)b * S.hp_bs;
    float c = 0.0f;
    for (int j = 0; j < H; j++) c = fmaf(hpb[(size_t)j * S.hp_ld], S.Wh[(size_t)j * H + u], c);
    const float h = act_f((S.Gx[(size_t)u * S.ld + col] + c) + S.bias[u], A.act);
    S.Hout[(size_t)u * S.ld + col] = h;
    if (S.hprev_out) S.hprev_out[(size_t)u * S.keep_ld + S.keep_c0 + (size_t)t * A.B + b] = hpb[(size_t)u * S.hp_ld];
}
void launch_rnn_step_t(hipStream_t st, const CellFwdArgs& a, int t) {
    const int n = a.H * a.B * a.nseq;
    hipLaunchKernelGGL(k_rnn_step, dim3((n + 255) / 256), dim3(256), 0, st, a, t);
}

// ------------------------------------------------------------------ one BPTT step (single workgroup: dh_{t-1} needs all H gate gradients of step t)
__global__ __launch_bounds__(1024) void k_rnn_bwd_step(CellBwdArgs A) {
    const int H = A.H, B = A.B, TB = A.TB, t = A.t, per = H * B;
    for (int e = threadIdx.x; e < per; e += blockDim.x) {
        const int u = e / B, b = e % B; const size_t k = (size_t)t * B + b;
        const float dhn = t == A.T - 1 ? 0.0f : A.dhn[e];
        const float dh = A.dH[(size_t)u * TB + k] + dhn;
        A.dG[(size_t)u * TB + k] = dact_f(dh, A.hout[(size_t)u * A.ld_h + k], A.act);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < per; e += blockDim.x) {     // dh_{t-1}[j][b] = sum_n dG[n][t,b] Wh[j][n], n ascending
        const int j = e / B, b = e % B; const size_t k = (size_t)t * B + b;
        float acc = 0.0f;
        for (int n = 0; n < H; n++) acc = fmaf(A.dG[(size_t)n * TB + k], A.Wh[(size_t)j * H + n], acc);
        A.dhn[e] = acc;
    }
    if (t == 0) {                                              // trainable state0: gradient summed over the batch, ascending b
        __syncthreads();
        for (int u = threadIdx.x; u < H; u += blockDim.x) state0_fold<false>(u, B, A.dhn, nullptr, A.g_h0, nullptr);
    }
}
void launch_rnn_bwd_step(hipStream_t st, const CellBwdArgs& a) {
    int bs = ((a.H * a.B + 63) / 64) * 64; if (bs > 1024) bs = 1024;
    hipLaunchKernelGGL(k_rnn_bwd_step, dim3(1), dim3(bs), 0, st, a);
}

// ------------------------------------------------------------------ whole-sequence kernels (the shape of gru.hip's k_gru_seq / k_gru_bwd_seq)
// When Wh (H x H) and one step's state fit in LDS, ONE launch runs the whole recurrence: workgroup = (sequence set, group of CB batch columns), Wh, the
// bias and h in LDS, t = 0..T-1 walked inside, thread = (unit, column), one barrier per step (h double-buffered).  Per-element arithmetic is
// k_rnn_step's / k_rnn_bwd_step's (same chains, same association), so every bit is too.  Fit rule: each kernel within 80 KB of dynamic LDS, so
// that two of its workgroups can share a gfx950 CU's 160 KB (the grids are nseq * B / CB and B / CB small workgroups, at most a few per CU on
// 256 CUs); that admits H <= 141 (H > 128: one column per workgroup, H*H + 3H floats), above ~H = 124 through a raised LDS limit.  T <= 64
// as for the LSTM and the GRU.
static size_t rnn_fwd_lds(int H, int cb) { return (size_t)H * H + (size_t)H + 2 * (size_t)H * cb; }       // Wh, bias, h [2][H*cb]
static size_t rnn_bwd_lds(int H, int cb) { return (size_t)H * (H + 1) + 2 * (size_t)H * cb; }            // Wh (padded rows), dG [H][cb], dh [H*cb]
static const size_t RNN_SEQ_LDS = 80 * 1024;
bool rnn_seq_fits(int H, int B, int T) {
    const int cb = cell_cb(H, B);
    return rnn_fwd_lds(H, cb) * sizeof(float) <= RNN_SEQ_LDS && rnn_bwd_lds(H, cb) * sizeof(float) <= RNN_SEQ_LDS && H * cb <= 1024 && T <= 64;
}
static void rnn_raise_lds(const void* f, size_t lds) {      // beyond the default 64 KB of dynamic LDS (gfx950: up to 160 KB per workgroup)
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// PF (T <= 8): the input projections Gx of ALL time steps are requested before the recurrence starts; otherwise one step ahead.
template <bool PF>
__global__ __launch_bounds__(1024) void k_rnn_seq(CellFwdArgs A, int CB) {
    extern __shared__ float lds[];
    const int H = A.H, B = A.B, per = H * CB, T = A.T, nsplit = B / CB;
    float* Wh_s = lds;                 // [H][H]
    float* bias_s = Wh_s + H * H;      // [H]
    float* h_s = bias_s + H;           // [2][H*CB]
    const CellSeq& S = A.s[blockIdx.x / nsplit];
    const int b0 = (blockIdx.x % nsplit) * CB;
    for (int i = threadIdx.x; i < H * H; i += blockDim.x) Wh_s[i] = S.Wh[i];
    for (int i = threadIdx.x; i < H; i += blockDim.x) bias_s[i] = S.bias[i];
    for (int e = threadIdx.x; e < per; e += blockDim.x) h_s[e] = S.hprev[e / CB];      // Flux.reset!: state0 broadcast over the batch
    const int e = threadIdx.x; const bool on = e < per;
    const int u = on ? e / CB : 0, bl = on ? e - u * CB : 0, b = b0 + bl;
    const float* gx = S.Gx + (size_t)u * S.ld + S.c0 + b;      // + t * B
    float all[PF ? 8 : 1];
    if constexpr (PF) {
#pragma unroll
        for (int t = 0; t < 8; t++) all[t] = t < T ? gx[(size_t)t * B] : 0.0f;
    }
    float nx = 0.0f; if constexpr (!PF) nx = gx[0];
    __syncthreads();
    int cur = 0;
    auto step = [&](int t, float g) {
        const float* hp = h_s + cur * per; float* hn = h_s + (cur ^ 1) * per;
        if (on) {
            float ch = 0.0f;
#pragma unroll 8
            for (int j = 0; j < H; j++) ch = fmaf(hp[j * CB + bl], Wh_s[j * H + u], ch);
            const float h = act_f((g + ch) + bias_s[u], A.act);
            S.Hout[(size_t)u * S.ld + S.c0 + t * B + b] = h;
            if (S.hprev_out) S.hprev_out[(size_t)u * S.keep_ld + S.keep_c0 + (size_t)t * B + b] = hp[e];
            hn[e] = h;
        }
        __syncthreads();
        cur ^= 1;
    };
    if constexpr (PF) {
#pragma unroll
        for (int t = 0; t < 8; t++) if (t < T) step(t, all[t]);
    } else {
        for (int t = 0; t < T; t++) { const float g = nx; if (t + 1 < T) nx = gx[(size_t)(t + 1) * B]; step(t, g); }
    }
}
void launch_rnn_seq(hipStream_t st, const CellFwdArgs& a) {
    const int cb = cell_cb(a.H, a.B);
    const size_t lds = rnn_fwd_lds(a.H, cb) * sizeof(float);
    const int bs = ((a.H * cb + 63) / 64) * 64;      // rnn_seq_fits: H * cb <= 1024
    const dim3 grid(a.nseq * (a.B / cb));
    if (a.T <= 8) { rnn_raise_lds((const void*)k_rnn_seq<true>, lds); hipLaunchKernelGGL((k_rnn_seq<true>), grid, dim3(bs), lds, st, a, cb); }
    else { rnn_raise_lds((const void*)k_rnn_seq<false>, lds); hipLaunchKernelGGL((k_rnn_seq<false>), grid, dim3(bs), lds, st, a, cb); }
}

// BPTT over the whole s-sequence, one workgroup per group of CB columns (the arithmetic of T calls of k_rnn_bwd_step); the state0 gradient
// (a sum over ALL columns, ascending b) is folded by k_state0_grad (cell.h) afterwards.  PF (T <= 8): dH and h of every step are requested before
// the loop; otherwise one step ahead.
template <bool PF>
__global__ __launch_bounds__(1024) void k_rnn_bwd_seq(CellBwdArgs A, int CB) {
    extern __shared__ float lds[];
    const int H = A.H, B = A.B, TB = A.TB, per = H * CB, b0 = blockIdx.x * CB;
    const int NP = H + 1;              // padded row stride (the lanes of a wave read different rows u at the same n)
    float* Wh_s = lds;                 // [H][H + 1]
    float* dG_s = Wh_s + H * NP;       // [H][CB] dG of the current step
    float* dhn_s = dG_s + per;         // [H*CB]
    for (int i = threadIdx.x; i < H * H; i += blockDim.x) Wh_s[(i / H) * NP + i % H] = A.Wh[i];
    for (int e = threadIdx.x; e < per; e += blockDim.x) dhn_s[e] = 0.0f;
    __syncthreads();
    const int e = threadIdx.x; const bool on = e < per;
    const int u = on ? e / CB : 0, bl = on ? e - u * CB : 0;
    struct St { float dH, h; };
    auto fetch = [&](int t) { St s; const size_t k = (size_t)t * B + b0 + bl; s.dH = A.dH[(size_t)u * TB + k]; s.h = A.hout[(size_t)u * A.ld_h + k]; return s; };
    St all[PF ? 8 : 1];
    if constexpr (PF) {
#pragma unroll
        for (int t = 0; t < 8; t++) if (t < A.T) all[t] = fetch(t);
    }
    St nx; if constexpr (!PF) nx = fetch(A.T - 1);
#pragma unroll
    for (int tt = 0; tt < (PF ? 8 : 1 << 30); tt++) {
        const int t = (PF ? 7 : A.T - 1) - tt;
        if (t < 0) break;
        if (PF && t >= A.T) continue;
        St c; if constexpr (PF) c = all[PF ? t : 0]; else c = nx;
        if (on) {
            const size_t k = (size_t)t * B + b0 + bl;
            const float dhn = t == A.T - 1 ? 0.0f : dhn_s[e];
            const float dh = c.dH + dhn;
            const float g = dact_f(dh, c.h, A.act);
            A.dG[(size_t)u * TB + k] = g;
            dG_s[e] = g;                                           // e == u * CB + bl
        }
        if constexpr (!PF) { if (t > 0) nx = fetch(t - 1); }
        __syncthreads();
        if (on) {                                                  // dh_{t-1}[j][b] = sum_n dG[n][t,b] Wh[j][n], n ascending   (j == u)
            float acc = 0.0f;
#pragma unroll 8
            for (int n = 0; n < H; n++) acc = fmaf(dG_s[n * CB + bl], Wh_s[u * NP + n], acc);
            dhn_s[e] = acc;
        }
        __syncthreads();
    }
    for (int e2 = threadIdx.x; e2 < per; e2 += blockDim.x) { const int u2 = e2 / CB, bl2 = e2 - u2 * CB; A.dhn[u2 * B + b0 + bl2] = dhn_s[e2]; }
}
void launch_rnn_bwd_seq(hipStream_t st, const CellBwdArgs& a) {
    const int cb = cell_cb(a.H, a.B);
    const size_t lds = rnn_bwd_lds(a.H, cb) * sizeof(float);
    const int bs = ((a.H * cb + 63) / 64) * 64;      // rnn_seq_fits: H * cb <= 1024
    if (a.T <= 8) { rnn_raise_lds((const void*)k_rnn_bwd_seq<true>, lds); hipLaunchKernelGGL((k_rnn_bwd_seq<true>), dim3(a.B / cb), dim3(bs), lds, st, a, cb); }
    else { rnn_raise_lds((const void*)k_rnn_bwd_seq<false>, lds); hipLaunchKernelGGL((k_rnn_bwd_seq<false>), dim3(a.B / cb), dim3(bs), lds, st, a, cb); }
    launch_state0_grad(st, a);
}
