// cell.h -- the kernels of the recurrent cells, written once for every cell.  A cell file (drqn.hip: LSTM, gru.hip, rnn.hip) states its cell as a struct
// -- the arithmetic of one element, each formula once, under the header comment that fixes the cell's canonical order -- and instantiates the kernel
// forms below with it: one time step (k_cell_step), one BPTT step (k_cell_bwd_step), the whole-sequence BPTT (k_cell_bwd_seq) and, for the gated
// cells, the gate-parallel whole-sequence forward (k_cell_seq; the RNN's forward has a thread mapping of its own and stays in rnn.hip).  Every form
// of a cell calls the same element functions, so the forms agree bit for bit by construction (-ffp-contract=off: inlining changes no association).
// A cell struct provides:
//   NG         gates, N = NG * H;   NE  the first NE gates are "early": their activation needs only their own pre-activation (gx + gh) + b
//   FIN        the gate whose thread finishes an element in k_cell_seq; its raw chain gh, gx and b are what finish() gets (the GRU's n; RNN: gate 0)
//   HAS_C      a cell state c beside h;   TWO_DG  BPTT writes dGh apart from dG;   ADD_DH  dh_{t-1} = chain + carry (the GRU's dh .* z)
//   SEQ_LDS    bytes of dynamic LDS either whole-sequence kernel may take (the fit rule)
//   gate_act(q, pre)                                   the activated early gate q (cells with NE > 0)
//   finish(a, gh, gx, b, hp, cp, act) -> CellFwd       a: the activated early gates; hp, cp: h_{t-1}, c_{t-1}; act: CellFwdArgs::act
//   St, fetch(A, u, k)                                 what BPTT reads back for unit u at stash column k
//   bwd(s, dhn, dcn, act, dG, dGh) -> carry            dhn: dh_{t-1} of step t+1, dcn: the LSTM's dc likewise (+0 at t = T-1); dG[NG], and dGh[NG] where
//                                                      TWO_DG (else the chain reads dG); carry: LSTM dc .* f, GRU dh .* z
#pragma once
#include "common.h"

// sigm / tanh through Float64, rounded once (Flux's Float32 activations)
__device__ __forceinline__ float sigm_f(float x) { return (float)(1.0 / (1.0 + exp(-(double)x))); }
__device__ __forceinline__ float tanh_f(float x) { return (float)tanh((double)x); }
struct CellFwd { float h, c, g, aux; };      // h'; c' (HAS_C); the gate finished last (NE < NG: stashed as gate FIN); aux (CellSeq)

// whole-sequence kernels: batch columns are independent in the recurrence, so a sequence set is split into groups of CB columns (one workgroup each,
// its own LDS copy of Wh); H*CB ~ 256 outputs per step.  CB divides B.
static inline int cell_cb(int H, int B) { int cb = 256 / H; if (cb < 1) cb = 1; if (cb > B) cb = B; while (B % cb) cb--; return cb; }
// their LDS floats: forward Wh, bias, h [2][H*cb], c [H*cb], the activated early gates [NE][H*cb]; backward Wh (padded rows), dGh [N][cb], dh [H*cb], dc [H*cb]
template <class Cell> static inline size_t cell_fwd_lds(int H, int cb) { return (size_t)H * Cell::NG * H + (size_t)Cell::NG * H + (2 + Cell::HAS_C + Cell::NE) * (size_t)H * cb; }
template <class Cell> static inline size_t cell_bwd_lds(int H, int cb) { return (size_t)H * (Cell::NG * H + 1) + (Cell::NG + 1 + Cell::HAS_C) * (size_t)H * cb; }
// the fit rule: both kernels within SEQ_LDS; gated cells: whole waves per gate and NG * H * cb threads; T <= 64 (k_cell_seq<64>)
template <class Cell> static bool cell_seq_fits(int H, int B, int T) {
    const int cb = cell_cb(H, B), per = H * cb;
    return cell_fwd_lds<Cell>(H, cb) * sizeof(float) <= Cell::SEQ_LDS && cell_bwd_lds<Cell>(H, cb) * sizeof(float) <= Cell::SEQ_LDS &&
           (Cell::NG > 1 ? per % 64 == 0 && per <= 256 : per <= 1024) && T <= 64;
}
static inline void cell_raise_lds(const void* f, size_t lds) {      // beyond the default 64 KB of dynamic LDS (gfx950: up to 160 KB per workgroup)
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

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

// ------------------------------------------------------------------ one time step for up to 3 sequence sets (online s, online sp, target sp)
// h_{t-1}(j, b) = hprev[j*hp_ld + b*hp_bs]: the acting programs step states that are not [H][B].  Gated cells stash when S.gates is set, the RNN
// (h_{t-1} alone) when S.hprev_out is.
template <class Cell>
__global__ void k_cell_step(CellFwdArgs A, int t) {
    constexpr int NG = Cell::NG, NE = Cell::NE, FIN = Cell::FIN;
    const int per = A.H * A.B;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per * A.nseq) return;
    const CellSeq& S = A.s[i / per];
    const int e = i % per, u = e / A.B, b = e % A.B, H = A.H, N = NG * H;
    const int col = S.c0 + t * A.B + b;
    const float* hpb = S.hprev + (size_t)b * S.hp_bs;
    float ch[NG], a[NE ? NE : 1];
#pragma unroll
    for (int q = 0; q < NG; q++) {
        const int n = q * H + u; float c = 0.0f;
        for (int j = 0; j < H; j++) c = fmaf(hpb[(size_t)j * S.hp_ld], S.Wh[(size_t)j * N + n], c);
        ch[q] = c;
    }
    if constexpr (NE > 0) {      // after ALL the chains: the early gates' Float64 activations are independent and interleave
#pragma unroll
        for (int q = 0; q < NE; q++) a[q] = Cell::gate_act(q, (S.Gx[(size_t)(q * H + u) * S.ld + col] + ch[q]) + S.bias[q * H + u]);
    }
    const float hp = hpb[(size_t)u * S.hp_ld], cp = Cell::HAS_C ? S.cprev[(size_t)u * S.cp_ld + (size_t)b * S.cp_bs] : 0.0f;
    const CellFwd o = Cell::finish(a, ch[FIN], S.Gx[(size_t)(FIN * H + u) * S.ld + col], S.bias[FIN * H + u], hp, cp, A.act);
    S.Hout[(size_t)u * S.ld + col] = o.h; if (Cell::HAS_C) S.Cst[(size_t)u * S.ld + col] = o.c;
    if (NG > 1 ? S.gates != nullptr : S.hprev_out != nullptr) {
        const size_t k = (size_t)S.keep_c0 + t * A.B + b; const size_t kl = S.keep_ld;
        if (NG > 1) {      // the RNN has no gate to stash: S.gates and S.aux are null
#pragma unroll
            for (int q = 0; q < NE; q++) S.gates[(size_t)(q * H + u) * kl + k] = a[q];
            if (NE < NG) S.gates[(size_t)(FIN * H + u) * kl + k] = o.g;
            S.aux[(size_t)u * kl + k] = o.aux;
        }
        S.hprev_out[(size_t)u * kl + k] = hp; if (Cell::HAS_C) S.cprev_out[(size_t)u * kl + k] = cp;
    }
}
template <class Cell> static void launch_cell_step(hipStream_t st, const CellFwdArgs& a, int t) {
    const int n = a.H * a.B * a.nseq;
    hipLaunchKernelGGL(k_cell_step<Cell>, dim3((n + 255) / 256), dim3(256), 0, st, a, t);
}

// ------------------------------------------------------------------ one BPTT step (single workgroup: dh_{t-1} needs all N gate gradients of step t)
// A.dh2 holds the carry: the LSTM's dc_{t-1} from launch to launch (folded into g_c0 at t = 0), the GRU's dh .* z across the barrier
template <class Cell>
__global__ __launch_bounds__(1024) void k_cell_bwd_step(CellBwdArgs A) {
    constexpr int NG = Cell::NG;
    const int H = A.H, B = A.B, TB = A.TB, N = NG * H, t = A.t, per = H * B;
    float* const dGh = Cell::TWO_DG ? A.dGh : A.dG;
    for (int e = threadIdx.x; e < per; e += blockDim.x) {
        const int u = e / B, b = e % B; const size_t k = (size_t)t * B + b;
        const typename Cell::St s = Cell::fetch(A, u, k);
        const float dhn = t == A.T - 1 ? 0.0f : A.dhn[e], dcn = Cell::HAS_C ? (t == A.T - 1 ? 0.0f : A.dh2[e]) : 0.0f;
        float g[NG], gh[NG];
        const float carry = Cell::bwd(s, dhn, dcn, A.act, g, gh);
        if (Cell::HAS_C || Cell::ADD_DH) A.dh2[e] = carry;
#pragma unroll
        for (int q = 0; q < NG; q++) A.dG[(size_t)(q * H + u) * TB + k] = g[q];
        if (Cell::TWO_DG) {
#pragma unroll
            for (int q = 0; q < NG; q++) dGh[(size_t)(q * H + u) * TB + k] = gh[q];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < per; e += blockDim.x) {     // dh_{t-1}[j][b] = sum_n dGh[n][t,b] Wh[j][n], n ascending (+ the GRU's dh[j][b] z[j][b])
        const int j = e / B, b = e % B; const size_t k = (size_t)t * B + b;
        float acc = 0.0f;
        for (int n = 0; n < N; n++) acc = fmaf(dGh[(size_t)n * TB + k], A.Wh[(size_t)j * N + n], acc);
        if constexpr (Cell::ADD_DH) A.dhn[e] = acc + A.dh2[e]; else A.dhn[e] = acc;      // never acc + 0: -0 + 0 is +0
    }
    if (t == 0) {                                              // trainable state0: gradient summed over the batch, ascending b
        __syncthreads();
        for (int u = threadIdx.x; u < H; u += blockDim.x) state0_fold<Cell::HAS_C>(u, B, A.dhn, A.dh2, A.g_h0, A.g_c0);
    }
}
template <class Cell> static void launch_cell_bwd_step(hipStream_t st, const CellBwdArgs& a) {
    int bs = ((a.H * a.B + 63) / 64) * 64; if (bs > 1024) bs = 1024;
    hipLaunchKernelGGL(k_cell_bwd_step<Cell>, dim3(1), dim3(bs), 0, st, a);
}

// ------------------------------------------------------------------ whole-sequence kernels
// The per-step launches above cost a dispatch and a cold walk over Wh per time step.  When Wh (H x N) and one step's state fit in LDS (cell_seq_fits),
// ONE launch runs the whole recurrence: workgroup = (sequence set, group of CB batch columns: cell_cb), Wh, the bias and the state in LDS, t = 0..T-1
// walked inside.  Gate-parallel: thread = (gate q, unit, column), one H-deep chain and ONE Float64 sigm / tanh each; the early gates meet in LDS and the
// (unit, column) thread of gate FIN finishes the element.  The input projections Gx of ALL time steps are requested before the recurrence starts
// (they do not depend on it): one round trip instead of one per time step.  TT: compile-time bound on T.
template <class Cell, int TT>
__global__ __launch_bounds__(1024) void k_cell_seq(CellFwdArgs A, int CB) {
    extern __shared__ float lds[];
    constexpr int NG = Cell::NG, NE = Cell::NE, FIN = Cell::FIN;
    const int H = A.H, B = A.B, N = NG * H, per = H * CB, T = A.T, nsplit = B / CB;
    float* Wh_s = lds;                                  // [H][N]
    float* bias_s = Wh_s + H * N;                       // [N]
    float* h_s = bias_s + N;                            // [2][H*CB]
    float* c_s = h_s + 2 * per;                         // [H*CB], HAS_C
    float* g_s = c_s + (Cell::HAS_C ? per : 0);         // [NE][H*CB] activated early gates of the current step
    const CellSeq& S = A.s[blockIdx.x / nsplit];
    const int b0 = (blockIdx.x % nsplit) * CB;
    for (int i = threadIdx.x; i < H * N; i += blockDim.x) Wh_s[i] = S.Wh[i];
    for (int i = threadIdx.x; i < N; i += blockDim.x) bias_s[i] = S.bias[i];
    for (int e = threadIdx.x; e < per; e += blockDim.x) { const int u = e / CB; h_s[e] = S.hprev[u]; if (Cell::HAS_C) c_s[e] = S.cprev[u]; }      // Flux.reset!: state0 broadcast over the batch
    const int q = threadIdx.x / per, e = threadIdx.x - q * per;      // gate, (unit, column) element; blockDim = NG * per, per a multiple of 64: a wave has one gate
    const bool on = q < NG;
    const int u = e / CB, bl = e - u * CB, b = b0 + bl;
    float gxr[TT];
#pragma unroll
    for (int t = 0; t < TT; t++) gxr[t] = (on && t < T) ? S.Gx[(size_t)(q * H + u) * S.ld + S.c0 + t * B + b] : 0.0f;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int t = 0; t < TT; t++) {
        if (t >= T) break;
        const float* hp = h_s + cur * per; float* hn = h_s + (cur ^ 1) * per;
        float ch = 0.0f;
        if (on) {
            const float* wr = Wh_s + q * H + u;
#pragma unroll 8
            for (int j = 0; j < H; j++) ch = fmaf(hp[j * CB + bl], wr[j * N], ch);
            if (q < NE) {
                const float act = Cell::gate_act(q, (gxr[t] + ch) + bias_s[q * H + u]);
                g_s[q * per + e] = act;
                if (S.gates) S.gates[(size_t)(q * H + u) * S.keep_ld + (size_t)S.keep_c0 + t * B + b] = act;
            }
        }
        __syncthreads();
        if (q == FIN) {
            float a[NE];
#pragma unroll
            for (int i = 0; i < NE; i++) a[i] = g_s[i * per + e];
            const float hpv = hp[e], cp = Cell::HAS_C ? c_s[e] : 0.0f;
            const CellFwd o = Cell::finish(a, ch, gxr[t], bias_s[FIN * H + u], hpv, cp, A.act);
            const int col = S.c0 + t * B + b;
            S.Hout[(size_t)u * S.ld + col] = o.h; if (Cell::HAS_C) S.Cst[(size_t)u * S.ld + col] = o.c;
            if (S.gates) {
                const size_t k = (size_t)S.keep_c0 + t * B + b; const size_t kl = S.keep_ld;
                if (NE < NG) S.gates[(size_t)(FIN * H + u) * kl + k] = o.g;
                S.aux[(size_t)u * kl + k] = o.aux; S.hprev_out[(size_t)u * kl + k] = hpv; if (Cell::HAS_C) S.cprev_out[(size_t)u * kl + k] = cp;
            }
            hn[e] = o.h; if (Cell::HAS_C) c_s[e] = o.c;
        }
        __syncthreads();
        cur ^= 1;
    }
}
template <class Cell> static void launch_cell_seq(hipStream_t st, const CellFwdArgs& a) {
    const int cb = cell_cb(a.H, a.B);
    const size_t lds = cell_fwd_lds<Cell>(a.H, cb) * sizeof(float);
    const dim3 grid(a.nseq * (a.B / cb)), bs(Cell::NG * a.H * cb);      // NG gates x (unit, column) elements; cell_seq_fits: H * cb is a multiple of 64 and <= 256
    if (a.T <= 8) hipLaunchKernelGGL((k_cell_seq<Cell, 8>), grid, bs, lds, st, a, cb);
    else if (a.T <= 32) hipLaunchKernelGGL((k_cell_seq<Cell, 32>), grid, bs, lds, st, a, cb);
    else hipLaunchKernelGGL((k_cell_seq<Cell, 64>), grid, bs, lds, st, a, cb);      // cell_seq_fits: T <= 64
}

// BPTT over the whole s-sequence, one workgroup per group of CB columns (the arithmetic of T calls of k_cell_bwd_step); the trainable state0's
// gradient (a sum over ALL columns, ascending b) is folded by k_state0_grad afterwards.  One (unit, column) element per thread (per <= blockDim by
// construction).  PF (T <= 8): the stash records of EVERY time step are requested before the loop (LSTM: 56 registers) instead of one step ahead,
// while step t's dh chain runs -- their round trip was longer than a step's arithmetic (r03: 4.6 us per time step).  The LSTM's carry dc lives in LDS
// and goes back to A.dh2 for the fold; the GRU's dh .* z is a register.
template <class Cell, bool PF>
__global__ __launch_bounds__(1024) void k_cell_bwd_seq(CellBwdArgs A, int CB) {
    extern __shared__ float lds[];
    constexpr int NG = Cell::NG;
    using St = typename Cell::St;
    const int H = A.H, B = A.B, TB = A.TB, N = NG * H, per = H * CB, b0 = blockIdx.x * CB;
    const int NP = N + 1;              // padded row stride: lanes of one wave hold different rows j of Wh at the same n -- stride N put all of them on ONE bank (LSTM: 8-way conflict on every read of the 128-deep chain)
    float* Wh_s = lds;                 // [H][N + 1]
    float* dG_s = Wh_s + H * NP;       // [N][CB] dGh of the current step
    float* dhn_s = dG_s + N * CB;      // [H*CB]
    float* dcn_s = dhn_s + per;        // [H*CB], HAS_C
    for (int i = threadIdx.x; i < H * N; i += blockDim.x) Wh_s[(i / N) * NP + i % N] = A.Wh[i];
    for (int e = threadIdx.x; e < per; e += blockDim.x) { dhn_s[e] = 0.0f; if (Cell::HAS_C) dcn_s[e] = 0.0f; }
    __syncthreads();
    const int e = threadIdx.x; const bool on = e < per;
    const int u = on ? e / CB : 0, bl = on ? e - u * CB : 0;
    int gl[NG];                        // where gate q of this element goes in dG_s
#pragma unroll
    for (int q = 0; q < NG; q++) gl[q] = (q * H + u) * CB + bl;
    St all[PF ? 8 : 1];
    if constexpr (PF) {
#pragma unroll
        for (int t = 0; t < 8; t++) if (t < A.T) all[t] = Cell::fetch(A, u, (size_t)t * B + b0 + bl);
    }
    St nx; if constexpr (!PF) nx = Cell::fetch(A, u, (size_t)(A.T - 1) * B + b0 + bl);
    float carry = 0.0f;
#pragma unroll
    for (int tt = 0; tt < (PF ? 8 : 1 << 30); tt++) {
        const int t = (PF ? 7 : A.T - 1) - tt;
        if (t < 0) break;
        if (PF && t >= A.T) continue;
        St c; if constexpr (PF) c = all[PF ? t : 0]; else c = nx;
        if (on) {
            const size_t k = (size_t)t * B + b0 + bl;
            const float dhn = t == A.T - 1 ? 0.0f : dhn_s[e], dcn = Cell::HAS_C ? (t == A.T - 1 ? 0.0f : dcn_s[e]) : 0.0f;
            float g[NG], gh[NG];
            const float cr = Cell::bwd(c, dhn, dcn, A.act, g, gh);
            if constexpr (Cell::HAS_C) dcn_s[e] = cr; else carry = cr;
#pragma unroll
            for (int q = 0; q < NG; q++) A.dG[(size_t)(q * H + u) * TB + k] = g[q];
#pragma unroll
            for (int q = 0; q < NG; q++) { if (Cell::TWO_DG) A.dGh[(size_t)(q * H + u) * TB + k] = gh[q]; dG_s[gl[q]] = Cell::TWO_DG ? gh[q] : g[q]; }
        }
        if constexpr (!PF) { if (t > 0) nx = Cell::fetch(A, u, (size_t)(t - 1) * B + b0 + bl); }
        __syncthreads();
        if (on) {                                                  // dh_{t-1}[j][b] = sum_n dGh[n][t,b] Wh[j][n], n ascending (+ the GRU's dh z)   (j == u)
            float acc = 0.0f;
#pragma unroll 8
            for (int n = 0; n < N; n++) acc = fmaf(dG_s[n * CB + bl], Wh_s[u * NP + n], acc);
            if constexpr (Cell::ADD_DH) dhn_s[e] = acc + carry; else dhn_s[e] = acc;      // never acc + 0: -0 + 0 is +0
        }
        __syncthreads();
    }
    for (int e2 = threadIdx.x; e2 < per; e2 += blockDim.x) { const int u2 = e2 / CB, i2 = u2 * B + b0 + e2 - u2 * CB; A.dhn[i2] = dhn_s[e2]; if (Cell::HAS_C) A.dh2[i2] = dcn_s[e2]; }
}
template <class Cell> static void launch_cell_bwd_seq(hipStream_t st, const CellBwdArgs& a) {      // a.t ignored
    const int cb = cell_cb(a.H, a.B);
    const size_t lds = cell_bwd_lds<Cell>(a.H, cb) * sizeof(float);
    int bs = ((a.H * cb + 63) / 64) * 64; if (bs > 1024) bs = 1024;
    if (a.T <= 8) { cell_raise_lds((const void*)k_cell_bwd_seq<Cell, true>, lds); hipLaunchKernelGGL((k_cell_bwd_seq<Cell, true>), dim3(a.B / cb), dim3(bs), lds, st, a, cb); }
    else { cell_raise_lds((const void*)k_cell_bwd_seq<Cell, false>, lds); hipLaunchKernelGGL((k_cell_bwd_seq<Cell, false>), dim3(a.B / cb), dim3(bs), lds, st, a, cb); }
    launch_state0_grad(st, a);
}

// the cell's entry of the table (common.h cell_ops): the struct's facts, the launchers above, and the whole-sequence forward the cell file names
template <class Cell> static inline CellOps cell_ops_entry(const char* name, const char* display, bool has_act, bool clear_junk, void (*launch_seq)(hipStream_t, const CellFwdArgs&)) {
    return {name, display, Cell::NG, has_act, Cell::HAS_C, Cell::TWO_DG, clear_junk, cell_seq_fits<Cell>, launch_cell_step<Cell>, launch_seq, launch_cell_bwd_step<Cell>, launch_cell_bwd_seq<Cell>};
}
