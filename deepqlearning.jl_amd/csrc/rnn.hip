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

// ------------------------------------------------------------------ the RNN cell (cell.h: what a cell struct provides, and the kernels built from it)
// One gate and no early one: finish() is the whole step.  Nothing is stashed but h_{t-1}: BPTT reads the head gradient and h_t, the forward's output.
// Fit rule of the whole-sequence kernels: each within 80 KB of dynamic LDS, so that two of its workgroups can share a gfx950 CU's 160 KB (the grids
// are nseq * B / CB and B / CB small workgroups, at most a few per CU on 256 CUs); that admits H <= 141 (H > 128: one column per workgroup,
// H*H + 3H floats), above ~H = 124 through a raised LDS limit.
struct RnnCell {
    static constexpr int NG = 1, NE = 0, FIN = 0;
    static constexpr bool HAS_C = false, TWO_DG = false, ADD_DH = false;
    static constexpr size_t SEQ_LDS = 80 * 1024;
    static __device__ __forceinline__ CellFwd finish(const float*, float gh, float gx, float b, float, float, int act) { return {act_f((gx + gh) + b, act), 0.0f, 0.0f, 0.0f}; }
    struct St { float dH, h; };
    static __device__ __forceinline__ St fetch(const CellBwdArgs& A, int u, size_t k) { St s; s.dH = A.dH[(size_t)u * A.TB + k]; s.h = A.hout[(size_t)u * A.ld_h + k]; return s; }
    static __device__ __forceinline__ float bwd(const St& s, float dhn, float, int act, float* dG, float*) {
        const float dh = s.dH + dhn;
        dG[0] = dact_f(dh, s.h, act);
        return 0.0f;
    }
};

// ------------------------------------------------------------------ the whole-sequence forward: thread = (unit, column), one barrier per step (h double-buffered)
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
            const float h = RnnCell::finish(nullptr, ch, g, bias_s[u], 0.0f, 0.0f, A.act).h;
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
static void launch_rnn_seq(hipStream_t st, const CellFwdArgs& a) {
    const int cb = cell_cb(a.H, a.B);
    const size_t lds = cell_fwd_lds<RnnCell>(a.H, cb) * sizeof(float);
    const int bs = ((a.H * cb + 63) / 64) * 64;      // cell_seq_fits: H * cb <= 1024
    const dim3 grid(a.nseq * (a.B / cb));
    if (a.T <= 8) { cell_raise_lds((const void*)k_rnn_seq<true>, lds); hipLaunchKernelGGL((k_rnn_seq<true>), grid, dim3(bs), lds, st, a, cb); }
    else { cell_raise_lds((const void*)k_rnn_seq<false>, lds); hipLaunchKernelGGL((k_rnn_seq<false>), grid, dim3(bs), lds, st, a, cb); }
}
const CellOps* rnn_cell_ops() { static const CellOps ops = cell_ops_entry<RnnCell>("rnn", "RNN", true, false, launch_rnn_seq); return &ops; }
