// gru.hip -- the GRU cell of the recurrent path (Flux 0.14 GRU = Recur(GRUCell); third-party, recalled like the LSTM's):
//   gates in the order r, z, n; gx = Wi*x (3H rows, bias-free, by the ordinary dense kernels over all T*B columns), gh = Wh*h_{t-1}
//   r = sigm(gx_r + gh_r + b_r),  z = sigm(gx_z + gh_z + b_z),  n = tanh(gx_n + r .* gh_n + b_n),  h' = (1 - z) .* n + z .* h_{t-1}
//   (r multiplies Wh_n*h, not h: GRU, not GRUv3).  Trainable state0 h0, broadcast over the batch (Flux.reset!).
// Canonical order, used by EVERY form below (step, sequence, policy step) so that they agree bit for bit:
//   gh_q   = chain_j (+0; j ascending) fma(h_{t-1}[j], Wh[j][q*H + u], .)                      q = r, z, n
//   r_pre  = (gx_r + gh_r) + b_r ;  z_pre = (gx_z + gh_z) + b_z ;  n_pre = (gx_n + (r * gh_n)) + b_n
//   h'     = ((1 - z) * n) + (z * h_{t-1})
//   sigm / tanh through Float64, rounded once (cell.h)
// BPTT per step, dh = (head gradient) + (dh_{t-1} of step t+1):
//   dn = (dh * (1 - z)) * (1 - n*n) ;  dz = ((dh * (h_{t-1} - n)) * z) * (1 - z) ;  dr = ((dn * gh_n) * r) * (1 - r)
//   dGx = [dr; dz; dn]        -> Wi | b dW and the input dX (dense contractions over T*B columns)
//   dGh = [dr; dz; dn * r]    -> Wh dW (X = h_{t-1})
//   dh_{t-1}[j] = (chain_n (+0; n ascending over 3H) fma(dGh[n], Wh[j][n], .)) + (dh[j] * z[j]) ;  dstate0[u] = sum_b (ascending) dh_{-1}[u][b]
#include "cell.h"

// ------------------------------------------------------------------ one time step for up to 3 sequence sets (online s, online sp, target sp)
__global__ void k_gru_step(CellFwdArgs A, int t) {
    const int per = A.H * A.B;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per * A.nseq) return;
    const CellSeq& S = A.s[i / per];
    const int e = i % per, u = e / A.B, b = e % A.B, H = A.H, N = 3 * H;
    const int col = S.c0 + t * A.B + b;
    const float* hpb = S.hprev + (size_t)b * S.hp_bs;
    float ch[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int n = q * H + u; float c = 0.0f;
        for (int j = 0; j < H; j++) c = fmaf(hpb[(size_t)j * S.hp_ld], S.Wh[(size_t)j * N + n], c);
        ch[q] = c;
    }
    const float r = sigm_f((S.Gx[(size_t)u * S.ld + col] + ch[0]) + S.bias[u]);
    const float z = sigm_f((S.Gx[(size_t)(H + u) * S.ld + col] + ch[1]) + S.bias[H + u]);
    const float hp = hpb[(size_t)u * S.hp_ld];
    const float rg = r * ch[2]; const float np_ = (S.Gx[(size_t)(2 * H + u) * S.ld + col] + rg) + S.bias[2 * H + u]; const float n = tanh_f(np_);
    const float omz = 1.0f - z; const float t1 = omz * n; const float t2 = z * hp; const float h = t1 + t2;
    S.Hout[(size_t)u * S.ld + col] = h;
    if (S.gates) {
        const size_t k = (size_t)S.keep_c0 + t * A.B + b; const size_t kl = S.keep_ld;
        S.gates[(size_t)u * kl + k] = r; S.gates[(size_t)(H + u) * kl + k] = z; S.gates[(size_t)(2 * H + u) * kl + k] = n;
        S.aux[(size_t)u * kl + k] = ch[2]; S.hprev_out[(size_t)u * kl + k] = hp;
    }
}
void launch_gru_step_t(hipStream_t st, const CellFwdArgs& a, int t) {
    const int n = a.H * a.B * a.nseq;
    hipLaunchKernelGGL(k_gru_step, dim3((n + 255) / 256), dim3(256), 0, st, a, t);
}

// ------------------------------------------------------------------ one BPTT step (single workgroup: dh_{t-1} needs all 3H gate gradients of step t)
__global__ __launch_bounds__(1024) void k_gru_bwd_step(CellBwdArgs A) {
    const int H = A.H, B = A.B, TB = A.TB, N = 3 * H, t = A.t, per = H * B;
    for (int e = threadIdx.x; e < per; e += blockDim.x) {
        const int u = e / B, b = e % B; const size_t k = (size_t)t * B + b;
        const float r = A.gates[(size_t)u * TB + k], z = A.gates[(size_t)(H + u) * TB + k], n = A.gates[(size_t)(2 * H + u) * TB + k];
        const float ghn = A.aux[(size_t)u * TB + k], hp = A.hprev[(size_t)u * TB + k];
        const float dhn = t == A.T - 1 ? 0.0f : A.dhn[e];
        const float dh = A.dH[(size_t)u * TB + k] + dhn;
        const float omz = 1.0f - z; const float n2 = n * n; const float omn2 = 1.0f - n2; const float a1 = dh * omz; const float dn = a1 * omn2;
        const float hmn = hp - n; const float b1 = dh * hmn; const float b2 = b1 * z; const float dz = b2 * omz;
        const float c1 = dn * ghn; const float c2 = c1 * r; const float omr = 1.0f - r; const float dr = c2 * omr;
        const float dnr = dn * r;
        A.dh2[e] = dh * z;
        A.dG[(size_t)u * TB + k] = dr; A.dG[(size_t)(H + u) * TB + k] = dz; A.dG[(size_t)(2 * H + u) * TB + k] = dn;
        A.dGh[(size_t)u * TB + k] = dr; A.dGh[(size_t)(H + u) * TB + k] = dz; A.dGh[(size_t)(2 * H + u) * TB + k] = dnr;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < per; e += blockDim.x) {     // dh_{t-1}[j][b] = (sum_n dGh[n][t,b] Wh[j][n], n ascending) + dh[j][b] z[j][b]
        const int j = e / B, b = e % B; const size_t k = (size_t)t * B + b;
        float acc = 0.0f;
        for (int n = 0; n < N; n++) acc = fmaf(A.dGh[(size_t)n * TB + k], A.Wh[(size_t)j * N + n], acc);
        A.dhn[e] = acc + A.dh2[e];
    }
    if (t == 0) {                                              // trainable state0: gradient summed over the batch, ascending b
        __syncthreads();
        for (int u = threadIdx.x; u < H; u += blockDim.x) state0_fold<false>(u, B, A.dhn, nullptr, A.g_h0, nullptr);
    }
}
void launch_gru_bwd_step(hipStream_t st, const CellBwdArgs& a) {
    int bs = ((a.H * a.B + 63) / 64) * 64; if (bs > 1024) bs = 1024;
    hipLaunchKernelGGL(k_gru_bwd_step, dim3(1), dim3(bs), 0, st, a);
}

// ------------------------------------------------------------------ whole-sequence kernels for small GRUs (the shape of drqn.hip's k_lstm_seq / k_lstm_bwd_seq)
// When Wh (H x 3H) and one step's state fit in LDS, ONE launch runs the whole recurrence: workgroup = (sequence set, group of CB batch columns), Wh, the
// bias and h in LDS, t = 0..T-1 walked inside.  Gate-parallel: thread = (gate q, unit, column); the r and z threads finish their sigmoid, the n thread
// keeps gh_n in a register and, once r and z are in LDS, finishes n and h'.  The input projections Gx of ALL time steps are requested before the
// recurrence starts.  Per-element arithmetic is k_gru_step's (same chains, same association), so every bit is too.  TT: compile-time bound on T.
static size_t gru_fwd_lds(int H, int cb) { return (size_t)H * 3 * H + 3 * (size_t)H + 4 * (size_t)H * cb; }      // Wh, bias, h [2][H*cb], r / z [2][H*cb]
static size_t gru_bwd_lds(int H, int cb) { return (size_t)H * (3 * H + 1) + 3 * (size_t)H * cb + (size_t)H * cb; }   // Wh (padded rows), dGh [3H][cb], dh [H*cb]
bool gru_seq_fits(int H, int B, int T) {     // both kernels within 64 KB of dynamic LDS; whole waves per gate
    const int cb = cell_cb(H, B);
    return gru_fwd_lds(H, cb) <= 16384 && gru_bwd_lds(H, cb) <= 16384 && (H * cb) % 64 == 0 && H * cb <= 256 && T <= 64;
}
template <int TT>
__global__ __launch_bounds__(1024) void k_gru_seq(CellFwdArgs A, int CB) {
    extern __shared__ float lds[];
    const int H = A.H, B = A.B, N = 3 * H, per = H * CB, T = A.T, nsplit = B / CB;
    float* Wh_s = lds;                 // [H][3H]
    float* bias_s = Wh_s + H * N;      // [3H]
    float* h_s = bias_s + N;           // [2][H*CB]
    float* g_s = h_s + 2 * per;        // [2][H*CB] r, z of the current step
    const CellSeq& S = A.s[blockIdx.x / nsplit];
    const int b0 = (blockIdx.x % nsplit) * CB;
    for (int i = threadIdx.x; i < H * N; i += blockDim.x) Wh_s[i] = S.Wh[i];
    for (int i = threadIdx.x; i < N; i += blockDim.x) bias_s[i] = S.bias[i];
    for (int e = threadIdx.x; e < per; e += blockDim.x) h_s[e] = S.hprev[e / CB];      // Flux.reset!: state0 broadcast over the batch
    const int q = threadIdx.x / per, e = threadIdx.x - q * per;      // blockDim = 3 * per, per a multiple of 64: a wave has one gate
    const int u = e / CB, bl = e - u * CB, b = b0 + bl;
    float gxr[TT];
#pragma unroll
    for (int t = 0; t < TT; t++) gxr[t] = t < T ? S.Gx[(size_t)(q * H + u) * S.ld + S.c0 + t * B + b] : 0.0f;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int t = 0; t < TT; t++) {
        if (t >= T) break;
        const float* hp = h_s + cur * per; float* hn = h_s + (cur ^ 1) * per;
        float ch = 0.0f;
        const float* wr = Wh_s + q * H + u;
#pragma unroll 8
        for (int j = 0; j < H; j++) ch = fmaf(hp[j * CB + bl], wr[j * N], ch);
        if (q < 2) {
            const float act = sigm_f((gxr[t] + ch) + bias_s[q * H + u]);
            g_s[q * per + e] = act;
            if (S.gates) S.gates[(size_t)(q * H + u) * S.keep_ld + (size_t)S.keep_c0 + t * B + b] = act;
        }
        __syncthreads();
        if (q == 2) {
            const float r = g_s[e], z = g_s[per + e], hpv = hp[e];
            const float rg = r * ch; const float np_ = (gxr[t] + rg) + bias_s[2 * H + u]; const float n = tanh_f(np_);
            const float omz = 1.0f - z; const float t1 = omz * n; const float t2 = z * hpv; const float h = t1 + t2;
            S.Hout[(size_t)u * S.ld + S.c0 + t * B + b] = h;
            if (S.gates) { const size_t k = (size_t)S.keep_c0 + t * B + b; const size_t kl = S.keep_ld; S.gates[(size_t)(2 * H + u) * kl + k] = n; S.aux[(size_t)u * kl + k] = ch; S.hprev_out[(size_t)u * kl + k] = hpv; }
            hn[e] = h;
        }
        __syncthreads();
        cur ^= 1;
    }
}
void launch_gru_seq(hipStream_t st, const CellFwdArgs& a) {
    const int cb = cell_cb(a.H, a.B);
    const size_t lds = gru_fwd_lds(a.H, cb) * sizeof(float);
    const int bs = 3 * a.H * cb;                      // 3 gates x (unit, column) elements; gru_seq_fits: H * cb is a multiple of 64 and <= 256
    if (a.T <= 8) hipLaunchKernelGGL((k_gru_seq<8>), dim3(a.nseq * (a.B / cb)), dim3(bs), lds, st, a, cb);
    else if (a.T <= 32) hipLaunchKernelGGL((k_gru_seq<32>), dim3(a.nseq * (a.B / cb)), dim3(bs), lds, st, a, cb);
    else hipLaunchKernelGGL((k_gru_seq<64>), dim3(a.nseq * (a.B / cb)), dim3(bs), lds, st, a, cb);      // gru_seq_fits: T <= 64
}

// BPTT over the whole s-sequence, one workgroup per group of CB columns (the arithmetic of T calls of k_gru_bwd_step); the state0 gradient
// (a sum over ALL columns, ascending b) is folded by k_state0_grad (cell.h) afterwards.  PF (T <= 8): the six stashed values of every step are
// requested before the loop; otherwise one step ahead.
template <bool PF>
__global__ __launch_bounds__(1024) void k_gru_bwd_seq(CellBwdArgs A, int CB) {
    extern __shared__ float lds[];
    const int H = A.H, B = A.B, TB = A.TB, N = 3 * H, per = H * CB, b0 = blockIdx.x * CB;
    const int NP = N + 1;              // padded row stride (the lanes of a wave read different rows j at the same n)
    float* Wh_s = lds;                 // [H][3H + 1]
    float* dG_s = Wh_s + H * NP;       // [3H][CB] dGh of the current step
    float* dhn_s = dG_s + N * CB;      // [H*CB]
    for (int i = threadIdx.x; i < H * N; i += blockDim.x) Wh_s[(i / N) * NP + i % N] = A.Wh[i];
    for (int e = threadIdx.x; e < per; e += blockDim.x) dhn_s[e] = 0.0f;
    __syncthreads();
    const int e = threadIdx.x; const bool on = e < per;
    const int u = on ? e / CB : 0, bl = on ? e - u * CB : 0;
    struct St { float r, z, n, ghn, hp, dH; };
    auto fetch = [&](int t) { St s; const size_t k = (size_t)t * B + b0 + bl;
        s.r = A.gates[(size_t)u * TB + k]; s.z = A.gates[(size_t)(H + u) * TB + k]; s.n = A.gates[(size_t)(2 * H + u) * TB + k];
        s.ghn = A.aux[(size_t)u * TB + k]; s.hp = A.hprev[(size_t)u * TB + k]; s.dH = A.dH[(size_t)u * TB + k]; return s; };
    St all[PF ? 8 : 1];
    if constexpr (PF) {
#pragma unroll
        for (int t = 0; t < 8; t++) if (t < A.T) all[t] = fetch(t);
    }
    St nx; if constexpr (!PF) nx = fetch(A.T - 1);
    float dhz = 0.0f;
#pragma unroll
    for (int tt = 0; tt < (PF ? 8 : 1 << 30); tt++) {
        const int t = (PF ? 7 : A.T - 1) - tt;
        if (t < 0) break;
        if (PF && t >= A.T) continue;
        St c; if constexpr (PF) c = all[PF ? t : 0]; else c = nx;
        if (on) {
            const size_t k = (size_t)t * B + b0 + bl;
            const float r = c.r, z = c.z, n = c.n, ghn = c.ghn, hp = c.hp;
            const float dhn = t == A.T - 1 ? 0.0f : dhn_s[e];
            const float dh = c.dH + dhn;
            const float omz = 1.0f - z; const float n2 = n * n; const float omn2 = 1.0f - n2; const float a1 = dh * omz; const float dn = a1 * omn2;
            const float hmn = hp - n; const float b1 = dh * hmn; const float b2 = b1 * z; const float dz = b2 * omz;
            const float c1 = dn * ghn; const float c2 = c1 * r; const float omr = 1.0f - r; const float dr = c2 * omr;
            const float dnr = dn * r;
            dhz = dh * z;
            A.dG[(size_t)u * TB + k] = dr; A.dG[(size_t)(H + u) * TB + k] = dz; A.dG[(size_t)(2 * H + u) * TB + k] = dn;
            A.dGh[(size_t)u * TB + k] = dr; A.dGh[(size_t)(H + u) * TB + k] = dz; A.dGh[(size_t)(2 * H + u) * TB + k] = dnr;
            dG_s[u * CB + bl] = dr; dG_s[(H + u) * CB + bl] = dz; dG_s[(2 * H + u) * CB + bl] = dnr;
        }
        if constexpr (!PF) { if (t > 0) nx = fetch(t - 1); }
        __syncthreads();
        if (on) {                                                  // dh_{t-1}[j][b] = (sum_n dGh[n][t,b] Wh[j][n], n ascending) + dh z   (j == u)
            float acc = 0.0f;
#pragma unroll 8
            for (int n = 0; n < N; n++) acc = fmaf(dG_s[n * CB + bl], Wh_s[u * NP + n], acc);
            dhn_s[e] = acc + dhz;
        }
        __syncthreads();
    }
    for (int e2 = threadIdx.x; e2 < per; e2 += blockDim.x) { const int u2 = e2 / CB, bl2 = e2 - u2 * CB; A.dhn[u2 * B + b0 + bl2] = dhn_s[e2]; }
}
void launch_gru_bwd_seq(hipStream_t st, const CellBwdArgs& a) {
    const int cb = cell_cb(a.H, a.B);
    const size_t lds = gru_bwd_lds(a.H, cb) * sizeof(float);
    int bs = ((a.H * cb + 63) / 64) * 64; if (bs > 1024) bs = 1024;
    if (a.T <= 8) hipLaunchKernelGGL((k_gru_bwd_seq<true>), dim3(a.B / cb), dim3(bs), lds, st, a, cb);
    else hipLaunchKernelGGL((k_gru_bwd_seq<false>), dim3(a.B / cb), dim3(bs), lds, st, a, cb);
    launch_state0_grad(st, a);
}
