// dropout.hip -- Flux Dropout(p), dims = :, over the batch-innermost Y[feature][column] layout, in the ONE pass where Flux 0.14's automatic mode makes the layer active:
// the online network's forward on the s columns of a train step (the forward Flux.gradient differentiates) and its backward.  In every other pass the layer is the identity
// and launches nothing (engine.hip aliases the layer's target / policy activation to its producer's).
//     scale = Float32(1 / (1 - p))  (quotient in Float64, rounded once, on the host)      y = keep ? x * scale : +0      dX = (keep ? dY * scale : +0) .* act_src'(y_src)
// with y_src the PRODUCING layer's own, unmasked output (which is why the forward writes a buffer of its own), exactly as the pool and LayerNorm backwards do.
//
// Mask law (DESIGN.md section 4 "Dropout layers"; the engine's own -- Julia's RNG is not matched): Philox4x32-10 keyed by hparams.seed on the counter
//     { k lo, k hi, q, 0x44520000 | layer index }      k = train steps completed before this one      q = f * ceil(C / 4) + col / 4 over the C active columns
// the four output words belong to columns 4 * (col / 4) + 0 .. 3;  u = (word >> 8) * 2^-24;  keep <=> (double)u >= p  (so p = 0 keeps everything: no special case).
// k is StepState::step read ON THE DEVICE, so graph replays and dqn_train_steps see the right step: the forward runs before the TD launch bumps it (k = step), the backward
// after (k = step - 1).  The mask depends on (seed, k, layer, f, col, C) alone: not on graph mode, launch geometry or which of the two work splits below runs.
//
// Work split: thread = (feature, column quad), ONE Philox call per quad and one 16-byte access per operand where every row start is 16-byte aligned; otherwise (B = 5: ten
// columns, unaligned rows) thread = (feature, column), which draws its quad's four words and keeps its own.  The forward's rows carry [s ; s'] (2 C columns with double-Q):
// the quad that straddles the boundary (C mod 4 != 0) is half active, so activity is decided per ELEMENT (col < C), never per access.  The backward's rows are C long.
// Every load of a thread -- the step counter, x or (dY, y_src) -- is issued before the first use: one dependent round trip.  One wave per workgroup, the grid sized from
// n * columns / 4.  No LDS, no atomics, plain vector stores.
#include "common.h"

struct DoArgs { int n, ld, ncols, C, nq /* Philox quads per feature: ceil(C / 4) */, act_src; unsigned k0, k1, tag; double p; float scale; };

// keep bits of the quad (f, qd) at train step k: bit j = column 4 qd + j is kept
__device__ __forceinline__ unsigned do_keep4(const DoArgs& A, unsigned long long k, int f, int qd) {
    uint32_t c[4] = {(uint32_t)k, (uint32_t)(k >> 32), (uint32_t)f * (uint32_t)A.nq + (uint32_t)qd, A.tag};
    philox4x32_10(A.k0, A.k1, c);
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) { const float u = (float)(c[j] >> 8) * 0x1p-24f; if ((double)u >= A.p) m |= 1u << j; }
    return m;
}

// V = 4: thread = (f, quad of the ncols columns), rows 16-byte aligned.  V = 1: thread = (f, column)
template <int V> __global__ __launch_bounds__(64) void k_do_fwd(DoArgs A, const StepState* __restrict__ st, const float* __restrict__ X, float* __restrict__ Y) {
    const int per = V == 4 ? (A.ncols + 3) / 4 : A.ncols;
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    const size_t f = t / per; const int j = (int)(t - f * per);
    if (f >= (size_t)A.n) return;
    const unsigned long long k = st->step;      // the TD launch of this step has not run yet
    if (V == 4) {
        const int c0 = 4 * j;
        float4 x = *reinterpret_cast<const float4*>(X + f * A.ld + c0);
        if (c0 < A.C) {      // else the quad lies in the s' half: copied
            const unsigned m = do_keep4(A, k, (int)f, j);
            if (c0 + 0 < A.C) x.x = (m & 1u) ? x.x * A.scale : 0.0f;
            if (c0 + 1 < A.C) x.y = (m & 2u) ? x.y * A.scale : 0.0f;
            if (c0 + 2 < A.C) x.z = (m & 4u) ? x.z * A.scale : 0.0f;
            if (c0 + 3 < A.C) x.w = (m & 8u) ? x.w * A.scale : 0.0f;
        }
        *reinterpret_cast<float4*>(Y + f * A.ld + c0) = x;
    } else {
        float x = X[f * A.ld + j];
        if (j < A.C) { const unsigned m = do_keep4(A, k, (int)f, j >> 2); x = ((m >> (j & 3)) & 1u) ? x * A.scale : 0.0f; }
        Y[f * A.ld + j] = x;
    }
}

// dY, dX: [n][C]; Ysrc: [n][ld], columns 0 .. C
template <int V> __global__ __launch_bounds__(64) void k_do_bwd(DoArgs A, const StepState* __restrict__ st, const float* __restrict__ dY, const float* __restrict__ Ysrc, float* __restrict__ dX) {
    const int per = V == 4 ? A.C / 4 : A.C;
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    const size_t f = t / per; const int j = (int)(t - f * per);
    if (f >= (size_t)A.n) return;
    const unsigned long long k = st->step - 1ull;      // the TD launch of this step bumped the counter
    if (V == 4) {
        const int c0 = 4 * j;
        const float4 d = *reinterpret_cast<const float4*>(dY + f * A.C + c0); const float4 y = *reinterpret_cast<const float4*>(Ysrc + f * A.ld + c0);
        const unsigned m = do_keep4(A, k, (int)f, j);
        float4 g;
        g.x = (m & 1u) ? d.x * A.scale : 0.0f; g.y = (m & 2u) ? d.y * A.scale : 0.0f; g.z = (m & 4u) ? d.z * A.scale : 0.0f; g.w = (m & 8u) ? d.w * A.scale : 0.0f;
        dact_v4(g, y, A.act_src);
        *reinterpret_cast<float4*>(dX + f * A.C + c0) = g;
    } else {
        const float d = dY[f * A.C + j], y = Ysrc[f * A.ld + j];
        const unsigned m = do_keep4(A, k, (int)f, j >> 2);
        dX[f * A.C + j] = dact_f(((m >> (j & 3)) & 1u) ? d * A.scale : 0.0f, y, A.act_src);
    }
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static DoArgs do_args(int n, double p, unsigned long long seed, int layer, int ld, int ncols, int C, int act_src) {
    DoArgs A; A.n = n; A.ld = ld; A.ncols = ncols; A.C = C; A.nq = (C + 3) / 4; A.act_src = act_src; A.k0 = (unsigned)seed; A.k1 = (unsigned)(seed >> 32); A.tag = DQN_DO_TAG | (unsigned)layer;
    A.p = p; A.scale = (float)(1.0 / (1.0 - p));
    return A;
}
void launch_do_fwd(hipStream_t stream, int n, double p, unsigned long long seed, int layer, const StepState* st, const float* X, float* Y, int ld, int ncols, int C) {
    const DoArgs A = do_args(n, p, seed, layer, ld, ncols, C, 0);
    const bool vec = ld % 4 == 0 && ncols % 4 == 0 && al16(X) && al16(Y);
    const size_t threads = (size_t)n * (vec ? ncols / 4 : ncols); const unsigned blocks = (unsigned)((threads + 63) / 64);
    if (vec) hipLaunchKernelGGL(k_do_fwd<4>, dim3(blocks), dim3(64), 0, stream, A, st, X, Y);
    else hipLaunchKernelGGL(k_do_fwd<1>, dim3(blocks), dim3(64), 0, stream, A, st, X, Y);
}
void launch_do_bwd(hipStream_t stream, int n, double p, unsigned long long seed, int layer, const StepState* st, const float* dY, const float* Ysrc, int ld, int C, float* dX, int act_src) {
    const DoArgs A = do_args(n, p, seed, layer, ld, C, C, act_src);
    const bool vec = ld % 4 == 0 && C % 4 == 0 && al16(dY) && al16(Ysrc) && al16(dX);
    const size_t threads = (size_t)n * (vec ? C / 4 : C); const unsigned blocks = (unsigned)((threads + 63) / 64);
    if (vec) hipLaunchKernelGGL(k_do_bwd<4>, dim3(blocks), dim3(64), 0, stream, A, st, dY, Ysrc, dX);
    else hipLaunchKernelGGL(k_do_bwd<1>, dim3(blocks), dim3(64), 0, stream, A, st, dY, Ysrc, dX);
}
