// skip.hip -- the join of a Flux SkipConnection(layers, +) block over the batch-innermost Y[feature][column] layout: three element-wise streams, no parameters.
//     forward, every pass      y = a + x                          a = the stored output of the block's last inner layer K (after K's activation)
//                                                                 x = the stored output of the block's entry P, the producer the first inner layer F reads (after P's)
//     backward at the join     dK = dY .* act_K'(y_K)             dY = dact[join], written by the layer above through an identity epilogue (the join has no activation)
//     backward at the entry    dP = (dF + dY) .* act_P'(y_P)      dF = F's raw input gradient: F's dX launch runs with the IDENTITY epilogue (src_act, engine_program.hip)
// One fp32 add of two operands per element: commutative, so there is no order to fix, and P's derivative is taken ONCE, after the sum (DESIGN.md section 4 "Skip connections").
// Nothing depends on graph mode, MFMA on / off, launch geometry or which of the two work splits below runs.
//
// Work split, as dropout.hip's: thread = (feature, column quad) with one 16-byte access per operand where every row start is 16-byte aligned and the column count is a
// multiple of 4; otherwise (B = 5: ten [s ; s'] columns, unaligned rows) thread = (feature, column).  Every load of a thread is issued before the first use: one dependent
// round trip.  One wave per workgroup, the grid sized from n * columns / 4.  No LDS, no atomics, plain vector stores.  The entry launch may run in place (dP == dF): each
// thread reads its own elements before it writes them and no other thread touches them.
#include "common.h"

struct SkipArgs { int n, ncols, lda, ldx, ldo, act; };      // ncols columns per row; lda, ldx: leading dimensions of the two operands; ldo: of the output (and of the B-long gradient rows)

// V = 4: thread = (f, quad of the ncols columns), rows 16-byte aligned.  V = 1: thread = (f, column).  A, X already point at the window's first column
template <int V> __global__ __launch_bounds__(64) void k_skip_fwd(SkipArgs S, const float* __restrict__ A, const float* __restrict__ X, float* __restrict__ Y) {
    const int per = V == 4 ? S.ncols / 4 : S.ncols;
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    const size_t f = t / per; const int j = (int)(t - f * per);
    if (f >= (size_t)S.n) return;
    if (V == 4) {
        const int c0 = 4 * j;
        const float4 a = *reinterpret_cast<const float4*>(A + f * S.lda + c0); const float4 x = *reinterpret_cast<const float4*>(X + f * S.ldx + c0);
        float4 y; y.x = a.x + x.x; y.y = a.y + x.y; y.z = a.z + x.z; y.w = a.w + x.w;
        *reinterpret_cast<float4*>(Y + f * S.ldo + c0) = y;
    } else {
        const float a = A[f * S.lda + j], x = X[f * S.ldx + j];
        Y[f * S.ldo + j] = a + x;
    }
}

// dY, dK: [n][B] (B = S.ncols = S.ldo); Yk: [n][lda], columns 0 .. B
template <int V> __global__ __launch_bounds__(64) void k_skip_bwd_join(SkipArgs S, const float* __restrict__ dY, const float* __restrict__ Yk, float* __restrict__ dK) {
    const int per = V == 4 ? S.ncols / 4 : S.ncols;
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    const size_t f = t / per; const int j = (int)(t - f * per);
    if (f >= (size_t)S.n) return;
    if (V == 4) {
        const int c0 = 4 * j;
        float4 g = *reinterpret_cast<const float4*>(dY + f * S.ldo + c0); const float4 y = *reinterpret_cast<const float4*>(Yk + f * S.lda + c0);
        dact_v4(g, y, S.act);
        *reinterpret_cast<float4*>(dK + f * S.ldo + c0) = g;
    } else {
        const float d = dY[f * S.ldo + j], y = Yk[f * S.lda + j];
        dK[f * S.ldo + j] = dact_f(d, y, S.act);
    }
}

// dF, dY, dP: [n][B]; Yp: [n][lda], columns 0 .. B.  dP may alias dF (not __restrict__)
template <int V> __global__ __launch_bounds__(64) void k_skip_bwd_entry(SkipArgs S, const float* dF, const float* __restrict__ dY, const float* __restrict__ Yp, float* dP) {
    const int per = V == 4 ? S.ncols / 4 : S.ncols;
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    const size_t f = t / per; const int j = (int)(t - f * per);
    if (f >= (size_t)S.n) return;
    if (V == 4) {
        const int c0 = 4 * j;
        const float4 a = *reinterpret_cast<const float4*>(dF + f * S.ldo + c0); const float4 b = *reinterpret_cast<const float4*>(dY + f * S.ldo + c0);
        const float4 y = *reinterpret_cast<const float4*>(Yp + f * S.lda + c0);
        float4 g; g.x = a.x + b.x; g.y = a.y + b.y; g.z = a.z + b.z; g.w = a.w + b.w;
        dact_v4(g, y, S.act);
        *reinterpret_cast<float4*>(dP + f * S.ldo + c0) = g;
    } else {
        const float a = dF[f * S.ldo + j], b = dY[f * S.ldo + j], y = Yp[f * S.lda + j];
        dP[f * S.ldo + j] = dact_f(a + b, y, S.act);
    }
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static unsigned skip_blocks(int n, int ncols, bool vec) { const size_t threads = (size_t)n * (vec ? ncols / 4 : ncols); return (unsigned)((threads + 63) / 64); }
void launch_skip_fwd(hipStream_t stream, int n, const float* A, int lda, const float* X, int ldx, int col0, int ncols, float* Y) {
    if (n <= 0 || ncols <= 0) return;
    SkipArgs S; S.n = n; S.ncols = ncols; S.lda = lda; S.ldx = ldx; S.ldo = ncols; S.act = DQN_ACT_IDENTITY;
    A += col0; X += col0;
    const bool vec = ncols % 4 == 0 && lda % 4 == 0 && ldx % 4 == 0 && al16(A) && al16(X) && al16(Y);
    if (vec) hipLaunchKernelGGL(k_skip_fwd<4>, dim3(skip_blocks(n, ncols, true)), dim3(64), 0, stream, S, A, X, Y);
    else hipLaunchKernelGGL(k_skip_fwd<1>, dim3(skip_blocks(n, ncols, false)), dim3(64), 0, stream, S, A, X, Y);
}
void launch_skip_bwd_join(hipStream_t stream, int n, const float* dY, const float* Yk, int ld, int B, float* dK, int act_k) {
    if (n <= 0 || B <= 0) return;
    SkipArgs S; S.n = n; S.ncols = B; S.lda = ld; S.ldx = 0; S.ldo = B; S.act = act_k;
    const bool vec = B % 4 == 0 && ld % 4 == 0 && al16(dY) && al16(Yk) && al16(dK);
    if (vec) hipLaunchKernelGGL(k_skip_bwd_join<4>, dim3(skip_blocks(n, B, true)), dim3(64), 0, stream, S, dY, Yk, dK);
    else hipLaunchKernelGGL(k_skip_bwd_join<1>, dim3(skip_blocks(n, B, false)), dim3(64), 0, stream, S, dY, Yk, dK);
}
void launch_skip_bwd_entry(hipStream_t stream, int n, const float* dF, const float* dY, const float* Yp, int ld, int B, float* dP, int act_p) {
    if (n <= 0 || B <= 0) return;
    SkipArgs S; S.n = n; S.ncols = B; S.lda = ld; S.ldx = 0; S.ldo = B; S.act = act_p;
    const bool vec = B % 4 == 0 && ld % 4 == 0 && al16(dF) && al16(dY) && al16(Yp) && al16(dP);
    if (vec) hipLaunchKernelGGL(k_skip_bwd_entry<4>, dim3(skip_blocks(n, B, true)), dim3(64), 0, stream, S, dF, dY, Yp, dP);
    else hipLaunchKernelGGL(k_skip_bwd_entry<1>, dim3(skip_blocks(n, B, false)), dim3(64), 0, stream, S, dF, dY, Yp, dP);
}
