// tiny_fwd.h -- what the single-workgroup acting kernels (tiny_act.hip: one vector step per launch; tiny_eval.hip: a whole greedy episode loop per launch) share:
// the layer table a workgroup stages in LDS, the level-by-level LDS forward of the online net on n columns, and the per-function request for dynamic LDS.
// The forward is stated here and nowhere else; both kernels inline it, so a column's values do not depend on which kernel computed it or on how many columns sit beside it.
#pragma once
#include "common.h"

enum { F_K, F_N, F_ACT, F_SRC, F_W, F_B, F_FKC, F_Y, F_NF };      // a layer's row of the LDS table LD: the descriptor's fields and the LDS float offset of its activations [N][n]

// forward of the online net (parameters at Pon) on the n columns x[E][n] at X0, level by level: layer l's activations land at sm + LD[l][F_Y] as [N][n].  The canonical
// order (k_tiny_step's statement): per plan chunk (fwd_kc) acc = +0, k ascending acc = fma(x[k], W[k][n], acc); chunk sums added ascending; + bias; activation.
// Workgroup-uniform; every level ends on an LDS barrier, so the caller may read the last level's outputs at once.  n % 4 == 0: four columns per item, 16-byte accesses
template <int NTH>
__device__ __forceinline__ void tiny_forward(float* sm, const int (*LD)[F_NF], const int (*LEV)[3], const int nlev, const float* Pon, const float* X0, const int n) {
    const int tid = threadIdx.x;
    auto qdiv = [](int x, float rcp) { return (int)(((float)x + 0.5f) * rcp); };      // x / d through one multiply, exact for x < 2^16: an item index is below N * n, which the LDS bound (tiny_act_decline) keeps under 25 856
    const bool v4 = (n & 3) == 0; const float rn = 1.0f / (float)n;
    for (int lv = 0; lv < nlev; lv++) {
        const int nlay = LEV[lv][0];
        // the level's one or two sibling layers share ONE item loop; their descriptors sit in registers (per-item selects, no LDS lookups)
        struct FD { int K, N, act, woff, boff, S, kc; const float* X; float* Y; } fd[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int l = LEV[lv][1 + (q < nlay ? q : 0)]; const int src = LD[l][F_SRC];
            fd[q].K = LD[l][F_K]; fd[q].N = LD[l][F_N]; fd[q].act = LD[l][F_ACT]; fd[q].woff = LD[l][F_W]; fd[q].boff = LD[l][F_B];
            fd[q].S = dqn_nchunks(fd[q].K, LD[l][F_FKC]); fd[q].kc = dqn_chunk_len(fd[q].K, LD[l][F_FKC]);
            fd[q].X = src < 0 ? X0 : sm + LD[src][F_Y]; fd[q].Y = sm + LD[l][F_Y];
        }
        if (v4) {
            // four consecutive columns per item with 16-byte LDS accesses (n % 4 == 0: every row is 16-B aligned)
            const int c4n = n >> 2; const float rc4 = 1.0f / (float)c4n;
            const int cnt_a = fd[0].N * c4n, cnt_b = nlay > 1 ? fd[1].N * c4n : 0;
            for (int it0 = tid; it0 < cnt_a + cnt_b; it0 += NTH) {
                const bool sec = it0 >= cnt_a; const int it = sec ? it0 - cnt_a : it0;
                const int K = sec ? fd[1].K : fd[0].K, N = sec ? fd[1].N : fd[0].N, S = sec ? fd[1].S : fd[0].S, kc = sec ? fd[1].kc : fd[0].kc;
                const int o = qdiv(it, rc4), c = 4 * (it - o * c4n);
                const float* W = Pon + (sec ? fd[1].woff : fd[0].woff) + o; const float bias = Pon[(sec ? fd[1].boff : fd[0].boff) + o];
                const float* X = (sec ? fd[1].X : fd[0].X) + c;
                f32x4c tot = {0.f, 0.f, 0.f, 0.f};
                for (int s = 0; s < S; s++) {
                    const int k0 = s * kc, k1 = min(K, k0 + kc);
                    f32x4c acc = {0.f, 0.f, 0.f, 0.f}; int k = k0;
                    for (; k + 4 <= k1; k += 4) {
                        f32x4c xv[4]; float wv[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) { xv[u] = *reinterpret_cast<const f32x4c*>(X + (k + u) * n); wv[u] = W[(k + u) * N]; }
#pragma unroll
                        for (int u = 0; u < 4; u++) { acc.x = fmaf(xv[u].x, wv[u], acc.x); acc.y = fmaf(xv[u].y, wv[u], acc.y); acc.z = fmaf(xv[u].z, wv[u], acc.z); acc.w = fmaf(xv[u].w, wv[u], acc.w); }
                    }
                    for (; k < k1; k++) { const f32x4c x = *reinterpret_cast<const f32x4c*>(X + k * n); const float w = W[k * N]; acc.x = fmaf(x.x, w, acc.x); acc.y = fmaf(x.y, w, acc.y); acc.z = fmaf(x.z, w, acc.z); acc.w = fmaf(x.w, w, acc.w); }
                    if (s == 0) tot = acc; else { tot.x = tot.x + acc.x; tot.y = tot.y + acc.y; tot.z = tot.z + acc.z; tot.w = tot.w + acc.w; }
                }
                const int act = sec ? fd[1].act : fd[0].act;
                const f32x4c y = {act_f(tot.x + bias, act), act_f(tot.y + bias, act), act_f(tot.z + bias, act), act_f(tot.w + bias, act)};
                *reinterpret_cast<f32x4c*>((sec ? fd[1].Y : fd[0].Y) + o * n + c) = y;
            }
            lds_barrier();
            continue;
        }
        const int cnt_a = fd[0].N * n, cnt_b = nlay > 1 ? fd[1].N * n : 0;
        for (int it0 = tid; it0 < cnt_a + cnt_b; it0 += NTH) {
            const bool sec = it0 >= cnt_a; const int it = sec ? it0 - cnt_a : it0;
            const int K = sec ? fd[1].K : fd[0].K, N = sec ? fd[1].N : fd[0].N, S = sec ? fd[1].S : fd[0].S, kc = sec ? fd[1].kc : fd[0].kc;
            const int o = qdiv(it, rn), c = it - o * n;
            const float* W = Pon + (sec ? fd[1].woff : fd[0].woff) + o; const float bias = Pon[(sec ? fd[1].boff : fd[0].boff) + o];
            const float* X = (sec ? fd[1].X : fd[0].X) + c;
            float tot = 0.0f;
            for (int s = 0; s < S; s++) {
                const int k0 = s * kc, k1 = min(K, k0 + kc);
                float acc = 0.0f; int k = k0;
                for (; k + 8 <= k1; k += 8) {      // 16 independent LDS reads in flight; the chain stays k-ascending
                    float xv[8], wv[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) { xv[u] = X[(k + u) * n]; wv[u] = W[(k + u) * N]; }
#pragma unroll
                    for (int u = 0; u < 8; u++) acc = fmaf(xv[u], wv[u], acc);
                }
                for (; k < k1; k++) acc = fmaf(X[k * n], W[k * N], acc);
                tot = s == 0 ? acc : tot + acc;
            }
            (sec ? fd[1].Y : fd[0].Y)[o * n + c] = act_f(tot + bias, sec ? fd[1].act : fd[0].act);
        }
        lds_barrier();
    }
}

// dynamic LDS beyond what a function is granted by default has to be requested per function AND per device (tiny_step.hip tiny_raise_lds): asked for on every enqueue,
// the largest size ever requested on the device and never less, a refusal reported.  The kernel's static arrays count against the same 160 KB: checked once against
// the budget the eligibility rules keep for them (TINY_ACT_TAIL_LDS)
struct TinyLdsAsk { unsigned asked[64] = {}; int checked = 0; };
inline int tiny_fn_raise_lds(const void* fn, TinyLdsAsk& s, unsigned lds_bytes) {
    if (!s.checked) {
        hipFuncAttributes fa; if (hipFuncGetAttributes(&fa, fn) != hipSuccess) { (void)hipGetLastError(); return -1; }
        if (fa.sharedSizeBytes > (size_t)TINY_ACT_TAIL_LDS) return -1;
        s.checked = 1;
    }
    int dev = 0; if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); dev = 0; }
    const unsigned want = lds_bytes > s.asked[dev] ? lds_bytes : s.asked[dev];
    if (want == s.asked[dev] && want != 0) return 0;
    if (want + TINY_ACT_TAIL_LDS <= 64 * 1024) return 0;
    const hipError_t le = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want);
    if (le != hipSuccess) { (void)hipGetLastError(); return -1; }
    s.asked[dev] = want;
    return 0;
}
