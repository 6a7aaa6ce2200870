// tiny_act.hip -- ONE vector step of the device environment loop (src/solver.jl:82-132) of a dense network that fits in LDS as ONE single-workgroup launch:
// policy forward on the n columns of pol_x -> Q, argmax, exploration, act!, add_exp! (metadata, leaf priorities, sum-tree ancestors) -> the ring rows of the transition
// and the next policy input.  A standalone engine's acting program is the forward launches + k_env_step + k_env_observe2, one or two workgroups each; an engine group
// (engine_group.hip, dqn_rollout_many) steps K members with ONE launch of K workgroups of this kernel, workgroup k on record Ap[k].  Everything a workgroup reads or
// writes is its member's own: members share nothing, there is no atomic and no traffic between workgroups.
//
// Every value follows the canonical order of the launches this replaces, so a member ends bit for bit where dqn_rollout_explore leaves it:
//   forward   per plan chunk (fwd_kc): acc = +0; k ascending: acc = fma(x[k], W[k][n], acc); chunk sums added ascending; + bias; activation  (k_tiny_step's statement)
//   tail      env_step_body<false> (env_body.h), THE statement of the step's tail, on a HeadSrc with S = 1 that points at the LDS activations
//   observe   k_env_observe2's elements: ring row s = observation of the saved pre-step state, sp = observe(env), x = the next policy input (of the reset state where the
//             episode just ended), through the observation / reset laws of env_body.h
#include "common.h"
#include "env_body.h"

template <int NTH>
__global__ __launch_bounds__(NTH) void k_tiny_act(const TinyActArgs* __restrict__ Ap, int first, int last) {
    extern __shared__ __align__(16) float sm[];
    // layer descriptors, the env set and the replay record in LDS: a per-item `A.L[l].field` / `A.V.field` is a dependent GLOBAL load (the record lives in device
    // memory); staged once, every later access is an LDS read
    enum { F_K, F_N, F_ACT, F_SRC, F_W, F_B, F_FKC, F_Y, F_NF };
    __shared__ int LD[TINY_MAX_LAYERS][F_NF];
    __shared__ int LEV[TINY_MAX_LAYERS][3];
    __shared__ EnvDev Vs; __shared__ ReplayMeta Rs;
    const TinyActArgs& A = Ap[blockIdx.x];
    const int tid = threadIdx.x, n = A.V.n, E = A.V.E, nlev = A.nlev, P = (int)A.P, ne = n * E;
    float* Pon = sm + A.p_off; float* X0 = sm + A.x_off;
    // ---- phase 0: ONE round trip for everything whose address is known at entry
    static_assert(sizeof(EnvDev) % 4 == 0 && sizeof(ReplayMeta) % 4 == 0, "the records are staged word by word");
    for (int i = tid; i < (int)(sizeof(EnvDev) / 4); i += NTH) reinterpret_cast<int*>(&Vs)[i] = reinterpret_cast<const int*>(&A.V)[i];
    for (int i = tid; i < (int)(sizeof(ReplayMeta) / 4); i += NTH) reinterpret_cast<int*>(&Rs)[i] = reinterpret_cast<const int*>(&A.R)[i];
    if (tid < A.nl) {
        const LayerDev& L = A.L[tid];
        LD[tid][F_K] = L.K; LD[tid][F_N] = L.N; LD[tid][F_ACT] = L.act; LD[tid][F_SRC] = L.src; LD[tid][F_W] = (int)L.w_off; LD[tid][F_B] = (int)L.b_off;
        LD[tid][F_FKC] = L.fwd_kc; LD[tid][F_Y] = A.y_off[tid];
    }
    if (tid >= 64 && tid < 64 + nlev) { const int v = tid - 64; LEV[v][0] = A.lev_n[v]; LEV[v][1] = A.lev_l[v][0]; LEV[v][2] = A.lev_l[v][1]; }
    for (int i = tid; i < P; i += NTH) Pon[i] = A.p_on[i];
    if (!first) for (int q = tid; q < ne; q += NTH) X0[q] = A.pol_x[q];      // what the step before left (or a standalone call of the member)
    __syncthreads();
    const EnvDev& V = Vs;
    if (first) {
        // a call's first step: x = observe(env) of the states as they stand (k_env_observe; no reset is pending between calls)
        for (int q = tid; q < ne; q += NTH) {
            const int f = q / n, i = q - f * n;
            uint32_t sw; int px, py; load_state(V, i, &sw, &px, &py);
            unsigned char b; X0[q] = obs_elem(V, sw, px, py, f, &b);
        }
        lds_barrier();
    }
    // ---- phase 1: forward of the online net on the n columns, level by level (k_tiny_step's phase 1 with one network and cols = ld = n)
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
    // ---- phase 2: the tail of the step, on the finished head outputs in LDS (S = 1: nothing is left to reduce, bias and activation are applied)
    {
        const int lq = A.dueling ? A.last_adv : A.last_base;
        auto head_of = [&](int l) { HeadSrc h; h.p = sm + LD[l][F_Y]; h.ld = n; h.S = 1; h.per_s = 0; h.bias = nullptr; h.act = DQN_ACT_IDENTITY; return h; };
        ActHeads Hd; Hd.adv = head_of(lq); Hd.val = head_of(A.dueling ? A.last_val : lq); Hd.dueling = A.dueling; Hd.q_out = A.pol_q; Hd.amax = A.pol_a;
        env_step_body<false>(V, A.rs, Hd, Rs, nullptr);
    }
    __syncthreads();      // (full: the env states, the pending flags and the record's t / widx travel through global memory from the thread of a copy to the threads of its elements)
    // ---- phase 3: the transition's rows into the ring, the next policy input (k_env_observe2's elements)
    const unsigned long long t = (unsigned long long)A.rs->t; const long long widx = A.rs->widx, cap = Rs.cap;
    for (int q = tid; q < ne; q += NTH) {
        const int i = q / E, f = q - i * E;      // f fastest: coalesced rows
        long long slot = widx + i; if (slot >= cap) slot -= cap;
        uint32_t sw0, sw1; int p0x, p0y, p1x, p1y;
        load_state(V, i, &sw1, &p1x, &p1y);
        load_prev(V, i, &sw0, &p0x, &p0y);
        unsigned char b0, b1;
        const float v0 = obs_elem(V, sw0, p0x, p0y, f, &b0), v1 = obs_elem(V, sw1, p1x, p1y, f, &b1);
        const size_t dst = (size_t)slot * E + f;
        if (A.rows_u8) { reinterpret_cast<unsigned char*>(A.s_rows)[dst] = b0; reinterpret_cast<unsigned char*>(A.sp_rows)[dst] = b1; }
        else { reinterpret_cast<float*>(A.s_rows)[dst] = v0; reinterpret_cast<float*>(A.sp_rows)[dst] = v1; }
    }
    for (int q = tid; q < ne; q += NTH) {
        const int f = q / n, i = q - f * n;      // i fastest
        uint32_t sw; int px, py, tm = 0; load_state(V, i, &sw, &px, &py);
        if (V.pending[i]) reset_state(V, i, t, &sw, &tm, &px, &py);
        unsigned char b; A.pol_x[q] = obs_elem(V, sw, px, py, f, &b);      // (to global memory as well as to the next launch: dqn_envs_peek and a standalone call of the member read it)
    }
    if (!last) return;
    // ---- a call's last step: the episode bookkeeping the step left pending (k_env_reset_pending, force_all = 0)
    __syncthreads();      // (the elements above read the pending flags and the states this rewrites)
    for (int i = tid; i < n; i += NTH) {
        if (!V.pending[i]) continue;
        V.fin_eps[i] += 1; V.fin_reward[i] += (double)V.ep_reward[i];
        V.ep_reward[i] = 0.0f; V.ep_step[i] = 0; V.pending[i] = 0;
        store_reset(V, i, t);
    }
}
// dynamic LDS beyond what the function is granted by default has to be requested per function AND per device (tiny_step.hip tiny_raise_lds): asked for on every enqueue,
// the largest size ever requested on the device and never less, a refusal reported.  The kernel's static arrays count against the same 160 KB: checked once
int tiny_act_raise_lds(unsigned lds_bytes) {
    static unsigned asked[64] = {}; static int checked = 0;
    const void* fn = reinterpret_cast<const void*>(&k_tiny_act<1024>);
    if (!checked) {
        hipFuncAttributes fa; if (hipFuncGetAttributes(&fa, fn) != hipSuccess) { (void)hipGetLastError(); return -1; }
        if (fa.sharedSizeBytes > (size_t)TINY_ACT_TAIL_LDS) return -1;      // the eligibility rule (tiny_act_decline) budgets TINY_ACT_TAIL_LDS for them
        checked = 1;
    }
    int dev = 0; if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); dev = 0; }
    const unsigned want = lds_bytes > asked[dev] ? lds_bytes : asked[dev];
    if (want == asked[dev] && want != 0) return 0;
    if (want + TINY_ACT_TAIL_LDS <= 64 * 1024) return 0;
    const hipError_t le = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want);
    if (le != hipSuccess) { (void)hipGetLastError(); return -1; }
    asked[dev] = want;
    return 0;
}
int launch_tiny_act(hipStream_t st, const TinyActArgs* a_dev, int K, unsigned max_lds_bytes, int first, int last) {
    if (tiny_act_raise_lds(max_lds_bytes)) return -1;
    hipLaunchKernelGGL((k_tiny_act<1024>), dim3(K), dim3(1024), max_lds_bytes, st, a_dev, first, last);
    return 0;
}
