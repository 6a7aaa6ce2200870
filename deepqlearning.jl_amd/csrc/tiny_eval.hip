// tiny_eval.hip -- basic_evaluation (src/evaluation_policy.jl:17-42) of a dense network that fits in LDS, the WHOLE greedy episode loop inside the kernel: a workgroup
// stages its member's record and online parameters once, resets the member's evaluation copies, and then repeats  observe -> forward -> tail  until every copy's one
// episode is over or the launch has run its n_steps (<= TINY_EVAL_STEPS) vector steps.  An engine group (engine_group.hip, dqn_evaluate_many) evaluates K members with
// ONE launch of K workgroups per TINY_EVAL_STEPS vector steps, workgroup k on record Ap[k]; the per-copy state (the member's eval_env arrays, the step record) lives in
// global memory, so a longer evaluation is back-to-back launches.  Everything a workgroup reads or writes is its member's own: no atomic, no traffic between workgroups,
// nothing waits on another workgroup.
//
// Every value follows the order of the launches dqn_evaluate enqueues per vector step, so a member's sums are bit for bit that call's:
//   forward   tiny_forward (tiny_fwd.h), THE statement k_tiny_act runs, on one TILE of copies at a time.  A column's chain reads that column alone, so neither the
//             tile width nor which columns share a tile can change a bit; tiles of a width that is a multiple of 4 take the 16-byte path, a ragged rest the scalar one
//   tail      env_step_body<false> (env_body.h) with eval_mode = 1 on ALL the copies at once: thread i = copy i, every draw keyed by (seed, t, i, purpose)
//   observe   obs_elem of the copy's post-step state; a finished copy is never reset in evaluation mode (envs.hip), it idles beside the live ones
#include "common.h"
#include "env_body.h"
#include "tiny_fwd.h"

// the tiles of n copies at tile width tw (a multiple of 4), in order: full tiles, then the rest cut into its multiple-of-4 part and a scalar tail of 1..3 columns
__host__ __device__ __forceinline__ int tiny_eval_tile(int n, int tw, int c0) {
    int w = n - c0 < tw ? n - c0 : tw;
    if (w > 4 && (w & 3)) w &= ~3;
    return w;
}

// CTL: as k_tiny_act's -- the instantiation for a group with a member of a control kind
template <int NTH, bool CTL>
__global__ __launch_bounds__(NTH) void k_tiny_eval(TinyEvalArgs* Ap, int n_steps, int first, int last) {
    extern __shared__ __align__(16) float sm[];
    __shared__ int LD[TINY_MAX_LAYERS][F_NF];
    __shared__ int LEV[TINY_MAX_LAYERS][3];
    __shared__ EnvDev Vs; __shared__ ReplayMeta Rs;
    TinyEvalArgs& T = Ap[blockIdx.x]; const TinyActArgs& A = T.a;
    const int tid = threadIdx.x, n = A.V.n, E = A.V.E, nlev = A.nlev, P = (int)A.P, tw = T.tw;
    float* Pon = sm + A.p_off; float* X0 = sm + A.x_off;
    // ---- stage the record, the descriptors and the parameters ONCE per launch (k_tiny_act's phase 0)
    for (int i = tid; i < (int)(sizeof(EnvDev) / 4); i += NTH) reinterpret_cast<int*>(&Vs)[i] = reinterpret_cast<const int*>(&A.V)[i];
    for (int i = tid; i < (int)(sizeof(ReplayMeta) / 4); i += NTH) reinterpret_cast<int*>(&Rs)[i] = reinterpret_cast<const int*>(&A.R)[i];
    if (tid < A.nl) {
        const LayerDev& L = A.L[tid];
        LD[tid][F_K] = L.K; LD[tid][F_N] = L.N; LD[tid][F_ACT] = L.act; LD[tid][F_SRC] = L.src; LD[tid][F_W] = (int)L.w_off; LD[tid][F_B] = (int)L.b_off;
        LD[tid][F_FKC] = L.fwd_kc; LD[tid][F_Y] = A.y_off[tid];
    }
    if (tid >= 64 && tid < 64 + nlev) { const int v = tid - 64; LEV[v][0] = A.lev_n[v]; LEV[v][1] = A.lev_l[v][0]; LEV[v][2] = A.lev_l[v][1]; }
    for (int i = tid; i < P; i += NTH) Pon[i] = A.p_on[i];
    __syncthreads();
    const EnvDev& V = Vs;
    // ---- reset!(env) of every copy at t = 0 (k_env_reset_pending with force_all = 1, and the memset of the reward sums)
    if (first) {
        for (int i = tid; i < n; i += NTH) {
            V.dones[i] = 0; V.ep_reward[i] = 0.0f; V.ep_step[i] = 0; V.pending[i] = 0; V.fin_reward[i] = 0.0;
            store_reset(V, i, 0ull);
        }
        __syncthreads();
    }
    const int lq = A.dueling ? A.last_adv : A.last_base, nA = V.nA;
    HeadSrc ha; ha.p = T.heads; ha.ld = n; ha.S = 1; ha.per_s = 0; ha.bias = nullptr; ha.act = DQN_ACT_IDENTITY;
    HeadSrc hv = ha; if (A.dueling) hv.p = T.heads + (size_t)nA * n;
    ActHeads Hd; Hd.adv = ha; Hd.val = hv; Hd.dueling = A.dueling; Hd.q_out = A.pol_q; Hd.amax = A.pol_a;
    for (int step = 0; step < n_steps; step++) {
        // every copy pending: the evaluation is over (workgroup-uniform: a block-wide count; copy i's flag was written by thread i, n <= NTH)
        if (__syncthreads_count(tid < n && !V.pending[tid]) == 0) break;
        for (int c0 = 0; c0 < n;) {
            const int w = tiny_eval_tile(n, tw, c0);
            // the tile's policy input x[E][w] = observe(env) of the copies' states as they stand (k_env_observe / k_env_observe2's x elements)
            for (int q = tid; q < E * w; q += NTH) {
                const int f = q / w, j = q - f * w;
                uint32_t sw; int px, py; load_state(V, c0 + j, &sw, &px, &py);
                unsigned char b; X0[q] = obs_elem(V, sw, px, py, f, &b);
            }
            lds_barrier();
            tiny_forward<NTH>(sm, LD, LEV, nlev, Pon, X0, w);
            // the tile's head outputs to their columns of heads[.][n] (the barrier behind the next tile's observe keeps that tile's forward off these rows)
            const float* Ya = sm + LD[lq][F_Y];
            for (int q = tid; q < nA * w; q += NTH) { const int a = q / w, j = q - a * w; T.heads[(size_t)a * n + c0 + j] = Ya[q]; }
            if (A.dueling) { const float* Yv = sm + LD[A.last_val][F_Y]; for (int j = tid; j < w; j += NTH) T.heads[(size_t)nA * n + c0 + j] = Yv[j]; }
            c0 += w;
        }
        __syncthreads();      // (full: the heads travel through global memory)
        env_step_body<false, CTL>(V, &T.roll, Hd, Rs, nullptr);
        __syncthreads();      // (full: the states, the pending flags and the record's t travel through global memory)
    }
    if (!last) return;
    // ---- avg_r += r_tot; avg_steps += step, in episode order (dqn_evaluate's host loop): staged in parallel, summed by one thread
    double* rb = reinterpret_cast<double*>(sm + T.r_off); int* sb = reinterpret_cast<int*>(rb + n);
    for (int i = tid; i < n; i += NTH) { rb[i] = V.fin_reward[i]; sb[i] = V.ep_step[i]; }
    __syncthreads();
    if (tid == 0) {
        double r = 0.0; long long s = 0;
        for (int i = 0; i < n; i++) { r += rb[i]; s += sb[i]; }
        EvalSums o; o.reward_sum = r; o.steps = s; *T.out = o;
    }
}
int tiny_eval_raise_lds(unsigned lds_bytes, int control) {
    static TinyLdsAsk ask[2];
    return tiny_fn_raise_lds(control ? reinterpret_cast<const void*>(&k_tiny_eval<1024, true>) : reinterpret_cast<const void*>(&k_tiny_eval<1024, false>), ask[control ? 1 : 0], lds_bytes);
}
int launch_tiny_eval(hipStream_t st, TinyEvalArgs* a_dev, int K, unsigned max_lds_bytes, int n_steps, int first, int last, int control) {
    if (tiny_eval_raise_lds(max_lds_bytes, control)) return -1;
    if (control) hipLaunchKernelGGL((k_tiny_eval<1024, true>), dim3(K), dim3(1024), max_lds_bytes, st, a_dev, n_steps, first, last);
    else hipLaunchKernelGGL((k_tiny_eval<1024, false>), dim3(K), dim3(1024), max_lds_bytes, st, a_dev, n_steps, first, last);
    return 0;
}
