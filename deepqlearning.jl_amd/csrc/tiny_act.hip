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
#include "tiny_fwd.h"

// CTL: the instantiation a group launches when any member's env set is of a control kind (env_body.h); every other group runs CTL = false
template <int NTH, bool CTL>
__global__ __launch_bounds__(NTH) void k_tiny_act(const TinyActArgs* __restrict__ Ap, int first, int last) {
    extern __shared__ __align__(16) float sm[];
    // layer descriptors, the env set and the replay record in LDS: a per-item `A.L[l].field` / `A.V.field` is a dependent GLOBAL load (the record lives in device
    // memory); staged once, every later access is an LDS read
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
    // ---- phase 1: forward of the online net on the n columns, level by level (tiny_fwd.h: k_tiny_step's phase 1 with one network and cols = ld = n)
    tiny_forward<NTH>(sm, LD, LEV, nlev, Pon, X0, n);
    // ---- phase 2: the tail of the step, on the finished head outputs in LDS (S = 1: nothing is left to reduce, bias and activation are applied)
    {
        const int lq = A.dueling ? A.last_adv : A.last_base;
        auto head_of = [&](int l) { HeadSrc h; h.p = sm + LD[l][F_Y]; h.ld = n; h.S = 1; h.per_s = 0; h.bias = nullptr; h.act = DQN_ACT_IDENTITY; return h; };
        ActHeads Hd; Hd.adv = head_of(lq); Hd.val = head_of(A.dueling ? A.last_val : lq); Hd.dueling = A.dueling; Hd.q_out = A.pol_q; Hd.amax = A.pol_a;
        env_step_body<false, CTL>(V, A.rs, Hd, Rs, nullptr);
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
// the function's dynamic-LDS request (tiny_fwd.h tiny_fn_raise_lds)
int tiny_act_raise_lds(unsigned lds_bytes, int control) {
    static TinyLdsAsk ask[2];
    return tiny_fn_raise_lds(control ? reinterpret_cast<const void*>(&k_tiny_act<1024, true>) : reinterpret_cast<const void*>(&k_tiny_act<1024, false>), ask[control ? 1 : 0], lds_bytes);
}
int launch_tiny_act(hipStream_t st, const TinyActArgs* a_dev, int K, unsigned max_lds_bytes, int first, int last, int control) {
    if (tiny_act_raise_lds(max_lds_bytes, control)) return -1;
    if (control) hipLaunchKernelGGL((k_tiny_act<1024, true>), dim3(K), dim3(1024), max_lds_bytes, st, a_dev, first, last);
    else hipLaunchKernelGGL((k_tiny_act<1024, false>), dim3(K), dim3(1024), max_lds_bytes, st, a_dev, first, last);
    return 0;
}
