// envs.hip -- vectorised environments on the device: the env loop of dqn_train! (src/solver.jl:82-132) for n
// lock-stepped copies without any host round trip.  TestMDP restates test/test_env.jl:10-87, SimpleGridWorld restates the
// POMDPModels defaults (third-party; recalled), a tabular (PO)MDP is stepped from its matrices (POMDPTools' MDPCommonRLEnv / POMDPCommonRLEnv; recalled), MountainCar and InvertedPendulum restate POMDPModels' laws on a Float64 state (recalled; env_body.h).  All randomness is Philox4x32-10 with counter (vector step, env, purpose) so
// that the CPU twin (oracle/dqn_ref.c) reproduces trajectories bit for bit.
//
// One vector step is: [policy forward on pol_x -> greedy]  k_env_step  k_env_observe2   -- every argument is a fixed device
// pointer (the step counter, the eps schedule and the ring cursor live in RolloutDev), so the whole step replays as a hipGraph.
#include "common.h"
#include "env_body.h"      // the draws, the observation / reset laws, env_tree_rebuild, env_step_body

// observation of every env into (a) the staged rows[i][E] in the replay storage dtype and (b) batch-innermost x[E][n] (policy input)
__global__ void k_env_observe(EnvDev V, void* __restrict__ rows, int rows_u8, float* __restrict__ x) {
    const int n = V.n, E = V.E;
    const size_t tot = (size_t)n * E;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < tot; q += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(q / E), f = (int)(q % E);
        uint32_t sw; int px, py; load_state(V, i, &sw, &px, &py);
        unsigned char vb; const float v = obs_elem(V, sw, px, py, f, &vb);
        if (rows) { if (rows_u8) ((unsigned char*)rows)[q] = vb; else ((float*)rows)[q] = v; }
        if (x) x[(size_t)f * n + i] = v;
    }
}
void launch_env_observe(hipStream_t st, const EnvDev& V, void* rows, int rows_u8, float* x) {
    const size_t tot = (size_t)V.n * V.E; unsigned blocks = (unsigned)((tot + 255) / 256); if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_env_observe, dim3(blocks), dim3(256), 0, st, V, rows, rows_u8, x);
}

// CTL: the instantiation for the control kinds (env_body.h); every other kind runs CTL = false
template <bool CTL> __global__ __launch_bounds__(1024) void k_env_step(EnvDev V, RolloutDev* rs, ActHeads Hd, ReplayMeta R) { env_step_body<false, CTL>(V, rs, Hd, R, nullptr); }
template <bool CTL> __global__ __launch_bounds__(1024) void k_env_step_rec(EnvDev V, RolloutDev* rs, ActHeads Hd, EpStage ES) { ReplayMeta R; R.cap = 1; R.cap2 = 1; R.a = nullptr; R.r = nullptr; R.done = nullptr; R.tree = nullptr; R.state = nullptr; R.eps = 0.0f; R.alpha = 0.0f; env_step_body<true, CTL>(V, rs, Hd, R, &ES); }
void launch_env_step(hipStream_t st, const EnvDev& V, RolloutDev* rs, const ActHeads& Hd, const ReplayMeta& R) {
    if (env_is_control(V.kind)) hipLaunchKernelGGL(k_env_step<true>, dim3(1), dim3(1024), 0, st, V, rs, Hd, R);
    else hipLaunchKernelGGL(k_env_step<false>, dim3(1), dim3(1024), 0, st, V, rs, Hd, R);
}
void launch_env_step_rec(hipStream_t st, const EnvDev& V, RolloutDev* rs, const ActHeads& Hd, const EpStage& ES) {
    if (env_is_control(V.kind)) hipLaunchKernelGGL(k_env_step_rec<true>, dim3(1), dim3(1024), 0, st, V, rs, Hd, ES);
    else hipLaunchKernelGGL(k_env_step_rec<false>, dim3(1), dim3(1024), 0, st, V, rs, Hd, ES);
}

// after k_env_step: the transition's rows go straight into the ring -- s = observation of the saved pre-step state, sp = observe(env)
// (src/solver.jl:90) -- and the NEXT step's observation (of the reset state if the episode just ended) becomes the policy input
// x[E][n].  Nothing is staged: every element is regenerated from the few bytes of env state (TestMDP images stay L2-resident).
// Workgroups [0, rows_blocks) walk the rows (blockIdx -> env, f fastest: coalesced rows), the rest walk x (i fastest).
template <int VEC>
__device__ __forceinline__ void obs_vec(const EnvDev& V, uint32_t sw, int px_, int py_, int f, float* of, unsigned char* ob) {
    if (V.kind == DQN_ENV_TESTMDP) {
        const int hw = V.H * V.W; int c = f / hw, px = f - c * hw;        // obs[.., c] = observations[s[end - c]]  (test/test_env.jl:56-58)
#pragma unroll
        for (int u = 0; u < VEC; u++) {
            const int sel = (int)((sw >> (8 * (3 - c))) & 0xffu) - 1;
            const unsigned char b = V.images[sel * hw + px];
            ob[u] = b; of[u] = (float)b / 255.0f;
            if (++px == hw) { px = 0; c++; }
        }
    } else if (V.kind == DQN_ENV_TABULAR) {      // VEC elements of ONE feature row (VEC == 4: E % 4 == 0 and f % 4 == 0, the rows of the table are 16-byte aligned)
        typedef float FeatV __attribute__((ext_vector_type(VEC)));
        const FeatV v = *(const FeatV*)(V.tb_feat + (size_t)px_ * V.E + f);
#pragma unroll
        for (int u = 0; u < VEC; u++) { ob[u] = 0; of[u] = v[u]; }
    } else if (VEC == 1 && env_is_control(V.kind)) {      // E = 2: never the 16-byte path (VEC is a template argument: the VEC = 4 kernels carry no such branch)
        ob[0] = 0; of[0] = __int_as_float(f == 0 ? px_ : py_);
    } else {
#pragma unroll
        for (int u = 0; u < VEC; u++) { ob[u] = 0; of[u] = (float)((f + u) == 0 ? px_ : py_); }
    }
}
template <typename RowT, int VEC>
__global__ __launch_bounds__(256) void k_env_observe2(EnvDev V, const RolloutDev* __restrict__ rs0, RowT* __restrict__ s_rows, RowT* __restrict__ sp_rows,
                                                      long long cap, float* __restrict__ x, unsigned bx, unsigned rows_blocks, int grouped, int tree_wg, ReplayMeta R) {
    typedef RowT RowV __attribute__((ext_vector_type(VEC)));
    typedef float FloatV __attribute__((ext_vector_type(VEC)));
    const unsigned n = V.n, E = V.E;
    if (tree_wg && blockIdx.x == 0) {
        // (k_act_head did the per-copy part of add_exp!) workgroup 0, dispatched first: the new leaves' ancestors, beside the row writers instead of in front of them
        __shared__ float lvl[2][1024]; __shared__ float rim[48][2];
        const long long start = rs0->widx;                          // ticked by k_act_head: first ring position of this step's n experiences
        for (unsigned i = threadIdx.x; i < n; i += blockDim.x) { long long slot = start + i; if (slot >= cap) slot -= cap; lvl[0][i] = R.tree[R.cap2 + slot]; }
        env_tree_rebuild(R, (int)n, start, lvl, rim);
        return;
    }
    const unsigned blk = blockIdx.x - (unsigned)tree_wg;
    if (blk < rows_blocks) {
        const unsigned i = blk / bx, fv = (blk - i * bx) * blockDim.x + threadIdx.x;
        if (fv >= E / VEC) return;
        const unsigned f = fv * VEC;
        const RolloutDev* rs = rs0 + (grouped ? (i >> 2) : 0u);
        long long slot = rs->widx + i; if (slot >= cap) slot -= cap;
        uint32_t sw0, sw1; int p0x, p0y, p1x, p1y;
        load_state<VEC == 1>(V, (int)i, &sw1, &p1x, &p1y);
        load_prev<VEC == 1>(V, (int)i, &sw0, &p0x, &p0y);
        float of[VEC]; unsigned char ob[VEC]; RowT r[VEC];
        const size_t dst = (size_t)slot * E + f;
        obs_vec<VEC>(V, sw0, p0x, p0y, (int)f, of, ob);
#pragma unroll
        for (int u = 0; u < VEC; u++) r[u] = sizeof(RowT) == 1 ? (RowT)ob[u] : (RowT)of[u];
        __builtin_nontemporal_store(*(const RowV*)r, (RowV*)(s_rows + dst));      // ring rows are next read by a gather, steps later: streamed past the L2s (a kernel boundary otherwise writes back what the launch left dirty)
        obs_vec<VEC>(V, sw1, p1x, p1y, (int)f, of, ob);
#pragma unroll
        for (int u = 0; u < VEC; u++) r[u] = sizeof(RowT) == 1 ? (RowT)ob[u] : (RowT)of[u];
        __builtin_nontemporal_store(*(const RowV*)r, (RowV*)(sp_rows + dst));
    } else {
        const unsigned nv = n / VEC, qv = (blk - rows_blocks) * blockDim.x + threadIdx.x;
        if (qv >= nv * E) return;
        const unsigned f = qv / nv, i0 = (qv - f * nv) * VEC;             // VEC | n: the VEC elements share the feature
        const RolloutDev* rs = rs0 + (grouped ? (i0 >> 2) : 0u);          // (grouped: VEC == 4, the four copies are one group; every group's record holds the same t)
        const unsigned long long t = (unsigned long long)rs->t;
        float nx[VEC];
#pragma unroll
        for (int u = 0; u < VEC; u++) {
            uint32_t sw; int px, py, tm = 0; load_state<VEC == 1>(V, (int)(i0 + u), &sw, &px, &py);
            if (V.pending[i0 + u] && !V.eval_mode) reset_state<VEC == 1>(V, (int)(i0 + u), t, &sw, &tm, &px, &py);
            unsigned char b; nx[u] = obs_elem<VEC == 1>(V, sw, px, py, (int)f, &b);
        }
        { typedef float obs_f4 __attribute__((ext_vector_type(4)));      // the policy input is read by the very next launch, mostly from other XCDs: written through (sc1) as it is produced
          if constexpr (VEC == 4) { const obs_f4 v = {nx[0], nx[1], nx[2], nx[3]}; asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(x + (size_t)f * n + i0), "v"(v) : "memory"); }
          else *(FloatV*)(x + (size_t)f * n + i0) = *(const FloatV*)nx; }
    }
}
void launch_env_observe2(hipStream_t st, const EnvDev& V, const RolloutDev* rs, int rows_u8, void* s_rows, void* sp_rows, long long cap, float* x, int grouped, const ReplayMeta* tree) {
    const bool v4 = V.E % 4 == 0 && V.n % 4 == 0; const unsigned vec = v4 ? 4 : 1;
    const unsigned bx = (V.E / vec + 255) / 256, rows_blocks = V.eval_mode ? 0 : bx * V.n, x_blocks = (unsigned)(((size_t)V.n / vec * V.E + 255) / 256);
    const int tw = (tree && !V.eval_mode) ? 1 : 0; ReplayMeta R; memset(&R, 0, sizeof R); if (tw) R = *tree;
    if (grouped && !v4) grouped = 0;      // (callers only group when n % 4 == 0; the four-byte path reads record 0)
    const dim3 g(rows_blocks + x_blocks + tw), b(256);
    if (rows_u8) { if (v4) hipLaunchKernelGGL((k_env_observe2<unsigned char, 4>), g, b, 0, st, V, rs, (unsigned char*)s_rows, (unsigned char*)sp_rows, cap, x, bx, rows_blocks, grouped, tw, R);
                   else hipLaunchKernelGGL((k_env_observe2<unsigned char, 1>), g, b, 0, st, V, rs, (unsigned char*)s_rows, (unsigned char*)sp_rows, cap, x, bx, rows_blocks, grouped, tw, R); }
    else { if (v4) hipLaunchKernelGGL((k_env_observe2<float, 4>), g, b, 0, st, V, rs, (float*)s_rows, (float*)sp_rows, cap, x, bx, rows_blocks, grouped, tw, R);
           else hipLaunchKernelGGL((k_env_observe2<float, 1>), g, b, 0, st, V, rs, (float*)s_rows, (float*)sp_rows, cap, x, bx, rows_blocks, grouped, tw, R); }
}

// apply pending resets (end of a rollout call) or reset everything (dqn_envs_reset)
__global__ void k_env_reset_pending(EnvDev V, const RolloutDev* rs, int force_all) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V.n) return;
    if (!force_all && !V.pending[i]) return;
    if (!force_all) { V.fin_eps[i] += 1; V.fin_reward[i] += (double)V.ep_reward[i]; } else V.dones[i] = 0;     // dones[] keeps the flags of the last act! (inspection)
    V.ep_reward[i] = 0.0f; V.ep_step[i] = 0; V.pending[i] = 0;
    store_reset(V, i, force_all ? 0ull : (unsigned long long)rs->t);
}
void launch_env_reset_pending(hipStream_t st, const EnvDev& V, const RolloutDev* rs, int force_all) {
    hipLaunchKernelGGL(k_env_reset_pending, dim3((V.n + 255) / 256), dim3(256), 0, st, V, rs, force_all);
}

// ---------------------------------------------------------------- recurrent engines (DRQN): per-copy resetstate!, add_exp! into the episode replay
// One vector step of a recurrent engine is: k_recur_reset  [Gx = Wi*x, cell step, k_state_copy per recurrent layer; the other layers' forwards]  k_env_step_rec
// k_env_observe_rec  k_ep_commit  k_ep_advance -- fixed device pointers throughout, the Recur state lives in ONE buffer set, so the step replays as a hipGraph.

// resetstate!(policy) (src/policy.jl:32-34) for the copies whose episode ended in the previous step (pending: done, or ep_step >= max_episode_length): their state
// columns become state0 of the ONLINE net as it is now (h0 / c0 are trainable); the other copies' columns are untouched
__global__ void k_recur_reset(const unsigned char* __restrict__ pending, int n, RecurState RS) {
    for (int l = 0; l < RS.nrec; l++) {
        const int H = RS.H[l];
        for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < H * n; q += gridDim.x * blockDim.x) {
            const int u = q / n, i = q - u * n;
            if (!pending[i]) continue;
            RS.h[l][q] = RS.h0[l][u];
            if (RS.c[l]) RS.c[l][q] = RS.c0[l][u];
        }
    }
}
void launch_recur_reset(hipStream_t st, const unsigned char* pending, int n, const RecurState& RS) {
    int hmax = 1; for (int l = 0; l < RS.nrec; l++) hmax = RS.H[l] > hmax ? RS.H[l] : hmax;
    unsigned blocks = (unsigned)(((size_t)hmax * n + 255) / 256); if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_recur_reset, dim3(blocks), dim3(256), 0, st, pending, n, RS);
}
// h_t of the cell step (the layer's activation, which every thread of the step read h_{t-1} beside) becomes the carried state
__global__ void k_state_copy(const float* __restrict__ src, float* __restrict__ dst, int m) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < m; q += gridDim.x * blockDim.x) dst[q] = src[q];
}
void launch_state_copy(hipStream_t st, const float* src, float* dst, int m) {
    unsigned blocks = (unsigned)((m + 255) / 256); if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_state_copy, dim3(blocks), dim3(256), 0, st, src, dst, m);
}

// after k_env_step_rec: the transition's rows -- s = observation of the saved pre-step state, sp = observe(env) -- go to staging position open_len[i] - 1 of copy i
// (while it is < trace_length), and the NEXT step's observation (of the reset state if the episode just ended) becomes the policy input x[E][n]
__global__ __launch_bounds__(256) void k_env_observe_rec(EnvDev V, const RolloutDev* __restrict__ rs, EpStage ES, float* __restrict__ x) {
    const size_t tot = (size_t)V.n * V.E, rows = V.eval_mode ? 0 : tot;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < rows + tot; q += (size_t)gridDim.x * blockDim.x) {
        unsigned char b;
        if (q < rows) {
            const int i = (int)(q / V.E), f = (int)(q - (size_t)i * V.E);      // f fastest: coalesced rows
            const int pos = ES.open_len[i] - 1;
            if (pos < 0 || pos >= ES.T) continue;
            uint32_t sw0, sw1; int p0x, p0y, p1x, p1y;
            load_state(V, i, &sw1, &p1x, &p1y);
            load_prev(V, i, &sw0, &p0x, &p0y);
            const size_t dst = ((size_t)i * ES.T + pos) * V.E + f;
            ES.st_s[dst] = obs_elem(V, sw0, p0x, p0y, f, &b);
            ES.st_sp[dst] = obs_elem(V, sw1, p1x, p1y, f, &b);
        } else {
            const size_t p = q - rows; const int f = (int)(p / V.n), i = (int)(p - (size_t)f * V.n);      // i fastest
            uint32_t sw; int px, py, tm = 0; load_state(V, i, &sw, &px, &py);
            if (V.pending[i] && !V.eval_mode) reset_state(V, i, (unsigned long long)rs->t, &sw, &tm, &px, &py);
            x[p] = obs_elem(V, sw, px, py, f, &b);
        }
    }
}
void launch_env_observe_rec(hipStream_t st, const EnvDev& V, const RolloutDev* rs, const EpStage& ES, float* x) {
    const size_t tot = (size_t)V.n * V.E * (V.eval_mode ? 1 : 2); unsigned blocks = (unsigned)((tot + 255) / 256); if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_env_observe_rec, dim3(blocks), dim3(256), 0, st, V, rs, ES, x);
}

// add_episode! (src/episode_replay.jl:54-60) for the copies whose transition of this step was terminal.  Workgroup i = copy i; k = the rank of copy i among this step's
// finishers in ascending copy index, F = their number: the staged prefix goes to ring slot (ep_widx + k) % ep_cap with the episode's TRUE length.  (More finishers than
// slots: only the last ep_cap of them are written, as if committed one after the other.)  The cursor is read here and advanced by k_ep_advance, the next launch.
__global__ __launch_bounds__(256) void k_ep_commit(EnvDev V, EpStage ES) {
    const int i = blockIdx.x, n = V.n;
    if (!V.dones[i]) return;                                    // uniform per workgroup
    __shared__ int cnt[2];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    int before = 0, all = 0;
    for (int j = threadIdx.x; j < n; j += blockDim.x) if (V.dones[j]) { all++; if (j < i) before++; }
    if (before) atomicAdd(&cnt[0], before);
    if (all) atomicAdd(&cnt[1], all);
    __syncthreads();
    const int k = cnt[0], F = cnt[1];
    if ((long long)(F - k) > ES.ep_cap) return;                 // a later finisher of this step takes the slot
    const long long slot = ((long long)ES.cur[0] + k) % ES.ep_cap;
    const int len = ES.open_len[i], m = len < ES.T ? len : ES.T;
    const size_t src = (size_t)i * ES.T, dst = (size_t)slot * ES.T, ne = (size_t)m * V.E;
    for (size_t q = threadIdx.x; q < ne; q += blockDim.x) { ES.ep_s[dst * V.E + q] = ES.st_s[src * V.E + q]; ES.ep_sp[dst * V.E + q] = ES.st_sp[src * V.E + q]; }
    for (int q = threadIdx.x; q < m; q += blockDim.x) { ES.ep_a[dst + q] = ES.st_a[src + q]; ES.ep_r[dst + q] = ES.st_r[src + q]; ES.ep_done[dst + q] = ES.st_done[src + q]; }
    if (threadIdx.x == 0) ES.ep_len[slot] = len;
}
// one workgroup: the finishers' open episodes are empty again; cursor and count advance by the number of finishers
__global__ __launch_bounds__(1024) void k_ep_advance(EnvDev V, EpStage ES) {
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < V.n; i += blockDim.x) if (V.dones[i]) { ES.open_len[i] = 0; mine++; }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0 && cnt) {
        ES.cur[0] = (int)(((long long)ES.cur[0] + cnt) % ES.ep_cap);
        const long long s = (long long)ES.cur[1] + cnt; ES.cur[1] = (int)(s > ES.ep_cap ? ES.ep_cap : s);
    }
}
void launch_ep_commit(hipStream_t st, const EnvDev& V, const EpStage& ES) {
    hipLaunchKernelGGL(k_ep_commit, dim3(V.n), dim3(256), 0, st, V, ES);
    hipLaunchKernelGGL(k_ep_advance, dim3(1), dim3(1024), 0, st, V, ES);
}
