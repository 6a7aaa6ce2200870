// env_body.h -- the device side of one vector step of the environment loop, shared by the kernels of envs.hip (the acting program of a standalone engine) and
// tiny_act.hip (the single-workgroup acting step of an engine group): the Philox draws, the observation and reset laws of the environment kinds, the sum-tree
// rebuild of add_exp! and env_step_body, the whole tail of a vector step as ONE workgroup.  The environment laws are stated here and nowhere else.
#pragma once
#include "common.h"

#define ENV_HEAD_LDS 8192      // floats of head outputs staged in LDS by k_env_step (32 KB)

__device__ __forceinline__ uint32_t env_rand(unsigned long long seed, unsigned long long t, int env, uint32_t purpose) {
    uint32_t c[4] = {(uint32_t)t, (uint32_t)(t >> 32), (uint32_t)env, purpose};
    philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), c);
    return c[0];
}
__device__ __forceinline__ float u01(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }

// tabular (PO)MDP draws (the law: include/dqn_mi355x.h).  cdf = one cumulative row of n non-decreasing fp32 values, u in [0, 1): the first j with u < cdf[j]; if
// the row's fp32 sum lies at or below u, the last j at which the row still rose (= the first j with cdf[j] >= cdf[n - 1]; an all-zero row gives 0).  Either is the
// first index at which a monotone predicate holds, and it holds at n - 1: ONE branch-free lower bound of at most 10 dependent loads for n <= 1024, whose trip
// count depends on n alone (uniform across the lanes); the result always lies in [0, n - 1]
__device__ __forceinline__ int cdf_pick(const float* __restrict__ cdf, int n, float u) {
    const float top = cdf[n - 1];
    const bool fb = !(u < top);
    int base = 0;
    for (int len = n; len > 1;) {
        const int half = len >> 1;
        const float v = cdf[base + half - 1];
        const bool ok = fb ? v >= top : u < v;
        base = ok ? base : base + half; len -= half;
    }
    return base;
}
// SoftmaxPolicy (the law: include/dqn_mi355x.h; POMDPTools' SoftmaxPolicy.action, third-party, recalled): q(k) = the copy's Q value of action k, recomputed per pass
// (the same operations on the same operands: the same bits) instead of kept in a per-lane array.  z_k = q_k / tau, m = max z, w_k = expf(z_k - m), c_k = c_{k-1} + w_k
// ascending, target = u * c_{nA-1}: the first k with target < c_k, else the last k at which c still rose -- cdf_pick's rule on a cumulative row that is never stored.
// The trip counts depend on nA alone (uniform across the lanes); the result always lies in [0, nA - 1]
template <class QF>
__device__ __forceinline__ int softmax_pick(QF q, int nA, float tau, float u) {
    float m = q(0) / tau;
    for (int k = 1; k < nA; k++) { const float z = q(k) / tau; m = z > m ? z : m; }
    float tot = 0.0f;
    for (int k = 0; k < nA; k++) tot = tot + expf(q(k) / tau - m);
    const float target = u * tot;
    float c = 0.0f; int first = -1, rose = 0;
    for (int k = 0; k < nA; k++) {
        const float cn = c + expf(q(k) / tau - m);
        if (cn > c) rose = k;
        if (first < 0 && target < cn) first = k;
        c = cn;
    }
    return first >= 0 ? first : rose;
}
enum { TAB_NEXT = DQN_ENV_RAND_TAB_NEXT, TAB_OBS = DQN_ENV_RAND_TAB_OBS, TAB_INIT = DQN_ENV_RAND_TAB_INIT, TAB_INIT_OBS = DQN_ENV_RAND_TAB_INIT_OBS };

// control kinds (the laws: include/dqn_mi355x.h; POMDPModels' MountainCar and InvertedPendulum, third-party, recalled).  Plain double arithmetic in the written order:
// no contraction (the pragma; the build's -ffp-contract=off says the same), the device library's double cos / sin.  c = the spec's constants (CT_*, common.h)
__device__ __forceinline__ void control_reset(const EnvDev& V, int i, unsigned long long t, double* s0, double* s1) {
#pragma clang fp contract(off)
    const double* __restrict__ c = V.ct_c;
    if (V.kind == DQN_ENV_MOUNTAINCAR) { *s0 = c[CT_X0]; *s1 = c[CT_V0]; return; }
    const double u13 = (double)u01(env_rand(V.seed, t, i, DQN_ENV_RAND_PEND_THETA0)), u14 = (double)u01(env_rand(V.seed, t, i, DQN_ENV_RAND_PEND_OMEGA0));
    *s0 = (u13 - 0.5) * 2.0 * c[CT_INITHALF]; *s1 = (u14 - 0.5) * 2.0 * c[CT_INITHALF];
}
// one step of copy i under action index a at vector step t: the state in place, the reward (still Float64) and the terminal flag
__device__ __forceinline__ void control_step(const EnvDev& V, int i, unsigned long long t, int a, double* s0, double* s1, double* r, unsigned char* done) {
#pragma clang fp contract(off)
    const double* __restrict__ c = V.ct_c;
    const double push = (double)(a - 1);
    if (V.kind == DQN_ENV_MOUNTAINCAR) {
        const double x = *s0, v = *s1, vmax = c[CT_VMAX];
        double vp = v + push * c[CT_FORCE] + cos(c[CT_FREQ] * x) * (-c[CT_GRAVITY]);
        vp = fmax(fmin(vmax, vp), -vmax);
        double xp = x + vp;
        if (xp < c[CT_XMIN]) { xp = c[CT_XMIN]; vp = 0.0; }
        const bool goal = xp >= c[CT_GOAL];
        *s0 = xp; *s1 = vp; *r = c[CT_COST] + (goal ? c[CT_JACKPOT] : 0.0); *done = goal ? 1 : 0;
        return;
    }
    const double th = *s0, om = *s1, g = c[CT_G], m = c[CT_M], l = c[CT_L], al = c[CT_ALPHA], dt = c[CT_DT];
    const double u = push * c[CT_UMAX] + c[CT_NOISE] * ((double)u01(env_rand(V.seed, t, i, DQN_ENV_RAND_PEND_NOISE)) - 0.5);
    const double sn = sin(th), cs = cos(th), s2 = sin(2.0 * th);
    const double acc = (g * sn - al * m * l * om * om * s2 * 0.5 - al * cs * u) / ((4.0 / 3.0) * l - al * m * l * cs * cs);
    const double thp = th + om * dt, omp = om + acc * dt;
    const bool fell = fabs(thp) > c[CT_THETAMAX];
    *s0 = thp; *s1 = omp; *r = fell ? c[CT_COST] : 0.0; *done = fell ? 1 : 0;
}

// element f of the observation of an env in state (sw = the 4 TestMDP state bytes packed little-endian | px, py; tabular: px = the observation index; control: px, py =
// the bits of Float32(state[1]), Float32(state[2]) -- convert_s is all an observation needs of the Float64 state).  No local arrays: a dynamically indexed one would
// live in scratch.
// CTL (here and in the three helpers below): false compiles the control kinds' branch out -- for a caller that a control set can never reach (k_env_observe2's 16-byte
// instantiations: E = 2), so that its code stays what it was
template <bool CTL = true>
__device__ __forceinline__ float obs_elem(const EnvDev& V, uint32_t sw, int px_, int py_, int f, unsigned char* raw) {
    if (V.kind == DQN_ENV_TESTMDP) {
        const int hw = V.H * V.W, c = f / hw, px = f - c * hw;            // obs[.., c] = observations[s[end - c]]  (test/test_env.jl:56-58)
        const int sel = (int)((sw >> (8 * (3 - c))) & 0xffu) - 1;
        const unsigned char b = V.images[sel * hw + px];
        *raw = b; return (float)b / 255.0f;
    }
    if (V.kind == DQN_ENV_TABULAR) { *raw = 0; return V.tb_feat[(size_t)px_ * V.E + f]; }      // convert_o / convert_s row of the index
    if (CTL && env_is_control(V.kind)) { *raw = 0; return __int_as_float(f == 0 ? px_ : py_); }       // Float32[state[1], state[2]]
    *raw = 0; return (float)(f == 0 ? px_ : py_);                          // Float32[x, y]
}
template <bool CTL = true>
__device__ __forceinline__ void reset_state(const EnvDev& V, int i, unsigned long long t, uint32_t* sw, int* tm_t, int* px, int* py) {
    if (V.kind == DQN_ENV_TESTMDP) { *sw = 0x01010101u; *tm_t = 1; }                                                  // initialstate, :46-52
    else if (V.kind == DQN_ENV_TABULAR) {      // s ~ b0, o ~ Z0[s] (an MDP: o = s); py = state, px = observation index
        const int s = cdf_pick(V.tb_b0, V.tb_S, u01(env_rand(V.seed, t, i, TAB_INIT)));
        *py = s; *px = V.tb_O ? cdf_pick(V.tb_Z0 + (size_t)s * V.tb_O, V.tb_O, u01(env_rand(V.seed, t, i, TAB_INIT_OBS))) : s;
    }
    else if (CTL && env_is_control(V.kind)) { double s0, s1; control_reset(V, i, t, &s0, &s1); *px = __float_as_int((float)s0); *py = __float_as_int((float)s1); }
    else { *px = 1 + (int)(env_rand(V.seed, t, i, 5u) % (uint32_t)V.size_x); *py = 1 + (int)(env_rand(V.seed, t, i, 6u) % (uint32_t)V.size_y); }
}
template <bool CTL = true>
__device__ __forceinline__ void load_state(const EnvDev& V, int i, uint32_t* sw, int* px, int* py) {
    *sw = 0x01010101u; *px = *py = 0;
    if (V.kind == DQN_ENV_TESTMDP) *sw = *(const uint32_t*)(V.tm_s + i * 4);
    else if (V.kind == DQN_ENV_TABULAR) { *px = V.tb_o[i]; *py = V.tb_s[i]; }
    else if (CTL && env_is_control(V.kind)) { *px = __float_as_int((float)V.ct_s[i * 2]); *py = __float_as_int((float)V.ct_s[i * 2 + 1]); }
    else { *px = V.gw_pos[i * 2]; *py = V.gw_pos[i * 2 + 1]; }
}
// the state the last k_env_step saved before it stepped: what the transition's s is the observation of
template <bool CTL = true>
__device__ __forceinline__ void load_prev(const EnvDev& V, int i, uint32_t* sw, int* px, int* py) {
    *sw = 0x01010101u; *px = *py = 0;
    if (V.kind == DQN_ENV_TESTMDP) *sw = *(const uint32_t*)(V.tm_prev + i * 4);
    else if (V.kind == DQN_ENV_TABULAR) *px = V.tb_oprev[i];
    else if (CTL && env_is_control(V.kind)) { *px = __float_as_int((float)V.ct_prev[i * 2]); *py = __float_as_int((float)V.ct_prev[i * 2 + 1]); }
    else { *px = V.gw_prev[i * 2]; *py = V.gw_prev[i * 2 + 1]; }
}
__device__ __forceinline__ void store_reset(const EnvDev& V, int i, unsigned long long t) {
    if (env_is_control(V.kind)) { double s0, s1; control_reset(V, i, t, &s0, &s1); V.ct_s[i * 2] = s0; V.ct_s[i * 2 + 1] = s1; return; }      // the Float64 state itself
    uint32_t sw; int tm = 1, px, py; reset_state(V, i, t, &sw, &tm, &px, &py);
    if (V.kind == DQN_ENV_TESTMDP) { *(uint32_t*)(V.tm_s + i * 4) = sw; V.tm_t[i] = tm; }
    else if (V.kind == DQN_ENV_TABULAR) { V.tb_s[i] = py; V.tb_o[i] = px; }
    else { V.gw_pos[i * 2] = px; V.gw_pos[i * 2 + 1] = py; }
}

// add_exp!'s tree part for n new leaves at ring positions start .. start + n - 1 (already stored): their sum-tree ancestors, replay size, pre_valid.  One workgroup;
// lvl[0][i] = leaf i's new priority (non-wrapping range), published by a barrier before the call.  Runs at the end of k_env_step, or -- with k_act_head doing the
// per-copy work -- as workgroup 0 of the observe launch.
__device__ __forceinline__ void env_tree_rebuild(const ReplayMeta& R, const int n, const long long start, float (*lvl)[1024], float (*rim)[2]) {
    const long long s0 = start % R.cap, e0 = (start + n - 1) % R.cap;
    const bool wrap = n >= R.cap || e0 < s0;
    if (!wrap) {
        // the n new leaves are one contiguous range: rebuild their ancestors out of LDS.  Only the two children at the rim of
        // each level's dirty range come from the (unchanged) tree; all of those are fetched up front in one round of loads.
        int nlev = 0; for (long long w = R.cap2; w > 1; w >>= 1) nlev++;
        if ((int)threadIdx.x < 2 * nlev) {
            const int d = threadIdx.x >> 1, right = threadIdx.x & 1;
            const long long lo = s0 >> d, hi = e0 >> d, width = R.cap2 >> d;
            float v = 0.0f;
            if (!right && (lo & 1)) v = R.tree[width + lo - 1];
            if (right && !(hi & 1)) v = R.tree[width + hi + 1];
            rim[d][right] = v;
        }
        __syncthreads();
        long long lo = s0, hi = e0, width = R.cap2; int cur = 0, d = 0;
        for (; d < nlev && hi - lo >= 2; d++) {
            const long long plo = lo >> 1, phi = hi >> 1;
            for (long long pp = plo + threadIdx.x; pp <= phi; pp += blockDim.x) {
                const long long c0 = 2 * pp, c1 = 2 * pp + 1;
                const float l = c0 < lo ? rim[d][0] : lvl[cur][c0 - lo];
                const float r = c1 > hi ? rim[d][1] : lvl[cur][c1 - lo];
                const float sum = l + r;
                lvl[cur ^ 1][pp - plo] = sum; R.tree[(width >> 1) + pp] = sum;
            }
            __syncthreads();
            lo = plo; hi = phi; width >>= 1; cur ^= 1;
        }
        if (threadIdx.x == 0) {
            // the dirty range is down to <= 2 nodes: the rest of the path to the root is a serial chain, walked without barriers
            float v0 = lvl[cur][0], v1 = hi > lo ? lvl[cur][1] : 0.0f;
            for (; d < nlev; d++) {
                const long long plo = lo >> 1, phi = hi >> 1;
                float n0, n1 = 0.0f;
                if (hi == lo) n0 = (lo & 1) ? rim[d][0] + v0 : v0 + rim[d][1];
                else if (plo == phi) n0 = v0 + v1;
                else { n0 = rim[d][0] + v0; n1 = v1 + rim[d][1]; }
                R.tree[(width >> 1) + plo] = n0; if (phi > plo) R.tree[(width >> 1) + phi] = n1;
                v0 = n0; v1 = n1; lo = plo; hi = phi; width >>= 1;
            }
        }
    } else {
        __syncthreads();
        long long lo[2], hi[2]; int nr = 1;
        if (n >= R.cap) { lo[0] = 0; hi[0] = R.cap - 1; }
        else { lo[0] = s0; hi[0] = R.cap - 1; lo[1] = 0; hi[1] = e0; nr = 2; }
        for (long long width = R.cap2; width > 1; width >>= 1) {
            for (int q = 0; q < nr; q++) {
                const long long a0 = (width + lo[q]) >> 1, a1 = (width + hi[q]) >> 1;
                for (long long node = a0 + threadIdx.x; node <= a1; node += blockDim.x) R.tree[node] = R.tree[2 * node] + R.tree[2 * node + 1];
                lo[q] >>= 1; hi[q] >>= 1;
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) { long long s = R.state->size + n; R.state->size = s > R.cap ? R.cap : s; R.state->pre_valid = 0; }     // the tree changed: pre-drawn indices are stale
}

// ONE workgroup, thread i = env i (n <= 1024):
//   tick the step counter and the ring cursor; apply the reset the previous step left pending (src/solver.jl:99-132);
//   Q column of the env's observation from the head outputs (split-K slabs reduced on the fly; dueling (v + a) - mean(a),
//   src/dueling.jl:13-16) and its first-max argmax = action(policy, obs) (src/policy.jl:38-64);
//   eps-greedy (POMDPTools EpsGreedyPolicy: rand(rng) < eps ? rand(rng, actions) : greedy), act! (:89): transition, reward, terminal;
//   add_exp!(replay, exp, abs(exp.r)) (:91-94): metadata + leaf priority, then the sum-tree ancestors of the written leaves.
// REC (recurrent engines, envs_drqn below): add_exp! goes to the copy's open-episode staging area instead of the prioritized ring -- no ring row, no leaf, no tree
// CTL: the instantiation that steps the control kinds.  Their law (double cos / sin: registers, and scratch for the argument reduction) is compiled into it alone, so the
// kernels that step the other kinds keep the code they had; a launcher picks CTL = true where a set (any member of a group launch) is of a control kind
template <bool REC, bool CTL>
__device__ __forceinline__ void env_step_body(const EnvDev& V, RolloutDev* rs, const ActHeads& Hd, const ReplayMeta& R, const EpStage* ES) {
    const int n = V.n;
    const unsigned long long t_prev = (unsigned long long)rs->t, t = t_prev + 1;
    const long long start = REC ? 0 : (rs->widx + n) % R.cap;
    float eps = rs->eps_start - (float)t * ((rs->eps_start - rs->eps_stop) / rs->eps_steps);     // LinearDecaySchedule, fp32
    if (!(rs->eps_steps > 0.0f) || eps < rs->eps_stop) eps = rs->eps_stop;
    // a table of per-step values (dqn_rollout_explore) replaces the linear law: eps itself, or the softmax temperature.  Uniform: every thread reads the same record
    const float* const xtab = rs->xtab; const bool softmax = xtab && rs->xkind == DQN_EXPLORE_SOFTMAX; float tau = 1.0f;
    if (xtab) {
        long long j = (long long)t - rs->xtab_t0; j = j < 0 ? 0 : j; j = j >= rs->xtab_n ? rs->xtab_n - 1 : j;
        const float xv = xtab[j];
        if (softmax) tau = xv; else eps = xv;
    }
    // head outputs of the acting forward -> LDS in one round of independent loads (split-K slabs included); the per-env
    // reduction below then adds them in canonical (ascending-slab) order out of LDS
    __shared__ float hl[ENV_HEAD_LDS];
    __shared__ float hbias[DQN_MAX_ACTIONS + 1];
    __shared__ float lvl[2][1024]; __shared__ float rim[48][2];      // sum-tree rebuild: dirty values of the current/next level, rim children per level
    for (int k = threadIdx.x; k <= V.nA; k += blockDim.x) hbias[k] = k < V.nA ? (Hd.adv.S > 1 ? Hd.adv.bias[k] : 0.0f) : (Hd.dueling && Hd.val.S > 1 ? Hd.val.bias[0] : 0.0f);
    const int Sa = Hd.adv.S < 1 ? 1 : Hd.adv.S, Sv = Hd.dueling ? (Hd.val.S < 1 ? 1 : Hd.val.S) : 0;
    const int per_col = Sa * V.nA + Sv;                     // floats per env: [a][slab] then [slab] of the value head
    const bool in_lds = (long long)per_col * n <= ENV_HEAD_LDS;
    if (in_lds) {
        // 4 independent loads in flight per thread (a runtime-trip-count loop would serialise the round trips)
        const int tot = per_col * n;
        for (int q0 = threadIdx.x; q0 < tot; q0 += 4 * blockDim.x) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int q = q0 + u * blockDim.x; v[u] = 0.0f;
                if (q < tot) {
                    const int i = q % n, k = q / n;             // consecutive lanes = consecutive columns: coalesced
                    if (k < Sa * V.nA) { const int a = k / Sa, sl = k - a * Sa; v[u] = Hd.adv.p[(size_t)sl * Hd.adv.per_s + (size_t)a * Hd.adv.ld + i]; }
                    else { const int sl = k - Sa * V.nA; v[u] = Hd.val.p[(size_t)sl * Hd.val.per_s + i]; }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) { const int q = q0 + u * blockDim.x; if (q < tot) hl[q] = v[u]; }
        }
    }
    __syncthreads();
    if (in_lds) {
        // one thread per (head value, env): canonical ascending-slab sum (+ bias, activation) out of LDS, 8 reads in flight;
        // the result replaces the value's slab-0 slot, which no other thread reads
        for (int q = threadIdx.x; q < (V.nA + (Hd.dueling ? 1 : 0)) * n; q += blockDim.x) {
            const int k = q / n, i = q - k * n;
            const bool isval = k == V.nA; const int S = isval ? Sv : Sa; const int base = (isval ? Sa * V.nA : k * Sa) * n + i;
            float tot = hl[base]; int sl = 1;
            for (; sl + 8 <= S; sl += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = hl[base + (sl + u) * n];
#pragma unroll
                for (int u = 0; u < 8; u++) tot = tot + v[u];
            }
            for (; sl < S; sl++) tot = tot + hl[base + sl * n];
            const HeadSrc& h = isval ? Hd.val : Hd.adv;
            hl[base] = h.S > 1 ? act_f(tot + hbias[k], h.act) : tot;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { rs->t = (long long)t; rs->widx = start; }
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        if (V.eval_mode && V.pending[i]) continue;              // evaluation: one episode per copy, finished copies idle
        if (V.pending[i]) {
            V.fin_eps[i] += 1; V.fin_reward[i] += (double)V.ep_reward[i]; V.ep_reward[i] = 0.0f; V.ep_step[i] = 0; V.pending[i] = 0;
            store_reset(V, i, t_prev);
        }
        if (V.kind == DQN_ENV_TESTMDP) *(uint32_t*)(V.tm_prev + i * 4) = *(const uint32_t*)(V.tm_s + i * 4);       // s of this transition = observation of the pre-step state
        else if (V.kind == DQN_ENV_TABULAR) V.tb_oprev[i] = V.tb_o[i];
        else if (env_is_control(V.kind)) { V.ct_prev[i * 2] = V.ct_s[i * 2]; V.ct_prev[i * 2 + 1] = V.ct_s[i * 2 + 1]; }
        else { V.gw_prev[i * 2] = V.gw_pos[i * 2]; V.gw_prev[i * 2 + 1] = V.gw_pos[i * 2 + 1]; }
        int a = 0;
        float v = 0.0f, mean = 0.0f;
        // Q column without per-lane arrays (they would live in scratch): advantages are re-read for the second pass
        auto adv_k = [&](int k) -> float {
            return in_lds ? hl[(k * Sa) * n + i] : head_val(Hd.adv, k, i);
        };
        {
            if (Hd.dueling) {
                v = in_lds ? hl[(Sa * V.nA) * n + i] : head_val(Hd.val, 0, i);
                float sum = adv_k(0);
                for (int k = 1; k < V.nA; k++) sum = sum + adv_k(k);
                mean = sum / (float)V.nA;
            }
            float qbest = 0.0f;
            for (int k = 0; k < V.nA; k++) {
                const float ak = adv_k(k), qk = Hd.dueling ? (v + ak) - mean : ak;
                Hd.q_out[(size_t)i * V.nA + k] = qk;
                if (k == 0 || qk > qbest) { qbest = qk; a = k; }
            }
            Hd.amax[i] = a;
        }
        if (softmax) a = softmax_pick([&](int k) -> float { const float ak = adv_k(k); return Hd.dueling ? (v + ak) - mean : ak; }, V.nA, tau, u01(env_rand(V.seed, t, i, DQN_ENV_RAND_SOFTMAX)));
        else if (u01(env_rand(V.seed, t, i, 1u)) < eps) a = (int)(env_rand(V.seed, t, i, 2u) % (uint32_t)V.nA);
        float r; unsigned char done;
        if (V.kind == DQN_ENV_TESTMDP) {
            signed char* s = V.tm_s + i * 4;
            const bool was_second = s[3] == 2;                                // was_in_second(s), :62-64
            const signed char s0 = s[1], s1 = s[2], s2 = s[3];               // circshift(s, -1)
            const signed char last = a < 3 ? (signed char)(a + 1) : s2;       // a < 4 ? a : s_new[end-1]  (1-based), :69-74
            s[0] = s0; s[1] = s1; s[2] = s2; s[3] = last;
            r = (last == 1 ? -0.1f : (last == 2 ? 0.0f : 0.1f));
            if (was_second) r = r * -10.0f;                                   // :77-83
            V.tm_t[i] += 1; done = V.tm_t[i] >= V.max_time;                   // isterminal: t >= max_time, :85-87
        } else if (V.kind == DQN_ENV_TABULAR) {      // sp ~ T[s][a], o ~ Z[a][sp] (an MDP: o = sp), r = R[s][a][sp], done = terminal[sp]
            const int s = V.tb_s[i];
            const size_t row = ((size_t)s * V.nA + a) * V.tb_S;
            const int sp = cdf_pick(V.tb_T + row, V.tb_S, u01(env_rand(V.seed, t, i, TAB_NEXT)));
            const int o = V.tb_O ? cdf_pick(V.tb_Z + ((size_t)a * V.tb_S + sp) * V.tb_O, V.tb_O, u01(env_rand(V.seed, t, i, TAB_OBS))) : sp;
            r = V.tb_R[row + sp]; done = V.tb_term[sp];
            V.tb_s[i] = sp; V.tb_o[i] = o;
        } else if (env_is_control(V.kind)) {
            if constexpr (!CTL) { r = 0.0f; done = 0; if (!REC && !V.eval_mode) R.state->err = 1; }      // (never launched on these kinds; if a launcher ever forgets the flag the copy stands still and, where the step has an assertion flag, the call fails)
            else {
            double s0 = V.ct_s[i * 2], s1 = V.ct_s[i * 2 + 1], rd;
            control_step(V, i, t, a, &s0, &s1, &rd, &done);
            V.ct_s[i * 2] = s0; V.ct_s[i * 2 + 1] = s1; r = (float)rd;                              // the replay holds Float32(r)
            }
        } else {
            int* p = V.gw_pos + i * 2; float rv = 0.0f;
            for (int k = 0; k < V.n_reward; k++) if (p[0] == V.reward_xy[k][0] && p[1] == V.reward_xy[k][1]) rv = V.reward_val[k];
            const bool at_reward = rv != 0.0f;
            const bool intended = u01(env_rand(V.seed, t, i, 3u)) < V.tprob;
            const int other = (int)(env_rand(V.seed, t, i, 4u) % 3u);
            const int eff = intended ? a : (a + 1 + other) % 4;
            const int dx = eff == 2 ? -1 : (eff == 3 ? 1 : 0), dy = eff == 0 ? 1 : (eff == 1 ? -1 : 0);
            const int nx = p[0] + dx, ny = p[1] + dy;
            if (!at_reward && nx >= 1 && nx <= V.size_x && ny >= 1 && ny <= V.size_y) { p[0] = nx; p[1] = ny; }
            r = rv; done = at_reward;
        }
        V.actions[i] = a; V.rewards[i] = r; V.dones[i] = done; V.ep_reward[i] += r; V.ep_step[i] += 1;
        if (V.eval_mode) {      // basic_evaluation: r_tot += rew in Float64; while !done && step <= max_episode_length (src/evaluation_policy.jl:27-34)
            V.fin_reward[i] += (double)r; V.pending[i] = (done || V.ep_step[i] > V.max_episode_length) ? 1 : 0; continue;
        }
        V.pending[i] = (done || V.ep_step[i] >= V.max_episode_length) ? 1 : 0;
        if (REC) {      // push!(r._episode, exp) (src/episode_replay.jl:46-52): only the first trace_length transitions can ever be sampled (:82-92); the length counts on
            const int pos = ES->open_len[i];
            if (pos < ES->T) { const size_t q = (size_t)i * ES->T + pos; ES->st_a[q] = a; ES->st_r[q] = r; ES->st_done[q] = done ? 1 : 0; }
            ES->open_len[i] = pos + 1;
            continue;
        }
        const long long slot = (start + i) % R.cap;
        R.a[slot] = a; R.r[slot] = r; R.done[slot] = done ? 1 : 0;
        const float td = V.prioritized ? fabsf(r) : 0.0f;                     // add_exp!(replay, exp, abs(exp.r)) / 0f0, src/solver.jl:91-94
        if (!(td + R.eps > 0.0f)) R.state->err = 1;
        const float pr = prio_f(td, R.eps, R.alpha);
        R.tree[R.cap2 + slot] = pr; lvl[0][i] = pr;
    }
    if (V.eval_mode || REC) return;                             // no add_exp! into the ring (uniform branch: eval_mode is a kernel argument)
    env_tree_rebuild(R, n, start, lvl, rim);
}
