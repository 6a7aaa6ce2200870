// engine_group.hip -- dqn_group_*: K engines whose whole train step is one single-workgroup launch (tiny_step.hip) stepped by ONE launch of K workgroups.
// A group owns a device array of its members' TinyArgs records (copies of the host record each engine keeps, dqn_engine::tiny_args), a stream and the events that
// order that stream against the members' streams.  Everything a step reads or writes is the member's own (parameters, Adam state, sum-tree, replay rows, StepState,
// the step workspaces): the group adds no state of its own to a member, so after a group call a member cannot tell it from dqn_train_steps.
#include "engine.h"

struct GroupScalars { float loss, gnorm; int err, pad; unsigned long long step; };      // what the standalone step's publish launch reports (StepMail), per member
// ... and what dqn_rollout_explore fetches per engine at the end of a call: the episode statistics of the env set beside the step's scalars
struct RolloutScalars { float loss, gnorm; int err, pad; unsigned long long step; long long episodes; double reward_sum; };

struct dqn_group {
    int device = 0, K = 0; unsigned max_lds = 0;
    std::vector<dqn_engine*> members;
    TinyArgs* args_dev = nullptr;
    hipStream_t stream = nullptr; std::vector<hipEvent_t> ev_in; hipEvent_t ev_done = nullptr;
    GroupScalars *out_dev = nullptr, *out_host = nullptr;      // out_host: pinned
    bool counted = false;      // the members' in_groups counts include this group
    // dqn_rollout_many: the members' acting records (host copy = what the device array holds; rebuilt per call, uploaded when they changed), the call's RolloutDev
    // records and exploration tables (ONE device array and ONE H2D copy each), the per-member results of a call
    std::vector<TinyActArgs> act_host; TinyActArgs* act_dev = nullptr; unsigned act_lds = 0;
    std::vector<RolloutDev> roll_host; RolloutDev* roll_dev = nullptr;
    std::vector<float> xtab_host; float* xtab_dev = nullptr; size_t xtab_cap = 0;
    struct RolloutScalars *ro_dev = nullptr, *ro_host = nullptr;      // ro_host: pinned
    // dqn_evaluate_many: the members' evaluation records (rebuilt and uploaded per call: ONE H2D copy), the head outputs of every member's copies (ONE device array),
    // the per-member sums of a call
    std::vector<TinyEvalArgs> eval_host; TinyEvalArgs* eval_dev = nullptr;
    float* heads_dev = nullptr; size_t heads_cap = 0;
    EvalSums *es_dev = nullptr, *es_host = nullptr;      // es_host: pinned
    DevScope mem;      // owns every device and pinned block above (devmem.h)
};

// per member, what k_publish_scalars does for a standalone engine after the last step of a call: globalnorm = the fold of the step's per-block maxima (ONE slot, the
// single-workgroup step's gmax_used), kept in the member's StepState; the device-side assertion flag is CONSUMED (reported once)
__global__ __launch_bounds__(256) void k_group_scalars(const TinyArgs* __restrict__ A, int K, GroupScalars* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    StepState* st = A[k].state;
    const float g = fmaxf(0.0f, A[k].gmax_part[0]);
    st->gnorm_bits = __float_as_uint(g);
    GroupScalars o; o.loss = st->loss; o.gnorm = g; o.err = atomicExch(&st->err, 0); o.pad = 0; o.step = st->step;
    out[k] = o;
}

// THE frame of a group call (dqn_group_train_steps, dqn_rollout_many, dqn_evaluate_many).  In: the group's stream behind everything the members have enqueued
// (replay_add, their own steps, target syncs, rollouts).  body() enqueues on the group's stream and returns 0, or -1 with its refusal.  Out: every member's stream
// behind whatever the group enqueued -- on the error paths too: a later member call must never run beside steps already enqueued, and whatever the member enqueues
// next sees the group's work without a host synchronise.  Then ONE synchronise of the group's stream: the results and the assertion flags of this call
template <class Body> static int group_call(dqn_group* g, const char* who, Body body) {
    for (int k = 0; k < g->K; k++) { HIPCHK(hipEventRecord(g->ev_in[k], g->members[k]->stream)); HIPCHK(hipStreamWaitEvent(g->stream, g->ev_in[k], 0)); }
    (void)hipGetLastError();
    const int rc = body();
    hipError_t he = hipEventRecord(g->ev_done, g->stream);
    for (int k = 0; k < g->K && he == hipSuccess; k++) he = hipStreamWaitEvent(g->members[k]->stream, g->ev_done, 0);
    const hipError_t hs = hipStreamSynchronize(g->stream);
    if (rc) return rc;
    if (he != hipSuccess || hs != hipSuccess) return fail("%s: HIP error %s ordering the members' streams behind the group", who, hipGetErrorString(he != hipSuccess ? he : hs));
    return 0;
}
// the last thing a body enqueues: the D2H copy of the call's per-member results, behind `what` -- whose launch errors surface here
static int group_gather(dqn_group* g, const char* who, const char* what, void* host, const void* dev, size_t bytes) {
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, g->stream);
    return he == hipSuccess ? 0 : fail("%s: HIP error %s behind the group's %s", who, hipGetErrorString(he), what);
}
// ... and what a call reports of its members' consumed assertion flags, over the (err, step) every per-member result carries: the first failing member, and whether others failed
template <class Rec> static int group_members_failed(const Rec* o, int K) {
    int bad = -1, nbad = 0;
    for (int k = 0; k < K; k++) if (o[k].err) { if (bad < 0) bad = k; nbad++; }
    if (bad < 0) return 0;
    const char* more = nbad > 1 ? "; further members failed too, the other members' steps stand" : "; the other members' steps stand";
    if (o[bad].err == 2) return fail("member %d: AssertionError: all(new_priorities .> 0f0) (at or before train step %llu)%s", bad, o[bad].step, more);
    return fail("member %d: device-side error %d at or before train step %llu%s", bad, o[bad].err, o[bad].step, more);
}
// does any member step a control kind: picks the acting / evaluation kernel's instantiation (env_body.h)
static int group_has_control(const dqn_group* g) { int c = 0; for (const dqn_engine* e : g->members) c |= env_is_control(e->env.kind) ? 1 : 0; return c; }

extern "C" int dqn_group_create(dqn_engine_t* const* members, int n_members, dqn_group_t** out) {
    if (!out) return fail("dqn_group_create: out is NULL");
    *out = nullptr;
    if (n_members < 1 || n_members > 4096) return fail("dqn_group_create: n_members = %d is outside 1..4096", n_members);
    if (!members) return fail("dqn_group_create: members is NULL");
    for (int k = 0; k < n_members; k++) {
        dqn_engine* e = members[k];
        if (!e) return fail("dqn_group_create: member %d is a null engine handle", k);
        for (int j = 0; j < k; j++) if (members[j] == e) return fail("dqn_group_create: member %d is the same engine as member %d (a member's step runs once per group step)", k, j);
        if (e->device != members[0]->device) return fail("dqn_group_create: member %d lives on device %d, member 0 on device %d (one launch, one device)", k, e->device, members[0]->device);
        const std::string why = tiny_decline(e);      // the rule build_program decides by (engine_program.hip)
        if (!why.empty()) return fail("dqn_group_create: member %d does not take the single-workgroup step: %s", k, why.c_str());
    }
    HIPCHK(hipSetDevice(members[0]->device));
    for (int k = 0; k < n_members; k++) {
        dqn_engine* e = members[k];
        if (build_program(e)) return -1;
        if (!e->tiny || e->tiny_args.size() != 1) return fail("dqn_group_create: internal error: member %d passed the eligibility rule but its program is not the single-workgroup step", k);
    }
    dqn_group* g = new dqn_group;
    g->device = members[0]->device; g->K = n_members; g->members.assign(members, members + n_members);
    std::vector<TinyArgs> recs((size_t)n_members);
    for (int k = 0; k < n_members; k++) { recs[k] = members[k]->tiny_args[0]; g->max_lds = std::max(g->max_lds, recs[k].lds_bytes); }
    auto bail = [&](const char* what, hipError_t err) { const int rc = fail("dqn_group_create: %s failed: %s", what, hipGetErrorString(err)); dqn_group_destroy(g); return rc; };
    hipError_t err; if (g->mem.get(&g->args_dev, (size_t)n_members) || g->mem.get(&g->out_dev, (size_t)n_members) || g->mem.get_pinned(&g->out_host, (size_t)n_members, hipHostMallocDefault)) { dqn_group_destroy(g); return -1; }      // (the message survives: destroy never calls fail)
    if ((err = hipMemcpy(g->args_dev, recs.data(), sizeof(TinyArgs) * (size_t)n_members, hipMemcpyHostToDevice)) != hipSuccess) return bail("the upload of the members' records", err);
    if ((err = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", err);
    if ((err = hipEventCreateWithFlags(&g->ev_done, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", err);
    g->ev_in.assign((size_t)n_members, nullptr);
    for (int k = 0; k < n_members; k++) if ((err = hipEventCreateWithFlags(&g->ev_in[k], hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", err);
    for (dqn_engine* e : g->members) e->in_groups++;      // (last: a failed create leaves every member free)
    g->counted = true;
    *out = g;
    return 0;
}

extern "C" int dqn_group_destroy(dqn_group_t* g) {
    if (!g) return 0;
    hipSetDevice(g->device);
    if (g->stream) hipStreamSynchronize(g->stream);
    if (g->counted) for (dqn_engine* e : g->members) e->in_groups--;
    for (hipEvent_t ev : g->ev_in) if (ev) hipEventDestroy(ev);
    if (g->ev_done) hipEventDestroy(g->ev_done);
    if (g->stream) hipStreamDestroy(g->stream);
    g->mem.release();
    delete g;
    return 0;
}

extern "C" int dqn_group_info(dqn_group_t* g, dqn_group_info_t* out) {
    if (!g) return fail("null group handle");
    if (!out) return fail("dqn_group_info: out is NULL");
    out->n_members = g->K; out->max_lds_bytes = g->max_lds; out->launches_per_step = 1; out->reserved = 0;
    return 0;
}

extern "C" int dqn_group_train_steps(dqn_group_t* g, int n, float* loss, float* grad_norm) {
    if (!g) return fail("null group handle");
    if (n < 1) return fail("dqn_group_train_steps: n = %d, at least one step is needed", n);
    // (a member's step program cannot change under a live group: dqn_comm_init, the one call that rebuilds it, is refused on a grouped engine)
    for (int k = 0; k < g->K; k++) if (g->members[k]->size < g->members[k]->B) return fail("member %d: AssertionError: r._curr_size >= r.batch_size", k);   // ...replay.jl:83
    HIPCHK(hipSetDevice(g->device));
    static const char who[] = "dqn_group_train_steps";
    if (group_call(g, who, [&]() {
            if (launch_tiny_group(g->stream, g->args_dev, g->K, g->max_lds, n))
                return fail("dqn_group_train_steps: the device refused %u bytes of dynamic LDS for the group launch (hipFuncSetAttribute)", g->max_lds);
            hipLaunchKernelGGL(k_group_scalars, dim3((g->K + 255) / 256), dim3(256), 0, g->stream, g->args_dev, g->K, g->out_dev);
            return group_gather(g, who, "steps", g->out_host, g->out_dev, sizeof(GroupScalars) * (size_t)g->K); })) return -1;
    for (int k = 0; k < g->K; k++) { if (loss) loss[k] = g->out_host[k].loss; if (grad_norm) grad_norm[k] = g->out_host[k].gnorm; }
    return group_members_failed(g->out_host, g->K);
}

// ---------------------------------------------------------------- grouped acting: dqn_rollout_many (tiny_act.hip)
// the dynamic-LDS layout of the single-workgroup acting step, in floats: the online parameters, the policy input x[E][n], then per layer its activations [N][n]
// (every part 16-byte aligned).  a != null: the offsets are recorded
static size_t tiny_act_layout(const dqn_engine* e, TinyActArgs* a) {
    const int n = e->env.n;
    size_t fl = 0; TinyActArgs tmp; TinyActArgs& A = a ? *a : tmp;
    auto take = [&](size_t m) { const int o = (int)fl; fl += (m + 3) / 4 * 4; return o; };
    A.p_off = take(e->Pint); A.x_off = take((size_t)e->E * n);
    for (int i = 0; i < e->nl && i < TINY_MAX_LAYERS; i++) A.y_off[i] = take((size_t)e->L[i].N * n);
    return fl;
}
// THE eligibility rule of the single-workgroup acting step, term by term: empty when the engine takes it, else the reason in words.  A pure function of the engine as
// it stands after dqn_envs_create / dqn_envs_create_tabular
std::string tiny_act_decline(const dqn_engine* e) {
    char buf[200];
    if (!e->has_envs) return "it has no device environments (dqn_envs_create / dqn_envs_create_tabular)";
    if (e->hp.recurrence) return "it is recurrent (recurrence = true)";
    for (int i = 0; i < e->nl; i++) if (e->L[i].kind != DQN_LAYER_DENSE) { snprintf(buf, sizeof buf, "layer %d is not a Dense layer (kind %d)", i, e->L[i].kind); return buf; }
    const int nlev = (int)net_levels(e).size();
    if (e->nl > TINY_MAX_LAYERS || nlev > TINY_MAX_LAYERS) { snprintf(buf, sizeof buf, "it has too many layers (%d in %d levels, at most %d)", e->nl, nlev, TINY_MAX_LAYERS); return buf; }
    // the one-CU arithmetic budget of the train step (tiny_decline), with the copies in the place of the batch columns; what the kernel costs at the bound: docs/history/group_rollout.md
    if (e->Pint > 16384 || (size_t)e->Pint * e->env.n > 262144) { snprintf(buf, sizeof buf, "it has too many parameters for %d copies (%zu, at most 16384 and 262144 / n_envs)", e->env.n, e->Pint); return buf; }
    const size_t bytes = tiny_act_layout(e, nullptr) * 4 + TINY_ACT_TAIL_LDS;
    if (bytes > 144 * 1024) { snprintf(buf, sizeof buf, "it needs %zu bytes of LDS for its parameters, the policy input and the activations of %d copies (at most %d)", bytes, e->env.n, 144 * 1024); return buf; }
    return std::string();
}
// the member's record, from the engine as it stands (the policy workspace is sized here: what build_act_program does for a standalone rollout)
static int tiny_act_record(dqn_engine* e, RolloutDev* rs, TinyActArgs* out) {
    if (policy_ws(e, std::max(e->env.n, std::max(e->pol_n, e->eval_n)))) return -1;
    TinyActArgs a; memset(&a, 0, sizeof a);
    const Levels levels = net_levels(e);
    for (int i = 0; i < e->nl; i++) a.L[i] = e->L[i];
    a.lds_bytes = (unsigned)(tiny_act_layout(e, &a) * 4);
    a.nl = e->nl; a.nlev = (int)levels.size(); a.dueling = e->hp.dueling; a.last_base = e->last_base; a.last_val = e->last_val; a.last_adv = e->last_adv;
    a.rows_u8 = e->hp.obs_dtype == DQN_OBS_U8 ? 1 : 0; a.P = e->Pint;
    for (size_t li = 0; li < levels.size(); li++) { a.lev_n[li] = (int)levels[li].size(); a.lev_l[li][0] = levels[li][0]; a.lev_l[li][1] = levels[li].size() > 1 ? levels[li][1] : levels[li][0]; }
    a.p_on = e->p_on; a.pol_x = e->pol_x; a.pol_q = e->pol_q; a.pol_a = e->pol_a; a.s_rows = e->s_rows; a.sp_rows = e->sp_rows; a.rs = rs; a.V = e->env;
    a.R = replay_meta(e);
    *out = a; return 0;
}
// Flux.loadparams!(target_q, params(active_q)) of every member: workgroup k copies member k's online parameters over its target parameters (dqn_sync_target keeps no host state)
__global__ __launch_bounds__(256) void k_group_sync_target(const TinyArgs* __restrict__ A) {
    const TinyArgs& a = A[blockIdx.x];
    float* tg = const_cast<float*>(a.p_tg);
    for (unsigned long long i = threadIdx.x; i < a.P; i += blockDim.x) tg[i] = a.p_on[i];
}
// per member, after the last step of a dqn_rollout_many call: the fold of the step's scalars (k_group_scalars; the grad norm only when the call trained), the consumed
// assertion flag, and the env set's episode statistics summed in copy order in Float64 -- the host loop of dqn_rollout_explore
__global__ __launch_bounds__(256) void k_group_rollout_scalars(const TinyArgs* __restrict__ A, const TinyActArgs* __restrict__ C, int K, int trained, RolloutScalars* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    StepState* st = A[k].state;
    RolloutScalars o; o.loss = 0.0f; o.gnorm = 0.0f; o.pad = 0;
    if (trained) { const float g = fmaxf(0.0f, A[k].gmax_part[0]); st->gnorm_bits = __float_as_uint(g); o.loss = st->loss; o.gnorm = g; }
    o.err = atomicExch(&st->err, 0); o.step = st->step;
    const EnvDev& V = C[k].V;
    long long ep = 0; double rw = 0.0;
    for (int i = 0; i < V.n; i++) { ep += V.fin_eps[i]; rw += V.fin_reward[i]; }
    o.episodes = ep; o.reward_sum = rw;
    out[k] = o;
}

// what every refusal below must be able to say of another member's refusal: the message of the last fail(), copied (fail() formats into the buffer it would read from)
static std::string last_message() { return std::string(dqn_last_error()); }

// the per-call validation of dqn_rollout_many: everything that can be refused, before anything is enqueued.  *train_at: per vector step of the call, 1 where the group train step runs
static int rollout_many_check(dqn_group* g, int n_steps, const dqn_rollout_cfg* cfgs, const dqn_exploration* const* explore, std::vector<char>* train_at) {
    if (n_steps < 1) return fail("dqn_rollout_many: n_steps = %d, at least one vector step is needed", n_steps);
    if (!cfgs) return fail("dqn_rollout_many: cfgs is NULL (one dqn_rollout_cfg per member)");
    const dqn_rollout_cfg& c0 = cfgs[0];
    for (int k = 0; k < g->K; k++) {
        const dqn_rollout_cfg& c = cfgs[k];
        if (c.t0 < 1) return fail("dqn_rollout_many: member %d: t0 counts from 1 (src/solver.jl:82)", k);
        if (c.cadence_env_steps != 0) return fail("dqn_rollout_many: member %d: cadence_env_steps = %d -- the group runs the vector-step cadence only (cadence_env_steps = 0)", k, c.cadence_env_steps);
        if (c.train_freq != c0.train_freq) return fail("dqn_rollout_many: train_freq differs between members 0 and %d (%d vs %d): the members run in lock step", k, c0.train_freq, c.train_freq);
        if (c.target_update_freq != c0.target_update_freq) return fail("dqn_rollout_many: target_update_freq differs between members 0 and %d (%d vs %d): the members run in lock step", k, c0.target_update_freq, c.target_update_freq);
        if (c.t0 != c0.t0) return fail("dqn_rollout_many: t0 differs between members 0 and %d (%lld vs %lld): the members run in lock step", k, (long long)c0.t0, (long long)c.t0);
    }
    for (int k = 0; k < g->K; k++) if (explore && explore[k] && explore_check(explore[k], n_steps)) { const std::string why = last_message(); return fail("dqn_rollout_many: member %d: %s", k, why.c_str()); }
    for (int k = 0; k < g->K; k++) {
        const std::string why = tiny_act_decline(g->members[k]);
        if (!why.empty()) return fail("dqn_rollout_many: member %d does not take the single-workgroup acting step: %s", k, why.c_str());
    }
    // the standalone loop trains a member only once its replay holds a batch, and a group launch cannot skip a member: size, n, cap and B are host-known, so every due
    // step of the call is decided here, and members that disagree at one are refused
    train_at->assign((size_t)n_steps, 0);
    if (c0.train_freq > 0) {
        std::vector<long long> size((size_t)g->K);
        for (int k = 0; k < g->K; k++) size[k] = g->members[k]->size;
        for (int j = 0; j < n_steps; j++) {
            const long long t = c0.t0 + j;
            for (int k = 0; k < g->K; k++) size[k] = std::min(g->members[k]->cap, size[k] + g->members[k]->env.n);
            if (!rollout_due(c0, t, g->members[0]->env.n).due) continue;      // (the vector-step cadence: n does not enter)
            const bool w0 = size[0] >= g->members[0]->B;
            for (int k = 1; k < g->K; k++) if ((size[k] >= g->members[k]->B) != w0)
                return fail("dqn_rollout_many: members 0 and %d disagree at vector step %lld on whether the train step runs (member 0 holds %lld of its batch of %d, member %d holds %lld of %d): "
                            "one launch trains every member or none -- fill the replays so that every member holds a batch at the same due step", k, t, size[0], g->members[0]->B, k, size[k], g->members[k]->B);
            (*train_at)[(size_t)j] = w0 ? 1 : 0;
        }
    }
    return 0;
}
// the members' records, rebuilt from the engines as they stand (an env set may be created or replaced, a policy workspace may grow between two calls) and uploaded
// when they differ from what the device array holds
static int rollout_many_records(dqn_group* g) {
    const size_t K = (size_t)g->K;
    if (!g->ro_host) { DM(g->mem, g->roll_dev, K); DM(g->mem, g->act_dev, K); DM(g->mem, g->ro_dev, K); if (g->mem.get_pinned(&g->ro_host, K, hipHostMallocDefault)) return -1; g->roll_host.resize(K); }      // (tested by the LAST of the four)
    std::vector<TinyActArgs> recs(K); unsigned lds = 0;
    for (size_t k = 0; k < K; k++) { if (tiny_act_record(g->members[k], g->roll_dev + k, &recs[k])) return -1; lds = std::max(lds, recs[k].lds_bytes); }
    if (g->act_host.size() != K || memcmp(g->act_host.data(), recs.data(), sizeof(TinyActArgs) * K) != 0) {
        HIPCHK(hipStreamSynchronize(g->stream));
        HIPCHK(hipMemcpy(g->act_dev, recs.data(), sizeof(TinyActArgs) * K, hipMemcpyHostToDevice));
        g->act_host.swap(recs);
    }
    g->act_lds = lds;
    return 0;
}

extern "C" int dqn_rollout_many_info(dqn_group_t* g, int* launches_per_vector_step, unsigned* max_lds_bytes) {
    if (!g) return fail("null group handle");
    unsigned lds = 0;
    for (int k = 0; k < g->K; k++) {
        const std::string why = tiny_act_decline(g->members[k]);
        if (!why.empty()) return fail("dqn_rollout_many_info: member %d does not take the single-workgroup acting step: %s", k, why.c_str());
        lds = std::max(lds, (unsigned)(tiny_act_layout(g->members[k], nullptr) * 4));
    }
    if (launches_per_vector_step) *launches_per_vector_step = 1;
    if (max_lds_bytes) *max_lds_bytes = lds;
    return 0;
}

extern "C" int dqn_rollout_many(dqn_group_t* g, int n_steps, const dqn_rollout_cfg* cfgs, const dqn_exploration* const* explore, dqn_rollout_stats* out) {
    if (!g) return fail("null group handle");
    std::vector<char> train_at;
    if (rollout_many_check(g, n_steps, cfgs, explore, &train_at)) return -1;
    HIPCHK(hipSetDevice(g->device));
    if (rollout_many_records(g)) return -1;
    const int control = group_has_control(g);
    if (tiny_act_raise_lds(g->act_lds, control)) return fail("dqn_rollout_many: the device refused %u bytes of dynamic LDS for the acting launch (hipFuncSetAttribute)", g->act_lds);
    const int K = g->K; const dqn_rollout_cfg& c0 = cfgs[0];
    // the call's records and tables: ONE contiguous array each, ONE H2D copy each
    size_t nx = 0;
    for (int k = 0; k < K; k++) if (explore && explore[k]) nx += (size_t)explore[k]->n_values;
    if (nx > g->xtab_cap) { HIPCHK(hipStreamSynchronize(g->stream)); if (grow(g->mem, &g->xtab_dev, &g->xtab_cap, nx, 1024)) return -1; }
    g->xtab_host.clear();
    for (int k = 0; k < K; k++) {
        RolloutDev h = rollout_record(&cfgs[k], g->members[k]);
        if (explore && explore[k]) {
            const dqn_exploration* x = explore[k];
            h.xkind = x->kind; h.xtab = g->xtab_dev + g->xtab_host.size(); h.xtab_t0 = cfgs[k].t0; h.xtab_n = x->n_values;
            g->xtab_host.insert(g->xtab_host.end(), x->values, x->values + x->n_values);      // the caller's arrays are not kept
        }
        g->roll_host[(size_t)k] = h;
    }
    static const char who[] = "dqn_rollout_many";
    long long trained = 0;
    if (group_call(g, who, [&]() {
            hipError_t he = hipMemcpyAsync(g->roll_dev, g->roll_host.data(), sizeof(RolloutDev) * (size_t)K, hipMemcpyHostToDevice, g->stream);
            if (he == hipSuccess && nx) he = hipMemcpyAsync(g->xtab_dev, g->xtab_host.data(), sizeof(float) * nx, hipMemcpyHostToDevice, g->stream);      // (both host arrays are the group's: they outlive the copies)
            if (he != hipSuccess) return fail("dqn_rollout_many: HIP error %s uploading the call's records", hipGetErrorString(he));
            for (int j = 0; j < n_steps; j++) {
                if (launch_tiny_act(g->stream, g->act_dev, K, g->act_lds, j == 0 ? 1 : 0, j == n_steps - 1 ? 1 : 0, control)) return fail("dqn_rollout_many: the device refused %u bytes of dynamic LDS for the acting launch (hipFuncSetAttribute)", g->act_lds);
                for (dqn_engine* e : g->members) { ring_advance(e, e->env.n); e->env_q_valid = true; }      // what dqn_rollout_explore keeps on the host
                if (train_at[(size_t)j]) {      // :134-139, for all members in one launch
                    if (launch_tiny_group(g->stream, g->args_dev, K, g->max_lds, 1)) return fail("dqn_rollout_many: the device refused %u bytes of dynamic LDS for the group train launch (hipFuncSetAttribute)", g->max_lds);
                    trained++;
                }
                if (rollout_due(c0, c0.t0 + j, g->members[0]->env.n).sync) hipLaunchKernelGGL(k_group_sync_target, dim3(K), dim3(256), 0, g->stream, g->args_dev);      // :142-145
            }
            hipLaunchKernelGGL(k_group_rollout_scalars, dim3((K + 255) / 256), dim3(256), 0, g->stream, g->args_dev, g->act_dev, K, trained > 0 ? 1 : 0, g->ro_dev);
            return group_gather(g, who, "steps", g->ro_host, g->ro_dev, sizeof(RolloutScalars) * (size_t)K); })) return -1;
    for (int k = 0; k < K && out; k++) { const RolloutScalars& o = g->ro_host[k]; out[k].episodes = o.episodes; out[k].reward_sum = o.reward_sum; out[k].train_steps = trained; out[k].last_loss = o.loss; out[k].last_grad_norm = o.gnorm; }
    return group_members_failed(g->ro_host, K);
}

// ---------------------------------------------------------------- grouped evaluation: dqn_evaluate_many (tiny_eval.hip)
// the dynamic-LDS layout of the single-workgroup evaluation, in floats: the online parameters, the staging area of the sums (n_eval Float64 + n_eval Int32), then for ONE
// TILE of tw copies the policy input x[E][tw] and per layer its activations [N][tw] (every part 16-byte aligned).  The tile width is the widest multiple of 4 the budget
// of tiny_act_decline (144 KB with the kernel's static arrays, TINY_ACT_TAIL_LDS) leaves room for, at most n_eval rounded up to 4; 0: not even four copies fit.
// t != null: the offsets are recorded
static const size_t TINY_EVAL_LDS_FLOATS = (144 * 1024 - TINY_ACT_TAIL_LDS) / 4;
static size_t tiny_eval_layout(const dqn_engine* e, int n_eval, TinyEvalArgs* t) {
    size_t fl = 0; TinyEvalArgs tmp; TinyEvalArgs& T = t ? *t : tmp;
    auto take = [&](size_t m) { const int o = (int)fl; fl += (m + 3) / 4 * 4; return o; };
    T.a.p_off = take(e->Pint); T.r_off = take((size_t)3 * n_eval);
    size_t per_copy = (size_t)e->E; for (int i = 0; i < e->nl; i++) per_copy += (size_t)e->L[i].N;
    const size_t room = fl < TINY_EVAL_LDS_FLOATS ? (TINY_EVAL_LDS_FLOATS - fl) / per_copy / 4 * 4 : 0;
    T.tw = (int)std::min<size_t>(room, ((size_t)n_eval + 3) / 4 * 4);
    T.a.x_off = take((size_t)e->E * T.tw);
    for (int i = 0; i < e->nl && i < TINY_MAX_LAYERS; i++) T.a.y_off[i] = take((size_t)e->L[i].N * T.tw);
    return fl;
}
// THE eligibility rule of the single-workgroup evaluation: empty when the engine takes it, else the reason in words.  It does not depend on n_eval (judged at the
// largest, 1024, whose staging area is the widest) nor on the training copies.  NOT every network that passes tiny_decline passes: that rule bounds 3 P + (2 E + 4 sum N)
// batch_size floats, so at batch_size = 1 a Dense(7000, 1) passes it, and four of its columns (28 000 floats beside 7001 parameters) exceed the 25 856 floats of a
// workgroup here.  A member with P at the limit of 16 384 fits while E + sum N <= 1600; every network of the README's tables is far inside
std::string tiny_eval_decline(const dqn_engine* e) {
    char buf[240];
    if (!e->has_envs) return "it has no device environments (dqn_envs_create / dqn_envs_create_tabular)";
    const std::string why = tiny_decline(e);
    if (!why.empty()) return why;
    TinyEvalArgs t;
    if (tiny_eval_layout(e, 1024, &t), t.tw < 4) {
        size_t per_copy = (size_t)e->E; for (int i = 0; i < e->nl; i++) per_copy += (size_t)e->L[i].N;
        snprintf(buf, sizeof buf, "its %zu parameters and a tile of 4 evaluation copies (%zu floats of policy input and activations each) do not fit the %zu floats of LDS of one workgroup",
                 e->Pint, per_copy, TINY_EVAL_LDS_FLOATS - 3072);
        return buf;
    }
    return std::string();
}
// everything dqn_evaluate_many and dqn_evaluate_many_info refuse, before anything is enqueued or changed
static int evaluate_many_check(const char* fn, dqn_group* g, int n_eval, int max_episode_length) {
    if (!g) return fail("null group handle");
    if (n_eval < 1 || n_eval > 1024) return fail("%s: n_eval = %d is outside 1..1024", fn, n_eval);
    if (max_episode_length < 1) return fail("%s: max_episode_length = %d, at least 1 is needed", fn, max_episode_length);
    for (int k = 0; k < g->K; k++) {
        const std::string why = tiny_eval_decline(g->members[k]);
        if (!why.empty()) return fail("%s: member %d does not take the single-workgroup evaluation: %s", fn, k, why.c_str());
    }
    return 0;
}

extern "C" int dqn_evaluate_many_info(dqn_group_t* g, int n_eval, int max_episode_length, int* launches, int* steps_per_launch, unsigned* max_lds_bytes) {
    if (evaluate_many_check("dqn_evaluate_many_info", g, n_eval, max_episode_length)) return -1;
    unsigned lds = 0;
    for (int k = 0; k < g->K; k++) lds = std::max(lds, (unsigned)(tiny_eval_layout(g->members[k], n_eval, nullptr) * 4));
    if (launches) *launches = (max_episode_length + 1 + TINY_EVAL_STEPS - 1) / TINY_EVAL_STEPS;
    if (steps_per_launch) *steps_per_launch = TINY_EVAL_STEPS;
    if (max_lds_bytes) *max_lds_bytes = lds;
    return 0;
}

extern "C" int dqn_evaluate_many(dqn_group_t* g, int n_eval, int max_episode_length, const uint64_t* seeds, double* avg_reward, double* avg_steps) {
    if (evaluate_many_check("dqn_evaluate_many", g, n_eval, max_episode_length)) return -1;
    if (!seeds) return fail("dqn_evaluate_many: seeds is NULL (one seed per member)");
    if (!avg_reward && !avg_steps) return fail("dqn_evaluate_many: avg_reward and avg_steps are both NULL");
    HIPCHK(hipSetDevice(g->device));
    const int K = g->K; const size_t Ks = (size_t)K;
    if (!g->es_host) { DM(g->mem, g->eval_dev, Ks); DM(g->mem, g->es_dev, Ks); if (g->mem.get_pinned(&g->es_host, Ks, hipHostMallocDefault)) return -1; g->eval_host.resize(Ks); }      // (tested by the LAST of the three)
    // the members' evaluation copies (allocated as dqn_evaluate allocates them, on first use and when n_eval changes) and the head outputs of all of them
    size_t nheads = 0;
    for (dqn_engine* e : g->members) { if (eval_envs_ensure(e, n_eval)) return -1; nheads += (size_t)(e->nA + (e->hp.dueling ? 1 : 0)) * n_eval; }
    if (nheads > g->heads_cap) { HIPCHK(hipStreamSynchronize(g->stream)); if (grow(g->mem, &g->heads_dev, &g->heads_cap, nheads, 0)) return -1; }
    // the call's records: the member's acting record with the evaluation set (this call's seed and episode bound) in the place of the training set, laid out by tile
    unsigned lds = 0; size_t hoff = 0;
    for (int k = 0; k < K; k++) {
        dqn_engine* e = g->members[k]; TinyEvalArgs& T = g->eval_host[(size_t)k];
        memset(&T, 0, sizeof T);
        if (tiny_act_record(e, &g->eval_dev[k].roll, &T.a)) return -1;
        T.a.lds_bytes = (unsigned)(tiny_eval_layout(e, n_eval, &T) * 4); lds = std::max(lds, T.a.lds_bytes);
        T.a.V = e->eval_env; T.a.V.seed = seeds[k]; T.a.V.max_episode_length = max_episode_length;      // (the engine's own copy keeps what its evaluation program was built with)
        T.roll = rollout_record(nullptr, e);      // always greedy
        T.heads = g->heads_dev + hoff; hoff += (size_t)(e->nA + (e->hp.dueling ? 1 : 0)) * n_eval;
        T.out = g->es_dev + k;
    }
    const int control = group_has_control(g);
    if (tiny_eval_raise_lds(lds, control)) return fail("dqn_evaluate_many: the device refused %u bytes of dynamic LDS for the evaluation launch (hipFuncSetAttribute)", lds);
    static const char who[] = "dqn_evaluate_many";
    if (group_call(g, who, [&]() {
            for (dqn_engine* e : g->members) e->env_q_valid = false;      // the evaluation copies' forward writes pol_q / pol_a, as dqn_evaluate's does
            const hipError_t he = hipMemcpyAsync(g->eval_dev, g->eval_host.data(), sizeof(TinyEvalArgs) * Ks, hipMemcpyHostToDevice, g->stream);      // (the host array is the group's: it outlives the copy)
            if (he != hipSuccess) return fail("dqn_evaluate_many: HIP error %s uploading the call's records", hipGetErrorString(he));
            const int total = max_episode_length + 1;      // while !done && step <= max_episode_length
            for (int s0 = 0; s0 < total; s0 += TINY_EVAL_STEPS) {
                const int ns = std::min(TINY_EVAL_STEPS, total - s0);
                if (launch_tiny_eval(g->stream, g->eval_dev, K, lds, ns, s0 == 0 ? 1 : 0, s0 + ns >= total ? 1 : 0, control)) return fail("dqn_evaluate_many: the device refused %u bytes of dynamic LDS for the evaluation launch (hipFuncSetAttribute)", lds);
            }
            return group_gather(g, who, "evaluation", g->es_host, g->es_dev, sizeof(EvalSums) * Ks); })) return -1;
    for (int k = 0; k < K; k++) {      // avg_r /= n_eval; avg_steps /= n_eval (dqn_evaluate's last lines)
        if (avg_reward) avg_reward[k] = g->es_host[k].reward_sum / n_eval;
        if (avg_steps) avg_steps[k] = (double)g->es_host[k].steps / n_eval;
    }
    return 0;
}
