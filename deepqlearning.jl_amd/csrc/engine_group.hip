// engine_group.hip -- dqn_group_*: K engines whose whole train step is one single-workgroup launch (tiny_step.hip) stepped by ONE launch of K workgroups.
// A group owns a device array of its members' TinyArgs records (copies of the host record each engine keeps, dqn_engine::tiny_args), a stream and the events that
// order that stream against the members' streams.  Everything a step reads or writes is the member's own (parameters, Adam state, sum-tree, replay rows, StepState,
// the step workspaces): the group adds no state of its own to a member, so after a group call a member cannot tell it from dqn_train_steps.
#include "engine.h"

struct GroupScalars { float loss, gnorm; int err, pad; unsigned long long step; };      // what the standalone step's publish launch reports (StepMail), per member

struct dqn_group {
    int device = 0, K = 0; unsigned max_lds = 0;
    std::vector<dqn_engine*> members;
    TinyArgs* args_dev = nullptr;
    hipStream_t stream = nullptr; std::vector<hipEvent_t> ev_in; hipEvent_t ev_done = nullptr;
    GroupScalars *out_dev = nullptr, *out_host = nullptr;      // out_host: pinned
    bool counted = false;      // the members' in_groups counts include this group
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
    hipError_t err;
    if ((err = hipMalloc((void**)&g->args_dev, sizeof(TinyArgs) * (size_t)n_members)) != hipSuccess) return bail("hipMalloc of the members' records", err);
    if ((err = hipMemcpy(g->args_dev, recs.data(), sizeof(TinyArgs) * (size_t)n_members, hipMemcpyHostToDevice)) != hipSuccess) return bail("the upload of the members' records", err);
    if ((err = hipMalloc((void**)&g->out_dev, sizeof(GroupScalars) * (size_t)n_members)) != hipSuccess) return bail("hipMalloc of the scalars", err);
    if ((err = hipHostMalloc((void**)&g->out_host, sizeof(GroupScalars) * (size_t)n_members, hipHostMallocDefault)) != hipSuccess) return bail("hipHostMalloc of the scalars", err);
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
    if (g->out_host) hipHostFree(g->out_host);
    hipFree(g->out_dev); hipFree(g->args_dev);
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
    // in: the group's stream behind everything the members have enqueued (replay_add, their own steps, target syncs, rollouts)
    for (int k = 0; k < g->K; k++) { HIPCHK(hipEventRecord(g->ev_in[k], g->members[k]->stream)); HIPCHK(hipStreamWaitEvent(g->stream, g->ev_in[k], 0)); }
    (void)hipGetLastError();
    int rc = 0;
    if (launch_tiny_group(g->stream, g->args_dev, g->K, g->max_lds, n))
        rc = fail("dqn_group_train_steps: the device refused %u bytes of dynamic LDS for the group launch (hipFuncSetAttribute)", g->max_lds);
    hipError_t he = hipSuccess;
    if (!rc) {
        hipLaunchKernelGGL(k_group_scalars, dim3((g->K + 255) / 256), dim3(256), 0, g->stream, g->args_dev, g->K, g->out_dev);
        he = hipGetLastError();
        if (he == hipSuccess) he = hipMemcpyAsync(g->out_host, g->out_dev, sizeof(GroupScalars) * (size_t)g->K, hipMemcpyDeviceToHost, g->stream);
        if (he != hipSuccess) rc = fail("dqn_group_train_steps: HIP error %s behind the group's steps", hipGetErrorString(he));
    }
    // out: every member's stream behind whatever the group enqueued -- on the error paths too: a later member call must never run beside steps already enqueued.
    // Whatever the member enqueues next sees the group's steps, without a host synchronise
    he = hipEventRecord(g->ev_done, g->stream);
    for (int k = 0; k < g->K && he == hipSuccess; k++) he = hipStreamWaitEvent(g->members[k]->stream, g->ev_done, 0);
    const hipError_t hs = hipStreamSynchronize(g->stream);      // the scalars and the assertion flags of this call
    if (rc) return rc;
    if (he != hipSuccess || hs != hipSuccess) return fail("dqn_group_train_steps: HIP error %s ordering the members' streams behind the group", hipGetErrorString(he != hipSuccess ? he : hs));
    int bad = -1, nbad = 0;
    for (int k = 0; k < g->K; k++) {
        const GroupScalars& o = g->out_host[k];
        if (loss) loss[k] = o.loss;
        if (grad_norm) grad_norm[k] = o.gnorm;
        if (o.err) { if (bad < 0) bad = k; nbad++; }
    }
    if (bad >= 0) {
        const GroupScalars& o = g->out_host[bad];
        const char* more = nbad > 1 ? "; further members failed too, the other members' steps stand" : "; the other members' steps stand";
        if (o.err == 2) return fail("member %d: AssertionError: all(new_priorities .> 0f0) (at or before train step %llu)%s", bad, o.step, more);
        return fail("member %d: device-side error %d at or before train step %llu%s", bad, o.err, o.step, more);
    }
    return 0;
}
