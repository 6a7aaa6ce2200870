// engine_envs.hip -- C ABI of the device-resident environments: dqn_envs_create / dqn_envs_create_tabular /
// dqn_envs_create_control / dqn_rollout / dqn_evaluate / dqn_envs_peek / dqn_envs_peek_q / dqn_envs_peek_state; kernels in envs.hip.
#include <cmath>
#include "engine.h"

// ---------------------------------------------------------------- vectorised environments on the device
// the evaluation copies: eval_mem holds their per-copy arrays, eval_roll and their private Recur state (images, spec and tables are the training set's)
static void free_eval_envs(dqn_engine* e) {
    e->eval_mem.release(); memset(&e->eval_env, 0, sizeof e->eval_env); e->eval_roll = nullptr; e->eval_n = 0; for (int i = 0; i < DQN_MAX_LAYERS; i++) e->eval_h[i] = e->eval_c[i] = e->eval_gx[i] = nullptr;
}
void free_envs(dqn_engine* e) {
    drop_act(e, e->act); drop_act(e, e->act_gen); drop_act(e, e->evalp); free_eval_envs(e);
    e->env_mem.release();      // the per-copy arrays, images, tables, roll, xtab and -- the open episodes go with the env set; the committed ring is the engine's -- ep_stage
    memset(&e->env, 0, sizeof e->env); memset(&e->ep_stage, 0, sizeof e->ep_stage); e->has_envs = false; e->env_q_valid = false; e->env_images = nullptr; e->env_tab = nullptr; e->env_term = nullptr; e->roll = nullptr; e->xtab = nullptr; e->xtab_cap = 0;
}
// what every kind of env set checks before it replaces the engine's current one
static int envs_admit(dqn_engine* e, int n_envs, int max_episode_length) {
    const bool rec = e->hp.recurrence != 0;
    if (rec) {
        // the episode commits and the host sampler's mirror of the ring are single-device
        if (e->comm) return fail("device environments on a recurrent engine are single-device: this engine has a communicator (dqn_comm_init)");
        if (e->opt.sim_world >= 1) return fail("device environments on a recurrent engine are single-device: this engine was created under DQN_SIM_WORLD");
        if (e->ep_cur_len > 0) return fail("an episode is open on the host side (dqn_episode_add without its terminal transition): finish it or call dqn_episode_commit before creating device environments");
        if (e->ep_cap > 0x7ffffff0ll) return fail("episode replay capacity %lld is too large for device environments", e->ep_cap);
        if (n_envs < 1 || n_envs > 1024) return fail("n_envs must be in 1..1024");      // buffer_size counts episodes: the transition-ring capacity does not apply
    } else
    if (n_envs < 1 || n_envs > std::min<long long>(1024, e->cap)) return fail("n_envs must be in 1..min(1024, replay capacity)");
    if (max_episode_length < 1) return fail("max_episode_length must be >= 1");
    return 0;
}
// THE start of every creator: the family's refusals that need nothing but the engine -- u8 rows, the network's shape, single device (each in the family's own
// wording) -- then envs_admit, then the header every kind shares, in H.  Nothing of the engine is touched: the creator validates the rest of its spec, then envs_install
enum { ENV_FAM_BUILTIN = 0, ENV_FAM_TABULAR = 1, ENV_FAM_CONTROL = 2 };
static int envs_begin(dqn_engine* e, int family, int kind, int n_envs, int max_episode_length, uint64_t seed, EnvDev& H) {
    const char* const who = kind == DQN_ENV_MOUNTAINCAR ? "MountainCar" : "InvertedPendulum";
    const char* const tag = family == ENV_FAM_TABULAR ? "tabular env" : "control env";
    if (family != ENV_FAM_BUILTIN) {      // (the built-in kinds take replicas; SimpleGridWorld refuses u8 rows with its own shape rules)
        if (e->hp.obs_dtype == DQN_OBS_U8) return family == ENV_FAM_TABULAR ? fail("%s: the feature rows are floats, this engine stores observations as u8: use obs_dtype f32", tag)
                                                                             : fail("%s: %s observations are Float32[state[1], state[2]], this engine stores observations as u8: use obs_dtype f32", tag, who);
        if (family == ENV_FAM_CONTROL && (e->E != 2 || e->nA != 3)) return fail("%s: %s has an observation of 2 floats and 3 actions (network: %d in, %d out)", tag, who, e->E, e->nA);
        const char* const sets = family == ENV_FAM_TABULAR ? "device environments from tables" : "these device environments";
        if (e->comm) return fail("%s: %s are single-device: this engine has a communicator (dqn_comm_init)", tag, sets);
        if (e->opt.sim_world >= 1) return fail("%s: %s are single-device: this engine was created under DQN_SIM_WORLD", tag, sets);
    }
    if (envs_admit(e, n_envs, max_episode_length)) return -1;
    memset(&H, 0, sizeof H);
    H.kind = kind; H.n = n_envs; H.E = e->E; H.nA = e->nA; H.max_episode_length = max_episode_length; H.seed = seed; H.prioritized = e->hp.prioritized_replay ? 1 : 0;
    return 0;
}
// the engine's current env set goes, H is the new one's header
static int envs_install(dqn_engine* e, const EnvDev& H) { HIPCHK(hipStreamSynchronize(e->stream)); free_envs(e); e->env = H; return 0; }
// THE per-copy arrays of n copies of V's kind, in M: the kind's state, then the eight loop arrays every kind shares.  The training set (envs_finish) and the evaluation
// copies (eval_envs_ensure) both come here, so a new kind is added once.  The two arrays a transition's s is read from before the set's first step are zeroed with
// their kind -- for the evaluation copies too, where nothing reads them before a step writes them
static int env_copy_state(DevScope& M, EnvDev& V, int n, hipStream_t st) {
    if (V.kind == DQN_ENV_TESTMDP) { DM(M, V.tm_s, (size_t)n * 4); DM(M, V.tm_prev, (size_t)n * 4); DM(M, V.tm_t, n); }
    else if (V.kind == DQN_ENV_TABULAR) { DM(M, V.tb_s, n); DM(M, V.tb_o, n); DM(M, V.tb_oprev, n); HIPCHK(hipMemsetAsync(V.tb_oprev, 0, (size_t)n * 4, st)); }
    else if (env_is_control(V.kind)) { DM(M, V.ct_s, (size_t)n * 2); DM(M, V.ct_prev, (size_t)n * 2); HIPCHK(hipMemsetAsync(V.ct_prev, 0, (size_t)n * 2 * sizeof(double), st)); }
    else { DM(M, V.gw_pos, (size_t)n * 2); DM(M, V.gw_prev, (size_t)n * 2); }
    DM(M, V.actions, n); DM(M, V.rewards, n); DM(M, V.dones, n); DM(M, V.pending, n); DM(M, V.ep_reward, n); DM(M, V.ep_step, n); DM(M, V.fin_eps, n); DM(M, V.fin_reward, n);
    return 0;
}
static int envs_finish(dqn_engine* e);
extern "C" int dqn_envs_create(dqn_engine_t* e, const dqn_env_spec* sp) { if (!e) return fail("null engine handle");
    HIPCHK(hipSetDevice(e->device));
    EnvDev H;
    if (envs_begin(e, ENV_FAM_BUILTIN, sp->kind, sp->n_envs, sp->max_episode_length, sp->seed, H) || envs_install(e, H)) return -1;
    EnvDev& V = e->env;
    const bool u8 = e->hp.obs_dtype == DQN_OBS_U8;
    if (sp->kind == DQN_ENV_TESTMDP) {
        if (!sp->images) return fail("TestMDP needs its three images");
        if (sp->o_stack < 1 || sp->o_stack > 4 || sp->o_stack != e->hp.obs_c) return fail("TestMDP: o_stack (%d) must equal obs_c (%d) and be <= 4", sp->o_stack, e->hp.obs_c);
        if (e->nA != 4) return fail("TestMDP has 4 actions, the network has %d outputs", e->nA);
        V.H = e->hp.obs_h; V.W = e->hp.obs_w; V.max_time = sp->max_time;
        const size_t ib = (size_t)3 * V.H * V.W;
        DM(e->env_mem, e->env_images, ib); HIPCHK(hipMemcpy(e->env_images, sp->images, ib, hipMemcpyHostToDevice)); V.images = e->env_images;
    } else if (sp->kind == DQN_ENV_GRIDWORLD) {
        if (u8) return fail("SimpleGridWorld observations are Float32[x, y]: use obs_dtype f32");
        if (e->E != 2 || e->nA != 4) return fail("SimpleGridWorld: observation has 2 elements and there are 4 actions (network: %d in, %d out)", e->E, e->nA);
        if (sp->n_reward_cells < 0 || sp->n_reward_cells > 8) return fail("at most 8 reward cells");
        V.size_x = sp->size_x; V.size_y = sp->size_y; V.tprob = sp->tprob; V.n_reward = sp->n_reward_cells;
        for (int k = 0; k < V.n_reward; k++) { V.reward_xy[k][0] = sp->reward_xy[k][0]; V.reward_xy[k][1] = sp->reward_xy[k][1]; V.reward_val[k] = sp->reward_val[k]; }
    } else return fail("unknown environment kind %d", sp->kind);
    return envs_finish(e);
}
// the per-copy loop state every kind shares, the open episodes of a recurrent engine, and the first reset
static int envs_finish(dqn_engine* e) {
    EnvDev& V = e->env; const int n = V.n; const bool rec = e->hp.recurrence != 0;
    if (env_copy_state(e->env_mem, V, n, e->stream)) return -1;
    DM(e->env_mem, e->roll, DQN_ROLL_RECORDS);
    HIPCHK(hipMemsetAsync(V.fin_eps, 0, (size_t)n * 8, e->stream)); HIPCHK(hipMemsetAsync(V.fin_reward, 0, (size_t)n * 8, e->stream));
    HIPCHK(hipMemsetAsync(V.actions, 0, (size_t)n * 4, e->stream)); HIPCHK(hipMemsetAsync(V.rewards, 0, (size_t)n * 4, e->stream));
    HIPCHK(hipMemsetAsync(e->roll, 0, sizeof(RolloutDev) * DQN_ROLL_RECORDS, e->stream));
    if (rec) {      // the copies' open episodes: staging [n][T] (rows of s, rows of sp, a, r, done) and the open length
        EpStage& S = e->ep_stage; const size_t nt = (size_t)n * e->T;
        S.T = e->T; S.ep_cap = e->ep_cap;
        DM(e->env_mem, S.st_s, nt * e->E); DM(e->env_mem, S.st_sp, nt * e->E); DM(e->env_mem, S.st_a, nt); DM(e->env_mem, S.st_r, nt); DM(e->env_mem, S.st_done, nt); DM(e->env_mem, S.open_len, n);
        S.ep_s = e->ep_s; S.ep_sp = e->ep_sp; S.ep_a = e->ep_a; S.ep_r = e->ep_r; S.ep_done = e->ep_done; S.ep_len = e->ep_len; S.cur = e->ep_len + e->ep_cap;
    }
    e->has_envs = true;
    return dqn_envs_reset(e);
}
// a tabular (PO)MDP from its matrices (the law: include/dqn_mi355x.h).  Everything is validated before the engine's current env set is touched.
extern "C" int dqn_envs_create_tabular(dqn_engine_t* e, const dqn_tabular_env* sp) { if (!e) return fail("null engine handle");
    if (!sp) return fail("null tabular spec");
    HIPCHK(hipSetDevice(e->device));
    const long long S = sp->n_states, O = sp->n_obs, A = e->nA, E = e->E, NO = O ? O : S;
    if (S < 1 || S > 1024) return fail("tabular env: n_states = %d must be in 1..1024", sp->n_states);
    if (O < 0 || O > 1024) return fail("tabular env: n_obs = %d must be in 0..1024 (0: an MDP)", sp->n_obs);
    EnvDev H;
    if (envs_begin(e, ENV_FAM_TABULAR, DQN_ENV_TABULAR, sp->n_envs, sp->max_episode_length, sp->seed, H)) return -1;
    if (!sp->T) return fail("tabular env: T (transition table [S][A][S]) is NULL");
    if (!sp->R) return fail("tabular env: R (reward table [S][A][S]) is NULL");
    if (!sp->terminal) return fail("tabular env: terminal ([S]) is NULL");
    if (!sp->b0) return fail("tabular env: b0 (initial-state distribution [S]) is NULL");
    if (!sp->features) return fail("tabular env: features ([%lld][%lld]) is NULL", NO, E);
    if (O > 0 && !sp->Z) return fail("tabular env: Z (observation table [A][S][O]) is NULL with n_obs = %d", sp->n_obs);
    if (O > 0 && !sp->Z0) return fail("tabular env: Z0 (initial observation table [S][O]) is NULL with n_obs = %d", sp->n_obs);
    if (O == 0 && sp->Z) return fail("tabular env: Z is given with n_obs = 0 (an MDP observes its state)");
    if (O == 0 && sp->Z0) return fail("tabular env: Z0 is given with n_obs = 0 (an MDP observes its state)");
    // one float block: cumulative T | R | cumulative Z | cumulative Z0 | cumulative b0 | features, each part 16-byte aligned
    auto up4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
    const size_t nT = (size_t)(S * A * S), nZ = (size_t)(A * S * O), nZ0 = (size_t)(S * O), nF = (size_t)(NO * E);
    const size_t oT = 0, oR = up4(oT + nT), oZ = up4(oR + nT), oZ0 = up4(oZ + nZ), oB = up4(oZ0 + nZ0), oF = up4(oB + (size_t)S), tot = up4(oF + nF);
    std::vector<float> h(tot, 0.0f);
    // rows of `len` probabilities -> cumulative rows by a plain fp32 loop in ascending index order.  `rank` is the table's own ([S][A][S]: 3, [S][O]: 2, [S]: 1), so a
    // message names a value by the caller's indices: row r of a rank-3 table is [r / d1][r % d1]
    auto rows = [&](const char* name, const float* p, int rank, long long nrows, long long d1, long long len, bool exempt_terminal, float* out) -> int {
        char at[64];
        for (long long r = 0; r < nrows; r++) {
            if (rank == 3) snprintf(at, sizeof at, "%s[%lld][%lld]", name, r / d1, r % d1); else if (rank == 2) snprintf(at, sizeof at, "%s[%lld]", name, r); else snprintf(at, sizeof at, "%s", name);
            double sum = 0.0; float acc = 0.0f;
            for (long long j = 0; j < len; j++) {
                const float v = p[r * len + j];
                if (!(v >= 0.0f) || !std::isfinite(v)) return fail("tabular env: %s[%lld] = %g is negative or not finite", at, j, (double)v);
                sum += (double)v; acc = acc + v; out[r * len + j] = acc;
            }
            if (exempt_terminal && sp->terminal[r / d1]) continue;
            if (!(sum >= 1.0 - 1e-3 && sum <= 1.0 + 1e-3)) return fail("tabular env: row %s sums to %.6f, further than 1e-3 from 1", at, sum);
        }
        return 0;
    };
    if (rows("T", sp->T, 3, S * A, A, S, true, h.data() + oT)) return -1;
    if (O > 0 && rows("Z", sp->Z, 3, A * S, S, O, false, h.data() + oZ)) return -1;
    if (O > 0 && rows("Z0", sp->Z0, 2, S, 1, O, false, h.data() + oZ0)) return -1;
    if (rows("b0", sp->b0, 1, 1, 1, S, false, h.data() + oB)) return -1;
    for (size_t q = 0; q < nT; q++) { const float v = sp->R[q]; if (!std::isfinite(v)) return fail("tabular env: R[%zu][%zu][%zu] = %g is not finite", q / (size_t)(A * S), q / (size_t)S % (size_t)A, q % (size_t)S, (double)v); h[oR + q] = v; }
    for (size_t q = 0; q < nF; q++) { const float v = sp->features[q]; if (!std::isfinite(v)) return fail("tabular env: features[%zu][%zu] = %g is not finite", q / (size_t)E, q % (size_t)E, (double)v); h[oF + q] = v; }
    if (envs_install(e, H)) return -1;
    EnvDev& V = e->env;
    V.tb_S = (int)S; V.tb_O = (int)O;
    DM(e->env_mem, e->env_tab, tot); HIPCHK(hipMemcpy(e->env_tab, h.data(), tot * sizeof(float), hipMemcpyHostToDevice));
    DM(e->env_mem, e->env_term, (size_t)S); HIPCHK(hipMemcpy(e->env_term, sp->terminal, (size_t)S, hipMemcpyHostToDevice));
    V.tb_T = e->env_tab + oT; V.tb_R = e->env_tab + oR; V.tb_Z = O ? e->env_tab + oZ : nullptr; V.tb_Z0 = O ? e->env_tab + oZ0 : nullptr; V.tb_b0 = e->env_tab + oB; V.tb_feat = e->env_tab + oF;
    V.tb_term = e->env_term;
    return envs_finish(e);
}
// MountainCar / InvertedPendulum (the laws: include/dqn_mi355x.h).  Everything is validated before the engine's current env set is touched.
extern "C" int dqn_envs_create_control(dqn_engine_t* e, const dqn_control_env* sp) { if (!e) return fail("null engine handle");
    if (!sp) return fail("null control spec");
    HIPCHK(hipSetDevice(e->device));
    if (!env_is_control(sp->kind)) return fail("control env: unknown kind %d (3: MountainCar, 4: InvertedPendulum)", sp->kind);
    EnvDev H;
    if (envs_begin(e, ENV_FAM_CONTROL, sp->kind, sp->n_envs, sp->max_episode_length, sp->seed, H)) return -1;
    static const char* const names[CT_N] = {"force", "freq", "gravity", "v_max", "x_min", "goal", "cost", "jackpot", "x0", "v0", "g", "m", "l", "M", "alpha", "dt", "u_max", "noise", "theta_max", "init_half"};
    static_assert(offsetof(dqn_control_env, init_half) - offsetof(dqn_control_env, force) == (CT_N - 1) * sizeof(double), "CT_* follows the struct's own order");
    const double* const c = &sp->force;
    for (int k = 0; k < CT_N; k++) if (!std::isfinite(c[k])) return fail("control env: %s = %g is not finite", names[k], c[k]);
    if (sp->kind == DQN_ENV_MOUNTAINCAR) {
        if (!(sp->v_max > 0.0)) return fail("control env: v_max = %g must be > 0", sp->v_max);
        if (!(sp->x_min < sp->goal)) return fail("control env: x_min = %g must lie below goal = %g", sp->x_min, sp->goal);
    } else {
        if (!(sp->dt > 0.0)) return fail("control env: dt = %g must be > 0", sp->dt);
        if (!(sp->l > 0.0)) return fail("control env: l = %g must be > 0", sp->l);
        if (!(sp->alpha * sp->m < 4.0 / 3.0)) return fail("control env: alpha * m = %g must lie below 4/3 (alpha = %g, m = %g): the denominator (4/3) l - alpha m l cos^2(theta) can reach 0", sp->alpha * sp->m, sp->alpha, sp->m);
    }
    if (envs_install(e, H)) return -1;
    double* cb = nullptr; DM(e->env_mem, cb, (size_t)CT_N); HIPCHK(hipMemcpy(cb, c, CT_N * sizeof(double), hipMemcpyHostToDevice)); e->env.ct_c = cb;
    return envs_finish(e);
}
extern "C" int dqn_envs_peek_state(dqn_engine_t* e, double* state, double* prev) { if (!e) return fail("null engine handle");
    HIPCHK(hipSetDevice(e->device));
    if (!e->has_envs) return fail("no device environments: call dqn_envs_create");
    if (!env_is_control(e->env.kind)) return fail("dqn_envs_peek_state: the env set is of kind %d; only MountainCar (3) and InvertedPendulum (4) carry a Float64 state", e->env.kind);
    const size_t bytes = (size_t)e->env.n * 2 * sizeof(double);
    HIPCHK(hipStreamSynchronize(e->stream));
    if (state) HIPCHK(hipMemcpy(state, e->env.ct_s, bytes, hipMemcpyDeviceToHost));
    if (prev) HIPCHK(hipMemcpy(prev, e->env.ct_prev, bytes, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int dqn_envs_reset(dqn_engine_t* e) { if (!e) return fail("null engine handle");
    HIPCHK(hipSetDevice(e->device));
    if (!e->has_envs) return fail("no device environments: call dqn_envs_create");
    launch_env_reset_pending(e->stream, e->env, e->roll, 1);
    if (e->hp.recurrence) {      // reset!(env) of every copy: their open episodes are dropped, resetstate!(policy) on n streams
        HIPCHK(hipMemsetAsync(e->ep_stage.open_len, 0, (size_t)e->env.n * 4, e->stream));
        if (policy_state(e, e->env.n, true)) return -1;
    }
    return 0;
}
int ep_mirror_push(dqn_engine* e) {
    const int cur[2] = {(int)e->ep_widx, (int)e->ep_size};
    HIPCHK(hipMemcpyAsync(e->ep_stage.cur, cur, sizeof cur, hipMemcpyHostToDevice, e->stream)); HIPCHK(hipStreamSynchronize(e->stream));      // cur lives in this scope
    return 0;
}
int ep_mirror_pull(dqn_engine* e) {
    std::vector<int> b((size_t)e->ep_cap + 2);
    HIPCHK(hipMemcpyAsync(b.data(), e->ep_len, b.size() * 4, hipMemcpyDeviceToHost, e->stream)); HIPCHK(hipStreamSynchronize(e->stream));
    for (long long i = 0; i < e->ep_cap; i++) e->ep_len_host[(size_t)i] = b[(size_t)i];
    e->ep_widx = b[(size_t)e->ep_cap]; e->ep_size = b[(size_t)e->ep_cap + 1];
    return 0;
}
// the Recur state an acting program of a recurrent engine carries: the policy state (training copies) or the evaluation set's private one
static RecurState recur_state(dqn_engine* e, bool eval) {
    RecurState R; memset(&R, 0, sizeof R);
    for (int i = 0; i < e->nl; i++) if (is_recurrent(e->L[i].kind)) {
        const int k = R.nrec++; const bool has_c = cell_ops(e->L[i].kind)->has_c;
        R.H[k] = e->L[i].H; R.h[k] = eval ? e->eval_h[i] : e->pol_h[i][e->pol_flip]; R.c[k] = has_c ? (eval ? e->eval_c[i] : e->pol_c[i][e->pol_flip]) : nullptr;
        R.h0[k] = e->p_on + e->L[i].h0_off; R.c0[k] = has_c ? e->p_on + e->L[i].c0_off : nullptr;
    }
    return R;
}
// the acting program of a recurrent engine: what policy_forward does on n streams (the same launchers under the same plan: the forward of a copy is, bit for bit,
// dqn_forward on a stream reset at the same points), with the state in ONE buffer set so that the step replays as a graph -- the cell writes h_t into the layer's
// activation and c_t over c_{t-1} (element-wise: each thread reads and writes its own element), then h_t is copied over h_{t-1}.
//   k_recur_reset (copies whose episode ended) | layers | k_env_step_rec (Q, argmax, eps-greedy, act!, staging of a / r / done) | k_env_observe_rec | k_ep_commit, k_ep_advance
static int emit_act_program_rec(dqn_engine* e, dqn_engine::ActProg& ap, const EnvDev& V, RolloutDev* rs) {
    const int n = V.n; const bool eval = V.eval_mode != 0;
    const bool mf = e->hp.use_mfma != 0; const float* P = e->p_on;
    const RecurState RS = recur_state(e, eval); const EnvDev Vc = V; const EpStage ES = e->ep_stage;
    if (!eval) ap.steps.push_back({"recur_reset", [=](dqn_engine* en) { launch_recur_reset(en->stream, Vc.pending, n, RS); }});
    int k = 0;
    for (int i = 0; i < e->nl; i++) {
        const LayerDev l = e->L[i]; const float* X = l.src < 0 ? e->pol_x : e->pol_act[l.src]; float* Y = e->pol_act[i];
        if (is_do(l.kind)) continue;      // a Dropout layer is the identity when acting: nothing is emitted, pol_act[i] is its producer's
        const float* X2 = is_skip(l.kind) ? e->pol_act[l.src2] : nullptr;      // a skip join adds the output of the block's entry
        if (!is_recurrent(l.kind)) { ap.steps.push_back({pname(e, "act_fwd", l, i), [=](dqn_engine* en) { launch_layer_fwd(en->stream, l, P, X, n, 0, n, Y, mf, 0, nullptr, en->partials, X2, n); }}); continue; }
        const CellOps* C = cell_ops(l.kind);
        const LayerDev Vw = gx_view(l);
        float* gx = eval ? e->eval_gx[i] : e->pol_gx[i]; float* h = RS.h[k]; float* c = RS.c[k]; k++;
        ap.steps.push_back({pname(e, "act_gx", l, i), [=](dqn_engine* en) { launch_layer_fwd(en->stream, Vw, P, X, n, 0, n, gx, mf, 0, nullptr, en->partials); }});
        CellFwdArgs a; memset(&a, 0, sizeof a); a.H = l.H; a.B = n; a.T = 1; a.nseq = 1; a.act = l.cell_act;
        CellSeq& q = a.s[0]; q.Gx = gx; q.Hout = Y; q.ld = n; q.c0 = 0; q.Wh = P + l.wh_off; q.bias = P + l.b_off; q.hprev = h; q.hp_ld = n; q.hp_bs = 1;
        if (C->has_c) { q.Cst = c; q.cprev = c; q.cp_ld = n; q.cp_bs = 1; }
        ap.steps.push_back({pname(e, "act_cell", l, i), [=](dqn_engine* en) { C->launch_step(en->stream, a, 0); launch_state_copy(en->stream, Y, h, l.H * n); }});
    }
    const int lq = e->hp.dueling ? e->last_adv : e->last_base;
    auto head_of = [&](int l) { HeadSrc h; h.p = e->pol_act[l]; h.ld = n; h.S = 1; h.per_s = 0; h.bias = P + e->L[l].b_off; h.act = e->L[l].act; return h; };
    ActHeads Hd; memset(&Hd, 0, sizeof Hd); Hd.adv = head_of(lq); if (e->hp.dueling) Hd.val = head_of(e->last_val); Hd.dueling = e->hp.dueling; Hd.q_out = e->pol_q; Hd.amax = e->pol_a;
    float* px = e->pol_x;
    ap.steps.push_back({"env_step_stage", [=](dqn_engine* en) { launch_env_step_rec(en->stream, Vc, rs, Hd, ES); }});
    ap.steps.push_back({"env_observe_stage", [=](dqn_engine* en) { launch_env_observe_rec(en->stream, Vc, rs, ES, px); }});
    if (!eval) ap.steps.push_back({"episode_commit", [=](dqn_engine* en) { launch_ep_commit(en->stream, Vc, ES); }});
    ap.fused_tail = false; return 0;
}
// THE description of the engine's transition ring the acting tails write into (emit_act_program, tiny_act_record of engine_group.hip)
ReplayMeta replay_meta(const dqn_engine* e) { return ReplayMeta{e->cap, e->cap2, e->ra, e->rr, e->rdone, e->tree, e->state, e->hp.prio_eps, e->hp.prio_alpha}; }
// the acting program: online net forward on the n columns of pol_x (batch-innermost), then Q columns + first-max argmax
// (action(policy, obs), src/policy.jl:38-64) -- the train step's forward emitter (emit_forward, engine_program.hip) with one pass: the same tiled kernels, plan and
// selection rules, compiled once per n
// general: keep the four-launch tail where the fused one would apply (a rollout that explores by table)
static int emit_act_program(dqn_engine* e, dqn_engine::ActProg& ap, const EnvDev& V, RolloutDev* rs, bool general) {
    const int n = V.n;
    const Levels levels = net_levels(e);
    const float* P = e->p_on;
    HeadSrc head[DQN_MAX_LAYERS][2];      // [layer][0]: the acting forward is one pass
    // the fused tail (act_head.hip): reduce of the heads' producers + heads + Q / argmax + eps-greedy + act! + add_exp!'s per-experience part in ONE launch, where the shapes allow
    // (the layout of the train step's fused reduce + head launch, fused_head_layout, + this kernel's own test); else k_reduce_multi + the heads' forward + k_env_step
    const int lq = e->hp.dueling ? e->last_adv : e->last_base, lvh = e->hp.dueling ? e->last_val : -1;
    const bool builtin_env = env_is_builtin(V.kind);      // k_act_head steps the two built-in kinds only: a tabular or a control set keeps the general four-launch tail
    // ... and so does a network with a padded conv, a LayerNorm layer, a Dropout layer (nothing is emitted for the layer itself) or a skip block (common.h general_only): fused_tail = 0
    bool use_ah = !general && !e->opt.no_act_head && !general_only(e->L, e->nl, true) && builtin_env; int ah_pa = -1, ah_pv = -1, ah_S = 0;
    if (use_ah) { ah_S = fused_head_layout(e, levels, lq, lvh, &ah_pa, &ah_pv); use_ah = ah_S > 0 && act_head_ok(n, e->L[lq].K, ah_S, e->nA, lvh >= 0 ? 2 : 1, e->L[lq].N, lvh >= 0 ? e->L[lvh].N : 0); }
    // one pass on the n columns of pol_x; the last level's consumer (k_env_step) reduces split-K slabs on the fly; no transposed copies, no byte arena, no LayerNorm statistics
    FwdEmit fe; fe.gemm = "act_fwd"; fe.valu = "act_fwd_valu"; fe.reduce = "act_reduce"; fe.skip_last = use_ah /* the head level runs inside k_act_head */; fe.last_on_the_fly = true; fe.head = head;
    if (use_ah) { fe.prod[0] = ah_pa; fe.prod[1] = ah_pv; fe.pm_ok = ah_S > 1 && !e->opt.no_rh_pm; }
    emit_forward(e, levels, 0, levels.size(), {{P, e->pol_x, n, 0, e->pol_act, e->pol_act, n, "act_fwd"}}, fe);
    const ReplayMeta R = replay_meta(e);
    const bool u8 = e->hp.obs_dtype == DQN_OBS_U8;
    void *srows = e->s_rows, *sprows = e->sp_rows; float* px = e->pol_x; const long long cap = e->cap; const EnvDev Vc = V;
    if (use_ah) {
        ActHeadArgs h; memset(&h, 0, sizeof h);
        const LayerDev& La = e->L[lq];
        h.n = n; h.nA = e->nA; h.K = La.K; h.S = ah_S; h.nstream = lvh >= 0 ? 2 : 1; h.NO = e->nA + (lvh >= 0 ? 1 : 0); h.pm = fe.pm ? 1 : 0;
        for (int st = 0; st < 2; st++) {
            const int hl_ = (st == 1 && lvh >= 0) ? lvh : lq, pl_ = (st == 1 && lvh >= 0) ? ah_pv : ah_pa; const LayerDev& H = e->L[hl_]; const LayerDev& Pl = e->L[pl_]; ActHeadStream& T = h.st[st];
            T.part = fe.part[(st == 1 && lvh >= 0) ? 1 : 0][0]; T.pbias = P + Pl.b_off; T.pact = Pl.act; T.W = P + H.w_off; T.hbias = P + H.b_off; T.N = H.N; T.hact = H.act;
        }
        const int Gc = n / 4, NC = La.K / 32;
        h.partials = palloc(e, (size_t)Gc * 4 * h.NO * NC); h.tickets = (unsigned*)palloc(e, (size_t)Gc);
        if (!h.tickets) return -1;      // (refused: the message is the scope's)
        HIPCHK(hipMemsetAsync(h.tickets, 0, (size_t)Gc * 4, e->stream));
        h.q_out = e->pol_q; h.amax = e->pol_a; h.rs = rs; h.V = V; h.R = R;
        ap.steps.push_back({"act_head_step", [=](dqn_engine* en) { launch_act_head(en->stream, h); }});
        ap.steps.push_back({"env_observe_tree", [=](dqn_engine* en) { launch_env_observe2(en->stream, Vc, rs, u8, srows, sprows, cap, px, 1, &R); }});
        ap.fused_tail = true; return 0;
    }
    ap.fused_tail = false;
    ActHeads Hd; memset(&Hd, 0, sizeof Hd); Hd.adv = head[lq][0]; if (e->hp.dueling) Hd.val = head[e->last_val][0]; Hd.dueling = e->hp.dueling; Hd.q_out = e->pol_q; Hd.amax = e->pol_a;
    // act!, add_exp!, observe, episode bookkeeping
    ap.steps.push_back({"env_step_commit", [=](dqn_engine* en) { launch_env_step(en->stream, Vc, rs, Hd, R); }});
    ap.steps.push_back({"env_observe", [=](dqn_engine* en) { launch_env_observe2(en->stream, Vc, rs, u8, srows, sprows, cap, px); }}); return 0;
}
// the acting program of V in ap, rebuilt when n or (recurrent engines) the Recur state it reads moved.  A refusal -- an emitter's, or an allocation of its scope refused below -- leaves ap empty, the sinks the step program's again
static int build_act_program(dqn_engine* e, dqn_engine::ActProg& ap, const EnvDev& V, RolloutDev* rs, bool general = false) {
    const int n = V.n; const bool rec = e->hp.recurrence != 0, eval = V.eval_mode != 0; const int gen = !rec ? -1 : eval ? -2 : e->pol_state_gen, flip = !rec ? -1 : eval ? 0 : e->pol_flip;      // (-1: ActProg's own initial values)
    if (ap.n == n && ap.state_gen == gen && ap.state_flip == flip) return 0;
    if (policy_ws(e, std::max(n, std::max(e->env.n, e->eval_n)))) return -1;      // one workspace serves both env sets (no realloc when they alternate)
    drop_act(e, ap); e->prog_names.reserve(512); e->sink = &ap.steps; e->alloc_sink = &ap.mem;
    int rc = rec ? emit_act_program_rec(e, ap, V, rs) : emit_act_program(e, ap, V, rs, general);      // act_head.hip and the GEMM grouping stay feed-forward only
    e->sink = nullptr; e->alloc_sink = nullptr;
    if (!rc && ap.mem.failed) { const std::string why = dqn_last_error(); rc = fail("build_act_program: a device allocation failed (%s)", why.c_str()); }
    if (rc) { drop_act(e, ap); return -1; }
    ap.n = n; ap.state_gen = gen; ap.state_flip = flip; return 0;
}
static int act_graph(dqn_engine* e, dqn_engine::ActProg& ap) {
    if (ap.graph) return 0;
    return capture_graph(e, "the acting step", [&]() { for (auto& s : ap.steps) s.fn(e); return 0; }, &ap.graph);
}
// F acting steps (+ one plain sampled train step) as one graph
static int cycle_graph(dqn_engine* e, dqn_engine::ActProg& ap, int F, bool with_train) {
    if (ap.cycle && ap.cycle_F == F && ap.cycle_train == with_train) return 0;
    if (ap.cycle) { hipGraphExecDestroy(ap.cycle); ap.cycle = nullptr; }
    if (capture_graph(e, "the rollout cycle", [&]() { for (int f = 0; f < F; f++) for (auto& s : ap.steps) s.fn(e); if (with_train) enqueue_step(e, StepKey()); return 0; }, &ap.cycle)) return -1;
    ap.cycle_F = F; ap.cycle_train = with_train; return 0;
}
// one vector step of the reference's cadence (src/solver.jl:136-140: a train step every train_freq ENV steps) as ONE graph: the acting step, then its `due` train steps
// back to back with the pipelined gather of dqn_train_steps (step i's Adam launch gathers step i + 1's batch) -- one graph launch instead of the acting graph + the
// first / grouped / last graphs of a dqn_train_steps(due) call
static int envc_graph(dqn_engine* e, dqn_engine::ActProg& ap, int due) {
    if (ap.envc && ap.envc_due == due) return 0;
    if (ap.envc) { hipGraphExecDestroy(ap.envc); ap.envc = nullptr; }
    const bool pg = e->pg_ok;
    if (capture_graph(e, "the env-cadence cycle", [&]() {
            for (auto& s : ap.steps) s.fn(e);
            for (int i = 0; i < due; i++) { StepKey k; k.take_pre = pg && i > 0; k.pregather = pg && i + 1 < due; enqueue_step(e, k); }
            return 0; }, &ap.envc)) return -1;
    ap.envc_due = due; return 0;
}
// dqn_rollout_explore's table.  explore_check refuses before anything is enqueued; explore_upload copies the values into the engine's buffer (grown on demand) and
// names them in the record every RolloutDev of the call is copied from.  x == nullptr: the linear law (xtab stays null)
int explore_check(const dqn_exploration* x, int n_steps) {
    if (!x) return 0;
    if (x->kind != DQN_EXPLORE_EPS_GREEDY && x->kind != DQN_EXPLORE_SOFTMAX) return fail("exploration: unknown kind %d (0: eps-greedy, 1: softmax)", x->kind);
    if (x->n_values != 1 && x->n_values != n_steps) return fail("exploration: n_values = %d is neither 1 nor n_vector_steps = %d", x->n_values, n_steps);
    if (!x->values) return fail("exploration: values is NULL (n_values = %d)", x->n_values);
    for (int j = 0; j < x->n_values; j++) {
        const float v = x->values[j];
        if (x->kind == DQN_EXPLORE_EPS_GREEDY && !(v >= 0.0f && v <= 1.0f)) return fail("exploration: eps values[%d] = %g is outside [0, 1]", j, (double)v);
        if (x->kind == DQN_EXPLORE_SOFTMAX && !(v > 0.0f && std::isfinite(v))) return fail("exploration: temperature values[%d] = %g is not a finite positive number", j, (double)v);
    }
    return 0;
}
static int explore_upload(dqn_engine* e, const dqn_exploration* x, long long t0, RolloutDev& h) {
    if (!x) return 0;
    const size_t m = (size_t)x->n_values;
    if (m > e->xtab_cap) { HIPCHK(hipStreamSynchronize(e->stream)); if (grow(e->env_mem, &e->xtab, &e->xtab_cap, m, 256)) return -1; }
    HIPCHK(hipMemcpyAsync(e->xtab, x->values, m * sizeof(float), hipMemcpyHostToDevice, e->stream)); HIPCHK(hipStreamSynchronize(e->stream));      // the caller's array is not kept
    h.xkind = x->kind; h.xtab = e->xtab; h.xtab_t0 = t0; h.xtab_n = x->n_values;
    return 0;
}
// THE RolloutDev record a call starts from: the step counter, the ring cursor behind which the first vector step writes (a recurrent engine keeps no host ring
// cursor: its episode ring's is on the device, ep_mirror_push) and the linear eps law.  cfg == NULL: the greedy record of an evaluation (t = 0, the schedule (0, 0, 1))
RolloutDev rollout_record(const dqn_rollout_cfg* cfg, const dqn_engine* e) {
    RolloutDev h; memset(&h, 0, sizeof h);
    if (!cfg) { h.eps_steps = 1.0f; return h; }
    h.t = cfg->t0 - 1; h.eps_start = cfg->eps_start; h.eps_stop = cfg->eps_stop; h.eps_steps = cfg->eps_steps;
    if (!e->hp.recurrence) { const int n = e->env.n; h.widx = ((e->widx - n) % e->cap + e->cap) % e->cap; }
    return h;
}
// ... uploaded as the DQN_ROLL_RECORDS records of an env set: one per group of four copies (k_act_head ticks its group's), record 0 = the four-launch tail's.  The
// synchronise that keeps the host copies alive is this function's -- or, mirror: ep_mirror_push's, which sends the host's episode cursor behind the records
static int roll_upload(dqn_engine* e, RolloutDev* dev, const RolloutDev& h, bool mirror) {
    const std::vector<RolloutDev> hs(DQN_ROLL_RECORDS, h);
    HIPCHK(hipMemcpyAsync(dev, hs.data(), sizeof(RolloutDev) * DQN_ROLL_RECORDS, hipMemcpyHostToDevice, e->stream));
    if (mirror) return ep_mirror_push(e);
    HIPCHK(hipStreamSynchronize(e->stream)); return 0;
}
// THE way a vector step is enqueued (the rollouts, dqn_evaluate): the program's graph, else its launches inside profiling brackets
static int act_step(dqn_engine* e, dqn_engine::ActProg& ap, bool graph) {
    if (graph) HIPCHK(hipGraphLaunch(ap.graph, e->stream)); else for (auto& s : ap.steps) RUN(e, s.name, s.fn(e));
    return 0;
}
// the statistics of a rollout call: the episodes finished and their rewards, summed in copy order, beside the last train step's scalars.  Where the two engine kinds
// synchronise differs and is kept: a recurrent engine pulls the episode mirror (dqn_episode_export / dqn_get_counters describe the committed ring) whether or not
// the caller wants statistics, and that pull is its synchronise; a feed-forward engine synchronises only for a caller who does (fetch_scalars, or the stream)
static int rollout_stats(dqn_engine* e, long long trained, dqn_rollout_stats* out) {
    const EnvDev& V = e->env; const int n = V.n; const bool rec = e->hp.recurrence != 0;
    std::vector<long long> fe(n); std::vector<double> fr(n);
    if (out || rec) {
        HIPCHK(hipMemcpyAsync(fe.data(), V.fin_eps, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(fr.data(), V.fin_reward, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
    }
    if (rec && ep_mirror_pull(e)) return -1;
    if (!out) return 0;
    out->last_loss = out->last_grad_norm = 0.0f;
    if (trained) { if (fetch_scalars(e, &out->last_loss, &out->last_grad_norm)) return -1; } else if (!rec) HIPCHK(hipStreamSynchronize(e->stream));
    out->episodes = 0; out->reward_sum = 0.0; out->train_steps = trained;
    for (int i = 0; i < n; i++) { out->episodes += fe[i]; out->reward_sum += fr[i]; }
    return 0;
}
// the `due` train steps behind a PLAIN unit, where the replay holds a batch; *trained counts them.  A feed-forward engine: the sampled step, or dqn_train_steps back to
// back under the env-step cadence (the pipelined gather applies).  A recurrent engine draws on the host (SplitMix), so its mirror of the episode ring is refreshed
// from the device before the draw; the train step works on its own sequence buffers and leaves the policy's Recur state alone (src/solver.jl:137-139)
static int rollout_train(dqn_engine* e, bool envc, long long due, long long* trained) {
    if (due <= 0) return 0;
    if (e->hp.recurrence) {
        if (ep_mirror_pull(e)) return -1;
        if (e->ep_size < e->B) return 0;
        if (envc ? drqn_train_steps(e, (int)due, nullptr, nullptr) : dqn_train_step_drqn(e, nullptr, nullptr, nullptr, nullptr)) return -1;
    } else {
        if (e->size < e->B) return 0;
        if (envc ? dqn_train_steps(e, (int)due, nullptr, nullptr) : run_step(e, true)) return -1;     // :134-139
    }
    *trained += due; return 0;
}
extern "C" int dqn_rollout(dqn_engine_t* e, int n_steps, const dqn_rollout_cfg* cfg, dqn_rollout_stats* out) { return dqn_rollout_explore(e, n_steps, cfg, nullptr, out); }
// THE rollout driver, feed-forward and recurrent engines: a prologue (refusals, programs, the call's record and table, the first observe, the acting graph), a loop
// over the units rollout_sched.h chooses, an epilogue (pending resets, statistics).  x == NULL: dqn_rollout.  Else the exploration table is validated (nothing is
// enqueued by a refused call), uploaded, and named by the RolloutDev records.  A recurrent engine differs in named places only: its refusals and policy_state here,
// the mirror push in roll_upload, no ring cursor (rollout_record, the loop), PLAIN units only (rollout_unit), rollout_train, the recur_reset before the last env
// reset, the mirror pull in rollout_stats
extern "C" int dqn_rollout_explore(dqn_engine_t* e, int n_steps, const dqn_rollout_cfg* cfg, const dqn_exploration* x, dqn_rollout_stats* out) { if (!e) return fail("null engine handle");
    HIPCHK(hipSetDevice(e->device));
    if (!e->has_envs) return fail("no device environments: call dqn_envs_create");
    if (cfg->t0 < 1) return fail("t0 counts from 1 (src/solver.jl:82)");
    if (explore_check(x, n_steps)) return -1;
    EnvDev& V = e->env; const int n = V.n; const bool rec = e->hp.recurrence != 0;
    if (rec) {
        if (e->ep_cur_len > 0) return fail("an episode is open on the host side (dqn_episode_add without its terminal transition): finish it or call dqn_episode_commit before dqn_rollout");
        if (e->comm) return fail("device environments on a recurrent engine are single-device: this engine has a communicator");
        if (policy_state(e, n, false)) return -1;      // (the host ran another stream count in between: n streams again, at state0)
    }
    if (build_act_program(e, e->act, V, e->roll)) return -1;
    // a table is read by the general tail only: where the set's program has the fused one, its general twin runs this call (both stay built)
    if (x && e->act.fused_tail && build_act_program(e, e->act_gen, V, e->roll, true)) return -1;
    dqn_engine::ActProg& act = (x && e->act.fused_tail) ? e->act_gen : e->act;
    if (cfg->train_freq > 0 && build_program(e)) return -1;       // may reallocate split-K workspaces: before any capture
    RolloutDev h = rollout_record(cfg, e);
    if (explore_upload(e, x, cfg->t0, h) || roll_upload(e, e->roll, h, rec)) return -1;
    launch_env_observe(e->stream, V, nullptr, 0, e->pol_x);
    const bool graph = e->hp.use_graph && !e->profiling;
    if (graph && act_graph(e, act)) return -1;
    // whole cycles -- train_freq acting steps ending on a train step (or 4 acting steps when nothing trains) -- and whole vector steps of the env-step cadence replay
    // as ONE graph where the schedule allows it (rollout_unit); d: what is due behind the unit's last step
    RollFacts f; f.graph = graph; f.single = e->world <= 1 && !(e->comm && e->force_comm); f.tiny = e->tiny; f.rec = rec; f.n = n; f.cap = e->cap; f.B = e->B;
    const int F = rollout_cycle_len(*cfg); const bool envc = cfg->cadence_env_steps != 0;
    long long trained = 0;
    for (int k = 0, len = 1; k < n_steps; k += len) {
        const long long t = cfg->t0 + k;
        f.left = n_steps - k; f.size = e->size;
        const RollUnit u = rollout_unit(*cfg, t, f);
        len = u == ROLL_CYCLE ? F : 1;
        const RollDue d = rollout_due(*cfg, t + len - 1, n);
        if (u == ROLL_ENVC) { if (envc_graph(e, act, (int)d.due)) return -1; HIPCHK(hipGraphLaunch(act.envc, e->stream)); }
        else if (u == ROLL_CYCLE) { if (cycle_graph(e, act, F, d.due > 0)) return -1; HIPCHK(hipGraphLaunch(act.cycle, e->stream)); }
        else if (act_step(e, act, graph)) return -1;
        if (!rec) ring_advance(e, (long long)len * n);
        if (u != ROLL_PLAIN) trained += d.due;      // (inside the unit's graph)
        else if (rollout_train(e, envc, d.due, &trained)) return -1;
        if (d.sync && dqn_sync_target(e)) return -1;      // :142-145
    }
    if (n_steps > 0) e->env_q_valid = true;      // pol_q / pol_a: the last vector step's (dqn_envs_peek_q)
    if (rec) launch_recur_reset(e->stream, V.pending, n, recur_state(e, false));      // resetstate!(policy) of the copies whose episode ended in the last step, then their env reset
    launch_env_reset_pending(e->stream, V, e->roll, 0);      // episode bookkeeping of the last step (src/solver.jl:99-132)
    return rollout_stats(e, trained, out);
}
// the evaluation copies of an engine: n_eval copies of the training MDP with per-copy arrays of their own (the images, the spec and the tables are the training
// set's), allocated on first use and again when n_eval changes.  dqn_evaluate and dqn_evaluate_many (engine_group.hip) step the same set
int eval_envs_ensure(dqn_engine* e, int n_eval) {
    EnvDev& W = e->eval_env;
    if (e->eval_n == n_eval) return 0;
    HIPCHK(hipStreamSynchronize(e->stream)); drop_act(e, e->evalp); free_eval_envs(e);
    W = e->env; W.n = n_eval; W.eval_mode = 1; DevScope& M = e->eval_mem;
    if (env_copy_state(M, W, n_eval, e->stream)) return -1;      // (the tables, constants and images stay the training set's)
    DM(M, e->eval_roll, DQN_ROLL_RECORDS);
    for (int i = 0; i < e->nl; i++) if (is_recurrent(e->L[i].kind)) {      // recurrent engines: the evaluation copies' private Recur state, n_eval streams
        DM(M, e->eval_h[i], (size_t)e->L[i].H * n_eval); if (cell_ops(e->L[i].kind)->has_c) DM(M, e->eval_c[i], (size_t)e->L[i].H * n_eval); DM(M, e->eval_gx[i], (size_t)e->L[i].N * n_eval);
    }
    e->eval_n = n_eval;
    return 0;
}
// basic_evaluation (src/evaluation_policy.jl:17-42) on the device: n_eval copies of the training MDP run one greedy episode each
// (while !done && step <= max_episode_length), rewards summed in Float64 like the reference's r_tot; returns the averages.
extern "C" int dqn_evaluate(dqn_engine_t* e, int n_eval, int max_episode_length, uint64_t seed, double* avg_reward, double* avg_steps) { if (!e) return fail("null engine handle");
    HIPCHK(hipSetDevice(e->device));
    if (!e->has_envs) return fail("no device environments: call dqn_envs_create (the evaluation copies share its MDP)");
    if (n_eval < 1 || n_eval > 1024) return fail("n_eval must be in 1..1024");
    if (max_episode_length < 1) return fail("max_episode_length must be >= 1");
    if (eval_envs_ensure(e, n_eval)) return -1;
    EnvDev& W = e->eval_env;
    for (int i = 0; i < e->nl; i++) if (e->eval_h[i]) {      // resetstate!(policy) of the evaluation: state0 of the online net on every stream
        launch_bcast_state(e->stream, e->p_on + e->L[i].h0_off, e->L[i].H, n_eval, e->eval_h[i]);
        if (e->eval_c[i]) launch_bcast_state(e->stream, e->p_on + e->L[i].c0_off, e->L[i].H, n_eval, e->eval_c[i]);
    }
    if (W.seed != seed || W.max_episode_length != max_episode_length) { W.seed = seed; W.max_episode_length = max_episode_length; drop_act(e, e->evalp); }   // baked into the program
    if (build_act_program(e, e->evalp, W, e->eval_roll)) return -1;
    e->env_q_valid = false;      // the evaluation copies' forward writes pol_q / pol_a (dqn_envs_peek_q is refused until the training set steps again)
    if (roll_upload(e, e->eval_roll, rollout_record(nullptr, e), false)) return -1;      // always greedy
    HIPCHK(hipMemsetAsync(W.fin_reward, 0, (size_t)n_eval * 8, e->stream));
    launch_env_reset_pending(e->stream, W, e->eval_roll, 1);                   // reset!(env), resetstate!(policy)
    launch_env_observe(e->stream, W, nullptr, 0, e->pol_x);
    const bool graph = e->hp.use_graph && !e->profiling;
    if (graph && act_graph(e, e->evalp)) return -1;
    std::vector<unsigned char> pend(n_eval);
    for (int k = 0; k <= max_episode_length; k++) {
        if (act_step(e, e->evalp, graph)) return -1;
        if ((k & 7) == 7) {     // every 8 vector steps: stop early once every episode is over
            HIPCHK(hipMemcpyAsync(pend.data(), W.pending, n_eval, hipMemcpyDeviceToHost, e->stream)); HIPCHK(hipStreamSynchronize(e->stream));
            bool alive = false; for (int i = 0; i < n_eval; i++) alive = alive || !pend[i];
            if (!alive) break;
        }
    }
    std::vector<double> fr(n_eval); std::vector<int> st(n_eval);
    HIPCHK(hipMemcpyAsync(fr.data(), W.fin_reward, (size_t)n_eval * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(st.data(), W.ep_step, (size_t)n_eval * 4, hipMemcpyDeviceToHost, e->stream)); HIPCHK(hipStreamSynchronize(e->stream));
    double r = 0.0, s = 0.0;
    for (int i = 0; i < n_eval; i++) { r += fr[i]; s += (double)st[i]; }      // avg_r += r_tot; avg_steps += step, episode order
    if (avg_reward) *avg_reward = r / n_eval;
    if (avg_steps) *avg_steps = s / n_eval;
    return 0;
}
extern "C" int dqn_envs_info(dqn_engine_t* e, int* n_envs, int* fused_tail) { if (!e) return fail("null engine handle");
    HIPCHK(hipSetDevice(e->device));
    if (!e->has_envs) return fail("no device environments: call dqn_envs_create");
    if (build_act_program(e, e->act, e->env, e->roll)) return -1;
    if (n_envs) *n_envs = e->env.n;
    if (fused_tail) *fused_tail = e->act.fused_tail ? 1 : 0;
    return 0;
}
extern "C" int dqn_envs_peek(dqn_engine_t* e, float* obs, int32_t* actions, float* rewards, uint8_t* dones) { if (!e) return fail("null engine handle");
    HIPCHK(hipSetDevice(e->device));
    if (!e->has_envs) return fail("no device environments: call dqn_envs_create");
    EnvDev& V = e->env; const int n = V.n;
    if (obs) {
        if (policy_ws(e, n)) return -1;
        launch_env_observe(e->stream, V, nullptr, 0, e->pol_x);
        std::vector<float> x((size_t)e->E * n); HIPCHK(hipMemcpyAsync(x.data(), e->pol_x, x.size() * 4, hipMemcpyDeviceToHost, e->stream)); HIPCHK(hipStreamSynchronize(e->stream));
        for (int i = 0; i < n; i++) for (int f = 0; f < e->E; f++) obs[(size_t)i * e->E + f] = x[(size_t)f * n + i];
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    if (actions) HIPCHK(hipMemcpy(actions, V.actions, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (rewards) HIPCHK(hipMemcpy(rewards, V.rewards, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (dones) HIPCHK(hipMemcpy(dones, V.dones, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}
// read-only: what the acting forward of the training set's last vector step left in pol_q / pol_a.  Nothing is launched, nothing is rewritten
extern "C" int dqn_envs_peek_q(dqn_engine_t* e, float* q, int32_t* greedy) { if (!e) return fail("null engine handle");
    HIPCHK(hipSetDevice(e->device));
    if (!e->has_envs) return fail("no device environments: call dqn_envs_create");
    if (!e->env_q_valid) return fail("dqn_envs_peek_q: the env set has not taken a vector step since it was created, or the policy workspace was used since its last one "
                                     "(dqn_forward, dqn_greedy_action, dqn_evaluate): call dqn_rollout first");
    const int n = e->env.n;
    HIPCHK(hipStreamSynchronize(e->stream));
    if (q) HIPCHK(hipMemcpy(q, e->pol_q, (size_t)n * e->nA * 4, hipMemcpyDeviceToHost));
    if (greedy) HIPCHK(hipMemcpy(greedy, e->pol_a, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

