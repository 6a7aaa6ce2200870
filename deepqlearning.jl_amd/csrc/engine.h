// engine.h -- internal header of libdqn_mi355x.so's host side: the engine record, error/alloc helpers and the functions the
// translation units engine.hip (ABI core, graphs, policy), engine_layers.hip (build_layers), engine_program.hip (static launch program of the train step),
// engine_drqn.hip (EpisodeReplayBuffer + recurrent step), engine_envs.hip (device-resident environments: env sets, acting programs, the rollout driver, evaluation)
// and engine_group.hip (dqn_group_*: the group frame, grouped train steps, rollouts and evaluation) share.  rollout_sched.h: the rollout cadence (no HIP).
#pragma once
#include <dlfcn.h>
#include <limits.h>
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <functional>
#include <string>
#include <vector>
#include "common.h"
#include "devmem.h"
#include "rollout_sched.h"

#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail("HIP error %s at %s:%d (%s)", hipGetErrorString(_e), __FILE__, __LINE__, #x); } while (0)

// ---------------------------------------------------------------- engine
struct ProfEntry { const char* name; hipEvent_t a, b; };

// Experiment / test switches.  Read ONCE from the environment of the call that creates the engine (read_opts, engine.hip -- the only getenv site of the
// library besides trace builds), kept in the engine: no function-local statics, nothing process-wide, a second engine in the same process never inherits the
// first one's switches.  The communicator switches (force_allreduce, dp_*) are re-read by dqn_comm_init, the call that makes them meaningful.
struct EngineOpts {
    int no_tiny = 0;              // DQN_NO_TINY: networks that fit in LDS take the multi-launch program
    int fwd_m32 = -1 /* -1: large launches only */, no_fwd_wres = 0;      // DQN_FWD_M32 / DQN_NO_FWD_WRES -> LayerDev::opt bits
    int sim_world = 0;            // DQN_SIM_WORLD=k: one process plays k ranks (tests)
    int no_act_head = 0;          // DQN_NO_ACT_HEAD (A/B, both schedules under test): the acting step keeps k_reduce_multi + heads + k_env_step where the fused tail (act_head.hip) would apply
    int no_rh_pm = 0;             // DQN_NO_RH_PM (A/B, r06): the hidden layers' split-K slabs stay [S][N][columns] where k_red_head reads them (default: piece-major, GFwdProb::pm)
    int dw_split = 128;            // DQN_DW_SPLIT=n: the last n units of a large-batch dW section run as two halves along N (nn_gemm.hip dw_section; 0 = off; LayerDev::opt bits 8..15 in units of 16)
    int no_head_cols4 = 0;        // DQN_NO_HEAD_COLS4=1: keep k_head_td (one workgroup per column) at large batches where k_head_cols4 (red_head.hip) would apply (A/B); =2: k_head_cols4 without the transposed copies (its fallback loader, under test)
    int no_red_head = 0;          // DQN_NO_RED_HEAD: keep k_reduce_multi + k_head_td where the fused reduce + head launch (red_head.hip) would apply (A/B, both schedules under test)
    int no_pregather = 0;         // DQN_NO_PREGATHER: dqn_train_steps keeps the gather launch in every step (A/B)
    int gru_stepwise = 0;         // DQN_GRU_STEPWISE: GRU layers take the per-step recurrence / BPTT launches where the whole-sequence kernels would apply (both schedules under test)
    int no_skip_fuse = 0;         // DQN_NO_SKIP_FUSE: a convolutional skip block keeps the join's launches of its own (skip.hip) where the residual epilogues of conv_own.hip would apply (both schedules under test: the same bits)
    int rnn_stepwise = 0;         // DQN_RNN_STEPWISE: RNN layers take the per-step recurrence / BPTT launches where the whole-sequence kernels would apply (both schedules under test)
    int force_allreduce = 0, dp_allreduce = 0, dp_overlap = -1 /* -1: decided from world size and bytes (engine_program.hip) */, dp_no_one_graph = 0;      // DQN_FORCE_ALLREDUCE / DQN_DP_ALLREDUCE / DQN_DP_OVERLAP / DQN_DP_NO_ONE_GRAPH
    // timing probes (wrong numbers, right schedule) and stamps
    int head_dbg = 0, probe_no_tg = 0, drqn_probe = 0, drqn_stamps = 0, tiny_stop = 0;
};
void read_opts(EngineOpts& o, bool comm_only = false);
// the per-step recurrence / BPTT launches are forced where the cell's whole-sequence kernels would apply (the LSTM has no such switch)
static inline bool stepwise(const EngineOpts& o, int kind) { return kind == DQN_LAYER_GRU ? o.gru_stepwise != 0 : kind == DQN_LAYER_RNN ? o.rnn_stepwise != 0 : false; }

enum { PH_ALL = 0, PH_PRE = 1, PH_POST = 2, PH_PRE1 = 3, PH_PRE2 = 4, PH_DP_ONE = 5 };      // PRE = PRE1 (up to the point where the wide layers' operands are final) + PRE2 (the rest of the backward pass)
// One variant of the train step: what enqueue_step enqueues and what names its graph in the engine's cache (get_or_capture keeps, per phase, only the fields that phase reads).
// take_pre / pregather (common.h PreGather, only between the steps of one dqn_train_steps call): this step runs without its gather launch / its Adam launch gathers the
// next batch.  publish: the step's last launch writes (loss, grad_norm) into the host mailbox.  repeat: steps back to back in one graph.  slot: the first draw slot of the
// fused recurrent step (a launch parameter, step r of the key reads slot + r).
struct StepKey {
    int phase = PH_ALL; bool sampled = true, take_pre = false, pregather = false, publish = false; int repeat = 1, slot = 0;
    bool operator==(const StepKey& o) const { return phase == o.phase && sampled == o.sampled && take_pre == o.take_pre && pregather == o.pregather && publish == o.publish && repeat == o.repeat && slot == o.slot; }
};

struct dqn_engine {
    EngineOpts opt;
    int device = 0; hipStream_t stream = nullptr, stream2 = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t stream3 = nullptr; hipEvent_t ev_xa = nullptr, ev_xb = nullptr, ev_xc = nullptr;      // replicas: the exchange runs on its own stream (dp_overlap)
    int nl = 0; LayerDev L[DQN_MAX_LAYERS]; LayerDev* L_dev = nullptr; bool plan_defaulted = false;      // plan == NULL at dqn_engine_create (dqn_comm_init may re-derive it for replicas)
    dqn_hparams hp; int B = 0, nA = 0, E = 0, ncon = 0;
    int last_base = -1, last_val = -1, last_adv = -1;
    size_t P = 0, Pint = 0;   // external (Flux.params) and internal (16-B aligned arrays) parameter counts
    float *p_on = nullptr, *p_tg = nullptr, *grad = nullptr, *m = nullptr, *v = nullptr, *io_tmp = nullptr;
    StepState* state = nullptr;
    // replay
    long long cap = 0, cap2 = 1, widx = 0, size = 0;
    void *s_rows = nullptr, *sp_rows = nullptr; int* ra = nullptr; float* rr = nullptr; unsigned char* rdone = nullptr; float* tree = nullptr;
    static const int ADD_CHUNK = 1024;
    int* st_a = nullptr; float* st_r = nullptr; unsigned char* st_done = nullptr; float* st_td = nullptr;
    // step workspace
    long long* idx = nullptr; long long* idx_pre = nullptr; float* x0 = nullptr;      // idx_pre: the next sample()'s indices, drawn by the priority block (StepState::pre_valid)
    float *act_on[DQN_MAX_LAYERS] = {}, *act_tg[DQN_MAX_LAYERS] = {}, *dact[DQN_MAX_LAYERS] = {};
    float *join_tmp = nullptr, *partials = nullptr, *gmax_part = nullptr; size_t partials_elems = 0;
    float *w_is = nullptr, *td = nullptr, *q_on_s = nullptr, *q_on_sp = nullptr, *q_tg_sp = nullptr, *ytarget = nullptr; int* best = nullptr;
    // get_batch seam workspace
    float *gb_rows = nullptr, *gb_r = nullptr, *gb_done = nullptr, *gb_w = nullptr; int* gb_a = nullptr; long long* gb_idx = nullptr;
    // train-step batch scalars (written by the gather launch, read by the fused head kernel)
    float *gb_r2 = nullptr, *gb_done2 = nullptr, *gb_w2 = nullptr; int* gb_a2 = nullptr;
    // policy workspace
    EnvDev env{}; bool has_envs = false; unsigned char* env_images = nullptr;
    float* env_tab = nullptr; unsigned char* env_term = nullptr;      // a tabular env set's tables (cumulative rows, rewards, feature rows) and terminal flags
    int pol_n = 0; float *pol_obs = nullptr, *pol_x = nullptr, *pol_act[DQN_MAX_LAYERS] = {}, *pol_q = nullptr; int* pol_a = nullptr;
    bool env_q_valid = false;      // pol_q / pol_a hold the last vector step of the training env set (dqn_envs_peek_q): set by the rollouts, cleared by whatever else writes or frees them
    // the train-step graphs, one per StepKey in use (linear lookup: a handful of entries); with a communicator the step is cut in two around the exchange
    struct StepGraph { StepKey key; hipGraphExec_t g; }; std::vector<StepGraph> graphs;
    StepKey cur;      // the variant enqueue_step is enqueuing, for the program's closures (default outside enqueue_step)
    bool arena_u8 = false;  // the observation arena x0 holds bytes (u8 replay, first layer converts in its tile loads): set by build_program
    unsigned long long* ktrace_buf = nullptr;     // dqn_debug_ktrace (trace builds): owned by the engine, freed with it
    // comm
    void* comm = nullptr; int rank = 0, world = 1; bool force_comm = false;
    // exchange mode of the replicas: gather = all-gather of the wide dense layers' operands + small gradients (dp.hip); else all-reduce of the gradient.
    // sim_world = k (env DQN_SIM_WORLD, tests): one process plays k identical ranks, the collective is k local copies.
    bool dp_gather = false, dp_pack_folds = false, dp_adam_folds = false; AdamSegs dp_adam_segs; int sim_world = 0; float *dp_send = nullptr, *dp_recv = nullptr; size_t dp_count = 0;
    // dp_overlap: the block is exchanged in TWO collectives -- [0, dp_count_a): X | dpre of the wide dense layers, final right after the head level, gathered (into dp_recv) on
    // stream3 WHILE the conv backward runs; [dp_count_a, dp_count): the small gradients, gathered (into dp_recv_b) after the backward pass
    long long* sim_idx = nullptr; float* sim_td = nullptr;      // dqn_sim_ranks_step (test hook): per-rank copies of the index lists and TD errors
    bool dp_overlap = false; size_t dp_count_a = 0; float* dp_recv_b = nullptr; DpPackArgs dp_pk_a;   // force_comm: run the all-reduce path even at world == 1 (tests)
    // DRQN (recurrence = true): column count per sequence set Bc = T*B (B otherwise); EpisodeReplayBuffer storage; LSTM workspaces
    int Bc = 0, T = 1; long long ep_cap = 0, ep_size = 0, ep_widx = 0, ep_cur_len = 0; std::vector<int> ep_len_host; std::vector<int64_t> ep_perm;
    float *ep_s = nullptr, *ep_sp = nullptr, *ep_r = nullptr; int* ep_a = nullptr; unsigned char* ep_done = nullptr; int* ep_len = nullptr;
    long long* ep_idx = nullptr; int* ep_start = nullptr; int* r_a = nullptr; float *r_r = nullptr, *r_done = nullptr, *r_mask = nullptr;
    float *gx_on[DQN_MAX_LAYERS] = {}, *gx_tg[DQN_MAX_LAYERS] = {}, *cst_on[DQN_MAX_LAYERS] = {}, *cst_tg[DQN_MAX_LAYERS] = {}, *gates[DQN_MAX_LAYERS] = {}, *tcb[DQN_MAX_LAYERS] = {},
          *hprev_buf[DQN_MAX_LAYERS] = {}, *cprev_buf[DQN_MAX_LAYERS] = {}, *dG[DQN_MAX_LAYERS] = {}, *dhn[DQN_MAX_LAYERS] = {}, *dcn[DQN_MAX_LAYERS] = {};
    float *pol_h[DQN_MAX_LAYERS][2] = {}, *pol_c[DQN_MAX_LAYERS][2] = {}, *pol_gx[DQN_MAX_LAYERS] = {}; int pol_flip = 0, pol_state_n = 0; uint64_t drqn_draws = 0;
    // device environments on a recurrent engine (engine_envs.hip): the training copies' Recur state IS the policy state above (n streams, buffer set pol_flip; pol_state_gen
    // counts its reallocations, an acting program is rebuilt when (pol_state_gen, pol_flip) moved); the evaluation copies own a private state; ep_stage: the open episodes
    int pol_state_gen = 0; EpStage ep_stage{}; float *eval_h[DQN_MAX_LAYERS] = {}, *eval_c[DQN_MAX_LAYERS] = {}, *eval_gx[DQN_MAX_LAYERS] = {};
    // static launch program
    struct Step { const char* name; std::function<void(dqn_engine*)> fn; };
    // acting programs (forward on n columns + env kernels), one for the training envs and one for the evaluation envs
    // cycle: ONE graph of `cycle_F` acting steps (+ a plain sampled train step when cycle_train) -- the device loop's unit of work between two
    // train steps; a graph launch costs ~5 us of stream time, a GridWorld vector step 28
    struct ActProg { std::vector<Step> steps; int n = 0; bool fused_tail = false; hipGraphExec_t graph = nullptr; DevScope mem; int state_gen = -1, state_flip = -1;
                     hipGraphExec_t cycle = nullptr; int cycle_F = 0; bool cycle_train = false;
                     hipGraphExec_t envc = nullptr; int envc_due = 0; };      // envc: one vector step of the reference's cadence (the acting step + its `envc_due` pipelined train steps) as ONE graph
    // act_gen: the training set's acting program with the general four-launch tail, built only where `act` has the fused one and a rollout explores by table
    // (dqn_rollout_explore): both are kept, neither is rebuilt when calls alternate.  xtab: that entry point's table in HBM (engine-owned, grown on demand; the
    // pointer travels in the RolloutDev record, not in a kernel argument, so growing it leaves the captured graphs valid)
    ActProg act_gen; float* xtab = nullptr; size_t xtab_cap = 0;
    ActProg act, evalp; std::vector<Step>* sink = nullptr; DevScope* alloc_sink = nullptr; RolloutDev *roll = nullptr, *eval_roll = nullptr;
    EnvDev eval_env{}; int eval_n = 0;
    std::vector<Step> prog; size_t prog_post_begin = 0, prog_pre1_end = 0; bool prog_built = false, prio_forked = false, prio_in_bwd = false;
    int gmax_used = 0;                    // live slots of gmax_part (per-block max |g| of the step's Adam jobs): what the on-demand fold reads
    StepState* state_host = nullptr;      // pinned landing buffer of fetch_scalars
    // scalar mailbox (StepMail, common.h): mapped pinned host ring the step's last launch writes (loss, grad_norm) into; pub_issued = publishes enqueued by the host,
    // pub_ctr = publishes executed by the device (the record of ticket t sits in slot t % DQN_MAIL_SLOTS once its seq == t)
    StepMail *mail_host = nullptr, *mail_dev = nullptr; unsigned long long* pub_ctr = nullptr; unsigned long long pub_issued = 0;
    unsigned long long mail_swept = 0; bool mail_plain = false;      // mail_swept: records [1, mail_swept] have been checked for device-side errors (mail_sweep); mail_plain: the ring is ordinary host memory (mapped allocation refused)
    bool pg_ok = false; PreGather pg; long adam_step = -1;      // pg_ok: the program supports the pre-gather (StepKey::take_pre / pregather)
    bool tiny = false;      // the whole step is ONE single-workgroup launch that samples and gathers itself (tiny_step.hip)
    std::vector<TinyArgs> tiny_args;      // tiny: the host copy of the record that launch reads (one element) -- what a group copies into its device array (engine_group.hip)
    int in_groups = 0;      // live dqn_group_t's this engine is a member of: dqn_engine_destroy is refused while any exists
    // fused recurrent step: episode draws travel through a mapped pinned host buffer of DQN_DRAW_SLOTS slots the kernel reads directly.  A slot is a LAUNCH PARAMETER, fixed per graph
    // node: two 8-step graphs (slots 0-7 / 8-15) and two single-step graphs (16 / 17) alternate, and before the host rewrites the slots of one it waits for the event recorded
    // behind that graph's previous launch
    long long *draw_idx_h = nullptr, *draw_idx_d = nullptr; int *draw_start_h = nullptr, *draw_start_d = nullptr;
    hipEvent_t draw_ev[4] = {nullptr, nullptr, nullptr, nullptr}; bool draw_ev_used[4] = {false, false, false, false}; int drqn_grp_par = 0, drqn_one_par = 0;
    unsigned long long* drqn_stamps = nullptr;      // timing probe of the fused recurrent step (DQN_DRQN_STAMPS)
    bool launch_failed = false;      // a launcher refused (an LDS attribute the device would not grant): reported by the entry point that enqueued the step
    bool drqn_fused = false;      // recurrent step = the column-parallel launch (which gathers its own episode rows) + the Adam launch (drqn_cols.hip)
    bool mid_big_warm = false;      // the graph of MID_BIG middle steps (dqn_train_steps) has been launched at least once (its first launch is the expensive one)
    int dp_one_state = 0;           // replicas: the WHOLE step incl. its collective(s) as ONE graph (PH_DP_ONE); state 0 untried, 1 works, -1 RCCL refused the capture
    AdamSegs adam_segs; long final_reduce_step = -1;   // deferred dW slabs: reduced inside k_adam unless a communicator needs the materialised gradient
    std::vector<std::string> prog_names;
    // device memory by lifetime (devmem.h; the table of scopes is DESIGN.md section 2).  prof_gate: the mapped flag dqn_profile_step's gate kernel spins on (in mem)
    DevScope mem, prog_mem, pol_mem, pol_state_mem, env_mem, eval_mem, dp_mem; int* prof_gate = nullptr;
    // profiling
    bool profiling = false; std::vector<ProfEntry> prof;
};

void prof_begin(dqn_engine* e, const char* name);
void prof_end(dqn_engine* e);
#define RUN(e, name, call) do { prof_begin(e, name); call; prof_end(e); } while (0)
// THE size rule of the split-K workspace `partials`: the slabs of the widest forward (ncon columns), dW and dense dX (Bc columns) the plan cuts, and a GroupNorm layer's chunk statistics (launch_layer_fwd)
static inline size_t partials_need(const LayerDev* L, int nl, size_t Bc, size_t ncon) {
    size_t need = 1;
    for (int i = 0; i < nl; i++) { const LayerDev& l = L[i];
        const size_t sf = dqn_nchunks(l.K, l.fwd_kc), sw = dqn_nchunks((int)std::min<size_t>((size_t)l.npos * Bc, INT_MAX), l.dw_kc), sx = !is_conv_kind(l.kind) ? dqn_nchunks(l.N, l.dx_kc) : 1;
        if (sf > 1) need = std::max(need, sf * (size_t)l.out_feat * ncon); if (sw > 1) need = std::max(need, sw * ((size_t)l.K + 1) * l.N); if (sx > 1) need = std::max(need, sx * (size_t)l.in_feat * Bc);
        if (is_gn(l.kind)) need = std::max(need, gn_part_floats(l, (int)ncon));
    }
    return need;
}
#define NEED_REC(e) do { if (!(e)->hp.recurrence) return fail("this engine was created with recurrence = false"); } while (0)

// engine_layers.hip (host only): the geometry of every layer, or -1 with the refusal; the last layer of each stream (-1: none), the external / internal parameter counts
int build_layers(const dqn_layer_desc* d, int n, const dqn_hparams* hp, LayerDev* L, int* lb, int* lv, int* la, size_t* P, size_t* Pint);
// engine.hip
void drop_graphs(dqn_engine* e);
void drop_act(dqn_engine* e, dqn_engine::ActProg& a);
// one layer's forward launched alone on the given columns, by kind: THE place (with emit_forward, engine_program.hip) where the forward side learns a new layer kind.
// xu8: X is the byte arena of a u8 replay (padded convs only); ln_stat: where a LayerNorm layer keeps (mu, sigma) per column, or null; partials: split-K workspace of the GEMM kinds
// X2, ldx2: the second operand of a skip block's join (the output of the block's entry, LayerDev::src2; X is the last inner layer's), null for every other kind
void launch_layer_fwd(hipStream_t st, const LayerDev& l, const float* P, const float* X, int ldx, int col0, int ncols, float* Y, bool use_mfma, int xu8, float* ln_stat, float* partials, const float* X2 = nullptr, int ldx2 = 0);
void fwd_layer(dqn_engine* e, const LayerDev& l, const float* P, const float* X, int ldx, int col0, int ncols, float* Y, const char* name, const float* X2 = nullptr, int ldx2 = 0);      // ... inside a profiling bracket
// a skip block's join whose last inner layer has no activation: the join's backward is the identity, so dact[join] IS dact[src] (one buffer; engine.hip allocates, skip.hip)
static inline bool skip_dact_alias(const dqn_engine* e, int i) { return is_skip(e->L[i].kind) && e->L[e->L[i].src].act == DQN_ACT_IDENTITY; }
// a map block (DQN_LAYER_SKIPADD_MAP) whose entry add runs in the epilogue of its first inner layer's input-gradient launch (conv_own.hip): every block, unless DQN_NO_SKIP_FUSE ...
static inline bool skip_fused_dx(const dqn_engine* e, int j) { return is_skip_map(e->L[j].kind) && !e->opt.no_skip_fuse; }
// ... and whose forward add runs in the epilogue of its last inner layer's launch, which then writes the JOIN's activation: where that layer has no activation (its own
// output is needed for nothing then: the join is its only consumer and the join's backward is the alias above).  The train step and the acting programs of emit_forward
static inline bool skip_fused_fwd(const dqn_engine* e, int j) { return skip_fused_dx(e, j) && skip_dact_alias(e, j); }
// the join whose block's LAST / FIRST inner layer is l, or -1
static inline int skip_join_of_last(const dqn_engine* e, int l) { for (int j = l + 1; j < e->nl; j++) if (is_skip(e->L[j].kind) && e->L[j].src == l) return j; return -1; }
static inline int skip_join_of_first(const dqn_engine* e, int l) { for (int j = l + 1; j < e->nl; j++) if (is_skip(e->L[j].kind) && j - e->L[j].cin == l) return j; return -1; }
// the activation whose derivative layer l's input-gradient launch applies in its epilogue: its producer's -- unless that producer is the entry P of a skip block (then l is
// the block's first inner layer and P has a second consumer, the join): the launch writes the RAW gradient and the block's entry launch (skip.hip) takes P's derivative
// once, after the sum.  THE statement of the rule: every dX site of engine_program.hip goes through it (a map block's fused entry hands its launch P's real activation
// instead: the sum is made in that launch's own epilogue, bwd_own_level)
static inline int src_act(const dqn_engine* e, int l) {
    const int s = e->L[l].src;
    for (int j = 0; j < e->nl; j++) if (is_skip(e->L[j].kind) && e->L[j].src2 == s) return DQN_ACT_IDENTITY;
    return e->L[s].act;
}
void enqueue_step(dqn_engine* e, const StepKey& k);
int capture_graph(dqn_engine* e, const char* what, const std::function<int()>& body, hipGraphExec_t* out);      // the one stream capture of the library
int run_phase(dqn_engine* e, const StepKey& k, bool eager = false);      // the cached graph of k (captured on first use), or k enqueued eagerly
int exchange_grads(dqn_engine* e);      // the one collective of a data-parallel step (all-gather or all-reduce)
int run_step(dqn_engine* e, bool sample, bool take_pre = false, bool pregather = false, bool publish = false, bool* published = nullptr);
int fetch_scalars(dqn_engine* e, float* loss, float* gn);
int policy_ws(dqn_engine* e, int n);
int policy_state(dqn_engine* e, int n, bool force_reset);
// engine_drqn.hip
int drqn_train_steps(dqn_engine* e, int n, float* loss, float* grad_norm);
// engine_program.hip
// a block of the program being built, in its scope: null after a refused allocation, which the scope latches -- the builders test the latch once at their end, whatever touches a fresh block from the host tests the pointer first
static inline DevScope& prog_scope(dqn_engine* e) { return e->alloc_sink ? *e->alloc_sink : e->prog_mem; }
template <class T> static T* upload(dqn_engine* e, const std::vector<T>& v) {
    T* d = nullptr; if (prog_scope(e).get(&d, v.size())) return nullptr;
    hipMemcpy(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice); return d;
}
static inline float* palloc(dqn_engine* e, size_t n) { float* d = nullptr; prog_scope(e).get(&d, n); return d; }
bool same_geo(const LayerDev& a, const LayerDev& b);
void flush_valu(dqn_engine* e, std::vector<VTask>& pend, const char* name, const PrioArgs* prio = nullptr);
void emit_reduce(dqn_engine* e, std::vector<RSeg>& segs, const char* name);
const char* lname(dqn_engine* e, const char* fmt, ...) __attribute__((format(printf, 2, 3)));      // THE interned launch name (kept in prog_names)
const char* pname(dqn_engine* e, const char* op, const LayerDev& L, int i);      // "<op>_<the kind's tag><i>" (KindTraits::tag)
typedef std::vector<std::vector<int>> Levels;
Levels net_levels(const dqn_engine* e);      // the launch levels of the network: the base chain one layer per level, then the (value, advantage) layers pairwise
LayerDev gx_view(const LayerDev& l);         // a recurrent layer's batched part: its bias-free input projection Gx = Wi*x as a dense layer K = n_in, N = ngates*H
// the layout half of the fused reduce + head launches (red_head.hip, act_head.hip): the dense heads ha (and hv, or -1) sit alone on the last level, their dense producers alone
// on the level before, with equal width and split count, and the heads' plan chunks are 32 long and tile K exactly.  Returns the producers' split count S (0: another layout)
int fused_head_layout(const dqn_engine* e, const Levels& levels, int ha, int hv, int* pa, int* pv);
// One network pass of emit_forward, as data: the parameter vector, where the observation columns are, the activations a layer reads (in[src]) and writes (out[l]: differs
// from in[l] for a recurrent layer, whose batched part writes its gx_* view) -- dense in the column, leading dimension = ncols -- and the tag of its single-pass launch names
struct FwdPass { const float* P; const float* x0; int ldx0, col0; float* const* in; float* const* out; int ncols; const char* tag; };
struct FwdEmit {
    // ---- in
    const char *gemm = nullptr, *valu = nullptr, *reduce = nullptr;      // launch-name prefixes of the grouped GEMM launch, the VALU task table and the split-K reduce of a level
    bool skip_last = false;                // the last level runs inside the caller's fused head launch
    int prod[2] = {-1, -1};                // the heads' producer layers (advantage / single stream, value) whose slabs or activations that launch reads unreduced ...
    bool pm_ok = false;                    // ... and whether it reads slabs piece-major (GFwdProb::pm)
    bool last_on_the_fly = false;          // the consumer of the last level reduces split-K slabs itself (HeadSrc::S > 1)
    bool byte_arena = false;               // LayerDev::xu8 holds for the observation columns of these passes
    int do_cols = 0;                       // Dropout layers are ACTIVE on the leading do_cols columns of the FIRST pass (the train step: online network, s); 0: inactive everywhere, no launch
    const bool* wantT = nullptr;           // layers whose consumer reads a transposed copy [column][feature] of their output (null: none)
    // ---- out (the arrays are the caller's)
    float* (*actT)[2] = nullptr;           // per (layer, pass): the transposed copy of a wantT layer (needed with wantT)
    float** ln_stat = nullptr;             // per LayerNorm layer: (mu, sigma) of the FIRST pass's columns, allocated here and kept for the backward (null: not kept)
    HeadSrc (*head)[2] = nullptr;          // per (layer, pass): where the layer's output is found
    const float *part[2][2] = {}, *partT[2][2] = {}; bool pm = false;      // per (producer stream, pass): slabs or finished activation, its transposed copy; slabs were written piece-major
};
// the forward launches of levels [li0, li1) into the current sink, for every pass: THE statement of the forward selection rules (train step and acting programs)
void emit_forward(dqn_engine* e, const Levels& levels, size_t li0, size_t li1, const std::vector<FwdPass>& passes, FwdEmit& E);
int build_program(dqn_engine* e);
std::string tiny_decline(const dqn_engine* e);      // why the engine does not take the single-workgroup step (tiny_step.hip); empty: it does.  THE eligibility rule
// engine_group.hip
std::string tiny_act_decline(const dqn_engine* e);      // why the engine does not take the single-workgroup acting step (tiny_act.hip); empty: it does.  THE eligibility rule
std::string tiny_eval_decline(const dqn_engine* e);      // why the engine does not take the single-workgroup evaluation (tiny_eval.hip); empty: it does.  THE eligibility rule
int eval_envs_ensure(dqn_engine* e, int n_eval);      // the engine's evaluation copies (engine_envs.hip), allocated for n_eval
// engine_envs.hip
void free_envs(dqn_engine* e);
int explore_check(const dqn_exploration* x, int n_steps);      // dqn_rollout_explore's table: 0, or -1 with the refusal (nothing is enqueued)
ReplayMeta replay_meta(const dqn_engine* e);      // the engine's transition ring as the acting tails are handed it
RolloutDev rollout_record(const dqn_rollout_cfg* cfg, const dqn_engine* e);      // the RolloutDev a call starts from; cfg == NULL: the greedy record of an evaluation
// THE host's ring cursor behind n added transitions (the device writes them; the host keeps count)
static inline void ring_advance(dqn_engine* e, long long n) { e->widx = (e->widx + n) % e->cap; e->size = std::min(e->cap, e->size + n); }
int ep_mirror_push(dqn_engine* e);     // recurrent env sets: host (ep_widx, ep_size) -> the device cursor, before a rollout
int ep_mirror_pull(dqn_engine* e);      // ... and the device cursor and lengths -> the host mirror (ep_widx, ep_size, ep_len_host): one D2H + one synchronize
