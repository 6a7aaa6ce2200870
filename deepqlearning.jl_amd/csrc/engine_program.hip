// engine_program.hip -- the static launch program of the train step (batch_train!, src/solver.jl:191-236 and :239-287): every pointer,
// shape and plan is fixed at engine creation, so the step is compiled ONCE into a list of launches (closures) and merely replayed (and captured into a hipGraph).
// Small independent kernels are batched: one k_valu_multi launch per network level, one k_reduce_multi per level, head reductions folded into k_td.
#include "engine.h"
bool same_geo(const LayerDev& a, const LayerDev& b) {
    return a.kind == b.kind && a.act == b.act && a.K == b.K && a.N == b.N && a.npos == b.npos && a.cin == b.cin && a.kh == b.kh && a.kw == b.kw &&
           a.sh == b.sh && a.sw == b.sw && a.ph == b.ph && a.pw == b.pw && a.dh == b.dh && a.dw == b.dw && a.groups == b.groups && a.ih == b.ih && a.iw == b.iw && a.fwd_kc == b.fwd_kc && a.src == b.src;
}
// THE interned launch name, printf-style: the string lives in the engine (prog_names) as long as the program that points at it
const char* lname(dqn_engine* e, const char* fmt, ...) {
    char b[96]; va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
    e->prog_names.push_back(b); return e->prog_names.back().c_str();
}
const char* pname(dqn_engine* e, const char* op, const LayerDev& L, int i) { return lname(e, "%s_%s%d", op, kind_traits(L).tag, i); }
static unsigned number_tasks(std::vector<VTask>& v) { unsigned blocks = 0; for (auto& t : v) { t.first_block = blocks; blocks += valu_task_blocks(t); } return blocks; }      // each task's first workgroup; the launch's grid
// prio: the step's priority block (update_priorities! + the next step's index draw) rides as workgroup 0 of this launch
void flush_valu(dqn_engine* e, std::vector<VTask>& pend, const char* name, const PrioArgs* prio) {
    if (pend.empty()) return;
    const unsigned blocks = number_tasks(pend);
    VTask* dev = upload(e, pend); const int n = (int)pend.size();
    if (prio) {
        const PrioArgs pa = *prio; StepState* stt = e->state;
        const char* name2 = lname(e, "%s+prio", name);
        (e->sink ? *e->sink : e->prog).push_back({name2, [=](dqn_engine* en) { launch_valu_multi(en->stream, dev, n, blocks, &pa, stt); }});
    }
    else (e->sink ? *e->sink : e->prog).push_back({name, [=](dqn_engine* en) { launch_valu_multi(en->stream, dev, n, blocks); }});
    pend.clear();
}
void emit_reduce(dqn_engine* e, std::vector<RSeg>& segs, const char* name) {
    if (segs.empty()) return;
    unsigned blocks = 0;
    for (auto& r : segs) { r.first_block = blocks; blocks += (unsigned)((r.elems + 255) / 256); }
    RSeg* dev = upload(e, segs); const int n = (int)segs.size();
    (e->sink ? *e->sink : e->prog).push_back({name, [=](dqn_engine* en) { launch_reduce_multi(en->stream, dev, n, blocks); }});
    segs.clear();
}
// layer l may be an LDS-tiled dW launch that carries the priority block: a GEMM kind (no own-level kind, no recurrent layer) whose dW the tiled kernel takes.  ld: its input's leading dimension
static bool dw_carrier_ok(const dqn_engine* e, int l, int B, int ld) { return kind_traits(e->L[l]).dw_carrier && gemm_dw_eligible(e->L[l], B, ld); }
Levels net_levels(const dqn_engine* e) {
    Levels levels; std::vector<int> val, adv;
    for (int i = 0; i < e->nl; i++) { if (e->L[i].stream == DQN_STREAM_BASE) levels.push_back({i}); else if (e->L[i].stream == DQN_STREAM_VAL) val.push_back(i); else adv.push_back(i); }
    for (size_t j = 0; j < std::max(val.size(), adv.size()); j++) { std::vector<int> lv; if (j < val.size()) lv.push_back(val[j]); if (j < adv.size()) lv.push_back(adv[j]); levels.push_back(lv); }
    return levels;
}
LayerDev gx_view(const LayerDev& l) { LayerDev v = l; v.kind = DQN_LAYER_DENSE; v.out_feat = l.N; v.b_off = l.z_off; v.act = DQN_ACT_IDENTITY; return v; }
int fused_head_layout(const dqn_engine* e, const Levels& levels, int ha, int hv, int* pa, int* pv) {
    if (levels.size() < 2 || ha < 0) return 0;
    const int ns = hv >= 0 ? 2 : 1; const LayerDev& La = e->L[ha]; *pa = La.src; *pv = hv >= 0 ? e->L[hv].src : -1;
    auto in_lv = [](const std::vector<int>& v, int l) { for (int x : v) if (x == l) return true; return false; };
    const auto& hl = levels.back(); const auto& pl = levels[levels.size() - 2];
    bool ok = La.kind == DQN_LAYER_DENSE && *pa >= 0 && (hv < 0 || (e->L[hv].kind == DQN_LAYER_DENSE && *pv >= 0 && *pv != *pa));
    ok = ok && (int)hl.size() == ns && in_lv(hl, ha) && (hv < 0 || in_lv(hl, hv)) && (int)pl.size() == ns && in_lv(pl, *pa) && (hv < 0 || in_lv(pl, *pv));
    if (!ok) return 0;
    const LayerDev& Pa = e->L[*pa]; const int S = dqn_nchunks(Pa.K, Pa.fwd_kc);
    ok = Pa.kind == DQN_LAYER_DENSE && Pa.N == La.K && dqn_chunk_len(La.K, La.fwd_kc) == 32 && dqn_nchunks(La.K, La.fwd_kc) * 32 == La.K;
    if (ok && hv >= 0) { const LayerDev& Pv = e->L[*pv]; const LayerDev& Lv = e->L[hv];
        ok = Pv.kind == DQN_LAYER_DENSE && Pv.N == Pa.N && dqn_nchunks(Pv.K, Pv.fwd_kc) == S && dqn_chunk_len(Lv.K, Lv.fwd_kc) == 32 && Lv.K == La.K; }
    return ok ? S : 0;
}
void emit_forward(dqn_engine* e, const Levels& levels, size_t li0, size_t li1, const std::vector<FwdPass>& passes, FwdEmit& E) {
    const bool mf = e->hp.use_mfma != 0; auto& prog = e->sink ? *e->sink : e->prog; const int np = (int)passes.size();
    auto view = [&](int l) { LayerDev V = is_recurrent(e->L[l].kind) ? gx_view(e->L[l]) : e->L[l]; if (!E.byte_arena) V.xu8 = 0; return V; };
    auto prod_stream = [&](int l) { return l == E.prod[0] ? 0 : l == E.prod[1] ? 1 : -1; };
    struct Prob { int l, pass; const float *P, *X; int ldx, col0, ncols; float *Y, *part; int S; };
    auto prob = [&](int l, int pi) {      // layer l on pass pi; the split-K slabs are allocated by the caller
        const FwdPass& ps = passes[pi]; const int src = e->L[l].src; Prob q; q.l = l; q.pass = pi; q.P = ps.P; q.ncols = ps.ncols; q.Y = ps.out[l]; q.part = nullptr; q.S = 1;
        q.X = src < 0 ? ps.x0 : ps.in[src]; q.ldx = src < 0 ? ps.ldx0 : ps.ncols; q.col0 = src < 0 ? ps.col0 : 0;
        return q;
    };
    for (size_t li = li0; li < li1; li++) {
        const auto& lv = levels[li]; const bool last = li + 1 == levels.size();
        if (E.skip_last && last) continue;
        if (kind_traits(e->L[lv[0]]).own_level) {
            // a layer launched alone on its level (base chain only): one launch per pass it is active in, never grouped with a GEMM layer.  Per kind:
            //   a pool (pool.hip; an adaptive / global pool whose resolved window is the whole map: pool_global.hip -- launch_layer_fwd decides), a padded or a dilated / grouped conv (conv_own.hip walks the plan chunks itself), a LayerNorm layer (layernorm.hip; the first pass keeps (mu, sigma) per column for the backward): every pass
            //   a GroupNorm layer (groupnorm.hip): every pass, TWO launches, "<pass>_gn<l>_stat" and "<pass>_gn<l>"; the first pass keeps (mu, r) per (group, column) for the backward
            //   the join of a skip block (skip.hip): every pass, y = (the last inner layer's stored output) + (the stored output of the block's entry, LayerDev::src2) on that pass's
            //     own activations -- where the entry or the last inner layer is a Dropout, its masked buffer in the train step's online pass and its producer's (the alias) elsewhere
            //   a Dropout layer (dropout.hip): ACTIVE in the first pass of the train step only, on its leading E.do_cols columns (online network, s): it writes a buffer of its own -- the producer's output
            //     must survive for the producer's backward -- and copies the s' columns behind them.  Every other pass emits NOTHING: the layer's activation pointer there is its producer's (engine.hip)
            //   a standalone activation layer (act_layer.hip): every pass, one element-wise launch on the producer's stored output of that pass
            //   a convolutional skip block whose last inner layer K has no activation (skip_fused_fwd): K's launch takes the entry's stored output of the pass as its residual
            //     operand and writes act(tot + bias) + y_P straight into the JOIN's activation (conv_own.hip), named "<pass>_conv<K>+skip<join>"; the join's level emits nothing.
            //     K's own activation buffer is then never written, and never read: its one consumer is the join, and the join's backward is the alias (skip_dact_alias)
            const int l = lv[0]; const LayerDev L = view(l); const bool dropout = is_do(L.kind), join = is_skip(L.kind);
            const int jn = is_padded(L) ? skip_join_of_last(e, l) : -1; const bool fuse_res = jn >= 0 && skip_fused_fwd(e, jn);
            const bool fused_join = join && skip_fused_fwd(e, l);
            float* stat0 = (is_ln(L.kind) && E.ln_stat) ? (E.ln_stat[l] = palloc(e, (size_t)2 * passes[0].ncols)) : nullptr;
            if (is_gn(L.kind) && E.ln_stat) stat0 = E.ln_stat[l] = palloc(e, (size_t)2 * L.kh * passes[0].ncols);      // (mu, r) per (group, column)
            for (int pi = 0; pi < np; pi++) {
                const Prob q = prob(l, pi);
                HeadSrc h; h.p = q.Y; h.ld = q.ncols; h.S = 1; h.per_s = 0; h.bias = (dropout || join || is_actl(L.kind)) ? nullptr : q.P + L.b_off; h.act = L.act; E.head[l][pi] = h;      // (a Dropout layer, a join, an Activation layer: no parameters, IDENTITY -- the Activation's σ is in cell_act and already applied)
                if (dropout) {
                    const double p = do_p(L); const unsigned long long seed = e->hp.seed; const StepState* stt = e->state; const int C = E.do_cols;
                    if (pi == 0 && C > 0) prog.push_back({pname(e, passes[pi].tag, L, l), [=](dqn_engine* en) { launch_do_fwd(en->stream, L.out_feat, p, seed, l, stt, q.X, q.Y, q.ncols, q.ncols, C); }});
                    continue;
                }
                if (fused_join) continue;      // written by the last inner layer's launch
                if (fuse_res) {
                    const char* name = lname(e, "%s_%s%d+skip%d", passes[pi].tag, kind_traits(L).tag, l, jn);
                    const float* R = passes[pi].in[e->L[jn].src2]; float* Yj = passes[pi].out[jn];
                    prog.push_back({name, [=](dqn_engine* en) { launch_conv_own_fwd(en->stream, L, q.P, q.X, q.ldx, q.col0, q.ncols, Yj, mf ? 1 : 0, 0, R, q.ncols, 0); }});
                    continue;
                }
                float* stat = pi == 0 ? stat0 : nullptr; const float* X2 = join ? passes[pi].in[L.src2] : nullptr;
                if (is_gn(L.kind)) {      // two launches (groupnorm.hip): the chunk statistics into a workspace of the pass's own, then the normalise pass, which combines them per workgroup
                    float* part = palloc(e, gn_part_floats(L, q.ncols));
                    const char* name = lname(e, "%s_%s%d_stat", passes[pi].tag, kind_traits(L).tag, l);
                    prog.push_back({name, [=](dqn_engine* en) { launch_gn_stat(en->stream, L, q.X, q.ldx, q.col0, q.ncols, part); }});
                    prog.push_back({pname(e, passes[pi].tag, L, l), [=](dqn_engine* en) { launch_gn_norm(en->stream, L, q.P, q.X, q.ldx, q.col0, q.ncols, q.Y, part, stat); }});
                    continue;
                }
                prog.push_back({pname(e, passes[pi].tag, L, l), [=](dqn_engine* en) { launch_layer_fwd(en->stream, L, q.P, q.X, q.ldx, q.col0, q.ncols, q.Y, mf, L.xu8, stat, nullptr, X2, q.ncols); }});
            }
            continue;
        }
        std::vector<Prob> pr;
        for (int l : lv) for (int pi = 0; pi < np; pi++) {
            const LayerDev L = view(l); Prob q = prob(l, pi);
            q.S = dqn_nchunks(L.K, L.fwd_kc); q.part = q.S > 1 ? palloc(e, (size_t)q.S * L.out_feat * q.ncols) : nullptr;
            pr.push_back(q);
        }
        bool geo = true; for (int l : lv) geo = geo && same_geo(view(lv[0]), view(l));
        std::vector<bool> done(pr.size(), false);
        auto emit_gemm = [&](const std::vector<int>& ids, const char* name, int pm) {
            const LayerDev L = view(pr[ids[0]].l); const int n = (int)ids.size();
            struct A { const float *W[4], *bias[4], *X[4]; int ldx[4], col0[4], ncols[4]; float* out[4]; float* outT[4]; } a;
            bool any_t = false;
            for (int i = 0; i < n; i++) {
                const Prob& q = pr[ids[i]]; const LayerDev Lq = view(q.l); a.W[i] = q.P + Lq.w_off; a.bias[i] = q.P + Lq.b_off; a.X[i] = q.X; a.ldx[i] = q.ldx; a.col0[i] = q.col0; a.ncols[i] = q.ncols; a.out[i] = q.S > 1 ? q.part : q.Y;
                // an UNSPLIT dense layer that feeds k_head_td writes the transposed copy of its output itself (r04: without it the head kernel read its columns one 64-byte
                // sector per element at B = 512 -- 11 us of its 25); split-K layers get theirs from the reduce launch below
                a.outT[i] = nullptr;
                if (E.wantT && E.wantT[q.l] && q.S == 1 && Lq.kind == DQN_LAYER_DENSE) { a.outT[i] = E.actT[q.l][q.pass] = palloc(e, (size_t)Lq.out_feat * q.ncols); any_t = true; }
            }
            if (any_t) for (int i = 0; i < n; i++) if (!a.outT[i]) { any_t = false; for (int j = 0; j < n; j++) { if (a.outT[j]) E.actT[pr[ids[j]].l][pr[ids[j]].pass] = nullptr; a.outT[j] = nullptr; } break; }      // all problems of the launch or none
            prog.push_back({name, [=](dqn_engine* en) { launch_gemm_fwd(en->stream, L, n, a.W, a.bias, a.X, a.ldx, a.col0, a.ncols, a.out, any_t ? a.outT : nullptr, pm); }});
        };
        // the grouping rule: ALL problems of the level in one LDS-tiled launch when they number at most four, share the geometry and are eligible; else one launch per layer
        // over that layer's passes, where eligible; the leftovers go to the direct MFMA launch or the level's VALU task table
        std::vector<std::pair<std::vector<int>, const char*>> groups;
        if (mf && pr.size() <= 4) {
            int ldx[4], c0[4], nc[4]; std::vector<int> all;
            for (size_t i = 0; i < pr.size(); i++) { all.push_back((int)i); ldx[i] = pr[i].ldx; c0[i] = pr[i].col0; nc[i] = pr[i].ncols; }
            if (geo && gemm_fwd_eligible(view(lv[0]), (int)pr.size(), ldx, c0, nc)) groups.push_back({all, pname(e, E.gemm, e->L[lv[0]], lv[0])});
            else for (size_t i = 0; i < pr.size(); i += np)
                if (gemm_fwd_eligible(view(pr[i].l), np, ldx + i, c0 + i, nc + i)) groups.push_back({std::vector<int>(all.begin() + i, all.begin() + i + np), pname(e, E.gemm, e->L[pr[i].l], pr[i].l)});
        }
        for (auto& g : groups) for (int id : g.first) done[id] = true;
        // split-K slabs that only the fused head launch reads are written piece-major (GFwdProb::pm).  That launch takes ONE flag for all its streams, so the layout is decided
        // once per level: every problem of the level is a split producer's AND sits in an LDS-tiled launch (the direct MFMA launch and the VALU tasks write [S][N][columns])
        bool pm_all = E.pm_ok; for (size_t i = 0; i < pr.size(); i++) pm_all = pm_all && done[i] && prod_stream(pr[i].l) >= 0 && pr[i].S > 1;
        if (pm_all) E.pm = true;
        for (auto& g : groups) emit_gemm(g.first, g.second, pm_all ? 1 : 0);
        std::vector<VTask> pend;
        for (size_t i = 0; i < pr.size(); i++) {
            if (done[i]) continue;
            const Prob q = pr[i]; const LayerDev L = view(q.l);
            if (mf && mfma_fwd_ok(L, q.ncols)) {
                prog.push_back({pname(e, passes[q.pass].tag, L, q.l), [=](dqn_engine* en) { launch_mfma_fwd(en->stream, L, q.P, q.X, q.ldx, q.col0, q.ncols, q.Y, q.part, false); }});
            } else {
                VTask t; memset(&t, 0, sizeof t); t.kind = 0; t.L = L; t.P = q.P; t.X = q.X; t.ldx = q.ldx; t.col0 = q.col0; t.ncols = q.ncols; t.S = q.S; t.kc = dqn_chunk_len(L.K, L.fwd_kc);
                t.out = q.S > 1 ? q.part : q.Y; pend.push_back(t);
            }
        }
        flush_valu(e, pend, pname(e, E.valu, e->L[lv[0]], lv[0]));
        std::vector<RSeg> segs;
        for (const Prob& q : pr) {
            const LayerDev L = view(q.l); const int st = prod_stream(q.l);
            HeadSrc h; h.p = q.Y; h.ld = q.ncols; h.S = 1; h.per_s = 0; h.bias = q.P + L.b_off; h.act = L.act;
            if (st >= 0) { E.part[st][q.pass] = q.S > 1 ? q.part : q.Y;      // reduced inside the fused head launch (S == 1: the finished activation)
                           E.partT[st][q.pass] = (q.S > 1 || !E.actT) ? nullptr : E.actT[q.l][q.pass]; }
            else if (q.S > 1) {
                // the last level's split-K slabs are reduced inside its consumer only while that is cheaper than a reduce launch (the train step's single-workgroup TD kernel at
                // small batches; at B = 512 the 7680 head values x 16 slabs belong on many workgroups)
                if (last && E.last_on_the_fly) { h.p = q.part; h.S = q.S; h.per_s = (unsigned long long)L.out_feat * q.ncols; }
                else { RSeg r; memset(&r, 0, sizeof r); r.part = q.part; r.S = q.S; r.elems = (unsigned long long)L.out_feat * q.ncols; r.mode = 0; r.bias = q.P + L.b_off; r.per_n = L.npos * q.ncols; r.act = L.act; r.out = q.Y;
                       if (E.wantT && E.wantT[q.l]) { r.outT = E.actT[q.l][q.pass] = palloc(e, (size_t)L.out_feat * q.ncols); r.ncolsT = q.ncols; }
                       segs.push_back(r); }
            }
            E.head[q.l][q.pass] = h;
        }
        emit_reduce(e, segs, pname(e, E.reduce, e->L[lv[0]], lv[0]));
    }
}
// the LDS layout of the single-workgroup step (tiny_step.hip), in floats: parameters of both nets and the gradient, the observation arena, the Q columns, then per layer
// the online / target activations and dL/dpre; at least the room the priority block's path state needs (it reuses the whole region).  a != null: the offsets are recorded
static size_t tiny_layout(const dqn_engine* e, TinyArgs* a) {
    const int B = e->Bc, ncon = e->ncon, ld0 = 2 * B;
    size_t fl = 0; TinyArgs tmp; TinyArgs& A = a ? *a : tmp;
    auto take = [&](size_t n) { const int o = (int)fl; fl += (n + 3) / 4 * 4; return o; };
    A.pon_off = take(e->Pint); A.ptg_off = take(e->Pint); A.g_off = take(e->Pint); A.x0_off = take((size_t)e->E * ld0); A.misc_off = take((size_t)B * 3 * e->nA);
    for (int i = 0; i < e->nl && i < TINY_MAX_LAYERS; i++) { A.on_off[i] = take((size_t)e->L[i].N * ncon); A.tg_off[i] = take((size_t)e->L[i].N * B); A.d_off[i] = take((size_t)e->L[i].N * B); }
    if (fl * 4 < 7808 + 64 * 4 + 1024) fl = (7808 + 64 * 4 + 1024) / 4;
    return fl;
}
// THE eligibility rule of the single-workgroup step, term by term: empty when the engine takes it, else the reason in words (build_program decides by it; dqn_group_create
// reports it by member).  A pure function of the engine as created (layers, plan, hyper-parameters, switches, communicator): no program needs to exist
std::string tiny_decline(const dqn_engine* e) {
    char buf[200];
    if (e->hp.recurrence) return "it is recurrent (recurrence = true)";
    for (int i = 0; i < e->nl; i++) if (e->L[i].kind != DQN_LAYER_DENSE) { snprintf(buf, sizeof buf, "layer %d is not a Dense layer (kind %d)", i, e->L[i].kind); return buf; }
    if (general_only(e->L, e->nl)) return "one of its layers takes the general train programs only";
    if (e->sim_world || e->comm || e->world > 1) return "it runs as data-parallel replicas (a communicator, or created under DQN_SIM_WORLD)";
    if (!e->hp.prioritized_replay) return "it has no prioritized replay (prioritized_replay = false)";
    if (e->B > 64) { snprintf(buf, sizeof buf, "B > 64 (batch_size = %d)", e->B); return buf; }
    if (e->opt.no_tiny) return "it was created under DQN_NO_TINY";
    const int nlev = (int)net_levels(e).size();
    if (e->nl > TINY_MAX_LAYERS || nlev > TINY_MAX_LAYERS) { snprintf(buf, sizeof buf, "it has too many layers (%d in %d levels, at most %d)", e->nl, nlev, TINY_MAX_LAYERS); return buf; }
    // ~5 MACs per parameter and column on ONE CU: <= ~9 us of arithmetic
    if (e->Pint > 16384 || (size_t)e->Pint * e->Bc > 262144) { snprintf(buf, sizeof buf, "it has too many parameters (%zu, at most 16384 and 262144 / batch_size)", e->Pint); return buf; }
    for (int i = 0; i < e->nl; i++) {
        const LayerDev& L = e->L[i];
        if (dqn_nchunks(L.N, L.dx_kc) != 1) { snprintf(buf, sizeof buf, "the plan cuts layer %d's dX sum into %d chunks (dx_kc = %d); the single-workgroup step sums it in one (dx_kc = 0)", i, dqn_nchunks(L.N, L.dx_kc), L.dx_kc); return buf; }
        if (L.src >= i) { snprintf(buf, sizeof buf, "layer %d reads a later layer (%d)", i, L.src); return buf; }
    }
    // one workgroup may hold up to 160 KB of LDS on gfx950 (beyond 64 KB the launcher raises the function's dynamic-LDS limit)
    const size_t bytes = tiny_layout(e, nullptr) * 4;
    if (bytes > 144 * 1024) { snprintf(buf, sizeof buf, "it needs %zu bytes of LDS (at most %d)", bytes, 144 * 1024); return buf; }
    return std::string();
}
// ---------------------------------------------------------------- the train step's program, stage by stage
// What the stages of build_program share, and nothing else: each stage below is a free function that names what it reads and writes of this record through `b`.
// NOT copyable: every launch closure of this file is [=] and outlives build_program, so a stage copies the scalars its closures need into const locals first; a
// closure that named the builder itself would have to copy the whole record into a std::function -- with the deleted copy constructor it does not compile
struct StepBuild {
    dqn_engine* const e; const int B /* columns of one sequence set: batch_size, or T*batch_size for DRQN */, Bb, T, ncon, ld0; const bool mf, rec;
    const bool general;      // declines, by name, every fusion below that pairs a layer with a neighbour or swallows the whole step: the fused recurrent step, the single-workgroup step, the fused reduce + head launches
    const Levels levels;
    bool fuse_heads = false; int ha_l = -1, hv_l = -1; bool fuse_rh = false; int rh_pa = -1, rh_pv = -1, rh_S = 0;      // the head decision (choose_head_fusion)
    float* hl_buf = nullptr;                       // per-column Huber terms (folded into the loss by a tail task)
    bool wantT[DQN_MAX_LAYERS] = {}; float* actT[DQN_MAX_LAYERS][2] = {};      // transposed copies [column][feature] of the head layers' inputs (written by the split-K reduce): wanted, made
    float* ln_stat[DQN_MAX_LAYERS] = {};           // per LayerNorm layer: (mu, sigma) of the online pass's columns, kept for the backward
    HeadSrc head[DQN_MAX_LAYERS][2]; FwdEmit fe;   // per (layer, net): where k_td finds the layer's output; the forward emitter's record
    std::vector<RSeg> final_segs;                  // dW split-K slabs: nothing reads the gradient before Adam, so ONE reduce launch at the end
    int W = 1; bool dp_on = false, dp_layer[DQN_MAX_LAYERS] = {}; int n_dp = 0; bool overlap_cand = false;      // data-parallel replicas (choose_dp_layers)
    std::vector<VTask> tail_pend;                  // small tasks waiting for a launch to ride on (fused heads: their dW/db and the loss fold)
    bool prio_in_adam = false, pg_want = false, prio_placed = false, prio_draw_pending = false;      // the priority block: place_priority_block decides, the backward levels place, the Adam launch takes what is left
    bool joined = false;                           // the first stream of a dueling join has written join_tmp
    explicit StepBuild(dqn_engine* en) : e(en), B(en->Bc), Bb(en->B), T(en->T), ncon(en->ncon), ld0(2 * en->Bc), mf(en->hp.use_mfma != 0), rec(en->hp.recurrence != 0),
                                         general(general_only(en->L, en->nl)), levels(net_levels(en)) {}
    StepBuild(const StepBuild&) = delete;
};
// the input operand of layer l in the online pass: the observation arena or its producer's activation, and the leading dimension
struct Operand { const float* X; int ldx; };
static Operand operand_of(const StepBuild& b, int l) { const int s = b.e->L[l].src; return {s < 0 ? b.e->x0 : b.e->act_on[s], s < 0 ? b.ld0 : b.ncon}; }
// a layer's input gradient has a reader unless the layer reads the observation -- directly, or through pool and Activation layers only (neither has parameters: its dY would feed nothing)
static bool wants_dx(const dqn_engine* e, int l) { int s = e->L[l].src; while (s >= 0 && (is_pool(e->L[s].kind) || is_actl(e->L[s].kind))) s = e->L[s].src; return s >= 0; }
// where the (K+1) x N gradient block of a layer (or of a recurrent layer's Wi | b / Wh | junk view) lands: its range of the flat gradient, or -- S > 1 plan chunks -- S slabs,
// registered here for the final reduce.  The ONE place that decides it; the order of the calls is the order of final_segs, which adam_segs and dp_pack read
static float* dw_dst(StepBuild& b, const LayerDev& L, int S) {
    if (S <= 1) return b.e->grad + L.w_off;
    float* part = palloc(b.e, (size_t)S * (L.K + 1) * L.N);
    RSeg r; memset(&r, 0, sizeof r); r.part = part; r.S = S; r.elems = (unsigned long long)(L.K + 1) * L.N; r.mode = 2; r.out = b.e->grad + L.w_off; b.final_segs.push_back(r); return part;
}
// the VALU task of one dW block: `cols`-long sample chains in the plan's dw_kc chunks, into the block or its slabs
static VTask valu_dw_task(const LayerDev& V, const float* X, int ldx, const float* dpre, int B, int cols, float* out) {
    VTask t; memset(&t, 0, sizeof t); t.kind = 1; t.L = V; t.X = X; t.ldx = ldx; t.dpre = dpre; t.B = B; t.S = dqn_nchunks(cols, V.dw_kc); t.kc = dqn_chunk_len(cols, V.dw_kc); t.out = out; return t;
}
// the VALU task of one dX problem: S plan chunks of the N-long chains into `out` (the input gradient, or its S slabs); addend: the other stream's dX of a dueling join
static VTask valu_dx_task(const LayerDev& V, const float* P, const float* dpre, int B, int S, float* out, const float* addend, const float* ysrc, int ldy, int act_src) {
    VTask t; memset(&t, 0, sizeof t); t.kind = 2; t.L = V; t.P = P; t.dpre = dpre; t.B = B; t.S = S; t.kc = dqn_chunk_len(V.N, V.dx_kc); t.out = out; t.addend = addend; t.ysrc = ysrc; t.ldy = ldy; t.act_src = act_src; return t;
}
// the reduce of a dX problem's S slabs (mode 1): the sum, + the addend, then the producing layer's activation derivative on its stored output
static RSeg dx_reduce_seg(const LayerDev& V, float* part, int S, int B, float* out, const float* addend, const float* ysrc, int ldy, int act_src) {
    RSeg r; memset(&r, 0, sizeof r); r.part = part; r.S = S; r.elems = (unsigned long long)V.in_feat * B; r.mode = 1; r.act = act_src; r.addend = addend; r.ysrc = ysrc; r.B = B; r.ldy = ldy; r.out = out; return r;
}
// the Adam job over nothing yet: pointers and hyper-parameters.  wt: m, v stored write-through on the engines whose GEMM launches store so (the column-group step never did)
static AdamJob plain_adam_job(const dqn_engine* e, bool wt) {
    AdamJob J; memset(&J, 0, sizeof J); J.p = e->p_on; J.m = e->m; J.v = e->v; J.g = e->grad; J.g_out = e->grad; J.state = e->state; J.gmax_part = e->gmax_part;
    J.f64mode = e->hp.adam_f64_scalars; J.lr = e->hp.learning_rate; J.b1 = e->hp.adam_beta1; J.b2 = e->hp.adam_beta2; J.eps = e->hp.adam_eps; J.gscale = 1.0f;
    J.wt = (wt && e->nl > 0 && (e->L[0].opt & DQN_LOPT_ST_WT)) ? 1 : 0; return J;
}
static PrioArgs prio_args(const StepBuild& b) {
    const dqn_engine* e = b.e; const int Bb = b.Bb;
    PrioArgs pa; memset(&pa, 0, sizeof pa); pa.n = b.B; pa.cap2 = e->cap2; pa.idx = e->idx; pa.td = e->td; pa.eps = e->hp.prio_eps; pa.alpha = e->hp.prio_alpha; pa.tree = e->tree;
    // hp.sample_distinct: pre-drawn (and deduped by the priority block) for the small batches whose fused sample + gather launch understands the list
    // r06: ... and for the large batches whose priority workgroup rides a backward launch (prio_in_bwd): the list it leaves in idx_pre is final -- the
    // Adam launch's pre-gather reads it as it reads a stratified one
    const bool dist_ok = !e->hp.sample_distinct || (Bb <= 64 && !(e->hp.obs_dtype == DQN_OBS_U8 && !e->arena_u8 && (e->E & 3) == 0)) || (Bb > 64 && e->prio_in_bwd);
    if ((Bb <= 64 || e->prio_in_bwd) && dist_ok) { pa.idx_pre = e->idx_pre; pa.seed = e->hp.seed; pa.B = Bb; pa.distinct = e->hp.sample_distinct ? 1 : 0; }      // the fused sample+gather launch (B <= 64) consumes them
    return pa;
}
// ---------------- stage 1: recurrent networks with column-group dW chunks (plan dw_kc = -cg): the step is ONE column-parallel launch + the Adam launch (drqn_cols.hip; BASELINE config 4).
// Returns 1 where it built the whole program, 0 where the plan asks for no column groups, -1 with the refusal
static int column_group_program(StepBuild& b) {
    dqn_engine* e = b.e; const int B = b.B, Bb = b.Bb, T = b.T; const bool mf = b.mf;
    int cgm = 0; bool all_same = true;
    for (int i = 0; i < e->nl; i++) { if (e->L[i].dw_kc < 0) cgm = -e->L[i].dw_kc; all_same = all_same && e->L[i].dw_kc == e->L[0].dw_kc; } if (!cgm) return 0;
    if (!b.rec || !all_same) return fail("plan: column-group dW chunks (dw_kc < 0) need recurrence = true and the same dw_kc on every layer");
    const int nset = e->hp.double_q ? 3 : 2; const LayerDev& L0 = e->L[0];
    bool ok = !b.general && drqn_fused_cg(e->L, e->nl, e->E, Bb, T, e->nA, e->hp.dueling, e->hp.double_q, 1) > 0 && Bb % cgm == 0 && nset * 4 * L0.H * cgm <= 1024 && !e->comm && !e->sim_world && e->world <= 1;
    if (ok) { ok = dqn_nchunks(L0.K, L0.fwd_kc) == 1; for (int i = 1; i < e->nl; i++) ok = ok && dqn_nchunks(e->L[i].N, e->L[i].dx_kc) == 1; }
    if (!ok) return fail("plan: column-group dW chunks (dw_kc = %d) need a network the fused recurrent step covers -- Chain(flattenbatch, LSTM, Dense) with or without the dueling split, "
                         "H a multiple of 8 up to 64, unsplit input projection and head dX, ONE device without a communicator -- use dw_kc >= 0 (plan = NULL picks a plan that fits; with a communicator dqn_comm_init re-derives it)", -cgm);
    DrqnColsArgs a; memset(&a, 0, sizeof a);
    a.B = Bb; a.T = T; a.H = L0.H; a.E = e->E; a.nA = e->nA; a.dueling = e->hp.dueling; a.double_q = e->hp.double_q; a.cg = cgm; a.nset = nset; a.gamma = e->hp.gamma; a.Pint = (unsigned)e->Pint;
    // a CALLER's group size: the default plan picks one whose workgroup fits (drqn_fused_cg); any other is held to the same two bounds here, by name, instead of at the
    // launch -- the per-column tables of the kernel (DRQN_COLS_MAX_CG) and one workgroup's 160 KB of LDS for both networks' parameters and the group's activations
    if (cgm > DRQN_COLS_MAX_CG || (drqn_cols_lds_floats(a) + 64) * sizeof(float) > (size_t)160 * 1024)
        return fail("plan: column-group dW chunks (dw_kc = %d): a group of %d batch columns needs %zu bytes of LDS in the fused recurrent step (at most %d columns and 160 KB) -- use a smaller group (plan = NULL picks one that fits)",
                    -cgm, cgm, drqn_cols_lds_floats(a) * sizeof(float), DRQN_COLS_MAX_CG);
    a.wi_off = (unsigned)L0.w_off; a.b_off = (unsigned)L0.b_off; a.wh_off = (unsigned)L0.wh_off; a.h0_off = (unsigned)L0.h0_off; a.c0_off = (unsigned)L0.c0_off;
    const int ha = e->hp.dueling ? e->last_adv : e->last_base, hv = e->hp.dueling ? e->last_val : -1;
    for (int hd = 0; hd < 2; hd++) { const int l = hd == 0 ? ha : hv; if (l < 0) continue; const LayerDev& L = e->L[l];
        a.hw_off[hd] = (unsigned)L.w_off; a.hb_off[hd] = (unsigned)L.b_off; a.hN[hd] = L.N; a.hact[hd] = L.act; a.h_S[hd] = dqn_nchunks(L.K, L.fwd_kc); a.h_kc[hd] = dqn_chunk_len(L.K, L.fwd_kc); }
    a.p_on = e->p_on; a.p_tg = e->p_tg; a.ep_s = e->ep_s; a.ep_sp = e->ep_sp; a.ep_a = e->ep_a; a.ep_r = e->ep_r; a.ep_done = e->ep_done; a.ep_len = e->ep_len;
    if (!e->draw_idx_h) {      // the draw ring: mapped, coherent pinned host memory (survives program rebuilds; freed with the engine)
        if (e->mem.get_pinned(&e->draw_idx_h, (size_t)DQN_DRAW_SLOTS * Bb, hipHostMallocMapped | hipHostMallocCoherent)) return -1;
        if (e->mem.get_pinned(&e->draw_start_h, (size_t)DQN_DRAW_SLOTS * Bb, hipHostMallocMapped | hipHostMallocCoherent)) return -1;
        memset(e->draw_idx_h, 0, sizeof(long long) * DQN_DRAW_SLOTS * Bb); memset(e->draw_start_h, 0, sizeof(int) * DQN_DRAW_SLOTS * Bb);
        HIPCHK(hipHostGetDevicePointer((void**)&e->draw_idx_d, e->draw_idx_h, 0)); HIPCHK(hipHostGetDevicePointer((void**)&e->draw_start_d, e->draw_start_h, 0));
        for (int k = 0; k < 4; k++) { HIPCHK(hipEventCreateWithFlags(&e->draw_ev[k], hipEventDisableTiming)); e->draw_ev_used[k] = false; }
    }
    a.ring_idx = e->draw_idx_d; a.ring_np = e->draw_start_d;
    if (e->opt.drqn_probe & 4) {      // TIMING PROBE: the draws come from DEVICE memory (episode 0, one row, for every column -- wrong numbers, right schedule): what the PCIe read of the host ring costs
        long long* di = (long long*)palloc(e, (size_t)DQN_DRAW_SLOTS * Bb * 2); int* dn = (int*)palloc(e, (size_t)DQN_DRAW_SLOTS * Bb);
        std::vector<long long> zi((size_t)DQN_DRAW_SLOTS * Bb, 0); std::vector<int> zn((size_t)DQN_DRAW_SLOTS * Bb, 1); if (!di || !dn) return -1;
        HIPCHK(hipMemcpy(di, zi.data(), zi.size() * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dn, zn.data(), zn.size() * 4, hipMemcpyHostToDevice));
        a.ring_idx = di; a.ring_np = dn;
    }
    const int G = Bb / cgm; a.slabs = palloc(e, (size_t)G * e->Pint); a.hl = palloc(e, (size_t)B); a.td = e->td; a.st = e->state;
    a.probe = e->opt.drqn_probe | (mf ? 0 : 2);      // hp.use_mfma = 0: the VALU form of the input projection (the same chains, the same bits)
    if (e->opt.drqn_stamps) { a.stamps = (unsigned long long*)palloc(e, 64); e->drqn_stamps = a.stamps; }
    e->prog.push_back({"drqn_cols", [=](dqn_engine* en) { if (launch_drqn_cols(en->stream, a, en->cur.slot)) en->launch_failed = true; }});      // the slot is baked into the captured node
    e->prog_post_begin = e->prog.size(); AdamJob J = plain_adam_job(e, false);
    J.segs.n = 1; J.segs.beg[0] = 0; J.segs.end[0] = e->Pint; J.segs.part[0] = a.slabs; J.segs.S[0] = G; J.segs.stride[0] = e->Pint; J.segs.blocks = (unsigned)((e->Pint + 255) / 256);
    J.nr = 0; J.sblocks = 1; J.tick = 1; J.slot0 = 0; J.fold_hl = a.hl; J.fold_T = T; J.fold_B = Bb;
    e->adam_step = (long)e->prog.size();
    e->prog.push_back({"adam", [=](dqn_engine* en) { launch_adam(en->stream, J); }});
    e->gmax_used = (int)(J.segs.blocks + J.sblocks); e->drqn_fused = true; return 1;
}
// ---------------- stage 2: networks that fit in LDS: the WHOLE step is one single-workgroup launch (tiny_step.hip; BASELINE config 1).  Returns whether it built the program
static bool single_workgroup_program(StepBuild& b) {
    dqn_engine* e = b.e; const Levels& levels = b.levels;
    if (!tiny_decline(e).empty()) return false; TinyArgs a; memset(&a, 0, sizeof a);
    for (int i = 0; i < e->nl; i++) a.L[i] = e->L[i]; const size_t fl = tiny_layout(e, &a);
    a.nl = e->nl; a.nlev = (int)levels.size(); a.B = b.B; a.nA = e->nA; a.E = e->E; a.ncon = b.ncon; a.dueling = e->hp.dueling; a.double_q = e->hp.double_q; a.obs_u8 = e->hp.obs_dtype == DQN_OBS_U8 ? 1 : 0; a.distinct = e->hp.sample_distinct ? 1 : 0;
    a.last_base = e->last_base; a.last_val = e->last_val; a.last_adv = e->last_adv;
    a.gamma = e->hp.gamma; a.beta = e->hp.prio_beta; a.prio_eps = e->hp.prio_eps; a.prio_alpha = e->hp.prio_alpha; a.cap2 = e->cap2; a.seed = e->hp.seed; a.P = e->Pint;
    for (size_t li = 0; li < levels.size(); li++) { a.lev_n[li] = (int)levels[li].size(); a.lev_l[li][0] = levels[li][0]; a.lev_l[li][1] = levels[li].size() > 1 ? levels[li][1] : levels[li][0]; }
    a.lds_bytes = (unsigned)(fl * 4);
    a.p_tg = e->p_tg; a.p_on = e->p_on; a.m = e->m; a.v = e->v; a.grad = e->grad; a.state = e->state; a.gmax_part = e->gmax_part; a.tree = e->tree;
    a.idx = e->idx; a.idx_pre = e->idx_pre; a.s_rows = e->s_rows; a.sp_rows = e->sp_rows; a.ra = e->ra; a.rr = e->rr; a.rdone = e->rdone;
    a.x0 = e->x0; a.w_is = e->w_is; a.td = e->td; a.q_on_s = e->q_on_s; a.q_on_sp = e->q_on_sp; a.q_tg_sp = e->q_tg_sp; a.ytarget = e->ytarget; a.best = e->best;
    a.f64mode = e->hp.adam_f64_scalars; a.lr = e->hp.learning_rate; a.b1 = e->hp.adam_beta1; a.b2 = e->hp.adam_beta2; a.adam_eps = e->hp.adam_eps;
    e->tiny_args.assign(1, a); const TinyArgs* a_dev = upload(e, e->tiny_args); const unsigned lds = a.lds_bytes;
    e->prog.push_back({"tiny_step", [=](dqn_engine* en) { if (launch_tiny_step(en->stream, a_dev, lds, en->cur.sampled ? 1 : 0, en->opt.tiny_stop)) en->launch_failed = true; }});
    e->tiny = true; e->prog_post_begin = e->prog.size(); e->gmax_used = 1; return true;
}
// ---------------- stage 3: u8 replay: keep the observation arena in BYTES when its only consumers are the LDS-tiled forward and dW launches of ONE
// first layer (they convert byte / 255 inside their tile loads): the gather writes 1 byte per element instead of 4 and the first layer reads
// a quarter of the bytes.  Everything else (VALU / direct-MFMA fallbacks, heads fed by the observation, the operand all-gather) needs floats.
static void choose_byte_arena(StepBuild& b) {
    dqn_engine* e = b.e; const int B = b.B, ld0 = b.ld0; const Levels& levels = b.levels;
    if (!(e->hp.obs_dtype == DQN_OBS_U8 && !b.rec && b.mf && B % 4 == 0 && e->E % 4 == 0 && levels.size() > 1)) return;
    int n_src = 0; for (int i = 0; i < e->nl; i++) if (e->L[i].src < 0) n_src++; const int l0 = levels[0][0];
    int ldx2[2] = {ld0, ld0}, c02[2] = {0, B}, nc2[2] = {b.ncon, B};
    if (n_src == 1 && levels[0].size() == 1 && e->L[l0].src < 0 && !is_pool(e->L[l0].kind) /* pool.hip reads floats: a pool as the first layer keeps the fp32 arena */ && (e->L[l0].kind == DQN_LAYER_CONV || (!e->comm && !e->sim_world)) &&
        (is_padded(e->L[l0]) || is_cdg(e->L[l0].kind) /* conv_own.hip converts bytes in its operand loads */ || (gemm_fwd_eligible(e->L[l0], 2, ldx2, c02, nc2) && gemm_dw_eligible(e->L[l0], B, ld0)))) { e->arena_u8 = true; e->L[l0].xu8 = 1; }
}
// ---------------- stage 4: small batches: the head level (forwards of both nets), the TD kernel and the head layers' dX run as ONE launch with a
// workgroup per batch column (k_head_td); the heads' dW/db and the loss fold ride as tail tasks of the next backward launch
// (r03: at ANY batch -- at B = 512 the four launches it replaces, head forwards / slab reduce / single-workgroup k_td / head dX, took 40 us)
static void choose_head_fusion(StepBuild& b) {
    dqn_engine* e = b.e; const int B = b.B; const Levels& levels = b.levels;
    if (!b.rec) {
        const auto& lv = levels.back();
        if (e->hp.dueling && lv.size() == 2 && lv[0] == e->last_val && lv[1] == e->last_adv) { b.hv_l = lv[0]; b.ha_l = lv[1]; }
        else if (!e->hp.dueling && lv.size() == 1 && lv[0] == e->last_base) b.ha_l = lv[0];
        if (b.ha_l >= 0) {
            b.fuse_heads = true; size_t lds = (size_t)(1 + e->nA) * 4;
            for (int l : lv) {
                const LayerDev& L = e->L[l];
                b.fuse_heads = b.fuse_heads && L.kind == DQN_LAYER_DENSE && dqn_nchunks(L.N, L.dx_kc) == 1 && (L.src < 0 || !is_recurrent(e->L[L.src].kind));
                lds += ((size_t)3 * L.K + (size_t)3 * L.N * dqn_nchunks(L.K, L.fwd_kc) + (size_t)3 * L.N) * 4;
            }
            b.fuse_heads = b.fuse_heads && lds <= 60 * 1024;
        }
    }
    b.hl_buf = b.fuse_heads ? palloc(e, (size_t)B) : nullptr;
    // ---------------- r05: when the head layers sit on dense hidden layers whose forward ran split-K, the split-K reduce AND the head level are ONE chip-filling launch
    // (red_head.hip: workgroup = 4 batch columns x stream x plan chunk of 32 hidden rows, the last arriver of a column group does TD + the heads' dX) instead of
    // k_reduce_multi (384 workgroups) + k_head_td (B workgroups)
    const int ha_l = b.ha_l, hv_l = b.hv_l;
    if (b.fuse_heads && !b.general && !e->opt.no_red_head && !e->opt.probe_no_tg && !e->opt.head_dbg) {
        b.rh_S = fused_head_layout(e, levels, ha_l, hv_l, &b.rh_pa, &b.rh_pv);
        // S > 1: k_red_head (split-K producers, small batches).  S == 1 -- finished activations of an unsplit forward, i.e. large batches: k_head_cols4, one workgroup per
        // column group (k_red_head's (group, stream, chunk) decomposition is SLOWER there: 27.4 vs 21.3 us for k_head_td at B = 512, profiles/history/r05_k_cfg5_red_head_ab.txt --
        // 4096 workgroups each staging both streams' head weights)
        b.fuse_rh = b.rh_S > 0 && (b.rh_S > 1 || e->opt.no_head_cols4 != 1) && red_head_ok(B, e->L[ha_l].K, b.rh_S, e->nA, hv_l >= 0 ? 2 : 1, e->L[ha_l].N, hv_l >= 0 ? e->L[hv_l].N : 0);
    }
    // k_head_td and k_head_cols4 (unsplit producers) read their input columns out of transposed copies
    if (b.fuse_heads && (!b.fuse_rh || b.rh_S == 1)) for (int l : levels.back()) if (e->L[l].src >= 0) b.wantT[e->L[l].src] = true;
}
// the recurrence of layer l behind its batched input projection: each launch advances the online s-sequence, the online sp-sequence (double-Q) and the target sp-sequence
// from the reset state (Flux.reset!, src/solver.jl:249-250,271) -- ONE launch for the whole recurrence where the cell's whole-sequence kernels fit, else T
static void emit_recurrence(StepBuild& b, int l) {
    dqn_engine* e = b.e; const int B = b.B, Bb = b.Bb, T = b.T, ncon = b.ncon;
    const LayerDev L = e->L[l]; const CellOps* C = cell_ops(L.kind); const int H = L.H;
    auto args = [&](int t) {      // the sequence sets before step t
        CellFwdArgs a; memset(&a, 0, sizeof a); a.H = H; a.B = Bb; a.T = T; a.act = L.cell_act;
        auto seq = [&](const float* P, const float* gx, float* hout, float* cst, int ld, int c0, bool keep) {
            CellSeq& q = a.s[a.nseq++]; q.Gx = gx; q.Hout = hout; q.Cst = cst; q.ld = ld; q.c0 = c0; q.Wh = P + L.wh_off; q.bias = P + L.b_off;
            if (t == 0) { q.hprev = P + L.h0_off; q.hp_ld = 1; q.hp_bs = 0; if (C->has_c) { q.cprev = P + L.c0_off; q.cp_ld = 1; q.cp_bs = 0; } }
            else { q.hprev = hout + c0 + (t - 1) * Bb; q.hp_ld = ld; q.hp_bs = 1; if (C->has_c) { q.cprev = cst + c0 + (t - 1) * Bb; q.cp_ld = ld; q.cp_bs = 1; } }
            if (keep) { q.gates = e->gates[l]; q.aux = e->tcb[l]; q.hprev_out = e->hprev_buf[l]; q.cprev_out = e->cprev_buf[l]; q.keep_ld = B; q.keep_c0 = 0; }      // null where the cell has none
        };
        seq(e->p_on, e->gx_on[l], e->act_on[l], e->cst_on[l], ncon, 0, true);
        if (e->hp.double_q) seq(e->p_on, e->gx_on[l], e->act_on[l], e->cst_on[l], ncon, B, false);
        seq(e->p_tg, e->gx_tg[l], e->act_tg[l], e->cst_tg[l], B, 0, false);
        return a;
    };
    if (C->seq_fits(H, Bb, T) && !stepwise(e->opt, L.kind)) {
        const CellFwdArgs a = args(0); e->prog.push_back({lname(e, "%s_seq_%s%d", C->name, kind_traits(L).tag, l), [=](dqn_engine* en) { C->launch_seq(en->stream, a); }});
    } else
    for (int t = 0; t < T; t++) {
        const CellFwdArgs a = args(t); e->prog.push_back({lname(e, "%s_step_%s%d", C->name, kind_traits(L).tag, l), [=](dqn_engine* en) { C->launch_step(en->stream, a, t); }});
    }
}
// ---------------- stage 5: forward: online net on [s ; sp] (src/solver.jl:210,220), target net on sp (:211), level by level, the recurrence launches behind a recurrent level
static void emit_forward_levels(StepBuild& b) {
    dqn_engine* e = b.e; const int B = b.B, ncon = b.ncon, ld0 = b.ld0; const Levels& levels = b.levels;
    // forward outputs: a recurrent layer's batched part is its bias-free input projection Gx = Wi*x over ALL columns (gx_view, writing gx_*); the recurrence then
    // runs as T small launches (or one).
    float *fwd_on[DQN_MAX_LAYERS], *fwd_tg[DQN_MAX_LAYERS];
    for (int i = 0; i < e->nl; i++) { const bool r = is_recurrent(e->L[i].kind); fwd_on[i] = r ? e->gx_on[i] : e->act_on[i]; fwd_tg[i] = r ? e->gx_tg[i] : e->act_tg[i]; }
    std::vector<FwdPass> passes = {{e->p_on, e->x0, ld0, 0, e->act_on, fwd_on, ncon, "fwd_on"}, {e->p_tg, e->x0, ld0, B, e->act_tg, fwd_tg, B, "fwd_tg"}};
    if (e->opt.probe_no_tg) passes.pop_back();      // TIMING PROBE (wrong numbers, right schedule): the forward launches without the target network's problems
    FwdEmit& fe = b.fe; fe.gemm = "fwd"; fe.valu = "fwd_valu"; fe.reduce = "fwd_reduce"; fe.skip_last = b.fuse_heads /* computed inside k_head_td */; fe.byte_arena = true;
    if (b.fuse_rh) { fe.prod[0] = b.rh_pa; fe.prod[1] = b.rh_pv; fe.pm_ok = b.rh_S > 1 && !e->opt.no_rh_pm; }
    fe.last_on_the_fly = !b.rec && e->B <= 64; fe.wantT = b.wantT; fe.actT = b.actT; fe.ln_stat = b.ln_stat; fe.do_cols = B /* the s columns of the online pass */; fe.head = b.head;
    for (size_t li = 0; li < levels.size(); li++) { emit_forward(e, levels, li, li + 1, passes, fe); if (is_recurrent(e->L[levels[li][0]].kind)) emit_recurrence(b, levels[li][0]); }
    if (e->opt.probe_no_tg) for (int l = 0; l < e->nl; l++) if (b.wantT[l] && b.actT[l][0]) b.actT[l][1] = palloc(e, (size_t)e->L[l].out_feat * B);      // (never written: the head kernel still gets a buffer)
}
// ---------------- stage 6: dueling reduce + argmax + Bellman target + TD + Huber + dL/dQ + priority update: one of four launches
// (a) split-K reduce + head level + TD + the heads' dX as one chip-filling launch (red_head.hip: k_red_head, or k_head_cols4 on unsplit producers)
static int emit_red_head(StepBuild& b) {
    dqn_engine* e = b.e; const int B = b.B, ncon = b.ncon, ha_l = b.ha_l, hv_l = b.hv_l; const FwdEmit& fe = b.fe;
    RedHeadArgs h; memset(&h, 0, sizeof h); const LayerDev& La = e->L[ha_l];
    h.B = B; h.nA = e->nA; h.K = La.K; h.S = b.rh_S; h.ncon = ncon; h.nstream = hv_l >= 0 ? 2 : 1; h.NO = e->nA + (hv_l >= 0 ? 1 : 0); h.double_q = e->hp.double_q;
    h.gamma = e->hp.gamma; h.pm = fe.pm ? 1 : 0;
    for (int st = 0; st < h.nstream; st++) {
        const int hl_ = st == 0 ? ha_l : hv_l, pl_ = st == 0 ? b.rh_pa : b.rh_pv; const LayerDev& H = e->L[hl_]; const LayerDev& P = e->L[pl_]; RedHeadStream& T = h.st[st];
        T.part[0] = fe.part[st][0]; T.part[1] = fe.part[st][1]; T.partT[0] = fe.partT[st][0]; T.partT[1] = fe.partT[st][1]; T.pbias[0] = e->p_on + P.b_off; T.pbias[1] = e->p_tg + P.b_off; T.pact = P.act;
        T.W[0] = e->p_on + H.w_off; T.W[1] = e->p_tg + H.w_off; T.hbias[0] = e->p_on + H.b_off; T.hbias[1] = e->p_tg + H.b_off; T.N = H.N; T.hact = H.act;
        T.y_on = e->act_on[pl_]; T.dpre = e->dact[hl_]; T.dsrc = e->dact[pl_];
    }
    if (h.nstream == 1) h.st[1] = h.st[0];      // (never read: keeps every pointer of the record valid)
    { bool allT = true; for (int st = 0; st < h.nstream; st++) allT = allT && h.st[st].partT[0] && h.st[st].partT[1];      // transposed copies: all four or none
      if (!allT || e->opt.no_head_cols4 == 2) for (int st = 0; st < 2; st++) h.st[st].partT[0] = h.st[st].partT[1] = nullptr; }
    h.bm_a = e->gb_a2; h.bm_r = e->gb_r2; h.bm_done = e->gb_done2; h.bm_w = e->gb_w2;
    h.w_is = e->w_is; h.td = e->td; h.q_on_s = e->q_on_s; h.q_on_sp = e->q_on_sp; h.q_tg_sp = e->q_tg_sp; h.ytarget = e->ytarget; h.best = e->best; h.hl = b.hl_buf; h.stt = e->state;
    h.idx = e->idx; h.idx_pre = e->idx_pre; const int Gc = B / 4, NC = h.K / 32;
    h.partials = palloc(e, (size_t)Gc * 12 * h.NO * NC); h.tickets = (unsigned*)palloc(e, (size_t)Gc);
    h.ypm = (h.S > 1 && !e->opt.no_rh_pm) ? palloc(e, (size_t)Gc * h.nstream * h.K * 4) : nullptr;
    if (!h.tickets) return -1;      // (refused: the message is the scope's, as below)
    HIPCHK(hipMemset(h.tickets, 0, (size_t)Gc * 4));      // armed once; every launch's last arrivers re-arm their groups
    if (e->opt.drqn_stamps) { h.stamps = (unsigned long long*)palloc(e, 64); if (!h.stamps) return -1; HIPCHK(hipMemset(h.stamps, 0, 256)); e->drqn_stamps = h.stamps; }
    const RedHeadArgs* h_dev = upload(e, std::vector<RedHeadArgs>(1, h));
    e->prog.push_back({h.S == 1 ? "head_cols4" : "red_head", [=](dqn_engine* en) { launch_red_head(en->stream, h, h_dev, en->cur.sampled ? 1 : 0, en->cur.take_pre ? 1 : 0); }});
    return 0;
}
// (b) head level + TD + the heads' dX with a workgroup per batch column (k_head_td)
static void emit_head_td(StepBuild& b) {
    dqn_engine* e = b.e; const int B = b.B, ncon = b.ncon, ld0 = b.ld0, ha_l = b.ha_l, hv_l = b.hv_l;
    HeadTdArgs h; memset(&h, 0, sizeof h); h.B = B; h.nA = e->nA; h.dueling = e->hp.dueling; h.double_q = e->hp.double_q; h.gamma = e->hp.gamma; h.prio_beta = e->hp.prio_beta; h.cap2 = e->cap2;
    h.bm_a = e->gb_a2; h.bm_r = e->gb_r2; h.bm_done = e->gb_done2; h.bm_w = e->gb_w2;
    h.w_is = e->w_is; h.td = e->td; h.q_on_s = e->q_on_s; h.q_on_sp = e->q_on_sp; h.q_tg_sp = e->q_tg_sp; h.ytarget = e->ytarget; h.best = e->best; h.st = e->state;
    h.hl = b.hl_buf; h.idx = e->idx; h.idx_pre = e->idx_pre;
    auto fill = [&](HeadLayer& H, int l) {
        const LayerDev& L = e->L[l];
        H.K = L.K; H.N = L.N; H.S = dqn_nchunks(L.K, L.fwd_kc); H.kc = dqn_chunk_len(L.K, L.fwd_kc); H.act = L.act;
        H.W[0] = e->p_on + L.w_off; H.bias[0] = e->p_on + L.b_off; H.W[1] = e->p_tg + L.w_off; H.bias[1] = e->p_tg + L.b_off;
        if (L.src < 0) { H.X[0] = H.X[1] = e->x0; H.ldx[0] = H.ldx[1] = ld0; H.c0[0] = 0; H.c0[1] = B; }
        else { H.X[0] = e->act_on[L.src]; H.ldx[0] = ncon; H.c0[0] = 0; H.X[1] = e->act_tg[L.src]; H.ldx[1] = B; H.c0[1] = 0; H.XT[0] = b.actT[L.src][0]; H.XT[1] = b.actT[L.src][1]; }
        H.dpre = e->dact[l];
        if (L.src >= 0) { H.dsrc = e->dact[L.src]; H.ysrc = e->act_on[L.src]; H.ldy = ncon; H.act_src = src_act(e, l); }
    };
    fill(h.adv, ha_l); if (hv_l >= 0) { fill(h.val, hv_l); h.join = (e->L[hv_l].src == e->L[ha_l].src && e->L[ha_l].src >= 0) ? 1 : 0; }
    {   // stage the head weights in LDS when they fit beside the input columns
        bool ok = true; for (int l : b.levels.back()) { const LayerDev& L = e->L[l]; ok = ok && ((size_t)L.K * L.N) % 4 == 0 && L.w_off % 4 == 0; }
        h.stage_w = 0; if (ok) { h.stage_w = 1; if (head_td_lds_bytes(h) > 60 * 1024) h.stage_w = 0; }
    }
    h.dbg = e->opt.head_dbg; const HeadTdArgs* h_dev = upload(e, std::vector<HeadTdArgs>(1, h));
    e->prog.push_back({"head_td", [=](dqn_engine* en) { launch_head_td(en->stream, h, h_dev, en->cur.sampled ? 1 : 0, en->cur.take_pre ? 1 : 0); }});
}
// (c), (d) the head level ran as forward launches: the single-workgroup TD kernel, or the masked sequence form of a recurrent network
static void emit_td_plain(StepBuild& b) {
    dqn_engine* e = b.e; const int B = b.B, ncon = b.ncon; TdArgs t; memset(&t, 0, sizeof t);
    t.B = B; t.nA = e->nA; t.ncon = ncon; t.dueling = e->hp.dueling; t.double_q = e->hp.double_q; t.prioritized = e->hp.prioritized_replay;
    t.gamma = e->hp.gamma; t.prio_beta = e->hp.prio_beta; t.prio_eps = e->hp.prio_eps; t.prio_alpha = e->hp.prio_alpha; t.cap2 = e->cap2;
    t.idx = e->idx; t.a = e->ra; t.r = e->rr; t.done = e->rdone; t.tree = e->tree;
    const int lq = e->hp.dueling ? e->last_adv : e->last_base;
    t.on_adv = b.head[lq][0]; t.tg_adv = b.head[lq][1]; t.d_adv = e->dact[lq];
    if (e->hp.dueling) { t.on_val = b.head[e->last_val][0]; t.tg_val = b.head[e->last_val][1]; t.d_val = e->dact[e->last_val]; }
    t.idx_mut = e->idx; t.idx_pre = e->idx_pre; t.w_is = e->w_is; t.td = e->td; t.q_on_s = e->q_on_s; t.q_on_sp = e->q_on_sp; t.q_tg_sp = e->q_tg_sp; t.ytarget = e->ytarget; t.best = e->best; t.st = e->state;
    if (!b.rec) { e->prog.push_back({"td_huber", [=](dqn_engine* en) { TdArgs a = t; a.bump_sample_ctr = en->cur.sampled ? 1 : 0; a.take_pre = en->cur.take_pre ? 1 : 0; launch_td(en->stream, a); }}); return; }
    TdDrqnArgs d; memset(&d, 0, sizeof d); d.B = b.Bb; d.T = b.T; d.nA = e->nA; d.ncon = ncon; d.dueling = e->hp.dueling; d.double_q = e->hp.double_q; d.gamma = e->hp.gamma;
    d.on_val = t.on_val; d.on_adv = t.on_adv; d.tg_val = t.tg_val; d.tg_adv = t.tg_adv; d.d_val = t.d_val; d.d_adv = t.d_adv;
    d.a = e->r_a; d.r = e->r_r; d.done = e->r_done; d.mask = e->r_mask; d.td = e->td; d.st = e->state;
    e->prog.push_back({"td_huber_drqn", [=](dqn_engine* en) { launch_td_drqn(en->stream, d); }});
}
static int emit_td(StepBuild& b) { if (b.fuse_rh) return emit_red_head(b); if (b.fuse_heads) emit_head_td(b); else emit_td_plain(b); return 0; }
// ---------------- stage 7: where the priority block runs.
// update_priorities! (src/solver.jl:231-233) needs only idx and td.  For small batches it rides as a dedicated block of the Adam launch; at
// B > 64 its B leaf paths x log2(cap) levels (~70 us at B = 512, 1e6 leaves) would be that launch's tail, so it runs on a side stream
// concurrently with the whole backward pass and is joined before the optimizer (a graph fork/join costs ~15 us -- only worth it here).
// ... unless a backward launch can carry it as a workgroup of its own (r03: the fork + join nodes themselves cost 12 + 10 us of the main
// stream at config 5, and the block -- split in two, update then draws -- is shorter than the 57-87 us launches it rides in)
static void place_priority_block(StepBuild& b) {
    dqn_engine* e = b.e; const int B = b.B, Bb = b.Bb; const bool rec = b.rec;
    int carriers = 0;      // levels with an LDS-tiled dW launch that can carry the block
    if (!rec && e->hp.prioritized_replay && Bb > 64 && Bb <= 1024 && b.mf && !e->comm && !e->sim_world)
        for (const auto& lvq : b.levels) for (int l2 : lvq) if (dw_carrier_ok(e, l2, B, operand_of(b, l2).ldx)) { carriers++; break; }
    e->prio_in_bwd = carriers >= 2;
    if (!rec && e->hp.prioritized_replay && Bb > 64 && !e->prio_in_bwd) {
        e->prio_forked = true;
        e->prog.push_back({"prio_fork", [](dqn_engine* en) {
            hipEventRecord(en->ev_fork, en->stream); hipStreamWaitEvent(en->stream2, en->ev_fork, 0);
            launch_update_priorities(en->stream2, en->B, en->cap2, en->idx, en->td, en->hp.prio_eps, en->hp.prio_alpha, en->tree, en->state, 0, 1.0, 1.0, nullptr, 0,
                                     en->hp.sample_distinct ? nullptr : en->idx_pre, en->hp.seed, en->B);      // + the next step's index draw (stratified mode)
            hipEventRecord(en->ev_join, en->stream2); }});
    }
    b.prio_in_adam = e->hp.prioritized_replay && !rec && (Bb <= 64 || e->prio_in_bwd);      // larger batches: a backward launch's workgroup, or the side stream (prio_fork)
    // pre-gather (common.h PreGather): needs the priority block (which also draws the next indices) OUT of the Adam launch -- it rides as
    // workgroup 0 of the first LDS-tiled backward launch instead
    // large batches: the priority update runs on the side stream (prio_fork) and draws the next indices there; k_td takes the pre-drawn batch
    b.pg_want = e->hp.prioritized_replay && !rec && (b.prio_in_adam ? (b.fuse_heads || e->prio_in_bwd) : e->prio_forked) && !e->sim_world &&
                (e->hp.obs_dtype != DQN_OBS_U8 || e->arena_u8) && !e->opt.no_pregather && (!e->hp.sample_distinct || Bb <= 64 || e->prio_in_bwd);      // u8 rows: only onto the byte arena; distinct mode at B > 64 without a carrying backward launch: sample launch + gather launch every step
}
// ---------------- stage 8: data-parallel replicas: which layers' dW is computed AFTER the exchange from gathered operands (dp.hip), and whether their operands travel early
static void choose_dp_layers(StepBuild& b) {
    dqn_engine* e = b.e; const int B = b.B; const Levels& levels = b.levels;
    b.W = e->sim_world ? e->sim_world : e->world; b.dp_on = (e->comm || e->sim_world) && !b.rec && !e->opt.dp_allreduce;
    if (b.dp_on) for (int i = 0; i < e->nl; i++) {
        const LayerDev& L = e->L[i];
        // a wide dense layer whose operands (X: K x B, dpre: N x B per rank) are smaller than its gradient, one chain over all W*B samples
        if (L.kind == DQN_LAYER_DENSE && b.mf && (size_t)(L.K + 1) * L.N > (size_t)4 * (L.K + L.N) * B && L.dw_kc == 0 && B % 32 == 0 && gemm_dw_eligible(L, b.W * B, B) && b.n_dp < 8) { b.dp_layer[i] = true; b.n_dp++; }
    }
    // dp_overlap: with fused heads the operands of the flagged wide dense layers (X from the forward pass, dpre from k_head_td) are final HERE, before any
    // backward launch: pack and exchange them now, on the exchange stream, while the conv backward runs (SURVEY 8e "overlapped with backward")
    // Measured at world 1, where there is nothing to hide, the fork + join of the exchange stream cost 26 us per step (one-graph replica step 155.8 -> 181.9 us): it pays
    // once the first all-gather takes longer than that.  r06: decided HERE from the world size and the bytes instead of by an environment knob -- the wide operands of one
    // rank over W - 1 ring hops of one 153 GB/s xGMI link + 15 us of collective latency (the worst shape RCCL can pick on point-to-point links; unmeasured: no multi-GPU
    // box) against the 26 us; DQN_DP_OVERLAP = 1 / 0 still forces it (tests, A/B on real hardware)
    bool want_overlap = e->opt.dp_overlap > 0;
    if (e->opt.dp_overlap < 0 && b.dp_on) {
        double bytes_a = 0.0; for (int i = 0; i < e->nl; i++) if (b.dp_layer[i]) bytes_a += 4.0 * (double)(e->L[i].K + e->L[i].N) * (double)B;
        want_overlap = b.W >= 2 && !e->sim_world && (double)(b.W - 1) * bytes_a / 153e9 * 1e6 + 15.0 > 26.0;
    }
    b.overlap_cand = b.dp_on && b.n_dp > 0 && b.fuse_heads && levels.size() >= 2 && want_overlap;
    if (b.overlap_cand) for (int i = 0; i < e->nl; i++) if (b.dp_layer[i]) { bool in_lvl = false; for (int l : levels[levels.size() - 2]) in_lvl = in_lvl || l == i; b.overlap_cand = b.overlap_cand && in_lvl; }
    if (b.overlap_cand) { e->prog.push_back({"dp_pack_wide", [](dqn_engine* en) { if (en->dp_overlap) launch_dp_pack(en->stream, en->dp_pk_a); }}); e->prog_pre1_end = e->prog.size(); }
}
// ---------------- stage 9: backward of the online net on the s columns (Zygote through src/solver.jl:219-225), level by level from the heads down
// (removed in r06: DQN_ADAM_MODE=1, the Adam update of layers whose gradient is already final carried as tail workgroups of the backward launches -- measured slower in
//  rounds 2, 3, 4 and, as "the stream in the free CU slots", 5: 159.3 vs 156.9 us/step in r02, +3.4 us per carrying launch for -2.75 us of Adam in r05; docs/history/r02.md, r05.md)
// What the layers of ONE level share: the level's VALU task table, the launches that run after every launch of the level, dwl / dxl -- the LDS-tiled dW / dX problem of a
// GEMM kind, held back until the next one of its kind or the level's end, where dW and dX become one launch and carry the waiting tails (finish_level) -- and whether the
// level's two sibling layers got their dW from one fused launch
struct DwL { bool on = false; LayerDev L; int nprob = 0; const float* X[2]; int ldx = 0; const float* d[2]; float* o[2]; const char* name = ""; };
struct DxL { bool on = false; LayerDev L; int nsrc = 0; const float* W[2]; const float* d[2]; float* out = nullptr; const float* ys = nullptr; int act_src = 0; const char* name = ""; };
struct LevelBwd { std::vector<VTask> pend; std::vector<dqn_engine::Step> post_level; DwL dwl; DxL dxl; bool dw_done_sibling = false; };
static void flush_dw(StepBuild& b, LevelBwd& v) {
    if (!v.dwl.on) return; const DwL a = v.dwl; const int B = b.B; v.dwl.on = false;
    b.e->prog.push_back({a.name, [=](dqn_engine* en) { launch_gemm_dw(en->stream, a.L, a.nprob, a.X, a.ldx, a.d, B, a.o); }});
}
static void flush_dx(StepBuild& b, LevelBwd& v) {
    if (!v.dxl.on) return; const DxL a = v.dxl; const int B = b.B, ncon = b.ncon; v.dxl.on = false;
    b.e->prog.push_back({a.name, [=](dqn_engine* en) { launch_gemm_dx(en->stream, a.L, a.nsrc, a.W, a.d, B, a.out, a.ys, ncon, a.act_src); }});
}
// THE contraction ladder of one dW block over B-long chains: LDS-tiled launch, else direct MFMA launch, else a VALU task of the level.  Returns where the block (or its
// slabs) lands.  small_dw: the caller's rule that sends the block to the VALU table whatever the MFMA kernels would take
static float* emit_dw_single(StepBuild& b, LevelBwd& v, const LayerDev V, const float* X, int ldx, const float* dpre, const char* name, bool small_dw) {
    dqn_engine* e = b.e; const int B = b.B; const bool mf = b.mf; float* grad = e->grad;
    const int S = dqn_nchunks(B, V.dw_kc); float* dst = dw_dst(b, V, S); float* part = S > 1 ? dst : nullptr;
    if (mf && !small_dw && gemm_dw_eligible(V, B, ldx)) { struct A { const float* X[1]; const float* d[1]; float* o[1]; } a; a.X[0] = X; a.d[0] = dpre; a.o[0] = dst;
        e->prog.push_back({name, [=](dqn_engine* en) { launch_gemm_dw(en->stream, V, 1, a.X, ldx, a.d, B, a.o); }}); }
    else if (mf && !small_dw && mfma_dw_ok(V, B)) e->prog.push_back({name, [=](dqn_engine* en) { launch_mfma_dw(en->stream, V, X, ldx, dpre, B, grad, part, false); }});
    else v.pend.push_back(valu_dw_task(V, X, ldx, dpre, B, B, dst));
    return dst;
}
// THE contraction ladder of one dX problem of layer l (V: the layer, or a recurrent layer's Wi view): LDS-tiled launch, else direct MFMA launch, else a VALU task; where the
// plan cuts the sum into S > 1 chunks the launch cannot combine itself: S slabs, the level's VALU table flushed, a one-segment reduce.  The arguments are the rules that differ:
//   hold    -- the LDS-tiled problem waits in the level's dxl for the level's end (GEMM kinds) instead of launching here (a recurrent layer's input projection)
//   mfma_n16-- the direct MFMA rung only takes N >= 16 (GEMM kinds)
//   addend  -- the second stream of a dueling join adds the first stream's dX: no LDS-tiled launch, no internal chunks
static void emit_dx_single(StepBuild& b, LevelBwd& v, int l, const LayerDev V, const float* dpre, int S_plan, bool hold, bool mfma_n16, const float* addend, float* out, const float* ysrc) {
    dqn_engine* e = b.e; const int B = b.B, ncon = b.ncon; const bool mf = b.mf; const LayerDev& L = e->L[l]; const float* P = e->p_on; const int act_src = src_act(e, l);
    const int S = (mf && !addend && gemm_dx_internal_chunks(V, B, ncon)) ? 1 : S_plan;      // internal: the launch combines its plan chunks itself (no slabs)
    float* part = S > 1 ? palloc(e, (size_t)S * V.in_feat * B) : nullptr;
    if (mf && !addend && gemm_dx_eligible(V, B, ncon)) {
        flush_dx(b, v); DxL& x = v.dxl; x.on = true; x.L = V; x.nsrc = 1; x.W[0] = x.W[1] = P + V.w_off; x.d[0] = x.d[1] = dpre;
        x.out = S > 1 ? part : out; x.ys = S > 1 ? nullptr : ysrc; x.act_src = act_src; x.name = pname(e, "dx", L, l);
        if (S > 1 || !hold) flush_dx(b, v);   // its partial slabs are reduced right below
    }
    else if (mf && (!mfma_n16 || V.N >= 16) && mfma_dx_ok(V, B, ncon)) e->prog.push_back({pname(e, "dx", L, l), [=](dqn_engine* en) { launch_mfma_dx(en->stream, V, P, dpre, B, out, part, addend, ysrc, ncon, act_src, false); }});
    else v.pend.push_back(valu_dx_task(V, P, dpre, B, S, S > 1 ? part : out, addend, ysrc, ncon, act_src));
    if (S > 1) { flush_valu(e, v.pend, pname(e, "bwd_valu", L, l)); std::vector<RSeg> one(1, dx_reduce_seg(V, part, S, B, out, addend, ysrc, ncon, act_src)); emit_reduce(e, one, pname(e, "dx_reduce", L, l)); }
}
// fused heads: the head layers' dX already ran inside k_head_td; their dW/db (one B-long chain per weight) and the loss fold are tail tasks
static void queue_head_tails(StepBuild& b, const std::vector<int>& lv) {
    dqn_engine* e = b.e; const int B = b.B;
    for (int l : lv) { const LayerDev L = e->L[l]; const Operand in = operand_of(b, l);      // large batches: plan chunks of the B-long chains, slabs summed with the other dW slabs
        b.tail_pend.push_back(valu_dw_task(L, in.X, in.ldx, e->dact[l], B, B, dw_dst(b, L, dqn_nchunks(B, L.dw_kc)))); }
    VTask f; memset(&f, 0, sizeof f); f.kind = 3; f.dpre = b.hl_buf; f.B = B; f.out = &e->state->loss; b.tail_pend.push_back(f);
}
// whatever its kind, l may be the FIRST inner layer of a skip block: the block's entry launch is queued behind its level (post_level)
static void queue_skip_entry(StepBuild& b, LevelBwd& v, int l) {
    dqn_engine* e = b.e; const int B = b.B, ncon = b.ncon;
    const int jf = skip_join_of_first(e, l); const bool fuse_entry = jf >= 0 && skip_fused_dx(e, jf);      // a map block: the entry's sum and derivative run in THIS layer's dX epilogue (bwd_own_level)
    for (int j = l + 1; j < e->nl; j++) if (is_skip(e->L[j].kind) && j - e->L[j].cin == l && !fuse_entry && wants_dx(e, l)) {
        // this layer is the FIRST inner layer of the skip block that joins at j: its input-gradient launch, whatever its kind, runs with the IDENTITY epilogue
        // (src_act) and leaves the raw dF in dact[P].  Behind every launch of this level the block's entry launch (skip.hip) adds the join's dY and takes P's
        // derivative once, after the sum, in place:  dact[P] = (dF + dY) .* act_P'(y_P)
        const int pp = e->L[j].src2; const LayerDev Pl = e->L[pp]; float* dP = e->dact[pp]; const float* dYj = e->dact[j]; const float* Yp = e->act_on[pp];
        v.post_level.push_back({pname(e, "bwd_entry", e->L[j], j), [=](dqn_engine* en) { launch_skip_bwd_entry(en->stream, Pl.out_feat, dP, dYj, Yp, ncon, B, dP, Pl.act); }});
    }
}
// the backward of the own-level kinds: launches of the layer's own, never grouped
static void bwd_own_level(StepBuild& b, int l) {
    dqn_engine* e = b.e; const int B = b.B, ncon = b.ncon; const bool mf = b.mf;
    const LayerDev L = e->L[l]; const Operand in = operand_of(b, l); const float* X = in.X; const int ldx = in.ldx; float* dpre = e->dact[l]; const bool dx = wants_dx(e, l);
    // the layer above wrote its dX into dact[l] through its dX epilogue with this layer's `act`: dY for a pool, a Dropout layer and a join (IDENTITY), dpre = dY .* act'(y) for a LayerNorm and a padded conv
    const int act_src = L.src >= 0 ? src_act(e, l) : DQN_ACT_IDENTITY; float* out = L.src >= 0 ? e->dact[L.src] : nullptr; const float* Ysrc = L.src >= 0 ? e->act_on[L.src] : nullptr;
    if (is_skip(L.kind)) {
        // the join hands dY to the block's last inner layer K with K's activation derivative on K's stored output; where K has no activation that is the identity and
        // dact[K] IS dact[l] (engine.hip): no launch.  The other half of the join's backward, the + dY at the block's entry, runs behind the first inner layer's level (queue_skip_entry)
        const LayerDev Kl = e->L[L.src]; if (!skip_dact_alias(e, l)) e->prog.push_back({pname(e, "bwd_join", L, l), [=](dqn_engine* en) { launch_skip_bwd_join(en->stream, Kl.out_feat, dpre, Ysrc, ncon, B, out, Kl.act); }});
    } else if (is_pool(L.kind)) {
        // gathers dY per input element and applies the producing layer's activation derivative.  No parameters, so no dW; a pool on the observation has no input gradient to compute
        const float* Yp = e->act_on[l];
        if (dx && is_global_pool(L)) e->prog.push_back({pname(e, "bwd", L, l), [=](dqn_engine* en) { launch_gpool_bwd(en->stream, L, dpre, X, ncon, B, out, act_src); }});      // whole-map window of an adaptive / global pool (pool_global.hip)
        else if (dx) e->prog.push_back({pname(e, "bwd", L, l), [=](dqn_engine* en) { launch_pool_bwd(en->stream, L, dpre, X, Yp, ncon, B, out, act_src); }});
    } else if (is_actl(L.kind)) {
        // dY σ′ -- σ′ from the layer's own output for the eleven codes of the fused epilogues, from its input for gelu / swish / mish / hardswish -- then the producing layer's
        // activation derivative on that layer's output, which IS the input (act_layer.hip).  No parameters, so no dW; nothing where the input reaches the observation through
        // pool / Activation layers only: nobody reads it
        const float* Yl = e->act_on[l]; const int sigma = L.cell_act;
        if (dx) e->prog.push_back({pname(e, "bwd", L, l), [=](dqn_engine* en) { launch_actl_bwd(en->stream, L.out_feat, sigma, dpre, X, Yl, ncon, B, out, act_src); }});
    } else if (is_do(L.kind)) {
        // regenerates the forward's mask (the TD launch bumped the step counter in between: dropout.hip subtracts) and applies the producing layer's activation derivative on
        // that layer's own, unmasked output.  No parameters, so no dW; always a dX: the layer never reads the observation
        const double p = do_p(L); const unsigned long long seed = e->hp.seed; const StepState* stt = e->state;
        e->prog.push_back({pname(e, "bwd", L, l), [=](dqn_engine* en) { launch_do_bwd(en->stream, L.out_feat, p, seed, l, stt, dpre, Ysrc, ncon, B, out, act_src); }});
    } else if (is_gn(L.kind)) {
        // four launches (groupnorm.hip): the chunk sums of g and g * x_hat, dX with the producing layer's activation derivative (neither where the input reaches the observation
        // through pool layers only: nobody reads it), the row sums of dpre * x_hat and dpre, and their per-channel sums dgamma / dbeta straight into the flat gradient, which
        // the Adam launch reads like any bias range
        const float* P = e->p_on; const float* stat = b.ln_stat[l]; float *gg = e->grad + L.w_off, *gb = e->grad + L.b_off; const char* tag = kind_traits(L).tag;
        if (dx) {
            float* part = palloc(e, gn_part_floats(L, B));
            e->prog.push_back({lname(e, "bwd_%s%d_sums", tag, l), [=](dqn_engine* en) { launch_gn_bwd_sums(en->stream, L, P, dpre, X, ncon, stat, ncon, B, part); }});
            e->prog.push_back({pname(e, "bwd", L, l), [=](dqn_engine* en) { launch_gn_bwd_dx(en->stream, L, P, dpre, X, ncon, stat, ncon, B, part, out, act_src); }});
        }
        float* rowp = palloc(e, (size_t)2 * L.out_feat); e->prog.push_back({lname(e, "bwd_%s%d_rows", tag, l), [=](dqn_engine* en) { launch_gn_bwd_rows(en->stream, L, dpre, X, ncon, stat, ncon, B, rowp); }});
        e->prog.push_back({lname(e, "bwd_%s%d_par", tag, l), [=](dqn_engine* en) { launch_gn_bwd_par(en->stream, L, rowp, gg, gb); }});
    } else if (is_ln(L.kind)) {
        // two launches (layernorm.hip): dX with the producing layer's activation derivative -- a recurrent producer's `act` is IDENTITY, so its dact is the cell's dH -- and the
        // column sums dscale / dbias straight into the flat gradient, which the Adam launch reads like any bias range.  Always a dX: the layer has parameters and never reads the observation
        const float* P = e->p_on; const float* stat = b.ln_stat[l]; float *gs = e->grad + L.w_off, *gb = e->grad + L.b_off;
        e->prog.push_back({pname(e, "bwd", L, l), [=](dqn_engine* en) { launch_ln_bwd(en->stream, L, P, dpre, X, ncon, stat, ncon, B, out, act_src, gs, gb); }});
    } else {
        // a padded or a dilated / grouped conv (conv_own.hip): dW / db into the gradient block or its plan slabs (summed with the other layers' slabs before / inside Adam),
        // then -- unless the layer reads the observation -- dX with the producing layer's activation derivative.  A dilated / grouped conv is never inside a skip block: no fused entry
        float* dst = dw_dst(b, L, dqn_nchunks(L.npos * B, L.dw_kc)); const int xu8 = L.xu8; const float* P = e->p_on;
        const int jf = skip_join_of_first(e, l); const bool fuse_entry = jf >= 0 && skip_fused_dx(e, jf);
        e->prog.push_back({pname(e, "dw", L, l), [=](dqn_engine* en) { launch_conv_own_dw(en->stream, L, X, ldx, dpre, B, dst, mf ? 1 : 0, xu8); }});
        // the FIRST inner layer of a convolutional skip block (fuse_entry): the launch adds the join's dY = dact[join] to its own sum and takes the entry's REAL activation
        // derivative after it -- dact[P] = (dF + dY) .* act_P'(y_P), what the bwd_entry launch (skip.hip) computes behind a raw dF; named "bwd_conv<F>+skip<join>".  With
        // one inner layer dpre IS dY (skip_dact_alias): read twice, written by nobody here
        if (dx && fuse_entry) {
            const float* dYj = e->dact[jf]; const int act_p = e->L[L.src].act;
            e->prog.push_back({lname(e, "bwd_%s%d+skip%d", kind_traits(L).tag, l, jf), [=](dqn_engine* en) { launch_conv_own_dx(en->stream, L, P, dpre, B, out, Ysrc, ncon, act_p, mf ? 1 : 0, dYj); }});
        }
        else if (dx) e->prog.push_back({pname(e, "bwd", L, l), [=](dqn_engine* en) { launch_conv_own_dx(en->stream, L, P, dpre, B, out, Ysrc, ncon, act_src, mf ? 1 : 0); }});
    }
}
// a recurrent layer: BPTT over the s-sequence: T single-workgroup steps produce dG (gate pre-activation gradients) for all columns,
// then Wi|b, Wh and the input gradient are ordinary dense contractions over the T*B columns.
// Cells whose Wh dW pass reads a gate gradient of its own (CellOps::two_dG; the GRU: gru.hip) get it in the second half of dG
static void bwd_recurrent(StepBuild& b, LevelBwd& v, int l) {
    dqn_engine* e = b.e; const int B = b.B, Bb = b.Bb, T = b.T, ncon = b.ncon;
    const LayerDev L = e->L[l]; const Operand in = operand_of(b, l); float* grad = e->grad; const char* tag = kind_traits(L).tag;
    const CellOps* C = cell_ops(L.kind);
    float* const dGh = C->two_dG ? e->dG[l] + (size_t)L.N * B : e->dG[l];
    CellBwdArgs a; memset(&a, 0, sizeof a); a.T = T; a.H = L.H; a.B = Bb; a.TB = B; a.act = L.cell_act;
    a.gates = e->gates[l]; a.aux = e->tcb[l]; a.hprev = e->hprev_buf[l]; a.cprev = e->cprev_buf[l]; a.hout = e->act_on[l]; a.ld_h = ncon; a.Wh = e->p_on + L.wh_off;
    a.dH = e->dact[l]; a.dG = e->dG[l]; a.dGh = dGh; a.dhn = e->dhn[l]; a.dh2 = e->dcn[l]; a.g_h0 = grad + L.h0_off; if (C->has_c) a.g_c0 = grad + L.c0_off;
    if (C->seq_fits(L.H, Bb, T) && !stepwise(e->opt, L.kind)) e->prog.push_back({lname(e, "%s_bwd_seq_%s%d", C->name, tag, l), [=](dqn_engine* en) { C->launch_bwd_seq(en->stream, a); }});
    else for (int t = T - 1; t >= 0; t--) { CellBwdArgs at = a; at.t = t; e->prog.push_back({lname(e, "%s_bwd_%s%d", C->name, tag, l), [=](dqn_engine* en) { C->launch_bwd_step(en->stream, at); }}); }
    LayerDev Vi = gx_view(L); Vi.b_off = L.b_off;                                                                 // Wi | b  : (K+1) x N (the bias row is real here)
    LayerDev Vh = Vi; Vh.K = L.H; Vh.in_feat = L.H; Vh.w_off = L.wh_off; Vh.b_off = L.wh_off + (size_t)L.H * L.N;  // Wh | junk
    const float* dGi = e->dG[l];      // the Wi | b and dX operand (the Wh operand: dGh)
    // small recurrent layers (config 4: (25+1) x 128 and (32+1) x 128 weights, 256 columns): the two dW contractions as VALU tasks of ONE launch
    // (15 us) beat two LDS-tiled MFMA launches of 13 us each (r03: 113.4 -> 102.7 us/step); the MFMA tiles win once the sample chains get long
    auto small_dw = [B](const LayerDev& V) { return B <= 256 && (size_t)(V.K + 1) * V.N <= 16384; };
    float* wh_dst = emit_dw_single(b, v, Vh, e->hprev_buf[l], B, dGh, pname(e, "dw_wh", L, l), small_dw(Vh));      // first: its junk bias row is then overwritten by nothing that matters
    emit_dw_single(b, v, Vi, in.X, in.ldx, dGi, pname(e, "dw_wi", L, l), small_dw(Vi));
    if (C->clear_junk) {      // the GRU's junk row (sum of dn .* r) is cleared once the level's launches have written it: Adam folds max |g| over it (gru.hip)
        float* jr = wh_dst + (size_t)L.H * L.N; const int nr = dqn_nchunks(B, Vh.dw_kc); const size_t stride = (size_t)(L.H + 1) * L.N; const int n = L.N;
        v.post_level.push_back({pname(e, "gru_junk_clear", L, l), [=](dqn_engine* en) { launch_clear_rows(en->stream, jr, nr, stride, n); }});
    }
    if (wants_dx(e, l)) emit_dx_single(b, v, l, Vi, dGi, dqn_nchunks(Vi.N, Vi.dx_kc), /*hold*/ false, /*mfma_n16*/ false, /*addend*/ nullptr, e->dact[L.src], e->act_on[L.src]);
}
// a GEMM kind, layer lv[k] of its level: dW / db, then dX with act' of the producing layer; the two streams of a dueling net meet at the base output (dX_val + dX_adv)
static void bwd_gemm(StepBuild& b, LevelBwd& v, const std::vector<int>& lv, int k) {
    dqn_engine* e = b.e; const int B = b.B, ncon = b.ncon; const bool mf = b.mf; DwL& dwl = v.dwl; DxL& dxl = v.dxl;
    const int l = lv[k]; const LayerDev L = e->L[l]; const Operand in = operand_of(b, l); const float* X = in.X; const int ldx = in.ldx; float* dpre = e->dact[l];
    if (!b.dp_layer[l] && !(v.dw_done_sibling && k == 0)) {   // dW / db  (layers flagged for the gather exchange get theirs after the collective; a second sibling got its in the pair's launch)
        const int S = dqn_nchunks(L.npos * B, L.dw_kc); float* grad = e->grad;
        const bool lds = mf && gemm_dw_eligible(L, B, ldx);
        // sibling layers of this level with identical geometry and the same input share ONE launch (the sibling's slabs enter final_segs first)
        const bool pair = lds && k == (int)lv.size() - 1 && lv.size() == 2 && same_geo(e->L[lv[0]], e->L[lv[1]]) && e->L[lv[0]].dw_kc == e->L[lv[1]].dw_kc;
        float* dst0 = pair ? dw_dst(b, e->L[lv[0]], S) : nullptr; float* dst = dw_dst(b, L, S);
        if (pair || lds) {      // held in dwl: one problem, or the pair's two on the same X
            flush_dw(b, v); dwl.on = true; dwl.L = L; dwl.nprob = pair ? 2 : 1; dwl.ldx = ldx; dwl.name = pname(e, pair ? "dw2" : "dw", L, l);
            dwl.X[0] = dwl.X[1] = X; dwl.d[0] = dpre; dwl.o[0] = dst; dwl.d[1] = pair ? e->dact[lv[0]] : dpre; dwl.o[1] = pair ? dst0 : dst;
            if (pair) v.dw_done_sibling = true;
        }
        else if (mf && mfma_dw_ok(L, B)) { float* part = S > 1 ? dst : nullptr; e->prog.push_back({pname(e, "dw", L, l), [=](dqn_engine* en) { launch_mfma_dw(en->stream, L, X, ldx, dpre, B, grad, part, false); }}); }
        else v.pend.push_back(valu_dw_task(L, X, ldx, dpre, B, L.npos * B, dst));
    }
    if (!wants_dx(e, l)) return;
    const int src = L.src; const bool is_join = e->hp.dueling && src == e->last_base && L.stream != DQN_STREAM_BASE;
    const bool dense = L.kind == DQN_LAYER_DENSE; const int S_plan = dense ? dqn_nchunks(L.N, L.dx_kc) : 1;
    const bool join_lds = is_join && lv.size() == 2 && mf && same_geo(e->L[lv[0]], e->L[lv[1]]) && e->L[lv[0]].dx_kc == e->L[lv[1]].dx_kc &&
                          gemm_dx_eligible(L, B, ncon, 2) && (S_plan == 1 || gemm_dx_internal_chunks(L, B, ncon, 2));
    if (join_lds && k == (int)lv.size() - 1) {      // both streams in ONE launch: the kernel accumulates dX_val and dX_adv separately and adds them (val first)
        const LayerDev Lv = e->L[lv[0]], La = e->L[lv[1]]; const float* P = e->p_on;
        flush_dx(b, v); dxl.on = true; dxl.L = Lv; dxl.nsrc = 2; dxl.W[0] = P + Lv.w_off; dxl.d[0] = e->dact[lv[0]]; dxl.W[1] = P + La.w_off; dxl.d[1] = e->dact[lv[1]];
        dxl.out = e->dact[src]; dxl.ys = e->act_on[src]; dxl.act_src = src_act(e, l); dxl.name = pname(e, "dx_join", L, l);
    }
    if (join_lds) return;
    float* out = e->dact[src]; const float *addend = nullptr, *ysrc = e->act_on[src];
    if (is_join && !b.joined) { out = e->join_tmp; ysrc = nullptr; b.joined = true; }
    else if (is_join) { addend = e->join_tmp; flush_dx(b, v); flush_valu(e, v.pend, pname(e, "bwd_valu", L, l)); }   // depends on the first stream's dX: an LDS-tiled one still waits in dxl
    emit_dx_single(b, v, l, L, dpre, S_plan, /*hold*/ true, /*mfma_n16*/ true, addend, out, ysrc);
}
// the end of level li: places the waiting tail tasks, lets the priority block ride, issues the level's LDS-tiled launch (dW and dX as one where both wait) and what was queued behind it
static void finish_level(StepBuild& b, LevelBwd& v, int li) {
    dqn_engine* e = b.e; const int B = b.B, ncon = b.ncon; const auto& lv = b.levels[li]; DwL& dwl = v.dwl; DxL& dxl = v.dxl;
    GemmTail tail = gemm_no_tail();
    if (!b.tail_pend.empty()) {
        if (dwl.on || dxl.on) { tail.blocks = number_tasks(b.tail_pend); tail.tasks = upload(e, b.tail_pend); tail.n = (int)b.tail_pend.size(); }      // rides in the last workgroups of this level's LDS-tiled launch
        else for (auto& t : b.tail_pend) v.pend.push_back(t);      // or joins this level's VALU task table
        b.tail_pend.clear();
    }
    if (b.pg_want && b.prio_in_adam && (dwl.on || dxl.on) && b.prio_draw_pending) {      // second half of a split priority block: the next sample()'s draws
        tail.adam = plain_adam_job(e, true); tail.adam.prio = prio_args(b); tail.adam.prio.phase = 2; tail.has_adam = 1; b.prio_draw_pending = false; b.prio_placed = true;
    }
    else if (b.pg_want && b.prio_in_adam && (dwl.on || dxl.on) && !b.prio_placed && !b.prio_draw_pending) {
        // the block rides as workgroup 0 of this launch.  When a LATER backward launch can carry a workgroup too, the block is SPLIT: update_priorities!
        // here, the draws there -- each half shorter than the dX chains it hides under (r03 ktrace: the whole block lived 11 us, longer than any)
        bool later = false; for (int lj = li - 1; lj >= 0 && !later; lj--) for (int l2 : b.levels[lj]) if (b.mf && !b.dp_layer[l2] && dw_carrier_ok(e, l2, B, operand_of(b, l2).ldx)) later = true;
        tail.adam = plain_adam_job(e, true); tail.adam.prio = prio_args(b); tail.has_adam = 1;
        if (later) { tail.adam.prio.phase = 1; b.prio_draw_pending = true; } else b.prio_placed = true;
    }
    if (b.pg_want && b.prio_in_adam && !b.prio_placed && !v.pend.empty() && !tail.has_adam && !e->prio_in_bwd /* large batches: only the long LDS-tiled launches can hide the block */) {
        PrioArgs pa = prio_args(b); if (b.prio_draw_pending) { pa.phase = 2; b.prio_draw_pending = false; }
        flush_valu(e, v.pend, pname(e, "bwd_valu", e->L[lv[0]], lv[0]), &pa); b.prio_placed = true;
    }
    flush_valu(e, v.pend, pname(e, "bwd_valu", e->L[lv[0]], lv[0]));
    const char* tsuf = !tail.has_adam ? "" : (adam_job_blocks(tail.adam) == 1 && tail.adam.prio.n > 0) ? "+prio" : "+adam_tail";      // a job that is only the priority block
    if (dwl.on && dxl.on) {      // dW and dX of this level in ONE launch
        const DwL a = dwl; const DxL x = dxl; dwl.on = dxl.on = false;
        e->prog.push_back({lname(e, "%s+%s%s", a.name, x.name, tsuf), [=](dqn_engine* en) { launch_gemm_dwdx(en->stream, a.L, a.nprob, a.X, a.ldx, a.d, B, a.o, x.L, x.nsrc, x.W, x.d, x.out, x.ys, ncon, x.act_src, tail); }});
    }
    else if (dwl.on) { const DwL a = dwl; dwl.on = false; e->prog.push_back({tail.has_adam ? lname(e, "%s%s", a.name, tsuf) : a.name, [=](dqn_engine* en) { launch_gemm_dw(en->stream, a.L, a.nprob, a.X, a.ldx, a.d, B, a.o, 0, 0, 0, tail); }}); }
    else if (dxl.on) { const DxL a = dxl; dxl.on = false; e->prog.push_back({tail.has_adam ? lname(e, "%s%s", a.name, tsuf) : a.name, [=](dqn_engine* en) { launch_gemm_dx(en->stream, a.L, a.nsrc, a.W, a.d, B, a.out, a.ys, ncon, a.act_src, tail); }}); }
    for (auto& st : v.post_level) e->prog.push_back(st);
}
static void emit_backward(StepBuild& b) {
    dqn_engine* e = b.e; const Levels& levels = b.levels;
    for (int li = (int)levels.size() - 1; li >= 0; li--) {
        const auto& lv = levels[li]; LevelBwd v;
        if (b.fuse_heads && li + 1 == (int)levels.size()) { queue_head_tails(b, lv); continue; }
        for (int k = (int)lv.size() - 1; k >= 0; k--) {
            const int l = lv[k]; queue_skip_entry(b, v, l);
            if (kind_traits(e->L[l]).own_level) bwd_own_level(b, l); else if (is_recurrent(e->L[l].kind)) bwd_recurrent(b, v, l); else bwd_gemm(b, v, lv, k);
        }
        finish_level(b, v, li);
    }
    if (!b.tail_pend.empty()) { std::vector<VTask> own(b.tail_pend); b.tail_pend.clear(); flush_valu(e, own, "head_dw"); }      // single-level network: nothing to ride on
    if (e->prio_forked) e->prog.push_back({"prio_join", [](dqn_engine* en) { hipStreamWaitEvent(en->stream, en->ev_join, 0); }});
}
// ---------------- stage 10: the deferred dW slabs: ONE reduce launch -- which the Adam launch takes over (adam_segs) where the ranges allow it
static void emit_final_reduce(StepBuild& b) {
    dqn_engine* e = b.e; const std::vector<RSeg>& final_segs = b.final_segs;
    bool ok = !final_segs.empty() && final_segs.size() <= 8; unsigned long long tot = 0;
    for (auto& r : final_segs) { const unsigned long long beg = (unsigned long long)(r.out - e->grad); ok = ok && beg % 4 == 0 && r.elems % 4 == 0 && r.S2 == 0; }
    if (ok) {
        for (auto& r : final_segs) { const int q = e->adam_segs.n++; e->adam_segs.beg[q] = (unsigned long long)(r.out - e->grad); e->adam_segs.end[q] = e->adam_segs.beg[q] + r.elems; e->adam_segs.part[q] = r.part; e->adam_segs.S[q] = r.S; tot += r.elems; }
        e->adam_segs.blocks = (unsigned)((tot + 255) / 256);
    }
    if (!final_segs.empty()) e->final_reduce_step = (long)e->prog.size();
    std::vector<RSeg> segs(final_segs);      // emit_reduce consumes its list; the replica pack layout still reads final_segs
    emit_reduce(e, segs, "dw_reduce_all");
}
// ---------------- stage 11: replicas: the pack layout of the one exchange, then the flagged layers' dW from the gathered operands
struct DpDw { LayerDev L; const float* X; unsigned long long x_off, d_off; };
// per-rank block: [X of each distinct producer: K x B][dpre of each flagged layer: N x B][every other gradient range]
static int emit_dp_pack(StepBuild& b, DpSumArgs& dsum, std::vector<DpDw>& dpdw) {
    dqn_engine* e = b.e; const int B = b.B, W = b.W;
    DpPackArgs pk; memset(&pk, 0, sizeof pk); unsigned long long off = 0;
    std::vector<std::pair<const float*, unsigned long long>> xs;
    for (int l = 0; l < e->nl; l++) if (b.dp_layer[l]) {
        const LayerDev& L = e->L[l]; const Operand in = operand_of(b, l); const float* X = in.X;
        unsigned long long xo = ~0ull; for (auto& q : xs) if (q.first == X) xo = q.second;
        if (xo == ~0ull) { xo = off; xs.push_back({X, xo}); DpRegion r; memset(&r, 0, sizeof r); r.S = 1; r.src = X; r.dst = off; r.n = (unsigned long long)L.K * B; r.B = B; r.ld = in.ldx; pk.r[pk.n++] = r; off += r.n; }
        DpRegion d; memset(&d, 0, sizeof d); d.S = 1; d.src = e->dact[l]; d.dst = off; d.n = (unsigned long long)L.N * B; d.B = 1; d.ld = 1; pk.r[pk.n++] = d;
        dpdw.push_back({L, X, xo, off}); off += d.n;
    }
    // the complement of the flagged layers' (K+1) x N blocks inside the internal gradient vector
    std::vector<std::pair<unsigned long long, unsigned long long>> holes;
    for (int l = 0; l < e->nl; l++) if (b.dp_layer[l]) holes.push_back({e->L[l].w_off, e->L[l].w_off + (unsigned long long)(e->L[l].K + 1) * e->L[l].N});
    std::sort(holes.begin(), holes.end()); unsigned long long cur = 0;
    // sub-ranges whose gradient still sits in split-K slabs (conv dW) are reduced by the pack kernel itself
    std::vector<RSeg> slabs(b.final_segs); std::sort(slabs.begin(), slabs.end(), [](const RSeg& x, const RSeg& y) { return x.out < y.out; });
    bool pack_folds = !slabs.empty(); for (auto& r : slabs) pack_folds = pack_folds && r.S2 == 0 && r.mode == 2;
    auto small = [&](unsigned long long a, unsigned long long z) {
        if (z <= a) return;
        DpRange q; q.src = off; q.dst = a; q.n = z - a; dsum.r[dsum.n++] = q; unsigned long long cur2 = a;
        auto plain = [&](unsigned long long x, unsigned long long y) { if (y <= x) return; DpRegion r; memset(&r, 0, sizeof r); r.src = e->grad + x; r.dst = off + (x - a); r.n = y - x; r.B = 1; r.ld = 1; r.S = 1; pk.r[pk.n++] = r; };
        if (pack_folds) for (auto& sg : slabs) {
            const unsigned long long sb = (unsigned long long)(sg.out - e->grad), se = sb + sg.elems;
            if (sb < a || se > z) continue; plain(cur2, sb);
            DpRegion r; memset(&r, 0, sizeof r); r.src = sg.part; r.dst = off + (sb - a); r.n = sg.elems; r.B = 1; r.ld = 1; r.S = sg.S; r.per_s = sg.elems; pk.r[pk.n++] = r; cur2 = se;
        }
        plain(cur2, z); off += z - a;
    };
    for (auto& h : holes) { small(cur, h.first); cur = h.second; }
    small(cur, e->Pint); off = (off + 3) / 4 * 4;
    DevScope& M = e->dp_mem; if (e->dp_count != off) { M.drop(e->dp_send); M.drop(e->dp_recv); e->dp_send = e->dp_recv = nullptr; e->dp_count = 0; DM(M, e->dp_send, off); DM(M, e->dp_recv, off * W); e->dp_count = off; }
    pk.send = e->dp_send; dsum.recv = e->dp_recv; dsum.stride = off; dsum.world = W; dsum.grad = e->grad;
    unsigned long long off_a = 0;      // end of the wide layers' operands inside the block
    for (auto& q : dpdw) off_a = std::max(off_a, q.d_off + (unsigned long long)q.L.N * B);
    if (b.overlap_cand && off_a % 4 == 0 && off_a < off) {
        e->dp_overlap = true; e->dp_count_a = off_a; M.drop(e->dp_recv_b); e->dp_recv_b = nullptr; DM(M, e->dp_recv_b, (off - off_a) * W);
        DpPackArgs pa; memset(&pa, 0, sizeof pa); DpPackArgs pb; memset(&pb, 0, sizeof pb); pa.send = pb.send = e->dp_send;
        for (int i = 0; i < pk.n; i++) { if (pk.r[i].dst < off_a) pa.r[pa.n++] = pk.r[i]; else pb.r[pb.n++] = pk.r[i]; }
        e->dp_pk_a = pa; pk = pb; dsum.recv = e->dp_recv_b; dsum.stride = off - off_a; for (int i = 0; i < dsum.n; i++) dsum.r[i].src -= off_a;
    }
    e->prog.push_back({"dp_pack", [=](dqn_engine* en) { launch_dp_pack(en->stream, pk); }});
    e->dp_gather = true; e->dp_pack_folds = pack_folds;
    // the ascending sum over ranks of the small gradient ranges rides inside k_adam (its slab-reduce blocks) when the ranges allow it
    memset(&e->dp_adam_segs, 0, sizeof e->dp_adam_segs);
    bool af = dsum.n > 0 && dsum.n <= 8; unsigned long long tot = 0;
    for (int i = 0; i < dsum.n; i++) af = af && dsum.r[i].dst % 4 == 0 && dsum.r[i].n % 4 == 0;
    if (af) for (int i = 0; i < dsum.n; i++) { AdamSegs& A = e->dp_adam_segs; const int q = A.n++; A.beg[q] = dsum.r[i].dst; A.end[q] = dsum.r[i].dst + dsum.r[i].n; A.part[q] = dsum.recv + dsum.r[i].src; A.S[q] = W; A.stride[q] = dsum.stride; tot += dsum.r[i].n; }
    e->dp_adam_segs.blocks = (unsigned)((tot + 255) / 256); e->dp_adam_folds = af; return 0;
}
// big dense dW over the W*B gathered samples (rank-major = the concatenated batch); siblings with the same X and geometry share a launch
static void emit_dp_dw(StepBuild& b, const DpSumArgs dsum, const std::vector<DpDw>& dpdw) {
    dqn_engine* e = b.e; const int B = b.B, W = b.W;
    const float* recv = e->dp_recv; const int cnt = (int)(e->dp_overlap ? e->dp_count_a : e->dp_count); float* grad = e->grad;      // rank stride of the buffer that holds X | dpre
    std::vector<bool> used(dpdw.size(), false);
    for (size_t i = 0; i < dpdw.size(); i++) {
        if (used[i]) continue; used[i] = true;
        size_t j = i + 1; for (; j < dpdw.size(); j++) if (!used[j] && dpdw[j].x_off == dpdw[i].x_off && same_geo(dpdw[i].L, dpdw[j].L)) break;
        const bool pair = j < dpdw.size(); if (pair) used[j] = true;
        const DpDw a = dpdw[i], c = pair ? dpdw[j] : dpdw[i]; const int np = pair ? 2 : 1;
        e->prog.push_back({pname(e, "dp_dw", a.L, (int)i), [=](dqn_engine* en) {
            const float* X[2] = {recv + a.x_off, recv + c.x_off}; const float* d[2] = {recv + a.d_off, recv + c.d_off}; float* o[2] = {grad + a.L.w_off, grad + c.L.w_off};
            launch_gemm_dw(en->stream, a.L, np, X, B, d, W * B, o, /*ldd*/ B, /*tiles per rank*/ B / 32, /*rank stride*/ cnt); }});
    }
    if (!e->dp_adam_folds) e->prog.push_back({"dp_sum_ranks", [=](dqn_engine* en) { launch_dp_unpack_sum(en->stream, dsum); }});
}
static int emit_replica_exchange(StepBuild& b) {
    dqn_engine* e = b.e; DpSumArgs dsum; memset(&dsum, 0, sizeof dsum); std::vector<DpDw> dpdw;
    if (b.n_dp > 0 && emit_dp_pack(b, dsum, dpdw)) return -1;
    e->prog_post_begin = e->prog.size();      // what follows runs after the exchange
    if (e->dp_gather) emit_dp_dw(b, dsum, dpdw);
    return 0;
}
// ---------------- stage 12: the Adam launch over the whole parameter vector -- with the priority block where no backward launch took it -- and the pre-gather record
static void emit_adam(StepBuild& b) {
    dqn_engine* e = b.e; const int B = b.B; AdamJob J = plain_adam_job(e, true);
    J.nr = 1; J.beg[0] = 0; J.end[0] = e->Pint; J.sblocks = (unsigned)adam_blocks(e->Pint); J.tick = 1; J.slot0 = 0;
    if (e->hp.prioritized_replay && !b.rec && !e->prio_forked && !b.prio_placed) { J.prio = prio_args(b); if (b.prio_draw_pending) { J.prio.phase = 2; b.prio_draw_pending = false; } }
    memset(&e->pg, 0, sizeof e->pg); e->pg_ok = b.pg_want && (b.prio_placed || e->prio_forked);
    if (e->pg_ok) {
        PreGather& G = e->pg; G.on = 1; G.s_rows = e->s_rows; G.sp_rows = e->sp_rows; G.E = e->E; G.B = B; G.idx_pre = e->idx_pre; G.x0 = e->x0; G.cap2 = e->cap2; G.tree = e->tree; G.seed = e->hp.seed; G.meta.distinct = e->hp.sample_distinct ? 1 : 0;
        G.meta.a = e->ra; G.meta.r = e->rr; G.meta.done = e->rdone; G.meta.beta = e->hp.prio_beta; G.meta.a_out = e->gb_a2; G.meta.r_out = e->gb_r2; G.meta.done_out = e->gb_done2; G.meta.w_out = e->gb_w2;
        G.u8b = e->arena_u8 ? 1 : 0; if (G.u8b) { G.gx = (e->E + 255) / 256; G.gy = (2 * B + 127) / 128; } else { G.gx = (e->E + 63) / 64; G.gy = (2 * B + 63) / 64; }
    }
    e->adam_step = (long)e->prog.size(); J.gscale = e->world > 1 ? 1.0f / (float)e->world : 1.0f;
    const bool fold = e->adam_segs.n > 0 && !e->comm && !e->sim_world;     // with a communicator the gradient must be materialised before the all-reduce
    if (e->dp_gather && e->dp_adam_folds) J.segs = e->dp_adam_segs; else if (fold) J.segs = e->adam_segs;
    e->prog.push_back({"adam", [=](dqn_engine* en) { launch_adam(en->stream, J, en->cur.pregather ? &en->pg : nullptr); }});
    e->gmax_used = (int)(J.segs.blocks + J.sblocks);
}
// The train step's program, in program order.  The first two stages build a whole step and return; the rest is the general program
static int build_stages(dqn_engine* e) {
    e->prog_names.reserve(512); StepBuild b(e);
    int whole = column_group_program(b);             //  1  recurrent, column-group dW chunks: drqn_cols + adam
    if (whole < 0) return whole;
    if (!whole) whole = single_workgroup_program(b); //  2  the network fits in LDS: tiny_step
    if (whole) return 0;
    choose_byte_arena(b);                            //  3  u8 replay: the observation arena in bytes
    choose_head_fusion(b);                           //  4  head level + TD + head dX as one launch, with or without the split-K reduce
    emit_forward_levels(b);                          //  5  forward levels, the recurrence behind a recurrent level
    if (emit_td(b)) return -1;                       //  6  the TD / head launch, one of four
    place_priority_block(b);                         //  7  Adam launch, a backward launch's workgroup, or the side stream
    choose_dp_layers(b);                             //  8  replicas: which layers' dW waits for the exchange
    emit_backward(b);                                //  9  backward levels
    emit_final_reduce(b);                            // 10  the dW slab reduce and adam_segs
    if (emit_replica_exchange(b)) return -1;         // 11  the replica pack layout, the post-exchange dW
    emit_adam(b);                                    // 12  the Adam launch and the pre-gather record
    return 0;
}
// the engine-side record of the program at rest: every exit of build_stages overwrites what its program sets differently, before anything reads it
static void program_at_rest(dqn_engine* e) {
    e->pg_ok = false; e->adam_step = -1; e->gmax_used = 0; e->tiny = false; e->drqn_fused = false; e->arena_u8 = false; e->prio_forked = false; e->prio_in_bwd = false;
    e->dp_gather = false; e->dp_overlap = false; e->prog_post_begin = e->prog_pre1_end = 0; e->final_reduce_step = -1; memset(&e->adam_segs, 0, sizeof e->adam_segs); for (int i = 0; i < e->nl; i++) e->L[i].xu8 = 0; e->drqn_stamps = nullptr;
}
// EVERY refusal -- a stage's own, or a refused allocation of the program's scope (the closures capture those pointers by value) -- leaves an empty program: no steps, no blocks, the record at rest.  The next call starts over
int build_program(dqn_engine* e) {
    if (e->prog_built) return 0;
    HIPCHK(hipSetDevice(e->device));
    program_at_rest(e);
    HIPCHK(hipMemsetAsync(e->gmax_part, 0, (size_t)gmax_slots(e->Pint) * 4, e->stream));      // per-block maxima of an earlier program shape must not survive
    int rc = build_stages(e); if (!rc && e->prog_mem.failed) { const std::string why = dqn_last_error(); rc = fail("build_program: a device allocation failed (%s)", why.c_str()); }
    if (rc) { hipStreamSynchronize(e->stream); e->prog.clear(); e->prog_mem.release(); program_at_rest(e); return -1; }
    e->prog_built = true; return 0;
}
