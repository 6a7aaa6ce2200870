"""The harness of the feed-forward parity tests (TEST INFRASTRUCTURE): one description of a case, its data, the per-step checker against the fp64 reference of
tests/feedforward_reference.py and the bit-for-bit companions, for every case table -- the edge table below (tests/test_feedforward_edges_cpu.py on the C twin,
tests/test_feedforward_edges_gpu.py on the HIP engine), tests/pool_reference.py and tests/conv_pad_reference.py.

The edge table: feed-forward train steps at the edges of the kernel-selection rules and on rectangular convolutions.  The selection rules of nn_gemm.hip /
nn_mfma.hip / engine_program.hip / engine.hip / red_head.hip are RESTATED here (facts()), evaluated on the plan the case runs under -- the default plan for the
tables of this file, an edited one for tests/plan_edges_common.py (case_plan) -- and every case states in `want` the side of each rule it was written for: a
case on the wrong side fails instead of silently testing something else.  launches() turns the same facts into the launch names profile_step must (and must
not) show.

Tolerances are those of tests/test_twin_vs_oracle.py::run_case (Q, td, loss, grad_norm, priorities), recurrent_reference.GRAD_C / GRAD_RTOL
(gradients per block) and recurrent_reference.check_params (parameters); none is widened here."""
import types

import numpy as np

import dqn_oracle as O
import feedforward_reference as FR
import ref
from test_twin_vs_oracle import check_priorities_after_step

I, RELU, TANH, SIG = O.ACT_IDENTITY, O.ACT_RELU, O.ACT_TANH, O.ACT_SIGMOID
TOL_Q = dict(atol=1e-5, rtol=1e-5)          # test_twin_vs_oracle.run_case
TOL_TD = dict(atol=2e-5, rtol=1e-5)
TOL_LOSS = dict(rtol=1e-5, atol=1e-7)
TOL_GN = dict(rtol=1e-4)
GAP = 1e-4                                   # fp64 top-two gap of every argmax column: best_a is then compared exactly
RELU_MARGIN = FR.RELU_MARGIN                 # relu pre-activations and MaxPool top-two gaps of the fp64 reference stay this far off their kinks (feedforward_reference.margins)
LR = 1e-3
WORST = {}                                   # largest error / tolerance seen per quantity (1.0 = at the bound); printed by the test files


# ------------------------------------------------------------------ geometry (engine_layers.hip build_layers, restated)
def _c4(x):
    return (x + 3) // 4 * 4


def nchunks(K, kc):
    return 1 if (kc <= 0 or kc >= K) else (K + kc - 1) // kc


def chunk_len(K, kc):
    return K if (kc <= 0 or kc >= K) else kc


def geometry(net, plan):
    """[layer record] in ABI order (base, val, adv), with the plan's chunk lengths, and Pint (floats of the internal parameter vector)"""
    out, off = [], 0
    last = {"base": -1, "val": -1, "adv": -1}
    streams = [("base", l) for l in net.base] + ([("val", l) for l in net.val] + [("adv", l) for l in net.adv] if net.dueling else [])
    for i, (st, l) in enumerate(streams):
        src = last["base"] if st == "base" else (last[st] if last[st] >= 0 else last["base"])
        if src < 0:
            shp = net.obs_shape if len(net.obs_shape) == 3 else (int(np.prod(net.obs_shape)), 1, 1)
        else:
            p = out[src]
            shp = (p.cout, p.oh, p.ow) if p.kind == "conv" else (p.N, 1, 1)
        g = types.SimpleNamespace(i=i, kind=l.kind, act=l.act, stream=st, src=src, in_feat=int(np.prod(shp)))
        if l.kind == "conv":
            g.cin, g.cout, g.kh, g.kw, g.sh, g.sw, g.ih, g.iw = l.cin, l.cout, l.kh, l.kw, l.sh, l.sw, shp[1], shp[2]
            g.oh, g.ow = (shp[1] - l.kh) // l.sh + 1, (shp[2] - l.kw) // l.sw + 1
            g.K, g.N, g.npos = l.cin * l.kh * l.kw, l.cout, g.oh * g.ow
        else:
            g.cin = g.cout = g.kh = g.kw = g.sh = g.sw = 0
            g.ih = g.iw = g.oh = g.ow = 1
            g.K, g.N, g.npos = l.n_in, l.n_out, 1
        g.out_feat = g.N * g.npos
        off = _c4(off); g.w_off = off; off += g.K * g.N + g.N
        g.fwd_kc, g.dx_kc, g.dw_kc = plan[i]
        g.name = f"{g.kind}{i}"
        last[st] = i
        out.append(g)
    return out, _c4(off)


def levels_of(G):
    lv = [[g.i] for g in G if g.stream == "base"]
    val, adv = [g.i for g in G if g.stream == "val"], [g.i for g in G if g.stream == "adv"]
    for j in range(max(len(val), len(adv))):
        lv.append(([val[j]] if j < len(val) else []) + ([adv[j]] if j < len(adv) else []))
    return lv


def same_geo(a, b):
    k = ("kind", "act", "K", "N", "npos", "cin", "kh", "kw", "sh", "sw", "ih", "iw", "fwd_kc", "src")
    return all(getattr(a, x) == getattr(b, x) for x in k)


# ------------------------------------------------------------------ the selection rules, restated
def gemm_fwd_eligible(L, probs):
    """nn_gemm.hip: the LDS-tiled forward.  probs: [(ldx, col0, ncols)]"""
    S, kc = nchunks(L.K, L.fwd_kc), chunk_len(L.K, L.fwd_kc)
    if L.N % 16 or L.K % 32 or (S > 1 and kc % 32) or L.K > 8192 or L.w_off % 4:
        return False
    return not any(nc % 16 or ldx % 4 or c0 % 4 for ldx, c0, nc in probs)


def mfma_fwd_ok(L, ncols):
    S, kc = nchunks(L.K, L.fwd_kc), chunk_len(L.K, L.fwd_kc)
    return not (L.N % 16 or ncols % 16 or L.K % 4 or (S > 1 and kc % 4) or L.K > 16384)


def gemm_dw_eligible(L, B, ldx):
    KK = L.npos * B; S, kc = nchunks(KK, L.dw_kc), chunk_len(KK, L.dw_kc)
    return not (L.N % 16 or B % 32 or ldx % 4 or L.K < 16 or (S > 1 and kc % 32))


def mfma_dw_ok(L, B):
    KK = L.npos * B; S, kc = nchunks(KK, L.dw_kc), chunk_len(KK, L.dw_kc)
    return not (L.N % 16 or B % 4 or (S > 1 and kc % B))


def conv_max_chunks(L):
    tc = L.dx_kc if 0 < L.dx_kc < L.kh * L.kw else L.kh * L.kw
    best = 0
    for py in range(L.sh):
        for px in range(L.sw):
            ids = [(ky * L.kw + kx) // tc for ky in range(py, L.kh, L.sh) for kx in range(px, L.kw, L.sw)]
            best = max(best, sum(1 for j, c in enumerate(ids) if j == 0 or c != ids[j - 1]))
    return best


U_MAX, U_FT = 4, 1


def dx_mode(L, nsrc, B, ldy):
    """nn_gemm.hip: 2 = 32 features x 128 samples per workgroup, 3 = 32 x 32 tiles with one wave per (source, chunk), -1 = not an LDS-tiled dX"""
    dense = L.kind == "dense"
    S = nchunks(L.N, L.dx_kc) if dense else 1; kc = chunk_len(L.N, L.dx_kc)
    if B % 32 or ldy % 4 or L.N % 32 or (S > 1 and kc % 32) or L.w_off % 4:
        return -1
    if not dense and (L.cin % (16 * U_FT) or L.kh * L.kw > 64 or L.npos > 65535):
        return -1
    nch = S if dense else conv_max_chunks(L)
    if B % 128 == 0 and (dense or (nch <= 1 and L.cin % 32 == 0)) and (nsrc == 1 or S == 1):
        return 2
    return 3 if nsrc * nch <= U_MAX else -1


def mfma_dx_ok(L, B, ldy):
    dense = L.kind == "dense"
    S = nchunks(L.N, L.dx_kc) if dense else 1; kc = chunk_len(L.N, L.dx_kc)
    if B % 16 or L.N % 4 or (S > 1 and kc % 4) or ldy % 4:
        return False
    return L.K % 16 == 0 if dense else L.cin % 16 == 0


def red_head_ok(B, K, S, nA, nstream, N0, N1):
    NO = N0 + (N1 if nstream > 1 else 0)
    return (B % 4 == 0 and 4 <= B <= 1024 and K % 32 == 0 and K <= 512 and K * nstream <= 1024 and K * NO <= 4096 and 1 <= S <= 16 and 1 <= nA <= 8 and N0 == nA and
            (nstream == 1 or N1 == 1) and 12 * max(N0, N1) <= 256 and 32 * max(N0, N1) <= 256 and 12 * NO <= 256)


def facts(net, plan, B, hp):
    """what the program builder decides for this network, plan and batch: one dict, keys as the cases' `want` uses them"""
    G, Pint = geometry(net, plan)
    lv = levels_of(G)
    mf, dq, nA = bool(hp.use_mfma), bool(hp.double_q), net.n_actions
    ncon, ld0, E = (2 * B if dq else B), 2 * B, int(np.prod(net.obs_shape))
    f = dict(G=G, levels=lv, Pint=Pint, ncon=ncon)
    # tiny_step.hip: the whole step as one single-workgroup launch
    fl = 3 * _c4(Pint) + _c4(E * ld0) + _c4(B * 3 * nA) + sum(_c4(g.N * ncon) + 2 * _c4(g.N * B) for g in G)
    fl = max(fl, (7808 + 64 * 4 + 1024) // 4)
    f["tiny_lds_fits"] = fl * 4 <= 144 * 1024
    f["tiny"] = bool(hp.prioritized_replay and B <= 64 and len(G) <= 8 and len(lv) <= 8 and Pint <= 16384 and Pint * B <= 262144 and
                     all(g.kind == "dense" and nchunks(g.N, g.dx_kc) == 1 for g in G) and f["tiny_lds_fits"])
    if f["tiny"]:
        return f
    # the byte arena of a u8 replay
    l0 = G[lv[0][0]]
    f["arena"] = bool(hp.obs_dtype and mf and B % 4 == 0 and E % 4 == 0 and len(lv) > 1 and sum(g.src < 0 for g in G) == 1 and len(lv[0]) == 1 and
                         gemm_fwd_eligible(l0, [(ld0, 0, ncon), (ld0, B, B)]) and gemm_dw_eligible(l0, B, ld0))
    # the fused head level
    heads = [G[i] for i in lv[-1]]
    ok = (len(heads) == 2 and heads[0].stream == "val") if net.dueling else len(heads) == 1
    lds = (1 + nA) * 4
    for g in heads:
        ok = ok and g.kind == "dense" and nchunks(g.N, g.dx_kc) == 1
        lds += (3 * g.K + 3 * g.N * nchunks(g.K, g.fwd_kc) + 3 * g.N) * 4
    f["head_lds"] = lds
    f["fuse_heads"] = fuse = bool(ok and lds <= 60 * 1024)
    rh, rh_S = False, 0
    if fuse and len(lv) >= 2:
        La = heads[-1]; Lv = heads[0] if len(heads) == 2 else None
        pa, pv = La.src, (Lv.src if Lv else -1)
        ok = pa >= 0 and (Lv is None or (pv >= 0 and pv != pa))
        ok = ok and pa in lv[-2] and (Lv is None or pv in lv[-2]) and len(lv[-2]) == (2 if Lv else 1)
        if ok:
            Pa = G[pa]; rh_S = nchunks(Pa.K, Pa.fwd_kc)
            ok = Pa.kind == "dense" and chunk_len(La.K, La.fwd_kc) == 32 and nchunks(La.K, La.fwd_kc) * 32 == La.K
            if ok and Lv:
                Pv = G[pv]
                ok = Pv.kind == "dense" and Pv.N == Pa.N and nchunks(Pv.K, Pv.fwd_kc) == rh_S and chunk_len(Lv.K, Lv.fwd_kc) == 32 and Lv.K == La.K
            ok = ok and red_head_ok(B, La.K, rh_S, nA, 2 if Lv else 1, La.N, Lv.N if Lv else 0)
        rh = bool(ok)
    f["head"] = ("red_head" if rh_S > 1 else "head_cols4") if rh else ("head_td" if fuse else "td_huber")
    # per layer: forward, dW, dX
    for li, lvl in enumerate(lv):
        in_head = fuse and li + 1 == len(lv)
        probs = {i: [(ld0 if G[i].src < 0 else ncon, 0, ncon), (ld0 if G[i].src < 0 else B, B if G[i].src < 0 else 0, B)] for i in lvl}
        whole = mf and all(same_geo(G[lvl[0]], G[i]) for i in lvl) and gemm_fwd_eligible(G[lvl[0]], [p for i in lvl for p in probs[i]])
        join_lds = False
        if net.dueling and len(lvl) == 2 and G[lvl[0]].src == G[lvl[1]].src and G[lvl[0]].stream != "base" and G[G[lvl[0]].src].stream == "base" and not in_head:
            a, b = G[lvl[0]], G[lvl[1]]
            Sp = nchunks(b.N, b.dx_kc) if b.kind == "dense" else 1
            join_lds = mf and same_geo(a, b) and a.dx_kc == b.dx_kc and dx_mode(b, 2, B, ncon) >= 0 and (Sp == 1 or dx_mode(b, 2, B, ncon) == 3)
            f[f"join{lvl[1]}"] = "lds" if join_lds else "tmp"
        for k, i in enumerate(lvl):
            g = G[i]
            f[f"fwdS{i}"] = nchunks(g.K, g.fwd_kc); f[f"dwS{i}"] = nchunks(g.npos * B, g.dw_kc); f[f"dxkc{i}"] = g.dx_kc
            f[f"dwNT{i}"] = 4 if g.N % 64 == 0 else (2 if g.N % 32 == 0 else 1)
            if in_head:
                f[f"fwd{i}"] = f[f"dw{i}"] = f[f"dx{i}"] = "head"
                continue
            f[f"fwd{i}"] = "lds" if (whole or (mf and gemm_fwd_eligible(g, probs[i]))) else ("mfma+valu" if mf and mfma_fwd_ok(g, ncon) and not mfma_fwd_ok(g, B) else
                                                                                               ("mfma" if mf and mfma_fwd_ok(g, ncon) else "valu"))
            ldx = ld0 if g.src < 0 else ncon
            f[f"dw{i}"] = "lds" if mf and gemm_dw_eligible(g, B, ldx) else ("mfma" if mf and mfma_dw_ok(g, B) else "valu")
            if g.src < 0:
                f[f"dx{i}"] = "none"
                continue
            is_join = f"join{lvl[-1]}" in f
            Sp = nchunks(g.N, g.dx_kc) if g.kind == "dense" else 1
            if is_join and join_lds:
                f[f"dx{i}"], f[f"dxmode{i}"], f[f"dxred{i}"] = "join", dx_mode(g, 2, B, ncon), False
                continue
            addend = is_join and k == 0          # the level runs back to front: the adv stream writes join_tmp, the val stream adds it
            mode = dx_mode(g, 1, B, ncon)
            f[f"dxmode{i}"] = mode
            S = 1 if (mf and not addend and mode == 3) else Sp
            f[f"dx{i}"] = "lds" if (mf and not addend and mode >= 0) else ("mfma" if mf and g.N >= 16 and mfma_dx_ok(g, B, ncon) else "valu")
            f[f"dxred{i}"] = S > 1
    # the dW slabs of plan chunks (engine_program.hip, final_segs): summed inside the Adam launch when every split block is a whole number of 16-byte sets and there
    # are at most eight of them, else by a launch of their own ("dw_reduce_all")
    split = [g for g in G if nchunks(g.npos * B, g.dw_kc) > 1]
    f["dwsum"] = "none" if not split else ("adam" if len(split) <= 8 and all(g.w_off % 4 == 0 and ((g.K + 1) * g.N) % 4 == 0 for g in split) else "launch")
    return f


def launches(f):
    """(must, must_not): launch-name tokens ('+'-separated parts of the names profile_step returns) the facts imply.  The LDS-tiled and the direct-MFMA
    dW (and dX) launches carry the same name ("dw_<layer>", "dx_<layer>"): names tell them from the VALU tasks only; the forward families differ in name."""
    if f["tiny"]:
        return {"tiny_step"}, {"head_td", "red_head", "head_cols4", "td_huber", "adam"}
    must, never = {f["head"], "adam"}, {"tiny_step"} | ({"head_td", "red_head", "head_cols4", "td_huber"} - {f["head"]})
    (must if f["dwsum"] == "launch" else never).add("dw_reduce_all")
    G = f["G"]
    for lvl in f["levels"]:
        for i in lvl:
            g = G[i]; nm = g.name
            fw = f[f"fwd{i}"]
            if fw == "head":
                never |= {f"fwd_{nm}", f"fwd_on_{nm}", f"fwd_tg_{nm}", f"dw_{nm}", f"dw2_{nm}", f"dx_{nm}"}
                continue
            if fw == "lds":
                never |= {f"fwd_on_{nm}", f"fwd_tg_{nm}"}
                if i == lvl[0]:
                    must.add(f"fwd_{nm}")
            else:
                never.add(f"fwd_{nm}")
                if fw == "mfma":
                    must |= {f"fwd_on_{nm}", f"fwd_tg_{nm}"}
                elif fw == "mfma+valu":
                    must.add(f"fwd_on_{nm}"); never.add(f"fwd_tg_{nm}")
                else:
                    never |= {f"fwd_on_{nm}", f"fwd_tg_{nm}"}; must.add(f"fwd_valu_{G[lvl[0]].name}")
            if f[f"dw{i}"] == "valu":
                never |= {f"dw_{nm}", f"dw2_{nm}"}
            elif len(lvl) == 1:
                must.add(f"dw_{nm}")
            dx = f[f"dx{i}"]
            if dx == "join":
                must.add(f"dx_join_{G[lvl[-1]].name}"); never.add(f"dx_{nm}")
            elif dx in ("lds", "mfma"):
                must.add(f"dx_{nm}")
            else:
                never |= {f"dx_{nm}", f"dx_join_{nm}"}
            if dx not in ("none", "join"):
                (must if f[f"dxred{i}"] else never).add(f"dx_reduce_{nm}")
    return must, never


def assert_launches(h, f, name):
    tokens = {t for n, _ in h.profile_step(max_entries=512) for t in n.split("+")}
    must, never = launches(f)
    assert must <= tokens and not (never & tokens), (name, "missing", sorted(must - tokens), "unexpected", sorted(never & tokens), "launched", sorted(tokens))
    return tokens


# ------------------------------------------------------------------ a case: network, options, data; deterministic from the case
class Case(types.SimpleNamespace):
    """obs: observation shape; layers: () -> [layers of feedforward_reference's vocabulary]; dueling; B; mfma, graph, u8, prio, dq, gamma; dup: duplicates in the step indices;
    want: {fact key: value} the case was written for; seed; live: every parameter block must have a gradient (False only where the network itself has a dead block);
    zero_conv: the first conv has all-zero weights (the exact-tie case of the pool table); draws: how many seeds (seed + 1000 * try) prepare() may try -- 1: the seed is FIXED"""


def case(name, obs, layers, B, dueling=False, mfma=1, graph=1, u8=0, prio=1, dq=1, gamma=0.95, dup=False, want=None, seed=1, live=True, zero_conv=False, draws=20):
    return Case(name=name, obs=tuple(obs) if not np.isscalar(obs) else (obs,), layers=layers, B=B, dueling=dueling, mfma=mfma, graph=graph, u8=u8, prio=prio,
                dq=dq, gamma=gamma, dup=dup, want=want or {}, seed=seed, live=live, zero_conv=zero_conv, draws=draws)


def network(c):
    ls = c.layers()
    return O.Network(c.obs, *O.create_dueling_network(ls)) if c.dueling else O.Network(c.obs, ls)


def hparams(c, net, graph=None, mfma=None):
    return ref.hparams_for(net, batch_size=c.B, buffer_size=c.B + 24, learning_rate=LR, gamma=c.gamma, double_q=c.dq, prioritized_replay=c.prio, obs_dtype=c.u8,
                           use_mfma=c.mfma if mfma is None else mfma, use_graph=c.graph if graph is None else graph, seed=5)


def case_plan(c, layers, hp):
    """the plan the case runs under: the default plan, through the case's `edit` where it has one (tests/plan_edges_common.py)"""
    plan = ref.default_plan(layers, hp)
    edit = getattr(c, "edit", None)
    return [tuple(p) for p in edit(plan)] if edit else plan


def case_facts(c):
    net = network(c); hp = hparams(c, net)
    return facts(net, case_plan(c, FR.layer_descs(net), hp), c.B, hp)


def check_want(c):
    f = case_facts(c)
    for k, v in c.want.items():
        assert k in f and f[k] == v, f"{c.name}: written for {k} = {v!r}, the rules give {f.get(k)!r}"
    return f


def _draw(c, net, seed, steps):
    rng = np.random.default_rng(seed)
    n = c.B + 24
    if c.u8:
        s, sp = (rng.integers(0, 256, (n,) + net.obs_shape).astype(np.uint8) for _ in range(2))
    else:
        s, sp = (rng.random((n,) + net.obs_shape, dtype=np.float32) for _ in range(2))
    a = rng.integers(0, net.n_actions, n).astype(np.int32); r = (2 * rng.standard_normal(n)).astype(np.float32); d = (rng.random(n) < 0.2).astype(np.uint8)
    p_on = O.Network.flatten(FR.init_params(net, seed)); p_on = (p_on + 0.02 * rng.standard_normal(p_on.shape)).astype(np.float32)
    if c.zero_conv:      # the exact-tie case: the first conv has all-zero weights and a non-zero bias, so every window of the pool behind it ties in both precisions
        l0 = net.base[0]; nw = int(np.prod(l0.param_shapes()[0]))
        p_on[:nw] = 0.0; p_on[nw:nw + l0.cout] = np.linspace(0.25, 0.75, l0.cout, dtype=np.float32)
    p_tg = (p_on + 0.05 * rng.standard_normal(p_on.shape)).astype(np.float32)
    idx = []
    for k in range(steps):
        ix = rng.choice(n, c.B, replace=False).astype(np.int64)
        if c.dup and c.B > 1:
            ix[rng.integers(0, c.B, max(1, c.B // 4))] = ix[0]
        idx.append(ix)
    return dict(s=s, sp=sp, a=a, r=r, d=d, p_on=p_on, p_tg=p_tg, idx=idx)


def _gap(q):
    t = np.sort(q, axis=1)[:, -2:]
    return float((t[:, 1] - t[:, 0]).min()) if q.shape[1] > 1 else np.inf


def _fp64_batch(c, D, ix, prio):
    """get_batch in fp64 from the drawn rows (IS weights from the given priorities)"""
    f = (lambda x: x.astype(np.float32) / np.float32(255)) if c.u8 else (lambda x: x)
    w = O.is_weights(prio[ix], prio, 0.4, np.float64)      # (solver.prioritized_replay only gates update_priorities!: the buffer weights every batch)
    return f(D["s"][ix]), D["a"][ix], D["r"][ix], f(D["sp"][ix]), D["d"][ix].astype(np.float64), w


def fp64_trajectory(c, net, D, steps):
    """the case's steps with the reference alone (fp64 Adam, fp64 priorities): yields (parameters before the step, batch, step_numpy's result)"""
    p = D["p_on"].astype(np.float64); adam = FR.Adam(p.size, lr=LR)
    prio = O.priority_from_td(np.abs(D["r"]), np.float32(1e-3), np.float32(0.6)).astype(np.float64)
    for k in range(steps):
        batch = _fp64_batch(c, D, D["idx"][k], prio)
        o = FR.step_numpy(net, p, D["p_tg"], batch, float(np.float32(c.gamma)), c.dq)
        yield p, batch, o
        if c.prio:
            prio[D["idx"][k]] = O.priority_from_td(np.abs(o["td"]), np.float32(1e-3), np.float32(0.6), np.float64)
        p = adam.step(p, o["grads"])


def trajectory_ok(c, net, D, steps):
    """along an fp64 trajectory of the steps: the top-two gap of every column of the network that picks the action > 2 GAP, relu and MaxPool margins > 2 RELU_MARGIN
    (a zero_conv case ties every window on purpose), (first step) no dead gradient block"""
    for k, (p, batch, o) in enumerate(fp64_trajectory(c, net, D, steps)):
        rm, pm = FR.margins(net, p, batch[0])
        if not (_gap(o["q_on_sp"] if c.dq else o["q_tg_sp"]) > 2 * GAP and rm > 2 * RELU_MARGIN and (c.zero_conv or pm > 2 * RELU_MARGIN) and
                (k > 0 or not c.live or not FR.dead_blocks(net, o["grads"]))):
            return False
    return True


_PREP = {}


def prepare(c, steps=3):
    """the case's network, data and parameters: drawn from seed + 1000 * try, try < c.draws, until trajectory_ok holds; fails after that, never skips.  A table whose
    cases say draws = 1 has FIXED seeds: the margins are asserted, never redrawn (the seeds were found on the CPU with the reference alone: find_seed)"""
    if (c.name, steps) not in _PREP:
        net = network(c)
        for t in range(c.draws):
            D = _draw(c, net, c.seed + 1000 * t, steps)
            if trajectory_ok(c, net, D, steps):
                D["tries"] = t
                _PREP[c.name, steps] = (c, net, D)
                break
        else:
            raise AssertionError(f"{c.name}: seed {c.seed} does not keep the margins (feedforward_edges_common.find_seed)" if c.draws == 1 else
                                 f"{c.name}: no draw in {c.draws} with every argmax gap > {GAP}, every relu and MaxPool margin > {RELU_MARGIN} and every gradient block alive")
    pc, net, D = _PREP[c.name, steps]
    assert pc is c, f"two cases are named {c.name}"
    return net, D


def find_seed(c, steps=3, cap=400):
    net = network(c)
    for seed in range(1, cap):
        if trajectory_ok(c, net, _draw(c, net, seed, steps), steps):
            return seed
    raise AssertionError(f"{c.name}: no seed below {cap} keeps the margins")


def check_legs_along_trajectory(c, steps=3):
    """the two legs of the reference, 1e-10 relative on every quantity, along the fp64 trajectory of the case's steps"""
    net, D = prepare(c, steps)
    for p, batch, o in fp64_trajectory(c, net, D, steps):
        FR.legs_agree(o, FR.step_torch(net, p, D["p_tg"], batch, float(np.float32(c.gamma)), c.dq))


def _worst(k, err, tol):
    WORST[k] = max(WORST.get(k, 0.0), float(np.max(np.asarray(err) / np.asarray(tol))))


def _close(k, got, want, atol=0.0, rtol=0.0, msg=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, tol = np.abs(got - want), atol + rtol * np.abs(want)
    _worst(k, err, tol)
    assert (err <= tol).all(), f"{msg}: {k} off by {err.max():.3g} (tolerance there {float(np.broadcast_to(tol, err.shape).ravel()[np.argmax(err)]):.3g})"


def make_handle(Engine, c, net, D, graph=None, mfma=None, layers=None, plan=None, s=None, sp=None, hp_net=None, **kw):
    """plan: None (the engine's own), a plan, or (layers, hyper-parameters) -> plan, e.g. ref.default_plan -- the twin has no planner of its own.
    layers / s / sp / hp_net: another network on the case's data (the pad table's exact check: the pad-0 network on the zero-extended observations).  kw: the engine's"""
    hp = hparams(c, hp_net or net, graph, mfma)
    layers = FR.layer_descs(net) if layers is None else layers
    h = Engine(layers, hp, plan=plan(layers, hp) if callable(plan) else plan, **kw)
    h.replay_add(D["s"] if s is None else s, D["a"], D["r"], D["sp"] if sp is None else sp, D["d"])
    h.set_params(D["p_on"], 0); h.set_params(D["p_tg"], 1)
    return h, hp


def run_checked(Engine, c, steps=3, **kw):
    """`steps` train steps on the case's indices, each compared with the fp64 reference evaluated at the engine's own previous parameters and batch.
    Returns the open handle and the per-step record (for the bit-for-bit companions)."""
    net, D = prepare(c, steps)
    h, hp = make_handle(Engine, c, net, D, **kw)
    gamma = float(np.float32(c.gamma))
    adam = FR.Adam(D["p_on"].size, lr=LR)
    rec = []
    for k in range(steps):
        msg = f"{c.name} step {k}"
        idx = D["idx"][k]
        p_prev = h.get_params(0)
        np.testing.assert_array_equal(h.get_params(1), D["p_tg"])                        # the target net does not move
        batch = h.get_batch(idx)
        o = FR.step_numpy(net, p_prev, D["p_tg"], batch, gamma, c.dq)
        pr_before = h.replay_priorities()
        _close("is_weights", batch[5], O.is_weights(pr_before[idx], pr_before, hp.prio_beta, np.float64), rtol=2e-6, msg=msg)
        rm, pm = FR.margins(net, p_prev, batch[0])
        assert rm > RELU_MARGIN, f"{msg}: a relu unit of the fp64 reference sits on its kink"
        assert c.zero_conv or pm > RELU_MARGIN, f"{msg}: a MaxPool window of the fp64 reference is a near-tie"
        loss, gn, td = h.train_step(idx)
        q = h.last_q()
        _close("q_on_s", q["q_on_s"], o["q_on_s"], msg=msg, **TOL_Q)
        _close("q_tg_sp", q["q_tg_sp"], o["q_tg_sp"], msg=msg, **TOL_Q)
        if c.dq:
            _close("q_on_sp", q["q_on_sp"], o["q_on_sp"], msg=msg, **TOL_Q)
        assert _gap(o["q_on_sp"] if c.dq else o["q_tg_sp"]) > GAP, f"{msg}: an argmax column of the fp64 reference is a near-tie"
        np.testing.assert_array_equal(q["best_a"], o["best_a"], err_msg=msg)
        _close("y", q["y"], o["y"], msg=msg, **TOL_TD)
        _close("td", td, o["td"], msg=msg, **TOL_TD)
        _close("loss", loss, o["loss"], msg=msg, **TOL_LOSS)
        g = h.get_grads()
        FR.check_grads(net, g, o["grads"], live=k == 0 and c.live)
        _close("grad_norm", gn, o["grad_norm"], msg=msg, **TOL_GN)
        newp = h.get_params(0)
        FR.check_params(newp, adam.step(p_prev, g))
        if not c.dup:
            check_priorities_after_step(h, hp, idx, pr_before, td, o["td"], batch[5])
        rec.append(dict(loss=loss, gn=gn, td=td, g=g, p=newp, q=q, pr=h.replay_priorities()))
    bp = h.get_adam_state()[2]
    _close("beta_powers", bp, [0.9 ** (steps + 1), 0.999 ** (steps + 1)], rtol=1e-12, msg=c.name)
    return h, rec


def same_bits(rec_a, rec_b, what):
    """two runs of a case (engine and twin, graph and eager): every recorded number equal bit for bit"""
    assert len(rec_a) == len(rec_b)
    for k, (a, b) in enumerate(zip(rec_a, rec_b)):
        assert a["loss"] == b["loss"] and a["gn"] == b["gn"], (what, k, a["loss"], b["loss"], a["gn"], b["gn"])
        for key in ("td", "g", "p", "pr"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what} step {k}: {key}")
        for key in ("q_on_s", "q_on_sp", "q_tg_sp", "best_a", "y"):
            np.testing.assert_array_equal(a["q"][key], b["q"][key], err_msg=f"{what} step {k}: {key}")


def replay_steps(Engine, c, steps=3, net_D=None, **kw):
    """the case's steps on another handle, unchecked: the record only (net_D: another network on the case's data -- the pool table's 1x1-window case)"""
    net, D = net_D or prepare(c, steps)
    h, _ = make_handle(Engine, c, net, D, **kw)
    rec = []
    for k in range(steps):
        loss, gn, td = h.train_step(D["idx"][k])
        rec.append(dict(loss=loss, gn=gn, td=td, g=h.get_grads(), p=h.get_params(0), q=h.last_q(), pr=h.replay_priorities()))
    h.close()
    return rec


# ------------------------------------------------------------------ a. the boundary table
def _hidden_act(n):
    """relu on narrow layers only: every relu unit of a batch must clear RELU_MARGIN over three steps, which a draw can satisfy for ~1e4 units, not for 1e5"""
    return RELU if n <= 32 else (TANH if n <= 128 else SIG)


def mlp(*dims, acts=None):
    return lambda: [O.Dense(dims[k], dims[k + 1], acts[k] if acts else (_hidden_act(dims[k + 1]) if k + 2 < len(dims) else I)) for k in range(len(dims) - 1)]


def conv2(c1, c2, hidden, nA, a1=TANH, a2=SIG, a3=None):
    """Conv(c1), Conv(c2), Dense(feat, hidden), Dense(hidden, nA); c = (k, cin, cout, stride), k and stride a scalar or (h, w); feat from the obs of the case"""
    def build(obs):
        l1, l2 = O.Conv(c1[0], c1[1], c1[2], a1, c1[3]), O.Conv(c2[0], c2[1], c2[2], a2, c2[3])
        feat = int(np.prod(l2.out_shape(l1.out_shape(obs))))
        return [l1, l2, O.Dense(feat, hidden, _hidden_act(hidden) if a3 is None else a3), O.Dense(hidden, nA, I)]
    return build


def _cv(name, obs, c1, c2, hidden, nA, B, acts=(TANH, SIG, None), **kw):
    b = conv2(c1, c2, hidden, nA, *acts)
    return case(name, obs, lambda: b(obs), B, **kw)


BOUNDARY = [
    # ---- forward, gemm_fwd_eligible (layer 0 is the layer under test; prio = 0 keeps these small networks off the single-launch step)
    case("fwd_n16", 64, mlp(64, 16, 48, 4), 32, prio=0, want={"fwd0": "lds", "fwd1": "mfma"}),                 # N % 16; layer 1: K = 16, not % 32
    case("fwd_n24", 64, mlp(64, 24, 48, 4), 32, prio=0, dup=True, want={"fwd0": "valu", "dw0": "valu"}),
    case("fwd_k32", 32, mlp(32, 32, 32, 4, acts=(TANH, SIG, I)), 32, prio=0, want={"fwd0": "lds"}),
    case("fwd_k33", 33, mlp(33, 32, 32, 4, acts=(SIG, TANH, I)), 32, prio=0, want={"fwd0": "valu"}),           # K % 32 and K % 4
    case("fwd_k36", 36, mlp(36, 32, 32, 4), 32, prio=0, u8=1, want={"fwd0": "mfma", "arena": False}),         # K % 32 only: the direct MFMA forward
    case("fwd_k8192", 8192, mlp(8192, 64, 32, 4), 32, want={"fwd0": "lds", "fwdS0": 16}),                       # the longest LDS-tiled contraction, 16 slabs
    case("fwd_k8224", 8224, mlp(8224, 64, 32, 4), 32, graph=0, want={"fwd0": "mfma", "fwdS0": 17}),             # K > 8192 (the largest Dense: 8224 x 64)
    case("fwd_k1024_b32", 1024, mlp(1024, 32, 32, 4), 32, want={"fwd0": "lds", "fwdS0": 1}),                   # split-K of the default plan: K > 1024 and B < 128
    case("fwd_k1028_b32", 1028, mlp(1028, 32, 32, 4), 32, dup=True, want={"fwd0": "mfma", "fwdS0": 3}),        # chunks of 344: not % 32
    case("fwd_k1056_b96", 1056, mlp(1056, 32, 32, 4), 96, want={"fwd0": "lds", "fwdS0": 3}),                    # chunks of 352
    case("fwd_k1024_b128", 1024, mlp(1024, 32, 32, 4), 128, graph=0, want={"fwd0": "lds", "fwdS0": 1}),
    case("fwd_k1056_b128", 1056, mlp(1056, 32, 32, 4), 128, want={"fwd0": "lds", "fwdS0": 1}),                  # B = 128: unsplit
    case("fwd_b16", 64, mlp(64, 32, 32, 4), 16, prio=0, want={"fwd0": "lds", "fwd1": "lds"}),                   # ncols % 16: the target net's B columns
    case("fwd_b8", 64, mlp(64, 32, 32, 4), 8, prio=0, want={"fwd0": "mfma+valu"}),                               # online 2B = 16 columns: direct MFMA; target 8: VALU
    case("fwd_b5", 64, mlp(64, 32, 32, 4), 5, prio=0, dup=True, want={"fwd0": "valu", "dw0": "valu"}),
    case("head_k127", 64, mlp(64, 127, 4), 32, prio=0, want={"fwdS1": 1, "head": "head_td"}),                   # the head rule N < 16 && K >= 128 -> fwd_kc = 32
    case("head_k128", 64, mlp(64, 128, 4), 32, prio=0, want={"fwdS1": 4, "head": "head_cols4", "dxkc0": 32}),
    # ---- dW, gemm_dw_eligible (LDS-tiled and direct-MFMA dW launches share a name: the facts tell them apart, the launch names only from VALU)
    case("dw_b32", 64, mlp(64, 32, 32, 4), 32, prio=0, want={"dw0": "lds", "dw1": "lds"}),
    case("dw_b33", 64, mlp(64, 32, 32, 4), 33, prio=0, want={"dw0": "valu", "fwd0": "valu"}),
    case("dw_b36", 64, mlp(64, 32, 32, 4), 36, prio=0, graph=0, want={"dw0": "mfma"}),                          # B % 32, but % 4: the direct MFMA dW
    case("dw_k15", 15, mlp(15, 32, 32, 4), 32, prio=0, want={"dw0": "mfma"}),                                    # K < 16
    case("dw_k16", 16, mlp(16, 32, 32, 4), 32, prio=0, want={"dw0": "lds"}),
    case("dw_nt4", 64, mlp(64, 64, 32, 4), 32, prio=0, want={"dw0": "lds", "dwNT0": 4}),
    case("dw_nt2", 64, mlp(64, 96, 32, 4), 32, prio=0, dup=True, want={"dw0": "lds", "dwNT0": 2}),
    case("dw_nt1", 64, mlp(64, 48, 32, 4), 32, prio=0, want={"dw0": "lds", "dwNT0": 1}),
    # (small_dw -- (K+1)*N <= 16384 at B <= 256 -- is a rule of the recurrent layers' dW only (engine_program.hip bwd_recurrent): no feed-forward network reaches it;
    #  tests/test_recurrent_edges_gpu.py runs recurrent layers on both sides of it)
    _cv("conv_dw_b32", (4, 12, 14), (3, 4, 16, 1), (3, 16, 32, 1), 32, 4, 32, want={"dw0": "lds", "dw1": "lds"}),          # chunks of whole 32-sample tiles
    _cv("conv_dw_b48", (4, 12, 14), (3, 4, 16, 1), (3, 16, 32, 1), 32, 4, 48, want={"dw0": "mfma", "dw1": "mfma"}),                           # sample-granular: multiples of B
    # ---- dX, dx_mode (layer 1 is the layer under test)
    case("dx_n48", 64, mlp(64, 32, 48, 4), 32, prio=0, want={"dxmode1": -1, "dx1": "mfma"}),                    # N % 32
    case("dx_n64", 64, mlp(64, 32, 64, 4), 32, prio=0, want={"dxmode1": 3, "dx1": "lds"}),
    case("dx_b96", 64, mlp(64, 64, 64, 4), 96, want={"dxmode1": 3}),
    case("dx_b128", 64, mlp(64, 64, 64, 4), 128, want={"dxmode1": 2}),                                           # B % 128: 128-sample tiles
    case("dx_b160", 64, mlp(64, 64, 64, 4), 160, graph=0, want={"dxmode1": 3}),
    case("dx_n127", 64, mlp(64, 64, 127, 4), 32, prio=0, want={"dxkc1": 0, "dx1": "valu"}),                      # dense dx_kc: N >= 128 and B <= 64 -> N / 4
    case("dx_n128", 64, mlp(64, 64, 128, 4), 32, want={"dxkc1": 32, "dxmode1": 3, "dxred1": False}),            # four chunks combined inside the launch
    case("dx_n512", 64, mlp(64, 64, 512, 4), 32, want={"dxkc1": 128, "dxmode1": 3}),
    case("dx_n544", 64, mlp(64, 64, 544, 4), 32, dup=True, want={"dxkc1": 256, "dxmode1": 3}),                  # N > 512: chunks of 256 (three)
    case("dx_n544_b128", 64, mlp(64, 64, 544, 4), 128, want={"dxkc1": 256, "dxmode1": 2, "dxred1": True}),      # ... through slabs and a reduce launch
    case("dx_units4", 64, mlp(64, 64, 1024, 4), 32, want={"dxmode1": 3, "dxred1": False}),                      # nsrc * nch = 4 = U_MAX
    case("dx_units5", 64, mlp(64, 64, 1056, 4), 32, graph=0, want={"dxmode1": -1, "dx1": "mfma", "dxred1": True}),     # five chunks
    _cv("dx_join_s2", (2, 14, 16), (3, 2, 16, 1), (3, 16, 32, 2), 128, 4, 32, dueling=True, want={"join4": "lds", "dxkc2": 64, "dxkc4": 64, "dxmode4": 3}),    # the dueling join: N / 2 per stream, 2 x 2 units
    _cv("dx_join_units6", (2, 14, 16), (3, 2, 16, 1), (3, 16, 32, 2), 544, 4, 32, dueling=True, want={"join4": "tmp", "dx4": "lds", "dx2": "mfma"}),          # 2 sources x 3 chunks > U_MAX: val adds to adv's
    _cv("dx_cin16", (2, 14, 16), (3, 2, 16, 1), (3, 16, 32, 1), 32, 4, 32, want={"dxmode1": 3, "dx1": "lds"}),
    _cv("dx_cin8", (2, 14, 16), (3, 2, 8, 1), (3, 8, 32, 1), 32, 4, 32, want={"dxmode1": -1, "dx1": "valu"}),                                  # cin % 16
    _cv("dx_taps64", (2, 14, 16), (3, 2, 16, 1), (8, 16, 32, 1), 32, 4, 32, want={"dxmode1": 3, "dx1": "lds", "dxkc1": 16}),                  # kh * kw = 64
    _cv("dx_taps66", (2, 14, 16), (3, 2, 16, 1), ((6, 11), 16, 32, 1), 32, 4, 32, graph=0, want={"dxmode1": -1, "dx1": "mfma"}),              # 6 x 11 = 66 > 64
    # ---- the single-launch step (tiny_step.hip)
    # (Pint <= 16384 never decides: the step keeps three copies of the parameters in LDS, so its 144 KB bound stops at Pint <= 12288; the pair below stands at that bound.
    #  Pint = 16384 and 16516 still run, on the multi-launch side)
    case("tiny_lds_in", 101, mlp(101, 100, 4), 8, want={"tiny": True, "Pint": 10604, "tiny_lds_fits": True}),                                                         # 147408 of 147456 bytes
    case("tiny_lds_out", 102, mlp(102, 100, 4), 8, want={"tiny": False, "Pint": 10704, "tiny_lds_fits": False}),                                                       # 148672
    case("tiny_pint_16384", 125, mlp(125, 126, 4), 16, want={"tiny": False, "Pint": 16384}),
    case("tiny_pint_16516", 125, mlp(125, 127, 4), 16, want={"tiny": False, "Pint": 16516}),
    case("tiny_pintb_at", 90, mlp(90, 44, 2, acts=(TANH, I)), 64, dup=True, want={"tiny": True, "Pint": 4096}),                                # Pint * B = 262144
    case("tiny_pintb_above", 90, mlp(90, 44, 3, acts=(TANH, I)), 64, want={"tiny": False, "Pint": 4140, "tiny_lds_fits": True}),
    case("tiny_b64", 16, mlp(16, 32, 3, acts=(SIG, I)), 64, u8=1, want={"tiny": True}),
    case("tiny_b65", 16, mlp(16, 32, 3, acts=(SIG, I)), 65, want={"tiny": False}),
    case("tiny_l8", 12, mlp(12, 16, 16, 16, 16, 16, 16, 16, 4), 8, graph=0, want={"tiny": True}),                                              # 8 layers
    case("tiny_l9", 12, mlp(12, 16, 16, 16, 16, 16, 16, 16, 16, 4), 8, want={"tiny": False}),
    case("tiny_dueling", 12, mlp(12, 24, 20, 4), 8, dueling=True, dq=0, want={"tiny": True}),
    case("tiny_noprio", 12, mlp(12, 24, 4), 8, prio=0, want={"tiny": False}),
    # ---- head fusion (fuse_heads / fuse_rh)
    case("heads_na1", 64, mlp(64, 32, 32, 1), 32, dueling=True, prio=0, live=False, want={"fuse_heads": True}),       # one action: adv - mean(adv) = 0, the adv stream has no gradient
    case("heads_na2", 64, mlp(64, 32, 32, 2), 32, dueling=True, prio=0, graph=0, want={"fuse_heads": True, "head": "head_cols4"}),
    case("heads_na7", 64, mlp(64, 32, 32, 7), 32, dueling=True, prio=0, dup=True, want={"fuse_heads": True, "head": "head_cols4"}),
    case("heads_na18", 64, mlp(64, 32, 32, 18), 32, dueling=True, prio=0, want={"fuse_heads": True, "head": "head_td"}),                      # nA > 8
    case("heads_redhead", 2048, mlp(2048, 128, 4), 32, dueling=True, want={"fwdS0": 4, "head": "red_head"}),                                   # split-K producers under the heads
    case("heads_lds_in", 64, mlp(64, 5056, 4), 32, want={"fuse_heads": True, "head": "head_td", "head_lds": 61220}),                          # the head level's LDS bound, 61440 bytes
    case("heads_lds_out", 64, mlp(64, 5088, 4), 32, want={"fuse_heads": False, "head": "td_huber", "head_lds": 61604}),
    # ---- the byte arena of a u8 replay
    _cv("arena_on", (4, 12, 12), (4, 4, 32, 2), (3, 32, 32, 1), 32, 4, 32, u8=1, want={"arena": True, "fwd0": "lds"}),
    _cv("arena_off_n", (4, 12, 12), (4, 4, 24, 2), (3, 24, 32, 1), 32, 4, 32, u8=1, want={"arena": False}),                                # first layer off the LDS-tiled kernels
    _cv("arena_off_b", (4, 12, 12), (4, 4, 32, 2), (3, 32, 32, 1), 32, 4, 36, u8=1, graph=0, want={"arena": False, "dw0": "mfma"}),        # ... its dW only (B % 32)
]
# use_mfma alternates: every second case also runs with use_mfma = 0 -- the VALU kernels on the same plan, i.e. the same summation order
BOUNDARY += [Case(**{**vars(c), "name": c.name + "_valu", "mfma": 0, "want": ({"tiny": c.want["tiny"]} if "tiny" in c.want else {})}) for c in BOUNDARY[1::2]]


# ------------------------------------------------------------------ b. rectangular convolutions: kernels (kh, kw) and strides (sh, sw), as a first and as a second layer
RECT = [
    # (5,3) / (2,3) first [kh > kw, sh < sw, both remainders non-zero]; (3,5) second on a 5 x 5 map [kh < kw, ow == 1]; raw-tap chunks: 15 valid taps x 64 > 256
    _cv("rect_53_35", (3, 14, 17), ((5, 3), 3, 16, (2, 3)), ((3, 5), 16, 64, 1), 32, 4, 32, acts=(SIG, TANH, RELU), want={"dxkc1": 4, "dxmode1": 3, "dx1": "lds", "fwd1": "mfma"}),
    # (3,5) / (2,3) first; (5,3) second on a 7 x 3 map [kh > kw, ow == 1], cin = 32; dueling
    _cv("rect_35_53_dueling", (2, 16, 13), ((3, 5), 2, 32, (2, 3)), ((5, 3), 32, 64, 1), 32, 5, 32, dueling=True, want={"dxkc1": 4, "dxmode1": 3, "dx1": "lds", "fwd1": "lds"}),
    # 1 x 4 first, 4 x 1 second, strides (1,3) and (3,1) with remainders; B = 128: the 128-sample dX tiles
    _cv("rect_14_41_b128", (4, 9, 20), ((1, 4), 4, 32, (1, 3)), ((4, 1), 32, 32, (3, 1)), 64, 3, 128, acts=(TANH, SIG, TANH), want={"dxmode1": 2, "dx1": "lds", "dw0": "lds"}),
    # 4 x 1 / (3,2) first [sh > sw], 1 x 4 second; use_mfma = 0
    _cv("rect_41_14_valu", (3, 17, 12), ((4, 1), 3, 16, (3, 2)), ((1, 4), 16, 32, 1), 32, 4, 32, mfma=0, acts=(TANH, SIG, RELU), want={"dx1": "valu"}),
    # (4,6) / (2,1) second: 12 valid taps x 32 > 256 -> raw-tap chunks of 3 with kw = 6 != kh; u8 replay on the byte arena
    _cv("rect_44_46_u8", (4, 12, 12), (4, 4, 16, 1), ((4, 6), 16, 32, (2, 1)), 32, 4, 32, u8=1, dup=True, want={"dxkc1": 3, "dxmode1": 3, "arena": True}),
    # (2,6) / (1,2) first, (6,2) / (2,1) second; B = 128, dueling, six actions
    _cv("rect_26_62_b128_dueling", (4, 12, 17), ((2, 6), 4, 32, (1, 2)), ((6, 2), 32, 32, (2, 1)), 64, 6, 128, dueling=True, graph=0, want={"dxmode1": 2}),
    # the first case's network at an odd batch on the VALU kernels, duplicates in the batch
    _cv("rect_53_35_b7_valu", (3, 14, 17), ((5, 3), 3, 16, (2, 3)), ((3, 5), 16, 64, 1), 32, 4, 7, mfma=0, dup=True, acts=(RELU, RELU, RELU), want={"dxkc1": 4}),
    # a kernel as tall as the map (oh == 1) as a first layer, (2,3) / (1,2) second; B = 48: direct MFMA dW and dX
    _cv("rect_oh1_b48", (3, 6, 19), ((6, 4), 3, 16, (1, 2)), ((1, 3), 16, 32, (1, 2)), 32, 4, 48, want={"dw1": "mfma", "dx1": "mfma"}),
]
CASES = BOUNDARY + RECT


# ------------------------------------------------------------------ c. seeded random configurations, kernels and strides drawn per axis
ACTS = [RELU, TANH, I, SIG]


def random_net(rng, B):
    """test_fuzz_gpu.random_net's vocabulary with the kernel and the stride of every convolution drawn independently per axis (relu only on layers of
    up to 4096 units per batch, see _hidden_act)"""
    act = lambda units, pool: int(rng.choice(pool if units * B <= 4096 else [a for a in pool if a != RELU]))
    layers = []
    if rng.random() < 0.7:
        c, h, w = int(rng.choice([1, 2, 3, 4])), int(rng.integers(8, 16)), int(rng.integers(8, 16))
        obs = (c, h, w)
        for _ in range(int(rng.integers(1, 3))):
            kh, kw = int(rng.choice([1, 2, 3, 4, 5])), int(rng.choice([1, 2, 3, 4, 5]))
            sh, sw = int(rng.choice([1, 2, 3])), int(rng.choice([1, 2, 3]))
            co = int(rng.choice([4, 8, 16, 32]))
            if h < kh or w < kw or ((h - kh) // sh + 1) * ((w - kw) // sw + 1) < 2:
                break
            layers.append(O.Conv((kh, kw), c, co, act(co * ((h - kh) // sh + 1) * ((w - kw) // sw + 1), [RELU, TANH, SIG]), (sh, sw)))
            c, h, w = co, (h - kh) // sh + 1, (w - kw) // sw + 1
        feat = c * h * w
    else:
        feat = int(rng.choice([2, 6, 25, 33, 64])); obs = (feat,)
    for _ in range(int(rng.integers(1, 3))):
        n = int(rng.choice([8, 16, 24, 32, 48, 64, 96]))
        layers.append(O.Dense(feat, n, act(n, ACTS)))
        feat = n
    layers.append(O.Dense(feat, int(rng.choice([2, 3, 4, 5, 7])), I))
    return obs, layers


N_RANDOM = 32


def random_case(seed):
    """the seed's configuration; prepare() redraws its data (never its shape) up to 20 times and fails the seed after that"""
    rng = np.random.default_rng(7000 + seed)
    B = int(rng.choice([1, 3, 8, 16, 17, 32, 48, 64, 96, 128]))
    obs, layers = random_net(rng, B)
    return case(f"random{seed}", obs, lambda: layers, B, dueling=bool(rng.random() < 0.5), mfma=int(rng.random() < 0.7),
                graph=int(rng.random() < 0.5), u8=int(rng.random() < 0.3), prio=int(rng.random() < 0.7), dq=int(rng.random() < 0.7), gamma=float(rng.choice([0.9, 0.99])),
                dup=bool(rng.random() < 0.3), seed=seed)


RANDOM = [random_case(s) for s in range(N_RANDOM)]
BY_NAME = {c.name: c for c in CASES + RANDOM}
assert len(BY_NAME) == len(CASES) + len(RANDOM)


# ------------------------------------------------------------------ d. Adam well past its first step
LONG = [
    case("long_mlp", 25, mlp(25, 48, 32, 4, acts=(TANH, RELU, I)), 32, dueling=True, prio=0),
    _cv("long_conv", (3, 12, 14), ((4, 3), 3, 8, (2, 1)), (3, 8, 16, 1), 32, 5, 32),
]


def long_adam(Engine, c, steps=200, **kw):
    """`steps` train steps on sampled batches: an fp64 Adam carried on the engine's own gradients against its parameters after every step, and the
    beta powers get_adam_state returns against beta ** (t + 1) (the powers the NEXT step divides by; Flux keeps them the same way) to 1e-12"""
    net = network(c)
    D = _draw(c, net, c.seed, 0)
    h, hp = make_handle(Engine, c, net, D, **kw)
    adam = FR.Adam(D["p_on"].size, lr=LR)
    p = h.get_params(0)
    for t in range(1, steps + 1):
        h.train_step()
        g, newp = h.get_grads(), h.get_params(0)
        assert np.isfinite(g).all() and np.abs(g).max() > 0
        FR.check_params(newp, adam.step(p, g))
        bp = h.get_adam_state()[2]
        _close("beta_powers", bp, [0.9 ** (t + 1), 0.999 ** (t + 1)], rtol=1e-12, msg=f"{c.name} step {t}")
        p = newp
    assert np.abs(p - D["p_on"]).max() > 50 * LR * 0.1, "200 Adam steps must have moved the parameters"
    return h
