"""Cases of the acting-step edge tests (TEST INFRASTRUCTURE): engines whose device environment loop sits on either side of a rule of the single-workgroup acting step
(tiny_act.hip: the LDS bound, the parameters x copies bound, the four-column / scalar item loops, contraction tails, chunked plans, the ring branches of add_exp!) or of
the step's tail (env_body.h: head values staged in LDS or read per use), how a case's engine is built, and THE comparison helper of the CPU and GPU files.

facts(case) restates the rules in this file's own words -- it calls nothing in the library -- and every case states in `want` the side of each rule it was written for,
as feedforward_edges_common does.  What is compared is everything group_rollout_common.observables returns (np.array_equal) plus what dqn_envs_peek_q returns: the Q
column and greedy action of the last vector step.  The only tolerance is feedforward_edges_common.TOL_Q, against the fp64 forward of feedforward_reference."""
import numpy as np

import activation_reference as AR
import dqn_oracle as O
import feedforward_edges_common as E
import feedforward_reference as FR
import ref
from engine_group_common import assert_same
from envs_common import gridworld_mlp_unequal_streams
from group_rollout_common import observables, replay_rows
from tabular_envs_common import Tables

I, R, T, SIG = O.ACT_IDENTITY, O.ACT_RELU, O.ACT_TANH, O.ACT_SIGMOID
abi = ref.abi
CALLS = (1, 1, 2, 1, 3)          # vector steps per call; the one-step calls have first = last = 1
TRAIN_FREQ, TARGET_FREQ = 2, 3
# the rules' constants, restated (tiny_act_decline, env_body.h)
LDS_LIMIT, TAIL_LDS, PXN_LIMIT, P_LIMIT, HEAD_LDS, MAX_LAYERS = 144 * 1024, 43 * 1024, 262144, 16384, 8192, 8
MAX_ITEMS = (LDS_LIMIT - TAIL_LDS) // 4      # 25 856: no activation array, hence no item loop, is longer than the dynamic LDS the rule admits


def up4(x):
    return (x + 3) // 4 * 4


def mlp(*dims, acts=None):
    """Dense chain dims[0] -> ... -> dims[-1]; acts: the hidden layers' activations (default relu, tanh alternating), the last layer is the identity"""
    acts = list(acts) if acts is not None else [(R, T)[i % 2] for i in range(len(dims) - 2)]
    return [O.Dense(dims[i], dims[i + 1], (acts + [I])[i]) for i in range(len(dims) - 1)]


def _duel(obs, layers):
    return O.Network(obs, *O.create_dueling_network(layers))


def tab_tables(nA, seed, S=3, Ef=3):
    """a tabular MDP of S states (the last one terminal), nA actions and Ef features per state: dense random rows, rewards away from zero"""
    rng = np.random.default_rng(seed)
    Tm = rng.random((S, nA, S)).astype(np.float32) + np.float32(0.1)
    Tm = (Tm / Tm.sum(-1, keepdims=True)).astype(np.float32)
    Rm = (rng.standard_normal((S, nA, S)) + 3.0 * np.sign(rng.standard_normal((S, nA, S)))).astype(np.float32)
    term = np.zeros(S, np.uint8); term[-1] = 1
    b0 = np.zeros(S, np.float32); b0[:-1] = 1.0 / (S - 1)
    return Tables(Tm, Rm, term, b0, rng.standard_normal((S, Ef)).astype(np.float32))


def _case(name, net, env, n, seed, B=4, cap=None, n_fill=None, u8=False, fwd_kc=None, last_kc=None, max_len=3, eps=(0.9, 0.1, 6.0), grouped=True, runs=True, twin=None, want=None,
          hp=None):
    """env: "grid" (SimpleGridWorld), "mdp12" (TestMDP on 3 x 2 images, two stacked: 12 features), ("tab", nA): tab_tables.  fwd_kc: that chunk length on EVERY layer;
    last_kc: on the last layer only.  grouped: the case is a member of engine groups; runs: it is not refused; twin: the CPU twin runs it (a built-in env kind and the
    four activations the twin knows)"""
    cap = cap if cap is not None else max(4 * n, 16)
    n_fill = n_fill if n_fill is not None else max(B, 4)
    assert B <= 8 and n_fill >= B and n <= cap
    builtin = env in ("grid", "mdp12")
    known = all(l.act <= SIG for l in net.all_layers())
    h = dict(double_q=seed % 2, gamma=0.95, learning_rate=1e-3, seed=seed); h.update(hp or {})
    return dict(name=name, net=net, env=env, n=n, B=B, cap=cap, n_fill=n_fill, u8=u8, fwd_kc=fwd_kc, last_kc=last_kc, max_len=max_len, eps=eps, grouped=grouped, runs=runs,
                twin=(builtin and known) if twin is None else twin, want=want or {}, hp=h)


def _grid(*layers):
    return O.Network((2,), list(layers))


def cases():
    """name -> case, in the order of the heterogeneous group"""
    tails = lambda: _grid(O.Dense(2, 7, R), O.Dense(7, 13, T), O.Dense(13, 4, I))
    edge = lambda: _grid(O.Dense(2, 21, R), O.Dense(21, 4, I))
    pxn = lambda: O.Network((2, 3, 2), mlp(12, 60, 4, acts=[T]))
    stage = lambda: O.Network((3,), mlp(3, 8, 64, acts=[R]))
    stage_duel = lambda: _duel((3,), mlp(3, 8, 16, acts=[R]))
    split = lambda: _grid(O.Dense(2, 64, R), O.Dense(64, 4, I))
    cs = [
        # the LDS bound from both sides: 152 + 1904 + 19992 + 3808 = 25 856 floats = 103 424 B, + the 43 KB tail = 144 KB exactly; n / 4 = 238 is no power of two;
        # the ring (cap 1000, 8 prefilled) wraps on the second step
        _case("lds_at", edge(), "grid", 952, 31, B=8, cap=1000, n_fill=8, max_len=4,
              want=dict(P=152, lds_floats=25856, lds_bytes=103424, total_bytes=LDS_LIMIT, refusal=None, path="v4", staged=True, max_item=21 * 238 - 1)),
        _case("lds_above", edge(), "grid", 953, 31, B=8, cap=1000, n_fill=8, max_len=4, runs=False,
              want=dict(P=152, lds_floats=25888, total_bytes=LDS_LIMIT + 128, refusal="lds", pxn_ok=True)),
        # parameters x copies: 780 + 244 = 1024 internal parameters, 256 copies = 262 144 exactly; 60 x 256 = 15 360 elements in the widest activation
        _case("pxn_at", pxn(), "mdp12", 256, 32, B=8, cap=600, n_fill=8, max_len=4,
              want=dict(P=1024, pxn=PXN_LIMIT, pxn_ok=True, refusal=None, path="v4", items=15360, max_item=60 * 64 - 1)),
        _case("pxn_above", pxn(), "mdp12", 257, 32, B=8, cap=600, n_fill=8, max_len=4, runs=False,
              want=dict(P=1024, pxn=PXN_LIMIT + 1024, pxn_ok=False, refusal="pxn", path="scalar")),
        # chunked plans with contraction tails on both item loops: K = 7 -> 5 + 2, K = 13 -> 5 + 5 + 3 (four-column loop: 4 + 1 | 2, 4 + 1 | 4 + 1 | 3)
        _case("tails_v4", tails(), "grid", 8, 33, fwd_kc=5, want=dict(path="v4", chunks=[1, 2, 3], chunk_len=[2, 5, 5], refusal=None)),
        _case("tails_scalar", tails(), "grid", 7, 34, fwd_kc=5, want=dict(path="scalar", chunks=[1, 2, 3], chunk_len=[2, 5, 5], refusal=None)),
        _case("kc1_scalar", tails(), "grid", 3, 35, fwd_kc=1, want=dict(path="scalar", chunks=[2, 7, 13], chunk_len=[1, 1, 1])),
        # the scalar loop is unrolled by 8: 19 = 2 x 8 + 3 leaves a tail, unchunked
        _case("k19_scalar", _grid(O.Dense(2, 19, R), O.Dense(19, 4, I)), "grid", 5, 36, want=dict(path="scalar", chunks=[1, 1], k_tail8=[2, 3])),
        # two siblings of one level that differ in K and N (value 32 -> 1, advantage 64 -> 4) share an item loop
        _case("unequal_streams", gridworld_mlp_unequal_streams(), "grid", 12, 37, B=8, n_fill=8, want=dict(path="v4", levels=[[(2, 32)], [(32, 32), (32, 64)], [(32, 1), (64, 4)]])),
        # eight layers, the most the kernel's tables hold; byte rows
        _case("l8", O.Network((2, 3, 2), mlp(12, 16, 16, 16, 16, 16, 16, 16, 4)), "mdp12", 4, 38, u8=True, max_len=4, want=dict(n_layers=MAX_LAYERS, path="v4")),
        # sigmoid, softsign and elu: the twin knows the first only (its act_f stops at sigmoid), so this case rests on the standalone engine and the fp64 forward
        _case("acts", _grid(*mlp(2, 9, 11, 10, 4, acts=[SIG, AR.SOFTSIGN, AR.ELU])), "grid", 6, 39, want=dict(path="scalar", twin=False)),
        # a dirty range of two goes straight to the serial chain of the tree rebuild; 4 prefilled: slots 4-5, then 6-7 (start + n == cap, no wrap), then s0 = 0
        _case("ring_two", _grid(O.Dense(2, 4, T), O.Dense(4, 4, I)), "grid", 2, 40, cap=8, n_fill=4, want=dict(path="scalar", cap2=8)),
        _case("ring_two_c9", _grid(O.Dense(2, 4, T), O.Dense(4, 4, I)), "grid", 2, 40, cap=9, n_fill=4, want=dict(path="scalar", cap2=16)),      # slots 8, 0: the wrapping branch
        # the tail's head staging from both sides, in k_tiny_act (the unstaged branch reads LDS through a generic pointer): 64 x 128 = 8192 floats, 64 x 129 = 8256
        _case("stage_at", stage(), ("tab", 64), 128, 41, B=8, n_fill=8, cap=300, want=dict(per_col=64, head_floats=HEAD_LDS, staged=True, staged_group=True, path="v4")),
        _case("stage_above", stage(), ("tab", 64), 129, 41, B=8, n_fill=8, cap=300, want=dict(per_col=64, head_floats=HEAD_LDS + 64, staged=False, staged_group=False, path="scalar")),
        _case("stage_duel_at", stage_duel(), ("tab", 16), 481, 42, B=8, n_fill=8, cap=1000, want=dict(per_col=17, head_floats=8177, staged=True, staged_group=True, path="scalar")),
        _case("stage_duel_above", stage_duel(), ("tab", 16), 482, 42, B=8, n_fill=8, cap=1000, want=dict(per_col=17, head_floats=8194, staged=False, staged_group=False, path="scalar")),
        # standalone only, a built-in kind: the unstaged branch of the four-launch tail under the CPU twin.  The last layer's contraction of 64 in chunks of 4: 16 slabs
        # per head value.  The fused tail wants head chunks of 32 (fused_head_layout), so it declines the shape: both settings run the four-launch tail
        _case("split_head_at", split(), "grid", 128, 43, B=8, n_fill=8, cap=300, last_kc=4, grouped=False, want=dict(per_col=64, head_floats=HEAD_LDS, staged=True, fused_tail=False)),
        _case("split_head_above", split(), "grid", 129, 43, B=8, n_fill=8, cap=300, last_kc=4, grouped=False, want=dict(per_col=64, head_floats=HEAD_LDS + 64, staged=False, fused_tail=False)),
    ]
    return {c["name"]: c for c in cs}


PAIRS = {"lds_at": ("lds_above", "lds"), "pxn_at": ("pxn_above", "pxn"), "stage_at": ("stage_above", "staged"), "stage_duel_at": ("stage_duel_above", "staged"),
         "split_head_at": ("split_head_above", "staged")}
CHUNKED = ("tails_v4", "tails_scalar", "kc1_scalar", "split_head_at", "split_head_above")


def runnable_grouped():
    return [c for c in cases().values() if c["grouped"] and c["runs"]]


# ------------------------------------------------------------------ the rules, restated
def case_plan(c, default):
    """the plan the case runs under: the default plan with its dX sums in one chunk (the single-workgroup train step takes no other), through the case's fwd_kc"""
    plan = [(f, 0, w) for f, _, w in default]
    if c["fwd_kc"]:
        plan = [(c["fwd_kc"], 0, w) for _, _, w in plan]
    if c["last_kc"]:
        plan = plan[:-1] + [(c["last_kc"], 0, plan[-1][2])]
    return plan


def _levels(net):
    """[[(K, N) of the level's one or two sibling layers]]: the base chain, then the value and advantage streams side by side"""
    lv = [[(l.n_in, l.n_out)] for l in net.base]
    if net.dueling:
        assert len(net.val) == len(net.adv)
        lv += [[(v.n_in, v.n_out), (a.n_in, a.n_out)] for v, a in zip(net.val, net.adv)]
    return lv


def facts(c, plan=None):
    """what the rules decide for this case, from the network, the copy count and the plan's fwd_kc alone (plan: [(fwd_kc, dx_kc, dw_kc)] per layer; None: unsplit unless the
    case itself names a chunk length)"""
    net, n = c["net"], c["n"]
    layers = net.all_layers()
    kcs = [p[0] for p in plan] if plan is not None else [c["fwd_kc"] or 0] * (len(layers) - 1) + [c["last_kc"] or c["fwd_kc"] or 0]
    P = sum(up4(l.n_in * l.n_out + l.n_out) for l in layers)      # every layer's weights and bias start 16-byte aligned
    Ef = int(np.prod(net.obs_shape))
    lds_floats = up4(P) + up4(Ef * n) + sum(up4(l.n_out * n) for l in layers)
    total = 4 * lds_floats + TAIL_LDS
    pxn_ok = P <= P_LIMIT and P * n <= PXN_LIMIT
    refusal = None if pxn_ok and total <= LDS_LIMIT else ("pxn" if not pxn_ok else "lds")      # the parameter rule is asked first
    v4 = n % 4 == 0
    lv = _levels(net)
    items = max(sum(N for _, N in level) * n for level in lv)
    S = [E.nchunks(l.n_in, kc) for l, kc in zip(layers, kcs)]
    head = net.adv[-1] if net.dueling else net.base[-1]
    Sa = S[layers.index(head)]; Sv = S[layers.index(net.val[-1])] if net.dueling else 0
    per_col = Sa * net.n_actions + Sv
    cap2 = 1
    while cap2 < c["cap"]:
        cap2 *= 2
    return dict(P=P, lds_floats=lds_floats, lds_bytes=4 * lds_floats, total_bytes=total, pxn=P * n, pxn_ok=pxn_ok, refusal=refusal, path="v4" if v4 else "scalar",
                items=items, max_item=(items // 4 if v4 else items) - 1, chunks=S, chunk_len=[E.chunk_len(l.n_in, kc) for l, kc in zip(layers, kcs)],
                k_tail8=[l.n_in % 8 for l in layers], levels=lv, n_layers=len(layers), per_col=per_col, head_floats=per_col * n, staged=per_col * n <= HEAD_LDS,
                staged_group=(net.n_actions + int(net.dueling)) * n <= HEAD_LDS,      # k_tiny_act hands the tail finished head outputs: one slab per value whatever the plan

                cap2=cap2, twin=c["twin"], fused_tail=False if E.chunk_len(head.n_in, kcs[layers.index(head)]) != 32 else None)


def check_want(c, plan=None):
    f = facts(c, plan)
    for k, v in c["want"].items():
        assert k in f and f[k] == v, f"{c['name']}: written for {k} = {v!r}, the rules give {f.get(k)!r}"
    return f


def refusal_text(c):
    """the words a refused case must be refused with (tiny_act_decline's), from facts alone"""
    f = facts(c)
    return {"lds": f"it needs {f['total_bytes']} bytes of LDS", "pxn": f"too many parameters for {c['n']} copies"}[f["refusal"]]


def qdiv(x, d):
    """k_tiny_act's item division: one multiply by the fp32 reciprocal, all in fp32"""
    f32 = np.float32
    return ((np.asarray(x).astype(f32) + f32(0.5)) * (f32(1.0) / f32(d))).astype(np.int64)


# ------------------------------------------------------------------ building a case's engine
def env_of(envs, c):
    if c["env"] == "grid":
        return envs.SimpleGridWorld(n=c["n"], seed=5)
    if c["env"] == "mdp12":
        return envs.TestMDP((2, 3), 2, 6, n=c["n"], seed=3)
    return None


def initial_params(c, seed=None):
    net, seed = c["net"], c["hp"]["seed"] if seed is None else seed
    p = O.Network.flatten(O.init_params(net, seed=seed))
    return (p + 0.05 * np.random.default_rng(seed).standard_normal(p.shape)).astype(np.float32)      # non-zero biases


def layers_hp(c):
    net = c["net"]
    return ref.layers_from_network(net), ref.hparams_for(net, batch_size=c["B"], buffer_size=c["cap"], obs_dtype=abi.OBS_U8 if c["u8"] else abi.OBS_F32, **c["hp"])


def build(c, factory, default_plan, envs, plan=None, params=None, env_seed=17, **factory_kw):
    """one engine of the case with its parameters, replay prefill (non-zero rewards) and env set: the group member, the standalone engine and the twin come from calls of this"""
    layers, hp = layers_hp(c)
    h = factory(layers, hp, plan=case_plan(c, default_plan(layers, hp)) if plan is None else plan, **factory_kw)
    h.set_params(initial_params(c) if params is None else params, 0); h.sync_target()
    h.replay_add(*replay_rows(c))
    seed = env_seed + c["hp"]["seed"]
    if isinstance(c["env"], tuple):
        h.envs_create_tabular(n_envs=c["n"], max_episode_length=c["max_len"], seed=seed, **tab_tables(c["env"][1], c["hp"]["seed"]).kwargs())
    else:
        h.envs_create(env_of(envs, c), max_episode_length=c["max_len"], seed=seed)
    return h


def unsplit_plan(c, default):
    return [(0, 0, w) for _, _, w in default]


# ------------------------------------------------------------------ the comparison helper
def q64(c, p_flat, obs):
    """the fp64 Q values of the case's network: feedforward_reference's forward; a network with an activation beyond its four codes walks the same Dense chain with
    activation_reference's closed forms"""
    net = c["net"]
    x = np.asarray(obs, np.float64).reshape(len(obs), -1)
    ps = net.unflatten(np.asarray(p_flat, np.float64))
    if all(l.act <= SIG for l in net.all_layers()):
        return FR.q_numpy(net, ps, x)[0]

    def chain(layers, ps, x):
        for k, l in enumerate(layers):
            x = AR.act_np(x @ ps[2 * k] + ps[2 * k + 1], l.act)
        return x
    xb = chain(net.base, ps, x)
    if not net.dueling:
        return xb
    nb = 2 * len(net.base); nv = 2 * len(net.val)
    v, a = chain(net.val, ps[nb:nb + nv], xb), chain(net.adv, ps[nb + nv:], xb)
    return v + a - a.mean(axis=1, keepdims=True)


def step_record(h, stats=None, trained=True, td=True):
    """observables (which hold envs_peek_q's q and greedy) of an engine after a call"""
    return observables(h, stats, td=td, trained=trained)


def acted_rows(c, rec):
    """the observations the last vector step acted on: the s rows it wrote into the ring (k_env_observe2: s = the observation of the pre-step state), as the policy saw them"""
    n, cap = c["n"], c["cap"]
    slots = (int(rec["counters.widx"]) - n + np.arange(n)) % cap
    s = rec["ck.s"][slots]
    return (s.astype(np.float32) / np.float32(255.0) if c["u8"] else s), slots


def check_record(c, got, want=None, p_acting=None, greedy_only=False, what=""):
    """THE comparison of one call's record.  want: another engine's record (everything np.array_equal, q and greedy included; keys the other engine lacks -- the twin
    has no TD getter -- are left out on both sides).  Always: greedy is the first-max argmax of the returned q, and the ring holds the executed actions; greedy_only:
    nothing explored in the call, the executed actions are the greedy ones.  p_acting: the online parameters the last step acted with -- q against the fp64 forward of
    the rows it acted on under E.TOL_Q, greedy against the fp64 argmax wherever the fp64 top-two gap is at least E.GAP"""
    name = f"{c['name']} {what}"
    q, greedy = got["peekq.q"], got["peekq.greedy"]
    assert q.shape == (c["n"], c["net"].n_actions) and q.dtype == np.float32 and greedy.dtype == np.int32, name
    assert np.array_equal(greedy, np.argmax(q, axis=1)), (name, "greedy is not the first-max argmax of q", greedy, np.argmax(q, axis=1))
    rows, slots = acted_rows(c, got)
    assert np.array_equal(got["ck.a"][slots], got["peek.actions"]), (name, "ring actions")
    if greedy_only:
        assert np.array_equal(got["peek.actions"], greedy), (name, "actions under eps = 0", got["peek.actions"], greedy)
    if want is not None:
        keys = set(got) & set(want)
        assert {k for k in set(got) ^ set(want) if not k.startswith(("td", "is_weights"))} == set(), (name, sorted(set(got) ^ set(want)))
        assert_same({k: got[k] for k in keys}, {k: want[k] for k in keys}, name)
    if p_acting is not None:
        ref64 = q64(c, p_acting, rows)
        E._close("acting_q", q, ref64, msg=name, **E.TOL_Q)
        top = np.sort(ref64, axis=1)
        clear = top[:, -1] - top[:, -2] >= E.GAP
        assert np.array_equal(greedy[clear], ref64.argmax(1)[clear]), (name, "greedy vs the fp64 argmax")


def trains_before_last_step(t0, k, train_freq=TRAIN_FREQ):
    """a call of k vector steps from t0 trains before its last step acts: the parameters that step acted with are then not observable from outside the call"""
    return any(t % train_freq == 0 for t in range(t0, t0 + k - 1))


def run_calls(h, c, roll, calls=CALLS, eps=None, check=None):
    """the calls of the run on one engine; roll(h, k, t0, eps) -> the call's statistics.  -> one record per call.  check(record, call index, parameters before the call, t0, k)"""
    t0, recs, trained = 1, [], False
    for j, k in enumerate(calls):
        p_before = h.get_params(0)
        st = roll(h, k, t0, c["eps"] if eps is None else eps)
        trained = trained or st["train_steps"] > 0
        rec = step_record(h, st, trained=trained, td=not getattr(h, "is_twin", False))
        if check:
            check(rec, j, p_before, t0, k)
        recs.append(rec); t0 += k
    return recs


def alone_roll(h, k, t0, eps):
    return h.rollout(k, t0=t0, train_freq=TRAIN_FREQ, target_update_freq=TARGET_FREQ, eps=eps)
