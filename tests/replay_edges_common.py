"""Shared case table and checker of tests/test_replay_edges_cpu.py (the C twin) and tests/test_replay_edges_gpu.py (the HIP engine) (TEST INFRASTRUCTURE): the
replay half of batch_train! -- add_exp!, sample, the get_batch IS weights, update_priorities! -- against the fp64 model and the stratified law of
tests/replay_reference.py, which share nothing with the twin.

A case is a capacity, a batch size, a tiny Dense network (the replay dominates; the network is not under test) and a script of operations.  run() plays
the script on an engine and on the model side by side:
  * after every operation that writes priorities, the leaves the engine reports are compared with the model's (RR.LEAF_RTOL);
  * every draw -- replay_sample, or the last_indices() of a sampled train step -- is judged by the law on the leaves the engine reported BEFORE it, at the call
    counter the model keeps (one per draw; set_counters overrides it), so an internal node left stale by any operation before it shows as a draw outside d;
  * the IS weights of get_batch on the drawn indices against fp64 (rtol 2e-6, as tests/feedforward_edges_common.py), the root recovered from a weight against the
    fp64 sum (L * 2^-24 relative plus the weight's own tolerance through the power 1 / beta);
  * a sampled train step's loss against mean(huber(w64 * td)) from the returned td, the drawn indices and the priorities read before the step (TOL_LOSS): the
    weights of the train path are not returned, the loss is;
  * at the end the engine's draw counter against the model's.
`want` states the side of the program builder's rules the case was written for (facts() of feedforward_edges_common.py: tiny, arena) and the launch names the GPU
test must see.  Sharpness (at most 1 % of a case's positions with two acceptable leaves) and, for hp.sample_distinct, the left-out share of redrawn positions
(at most 5 %) with the case's stated minimum of judged redraws (`min_redrawn`) are asserted twice: by model_sharpness() on the model's own leaves and the model's own
play of every draw it can follow (RR.model_distinct: no engine, no drawn index), before any engine exists; and again at the end of a run, where sharpness comes from the
reference on the reported leaves and the redraw counts from judging the engine's own lists (which positions were redrawn is only known from them)."""
import types

import numpy as np

import dqn_oracle as O
import feedforward_edges_common as FC
import ref
import replay_reference as RR

TOL_W = 2e-6
WORST = {}                                   # largest margin / tolerance seen per quantity (1.0 = at the bound)
EPS = 1e-6
REDRAWS = {}                                 # hp.sample_distinct cases: (redrawn positions judged, left out, with R < S / 4) of the last run


def _worst(k, v):
    WORST[k] = max(WORST.get(k, 0.0), float(v))


# ------------------------------------------------------------------ priority patterns: n desired priorities
def uniform(n, rng):
    return np.ones(n)


def spread6(n, rng):
    return 10.0 ** (6.0 * rng.random(n))                            # six orders of magnitude


def mass90(n, rng):
    p = np.ones(n)
    if n > 1:
        p[int(rng.integers(0, n))] = 9.0 * (n - 1)                  # one leaf holds 90 % of the mass
    return p


def few_heavy(n, rng):
    """64 heavy leaves hold all but ~1e-4 of the mass (the light ones 80 in all): what keeps a deep tree sharp (2 d x the number of leaves wider than d must stay under 1 % of S)"""
    p = np.full(n, 80.0 / n)
    k = rng.choice(n, min(64, n), replace=False)
    p[k] = 1e4 * (1.0 + rng.random(k.size))
    return p


def heavy4(n, rng):
    """four leaves of 10 % of the mass each, the rest shared by the others within a factor of 3: at B = 16 a heavy leaf spans 1.6 strata, so most calls redraw,
    and the residual after any redraw keeps more than half of S (R >= S / 4: the redraws are judged)"""
    p = 0.6 / max(1, n - 4) * 3.0 ** (rng.random(n) - 0.5)
    p[rng.choice(n, min(4, n), replace=False)] = 0.1
    return p * 100.0


def ends_heavy(n, rng):
    p = np.ones(n); p[0] = p[-1] = 50.0                             # slot 0 and slot size - 1 (or the last row of the call)
    return p


class Case(types.SimpleNamespace):
    pass


def case(name, cap, B, ops, net=(4, 2), alpha=1.0, beta=0.4, u8=0, prio=1, distinct=0, graph=1, seed=11, want=None, names=(), min_redrawn=0):
    """ops: [(op, ...)], see run().  net: Dense widths, the first the observation length.  names: launch-name tokens a profiled step must show.  min_redrawn
    (hp.sample_distinct): redrawn positions with R >= S / 4 the case must have judged, on the model alone and on an engine"""
    return Case(name=name, cap=cap, B=B, ops=ops, net=net, alpha=alpha, beta=beta, u8=u8, prio=prio, distinct=distinct, graph=graph, seed=seed, want=want or {}, names=tuple(names),
                min_redrawn=min_redrawn)


def network(c):
    d = c.net
    return O.Network((d[0],), [O.Dense(d[k], d[k + 1], O.ACT_TANH if k + 2 < len(d) else O.ACT_IDENTITY) for k in range(len(d) - 1)])


def hparams(c, net, graph=None):
    return ref.hparams_for(net, batch_size=c.B, buffer_size=c.cap, learning_rate=1e-3, gamma=0.9, double_q=1, prioritized_replay=c.prio, obs_dtype=c.u8, use_mfma=1,
                           use_graph=c.graph if graph is None else graph, seed=c.seed, prio_alpha=c.alpha, prio_beta=c.beta, prio_eps=EPS, sample_distinct=c.distinct)


def check_want(c):
    net = network(c); hp = hparams(c, net)
    f = FC.facts(net, ref.default_plan(ref.layers_from_network(net), hp), c.B, hp)
    for k, v in c.want.items():
        assert f.get(k) == v, f"{c.name}: written for {k} = {v!r}, the rules give {f.get(k)!r}"
    return f


def _td_for(p, alpha):
    """the td_err whose priority (td + eps)^alpha is p (alpha = 0: every priority is 1 whatever the td)"""
    return np.maximum(np.asarray(p, np.float64) ** (1.0 / alpha) - EPS, 0.0).astype(np.float32) if alpha > 0 else np.asarray(p, np.float32)


def _rows(c, n, rng):
    E, nA = c.net[0], c.net[-1]
    if c.u8:
        s, sp = (rng.integers(0, 256, (n, E)).astype(np.uint8) for _ in range(2))
    else:
        s, sp = (rng.random((n, E), dtype=np.float32) for _ in range(2))
    return s, rng.integers(0, nA, n).astype(np.int32), (0.5 + rng.random(n)).astype(np.float32), sp, (rng.random(n) < 0.2).astype(np.uint8)


class Run:
    """one engine and the model, side by side"""

    def __init__(self, Engine, c, graph=None, judge=True, **kw):
        self.c, self.judge, self.Engine, self.kw = c, judge, Engine, kw
        net = network(c); self.hp = hp = hparams(c, net, graph)
        layers = ref.layers_from_network(net)
        self.h = Engine(layers, hp, plan=ref.default_plan(layers, hp), **kw)
        p = O.Network.flatten(O.init_params(net, seed=3))
        self.h.set_params(p, 0); self.h.set_params((0.9 * p).astype(np.float32), 1)
        self.m = RR.Replay(c.cap, float(hp.prio_alpha), float(hp.prio_eps))
        self.rng = np.random.default_rng(1000 + c.seed)
        self.rec = []                                                # every index list, priority vector and loss, for the bit-for-bit companions
        self.pos = self.amb = self.redrawn = self.left_out = self.small_R = self.draws = 0
        self.L = RR.depth(c.cap)

    # ---- comparisons
    def leaves(self):
        pr = self.h.replay_priorities().astype(np.float64)
        self.rec.append(pr.copy())
        if self.judge:
            want = self.m.live()
            assert pr.size == want.size == self.h.replay_size()[0], (self.c.name, pr.size, want.size)
            err = np.abs(pr - want) / want
            _worst("leaf", err.max() / RR.LEAF_RTOL(self.m.alpha))
            j = int(np.argmax(err))
            assert err[j] <= RR.LEAF_RTOL(self.m.alpha), f"{self.c.name}: leaf {j} is {pr[j]!r}, the model has {want[j]!r}"
        return pr

    def drawn(self, pr, idx, what):
        """judge one call's indices on the leaves reported before it, then the IS weights of get_batch on them"""
        c, ctr = self.c, self.m.ctr
        self.rec.append(np.asarray(idx).copy())
        self.m.ctr += 1; self.draws += 1
        if not self.judge:
            return
        what = f"{c.name}: {what}"
        if c.distinct:
            worst, amb, red, lo, small = RR.judge_distinct(pr, idx, c.seed, ctr, c.B, c.cap, what)
            self.redrawn += red; self.left_out += lo; self.small_R += small
        else:
            worst, amb = RR.judge(pr, idx, c.seed, ctr, c.B, c.cap, what)
        _worst("draw", worst); self.pos += c.B; self.amb += amb

    def weights(self, pr, idx, what):
        c = self.c
        w = self.h.get_batch(idx)[5].astype(np.float64)
        w64 = RR.is_weights(pr, idx, self.hp.prio_beta)
        err = np.abs(w - w64) / w64
        _worst("is_weight", err.max() / TOL_W)
        assert err.max() <= TOL_W, f"{c.name}: {what}: IS weight off by {err.max():.3g} relative"
        beta = float(self.hp.prio_beta)
        if beta > 0:                                                 # (beta = 0: every weight is 1 and carries no root)
            k = int(np.argmax(pr[idx])); S = pr.sum()
            root = pr.size * pr[idx[k]] * w[k] ** (1.0 / beta)       # w = (size p / root)^-beta
            tol = self.L * RR.U24 + TOL_W / beta
            _worst("root", abs(root - S) / S / tol)
            assert abs(root - S) <= tol * S, f"{c.name}: {what}: the root a weight implies is {root!r}, the leaves sum to {S!r}"

    # ---- operations
    def add(self, n, pattern=uniform, explicit=True, chunk=None):
        s, a, r, sp, d = _rows(self.c, n, self.rng)
        if explicit:
            td = _td_for(pattern(n, self.rng), self.m.alpha)
        else:
            td = None                                                # the default td_err = |r| (…replay.jl:65)
        for o in range(0, n, chunk or n):
            e = min(n, o + (chunk or n))
            self.h.replay_add(s[o:e], a[o:e], r[o:e], sp[o:e], d[o:e], td_err=None if td is None else td[o:e])
            self.m.add(np.abs(r[o:e]) if td is None else td[o:e])
        self.leaves()

    def set_leaf(self, frac):
        """replay_add of ONE row (at the ring cursor) that then holds about `frac` of the mass"""
        S = self.m.live().sum()
        self.add(1, lambda n, rng: np.array([frac / (1.0 - frac) * S]))

    def update(self, idx, pattern=spread6):
        idx = np.asarray(idx, np.int64)
        td = _td_for(pattern(idx.size, self.rng), self.m.alpha) * self.rng.choice([-1.0, 1.0], idx.size).astype(np.float32)
        self.h.update_priorities(idx, td)
        self.m.update(idx, td)
        self.leaves()

    def sample(self, k=1):
        for _ in range(k):
            pr = self.h.replay_priorities().astype(np.float64)
            idx = self.h.replay_sample()
            self.drawn(pr, idx, "replay_sample")
            if self.judge:
                self.weights(pr, idx, "replay_sample")

    def train(self, k=1):
        """k sampled train steps, each judged on its own"""
        for _ in range(k):
            pr = self.h.replay_priorities().astype(np.float64)
            loss, gn, td = self.h.train_step()
            idx = self.h.last_indices()
            self.rec.append(np.array([loss, gn], np.float32)); self.rec.append(td.copy())
            self.drawn(pr, idx, "train_step")
            if self.judge:
                want = RR.huber_mean(RR.is_weights(pr, idx, self.hp.prio_beta) * td.astype(np.float64))
                tol = FC.TOL_LOSS["atol"] + FC.TOL_LOSS["rtol"] * abs(want)
                _worst("loss", abs(loss - want) / tol)
                assert abs(loss - want) <= tol, f"{self.c.name}: train_step: loss {loss!r}, mean(huber(w64 * td)) = {want!r}"
            if self.c.prio:
                self.m.update(idx, td)
            self.leaves()

    def train_n(self, n):
        """train_steps(n), pipelined: only the last step's indices can be read.  With a static tree (prioritized_replay = 0), or n = 1, they are judged; otherwise the calls are
        counted, and the draw that FOLLOWS is judged on the tree these steps left (a pre-drawn list must belong to it)"""
        pr = self.h.replay_priorities().astype(np.float64)
        loss, gn = self.h.train_steps(n)
        idx = self.h.last_indices()
        self.rec.append(np.array([loss, gn], np.float32))
        if self.c.prio:
            if n == 1:                                              # one step: its list is the call's only draw, on the tree read just before
                self.drawn(pr, idx, "train_steps(1)")
            else:
                self.m.ctr += n; self.draws += n
                self.rec.append(idx.copy())
            got = self.h.replay_priorities().astype(np.float64)     # the model cannot follow (the td of the steps are not returned): take the engine's leaves
            self.rec.append(got.copy())
            self.m.leaves[:self.m.size] = got
        else:
            self.m.ctr += n - 1; self.draws += n - 1
            self.drawn(pr, idx, f"train_steps({n}), last step")
            self.leaves()

    def import_(self, n, pattern=spread6):
        s, a, r, sp, d = _rows(self.c, n, self.rng)
        p = pattern(n, self.rng).astype(np.float32)
        self.h.replay_import(s, sp, a, r, d, p)
        self.m.import_(p)
        self.leaves()

    def set_ctr(self, ctr):
        cn = self.h.get_counters()
        self.h.set_counters(cn["size"], cn["widx"], ctr, cn["train_steps"])
        self.m.ctr = ctr

    def refused(self):
        """size < B: the API permits no draw (…replay.jl:83)"""
        for f in (self.h.replay_sample, self.h.train_step):
            try:
                f()
            except ref.abi.DQNError as e:
                assert "r._curr_size >= r.batch_size" in str(e)
            else:
                raise AssertionError(f"{self.c.name}: a draw from {self.m.size} < B transitions was not refused")

    def checkpoint_into(self, Engine):
        """export -> import into a fresh engine, counters and parameters restored (the Adam moments are not: the replay is under test): the run continues there"""
        old = self.h
        s, sp, a, r, d, pr = old.replay_export()
        cn, p_on, p_tg = old.get_counters(), old.get_params(0), old.get_params(1)
        net = network(self.c); layers = ref.layers_from_network(net)
        self.h = Engine(layers, self.hp, plan=ref.default_plan(layers, self.hp), **self.kw)
        self.h.replay_import(s, sp, a, r, d, pr)
        self.h.set_counters(cn["size"], cn["widx"], cn["sample_ctr"], cn["train_steps"])
        self.h.set_params(p_on, 0); self.h.set_params(p_tg, 1)
        old.close()
        self.m.import_(pr)                                           # slots 0 .. size - 1, every other leaf 0
        self.m.widx = cn["widx"]
        assert self.h.get_counters()["sample_ctr"] == self.m.ctr
        self.leaves()

    def finish(self):
        c = self.c
        assert self.h.get_counters()["sample_ctr"] == self.m.ctr, (c.name, self.h.get_counters(), self.m.ctr)
        if self.judge:
            assert self.amb <= 0.01 * self.pos, f"{c.name}: {self.amb} of {self.pos} positions have more than one acceptable leaf: the case is not sharp"
            assert self.left_out <= 0.05 * self.redrawn, f"{c.name}: {self.left_out} of {self.redrawn} redrawn positions left out"
            assert self.redrawn >= c.min_redrawn, f"{c.name}: {self.redrawn} redrawn positions judged ({self.small_R} more with R < S / 4), the case promises {c.min_redrawn}"
            if c.distinct:
                REDRAWS[c.name] = (self.redrawn, self.left_out, self.small_R)
        return self.rec


def run(Engine, c, graph=None, judge=True, keep=False, **kw):
    r = Run(Engine, c, graph=graph, judge=judge, **kw)
    for op in c.ops:
        getattr(r, op[0])(*[(a(r) if callable(a) and getattr(a, "late", False) else a) for a in op[1:]])
    rec = r.finish()
    if keep:
        return r, rec
    r.h.close()
    return rec


def late(f):
    """an operation argument computed from the run (sizes, the ring cursor) when the operation starts"""
    f.late = True
    return f


def same_bits(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: record {k}")


# ------------------------------------------------------------------ index patterns of update_priorities
def _subtree8(r):
    b = 8 * int(r.rng.integers(0, max(1, r.m.size // 8)))
    return np.arange(b, min(b + 8, r.m.size))


def _siblings(r):
    j = 2 * int(r.rng.integers(0, max(1, r.m.size // 2 - 1)))
    return np.array([j, j + 1])


def _triples(r):
    j = r.rng.choice(r.m.size, 3, replace=False)
    return np.repeat(j, 3)[r.rng.permutation(9)]                     # each index three times, each time with another td


def _mixed(r):
    return np.concatenate([_triples(r), _siblings(r), _siblings(r), r.rng.integers(0, r.m.size, 20)])


def _rand(n):
    return late(lambda r: r.rng.integers(0, r.m.size, n))            # with replacement: duplicates as they come


_ends = late(lambda r: np.array([0, r.m.size - 1]))
_same = late(lambda r: np.full(5, int(r.rng.integers(0, r.m.size))))
UPDATES = [("update", _rand(n)) for n in (1, 2, 63, 64, 65, 256, 1024)] + [("update", late(_subtree8)), ("update", late(_siblings)), ("update", _ends), ("update", _same),
                                                                           ("update", late(_triples)), ("update", late(_mixed))]


def _interleave(ops, draw):
    out = []
    for o in ops:
        out += [o, draw]
    return out


def _fill(pattern, frac=1.0, **kw):
    return ("add", late(lambda r: max(r.c.B, int(r.c.cap * frac))), pattern, True)


# ------------------------------------------------------------------ the table
S1 = ("sample", 1)
CAPS = [
    # ---- capacity / depth through replay_sample: every update shape, a draw after each
    case("cap1", 1, 1, [("add", 1), ("sample", 2), ("update", np.array([0])), S1, ("add", 3, spread6), S1]),
    case("cap2", 2, 1, [("add", 1), S1, ("add", 1, spread6), S1, ("update", np.array([1, 0, 1])), ("sample", 3)]),
    case("cap3_full", 3, 2, [("add", 2), S1, ("add", 2, spread6), ("sample", 3), ("update", _ends), S1]),                                    # a wrap: two ring ranges
    case("cap63", 63, 4, [_fill(spread6)] + _interleave(UPDATES, S1), alpha=0.6),
    case("cap64", 64, 64, [_fill(mass90)] + _interleave(UPDATES, S1), beta=1.0),                                                            # size == cap == B
    case("cap65_part", 65, 4, [_fill(spread6, 0.7)] + _interleave(UPDATES, S1), beta=0.0),                                                   # size < cap: cap2 = 128, no dense top (cap2 / 2 = 64)
    case("cap100_uniform", 100, 65, [("add", 65, uniform), S1, ("add", 35, uniform), ("sample", 3), ("update", _rand(65), uniform), S1], alpha=0.0),      # size == B, then size == cap
    case("cap127", 127, 4, [_fill(ends_heavy)] + _interleave(UPDATES, S1), alpha=0.6, beta=1.0),
    case("cap129", 129, 64, [_fill(spread6)] + _interleave(UPDATES, S1)),
    case("cap8191", 8191, 512, [_fill(few_heavy)] + _interleave(UPDATES, S1), alpha=0.6),
    case("cap8193_part", 8193, 1024, [_fill(few_heavy, 0.5)] + _interleave(UPDATES, S1)),                                                      # cap2 = 16384, size < cap
    case("below_B", 16, 8, [("add", 7), ("refused",), ("add", 1), S1]),                                                                      # size < B: no draw is permitted; size == B
]
ADDS = [
    case("add_one_by_one", 37, 4, [("add", 1)] * 4 + [S1] + [("add", 1, spread6), S1] * 40),                                                    # repeated adds to reach size, then round the ring
    case("add_exactly_cap", 50, 8, [("add", 50, spread6), ("sample", 2), ("add", 50, mass90), ("sample", 2)]),
    case("add_more_than_cap", 50, 8, [("add", 20, spread6), ("add", 173, spread6), ("sample", 3)]),                                            # n > cap in one call: later rows win
    case("add_wrap", 50, 8, [("add", 40, spread6), S1, ("add", 25, ends_heavy), ("sample", 3)]),                                               # two ranges; the heavy rows land either side of the ring cursor's wrap
    case("add_default_td", 50, 8, [("add", 50, None, False), ("sample", 2), ("add", 7, None, False), ("sample", 2)], alpha=0.6),                # the |r| default
    case("add_heavy_at_cursor", 40, 8, [("add", 40, uniform), ("add", 13, uniform), ("set_leaf", 0.5), S1, ("set_leaf", 0.5), ("sample", 2)]),
]
DEEP = [
    # L = 23 > 22: an n <= 64 update goes down the level-by-level path; rows of 2 floats, imported (one pass) and added in chunks
    case("deep_L23", (1 << 22) + 5, 64, [("import_", (1 << 22) + 1, few_heavy), ("sample", 2), ("update", _rand(64)), S1, ("update", late(_mixed)), S1,
                                         ("add", 9, spread6), S1, ("train", 2)], net=(2, 2)),
]
NOT_TINY = (90, 44, 3)                                               # Pint * B = 4140 * 64 > 262144: off the single-launch step at B = 64
SITES = [
    case("site_tiny", 129, 32, [_fill(spread6), ("train", 6)], want={"tiny": True}, names=["tiny_step"]),
    case("site_tiny_eager", 100, 8, [_fill(mass90, 0.6), ("train", 6)], graph=0, alpha=0.6, want={"tiny": True}, names=["tiny_step"]),
    case("site_fused_f32", 200, 64, [_fill(spread6), ("train", 5)], net=NOT_TINY, want={"tiny": False}, names=["sample_gather", "adam"]),
    case("site_fused_u8_e4", 200, 64, [_fill(spread6), ("train", 5)], net=(92, 44, 3), u8=1, want={"tiny": False, "arena": False}, names=["sample_gather"]),
    case("site_fused_u8_e3", 200, 64, [_fill(spread6), ("train", 5)], net=(91, 44, 3), u8=1, graph=0, seed=12, want={"tiny": False, "arena": False}, names=["sample_gather"]),
    case("site_fused_arena", 200, 64, [_fill(spread6), ("train", 5)], net=(128, 48, 3), u8=1, want={"tiny": False, "arena": True}, names=["sample_gather"]),
    case("site_b128_in_bwd", 300, 128, [_fill(spread6), ("train", 5)], net=(32, 32, 32, 4), want={"tiny": False, "dw0": "lds", "dw1": "lds"}, names=["sample", "gather", "-prio_fork"]),
    case("site_b65_forked", 300, 65, [_fill(spread6), ("train", 5)], names=["sample", "gather", "prio_fork"]),
    case("site_b512_forked_eager", 1000, 512, [_fill(spread6), ("train", 4)], graph=0, names=["sample", "gather", "prio_fork"]),
    case("site_pipelined", 200, 64, [_fill(spread6), ("train_n", 5), ("train_n", 1), ("train", 2), ("train_n", 3), ("train_n", 1), S1], net=NOT_TINY, names=["sample_gather"]),
    case("site_pipelined_tiny", 129, 32, [_fill(spread6), ("train_n", 5), ("train_n", 1), ("train", 2), ("train_n", 2), ("train_n", 1), S1], want={"tiny": True}),
    case("site_pipelined_b128", 300, 128, [_fill(spread6), ("train_n", 4), ("train_n", 1), ("train", 2)], net=(32, 32, 32, 4)),
    case("site_noprio", 100, 16, [_fill(uniform, 0.5), ("train", 3), ("train_n", 4), S1], prio=0, want={"tiny": False}),                      # uniform leaves, never updated
    case("site_noprio_spread", 100, 16, [_fill(spread6), ("train", 2), ("train_n", 4), ("train_n", 2)], prio=0, graph=0),
]
_half = ("set_leaf", 0.5)
_smaller = ("import_", 40, spread6)


def _invalidate(name, op, **kw):
    """a step that pre-drew, the operation, a step: the new draws belong to the NEW tree and counter"""
    return case("inval_" + name, 129, 32, [_fill(spread6), ("train", 2), op, ("train", 2), ("train_n", 3), op, ("train", 1)], **kw)


INVALIDATE = [
    _invalidate("add_tiny", _half, want={"tiny": True}), _invalidate("add_fused", _half, net=NOT_TINY),
    _invalidate("update_tiny", ("update", _rand(40))), _invalidate("update_fused", ("update", _rand(40)), net=NOT_TINY, graph=0),
    _invalidate("import_tiny", _smaller), _invalidate("import_fused", _smaller, net=NOT_TINY),
    _invalidate("sample_tiny", S1), _invalidate("sample_fused", S1, net=NOT_TINY),
    _invalidate("counter_tiny", ("set_ctr", (1 << 32) + 12345)), _invalidate("counter_fused", ("set_ctr", (7 << 32) + 3), net=NOT_TINY),
    case("inval_add_b128", 300, 128, [_fill(spread6), ("train", 2), _half, ("train", 2), ("update", _rand(40)), ("train", 1), S1, ("train", 1)], net=(32, 32, 32, 4)),
    case("inval_add_b65", 300, 65, [_fill(spread6), ("train", 2), _half, ("train", 2), ("set_ctr", 1 << 33), ("train", 2)]),
]
DISTINCT = [
    # one leaf with 90 % of the mass: the residual of every redraw is 10 % of S, below S / 4, so NO redraw is judged here: the case checks distinctness (and the leaves,
    # weights and counters) only; the redraw law is held by the three cases below
    case("distinct_mass90", 96, 16, [_fill(mass90), ("sample", 20)], distinct=1),
    case("distinct_heavy4", 96, 16, [_fill(heavy4), ("sample", 40), ("update", _rand(30), heavy4), ("sample", 20)], distinct=1, min_redrawn=60),
    case("distinct_size_eq_B", 20, 16, [("add", 16, heavy4), ("sample", 30)], distinct=1, min_redrawn=20),
    case("distinct_train", 96, 16, [_fill(heavy4), ("sample", 10), ("train", 6)], distinct=1, net=NOT_TINY, min_redrawn=10),
]
CHECKPOINT = [
    case("checkpoint_tiny", 129, 32, [_fill(spread6, 0.8), ("train", 3), ("set_ctr", (1 << 32) - 2), ("train", 1), ("checkpoint_into", late(lambda r: r.Engine)), ("train", 3)]),
    case("checkpoint_fused", 200, 64, [_fill(spread6), ("train", 3), ("checkpoint_into", late(lambda r: r.Engine)), ("train", 2), S1], net=NOT_TINY),
]
CASES = CAPS + ADDS + SITES + INVALIDATE + DISTINCT + CHECKPOINT
BY_NAME = {c.name: c for c in CASES + DEEP}
assert len(BY_NAME) == len(CASES) + len(DEEP)


def model_sharpness(c):
    """before any engine: the operations the model can follow by itself (adds, imports, updates, replay_sample) played on the model alone; at most 1 % of the
    positions drawn on its leaves may have two acceptable leaves, and with hp.sample_distinct the model's own play of those draws (RR.model_distinct) must leave
    out at most 5 % of its redrawn positions and reach the case's min_redrawn.  Stops at the first train step (its priorities come from a network), whose own
    draw -- on leaves the model still knows -- is the last one counted."""
    r = types.SimpleNamespace(c=c, m=RR.Replay(c.cap, np.float32(c.alpha), np.float32(EPS)), rng=np.random.default_rng(1000 + c.seed))
    pos = amb = red = out = small = 0

    def draw():
        nonlocal pos, amb, red, out, small
        amb += RR.sharp(r.m.live(), c.seed, r.m.ctr, c.B, c.cap); pos += c.B
        if c.distinct:
            _, a_, b_, c_ = RR.model_distinct(r.m.live(), c.seed, r.m.ctr, c.B, c.cap)
            red += a_; out += b_; small += c_
        r.m.ctr += 1

    for op in c.ops:
        a = [(x(r) if callable(x) and getattr(x, "late", False) else x) for x in op[1:]]
        if op[0] == "add":
            n, pattern, explicit = a[0], (a[1] if len(a) > 1 else uniform), (a[2] if len(a) > 2 else True)
            _, _, rw, _, _ = _rows(c, n, r.rng)
            r.m.add(_td_for(pattern(n, r.rng), r.m.alpha) if explicit else np.abs(rw))
        elif op[0] == "import_":
            _rows(c, a[0], r.rng); r.m.import_((a[1] if len(a) > 1 else spread6)(a[0], r.rng).astype(np.float32))
        elif op[0] == "update":
            idx = np.asarray(a[0]); pattern = a[1] if len(a) > 1 else spread6
            r.m.update(idx, _td_for(pattern(idx.size, r.rng), r.m.alpha) * r.rng.choice([-1.0, 1.0], idx.size).astype(np.float32))
        elif op[0] == "sample":
            for _ in range(a[0]):
                draw()
        elif op[0] == "refused":
            pass
        else:
            if r.m.size >= c.B:
                draw()
            break
    assert pos > 0 and amb <= 0.01 * pos, f"{c.name}: {amb} of {pos} positions have more than one acceptable leaf on the model"
    assert out <= 0.05 * red, f"{c.name}: the model leaves out {out} of its {red} redrawn positions"
    assert red >= c.min_redrawn, f"{c.name}: the model redraws {red} positions with R >= S / 4 ({small} more below), the case promises {c.min_redrawn}"
    return dict(ambiguous=amb, positions=pos, redrawn=red, left_out=out, small_R=small)


# ------------------------------------------------------------------ statistics: inclusion counts against the strata's own expectation
def chi_square(Engine, cap, size, B, draws, seed=77, **kw):
    """the 5-sigma chi-square of parity_common.sampler_distribution with expected counts summed over the strata (RR.stratum_probabilities), at a capacity that is
    no power of two with size < cap, and at B = 512"""
    c = case(f"chi_{cap}_{B}", cap, B, [], seed=seed)
    r = Run(Engine, c, **kw)
    r.add(size, lambda n, rng: 0.5 + 40.0 * rng.random(n) ** 4)
    pr = r.h.replay_priorities().astype(np.float64)
    counts = np.zeros(size)
    for _ in range(draws):
        idx = r.h.replay_sample()
        assert idx.min() >= 0 and idx.max() < size
        np.add.at(counts, idx, 1)
    q = RR.stratum_probabilities(pr, B)
    expect = draws * q.sum(axis=0)
    np.testing.assert_allclose(expect, draws * B * pr / pr.sum(), rtol=1e-9)
    chi2 = float(((counts - expect) ** 2 / expect).sum()); dof = size - 1
    assert chi2 < dof + 5.0 * np.sqrt(2.0 * dof), (chi2, dof)
    var = draws * (q * (1.0 - q)).sum(axis=0)                        # a sum of independent Bernoulli draws, one per stratum and call
    z = np.abs(counts - expect) / np.sqrt(np.maximum(var, 1e-300))
    assert z[var > 25].max() < 6.0, float(z[var > 25].max())         # and per leaf against the strata's own (smaller than multinomial) variance
    uniform_ = np.full(size, draws * B / size)
    assert ((counts - uniform_) ** 2 / uniform_).sum() > 50 * dof
    r.h.close()
    return chi2
