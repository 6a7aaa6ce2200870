"""Seeded random CROSS-KIND networks against the one fp64 step reference (TEST INFRASTRUCTURE): the grammar, the generator, the fixed tables FF and REC, the probe that
is the union of the per-kind observers, the seed search and its screens.  tests/test_composition_cpu.py and tests/test_composition_gpu.py stand on it.

THE GRAMMAR is this module's own statement of where a layer may stand -- a restatement of the placement rules nn.lower and the engine's build_layers enforce, not a
"draw and redraw when nn.lower raises" (that would hide a wrong refusal): a case the grammar admits and either of the two refuses is a finding.  A chain is a sequence of
TOKENS: the layer kinds, with "activation" and "skip" carrying the shape they stand on (":map" / ":vec"); a skip block is ONE token.  NEXT[a] lists what may directly
follow a; PAIRS is every (a, b) with b in NEXT[a], and every one of them appears in a case of FF (test_composition_cpu asserts it).
    obs:map -> conv | a pool                      (Activation, GroupNorm and a skip block are never first)
    a map token -> any map token | dense          (the flatten; LayerNorm, Dropout and a vector block never stand on a map)
    obs:vec -> dense
    dense, skip:vec -> any vector token           layernorm -> all but layernorm      dropout -> all but dropout
    activation:vec -> dense | activation:vec | skip:vec whose first inner layer is a Dense      (LayerNorm and Dropout never stand directly behind an Activation --
                                                                                                  the first inner layer of a block behind one included)
    skip:map = 1-2 Conv(3, c => c, pad = 1 | SamePad()), dilation 1, groups 1      skip:vec = 1-3 of Dense / LayerNorm / Dropout, n -> n, the same adjacency inside
    the chain ends in Dense(n, nA); create_dueling_network splits the trailing Dense run, so everything else is the base chain: Activation, GroupNorm, adaptive pools,
    general Convs and skip blocks are base-chain only by construction.  At most 32 descriptors (DQN_MAX_LAYERS) -- the depth limit is the grammar's.
Recurrent chains (REC): [conv | dense] -> optional activation | maxpool | adaptivemeanpool -> cell -> optional layernorm | dropout | activation:vec | skip:vec | cell ->
Dense head; REC_PAIRS states the pairs around a cell with the three cells as one token "cell" (16 cases cannot hold 3 x 12 pairs; every cell kind appears first and second).

SHAPES are the smallest at which the index arithmetic can go wrong (6x6 .. 9x9 maps, 1 / 2 / 4 / 8 channels, Dense 7 / 12 / 16); one image case in six draws an MFMA-sized
first Conv (16 or 32 channels at B = 32), one case in eight a split-sum Dense width (SPLIT_WIDTH: feedforward_edges_common's head_k128 -- four forward chunks, dx_kc 32).
The RELU BUDGET: at most KINK_BUDGET kinked units x columns per case (thousands of relu units leave no seed off the kinks: conv_dg_reference's table); past it a layer
draws a smooth activation.  The other DATA RULES of the builder (_Builder._code, instantiate) keep exact ties and exact kink hits out by construction -- no plateau
activation in front of a max-type pool (but a relu DIRECTLY in front of it, whose zeros the margin exempts), no max-type pool on bytes, no kinked standalone activation on exact values, no squasher in front of a normalisation -- and the
NETWORK SCREEN (ALTS, below) keeps a drawn network only if a data seed of at most SEED_CAP passes seed_ok; docs/history/composition_tests.md tells how each was found.

No tolerance is introduced here: every constant is imported."""
import types
from collections import deque

import numpy as np

import activation_layer_reference as AL
import dropout_reference as DR
import groupnorm_reference as GR
import layernorm_reference as LN
import recurrent_reference as R
import skip_reference as SR
import step_reference as S
from adaptive_pool_reference import resolve
from feedforward_edges_common import GAP, TOL_GN, TOL_LOSS, TOL_Q, TOL_TD      # noqa: F401  (one set of constants)
from feedforward_reference import RELU_MARGIN      # noqa: F401
from layernorm_reference import SIGMA_MIN      # noqa: F401
from recurrent_reference import GRAD_C, GRAD_RTOL, LIVE_BLOCK, Adam, check_params      # noqa: F401
from step_reference import blocks, check_grads, distance, ff_batch, ff_data, legs_agree, rec_data      # noqa: F401

nn = S.nn
LRATE = S.LR
STEPS = 2                  # train steps the GPU test runs per feed-forward case
ENGINE_SEED = DR.ENGINE_SEED
KINK_BUDGET = 2048         # kinked units x batch columns per case
SPLIT_WIDTH = 128          # feedforward_edges_common head_k128 / dx_n128: the head's forward in four chunks, the producer's dX in chunks of 32
MAX_DESCS = 32             # DQN_MAX_LAYERS
COND_BOUND = 0.25          # the one-ulp screen: the fp64 step moves by less than this many tolerances
N_FF, N_REC = 64, 16
CODE_MIX = (1, 2, 4)     # how a case's k-th activation code is cycled from its seed (chosen so that every code has a case: test_composition_cpu)

# ------------------------------------------------------------------ the grammar
POOLS = ("maxpool", "meanpool", "adaptivemaxpool", "adaptivemeanpool")
MAPT = ("conv",) + POOLS + ("groupnorm", "activation:map", "skip:map")
VECT = ("dense", "layernorm", "dropout", "activation:vec", "skip:vec")
CELLS = ("lstm", "gru", "rnn")
NEXT = {"obs:map": ("conv",) + POOLS, "obs:vec": ("dense",)}
NEXT.update({m: MAPT + ("dense",) for m in MAPT})
NEXT.update({"dense": VECT, "skip:vec": VECT, "layernorm": tuple(t for t in VECT if t != "layernorm"), "dropout": tuple(t for t in VECT if t != "dropout"),
             "activation:vec": ("dense", "activation:vec", "skip:vec")})
PAIRS = sorted((a, b) for a in MAPT + VECT for b in NEXT[a])
MAP_PAIRS = [p for p in PAIRS if p[0] in MAPT and p[1] in MAPT]
FLAT_PAIRS = [p for p in PAIRS if p[0] in MAPT and p[1] == "dense"]
VEC_PAIRS = [p for p in PAIRS if p[0] in VECT]
REC_BEFORE = ("conv", "dense", "activation:map", "activation:vec", "maxpool", "adaptivemeanpool")
REC_AFTER = ("layernorm", "dropout", "activation:vec", "skip:vec", "cell", "dense")
REC_PAIRS = sorted([(a, "cell") for a in REC_BEFORE] + [("cell", b) for b in REC_AFTER])
KINKED = tuple(sorted(AL.KINKS))      # the codes with a kink
PLATEAU = (1, 9, 10, 14)      # relu, relu6, hardtanh, hardswish: whole intervals map to ONE value -- exact ties in a MaxPool window, exact hits of the next layer's kink
UNBOUNDED = (0, 1, 4, 5, 6, 7, 11, 12, 13, 14)      # not a squasher: a normalisation layer behind tanh / sigmoid / softsign / relu6 / hardtanh sees sigma ~ 0.01


def route(a, b):
    """the shortest token path from behind a to in front of b (both excluded) through NEXT"""
    seen, todo = {a: None}, deque([a])
    while todo:
        t = todo.popleft()
        if b in NEXT[t]:
            path = []
            while t != a:
                path.append(t); t = seen[t]
            return path[::-1]
        for u in NEXT[t]:
            if u not in seen:
                seen[u] = t; todo.append(u)
    raise AssertionError(f"the grammar has no path from {a} to {b}")


class Infeasible(Exception):
    """the drawn token sequence does not fit the drawn shapes (the GRAMMAR's own shape rules): the generator takes its next alternative"""


# ------------------------------------------------------------------ token -> layer specification (plain tuples: a case's network is data, compared by ==)
class _Builder:
    def __init__(self, rng, B, sid, mfma_draw=False, split_draw=False):
        self.rng, self.B, self.sid, self.kinks, self.nfused, self.nact = rng, B, sid, 0, 0, 0
        self.mfma_draw, self.split_draw = mfma_draw, split_draw
        self.exact = self.no_plateau = self.unbounded = self.relu_ok = self.relu_zeros = False      # the data rules' state: see _code

    def pick(self, xs, p=None):
        return xs[int(self.rng.choice(len(xs), p=p))]

    def _code(self, units, n_codes, k, kinked_ok=True):
        """the k-th code of the case, cycled from the seed so that all codes appear over the table -- unless a DATA RULE forbids it here, then the nearest allowed one:
        no kinked code past the relu budget or on exact values; no plateau (PLATEAU) in front of a max-type pool; no squasher in front of a normalisation"""
        budget = self.kinks + units * self.B <= KINK_BUDGET
        ok = [x for x in range(n_codes) if (not self.unbounded or x in UNBOUNDED) and (not self.no_plateau or x not in PLATEAU or (x == 1 and self.relu_ok)) and (x not in KINKED or (kinked_ok and budget))]
        a = (CODE_MIX[0] * self.sid + CODE_MIX[1] * (k - 1) + CODE_MIX[2]) % n_codes
        if a not in ok:
            a = ok[(self.sid + k) % len(ok)]
        if self.relu_ok and 1 in ok:      # relu -> MaxPool, the commonest interface of all: every case that can hold it within its relu budget does (the cycle alone never put it there)
            a = 1
        if a in KINKED:
            self.kinks += units * self.B
        return a

    def fused(self, units):
        self.nfused += 1
        a = self._code(units, 11, self.nfused); self.exact = a in PLATEAU; self.relu_zeros = a == 1
        return a

    def standalone(self, units):
        self.nact += 1
        a = self._code(units, 15, self.nact, kinked_ok=not self.exact); self.exact = self.exact or a in PLATEAU; self.relu_zeros = a == 1      # (a kinked code stands on no exact values: relu's zeros are the only ones then)
        return a

    def conv(self, shp, need, first):
        c, h, w = shp; r = self.rng
        for _ in range(200):
            k = self.pick([(1, 1), (2, 2), (3, 3), (3, 2)], [0.15, 0.2, 0.45, 0.2]); s = int(r.choice([1, 2], p=[0.75, 0.25])); d = int(r.choice([1, 2], p=[0.7, 0.3]))
            pad = self.pick([0, 1, "same"], [0.4, 0.35, 0.25]); g = self.pick([1, 2, "dw"], [0.6, 0.2, 0.2])
            cout = int(r.choice([16, 32])) if (first and self.mfma_draw) else int(r.choice([1, 2, 4, 8], p=[0.1, 0.25, 0.4, 0.25]))
            g = c if g == "dw" else g
            if g == c and c > 1:
                cout = c * int(r.choice([1, 2]))
            if c % g or cout % g or cout > 32:
                continue
            eh, ew = (k[0] - 1) * d, (k[1] - 1) * d
            if pad == "same":
                if eh % 2 or ew % 2:
                    continue
                ph, pw = eh // 2, ew // 2
            else:
                ph = pw = pad
            if ph > eh or pw > ew or eh + 1 > h + 2 * ph or ew + 1 > w + 2 * pw:
                continue
            oh, ow = (h + 2 * ph - eh - 1) // s + 1, (w + 2 * pw - ew - 1) // s + 1
            if oh < need[0] or ow < need[1]:
                continue
            return ("conv", k, c, cout, self.fused(cout * oh * ow), s, pad, d, g), (cout, oh, ow)
        raise Infeasible("conv")

    def pool(self, kind, shp, need):
        c, h, w = shp
        ks = [k for k in ((2, 2), (2, 1)) if h >= k[0] and w >= k[1] and (h - k[0]) // k[0] + 1 >= need[0] and (w - k[1]) // k[1] + 1 >= need[1]]
        if not ks:
            raise Infeasible(kind)
        k = self.pick(ks)
        return (kind, k), (c, (h - k[0]) // k[0] + 1, (w - k[1]) // k[1] + 1)

    def adaptive(self, kind, shp, need):
        c, h, w = shp
        outs = [o for o in ((2, 2), (1, 2), (1, 1)) if o[0] <= h and o[1] <= w and o[0] >= need[0] and o[1] >= need[1]]
        if kind == "adaptivemaxpool" and self.no_plateau:      # Flux's windows overlap where out does not divide in: two windows then share their maximum, and a max-type pool behind them ties
            outs = [o for o in outs if h % o[0] == 0 and w % o[1] == 0]
        if not outs:
            raise Infeasible(kind)
        o = self.pick(outs)
        return (kind, o), (c, o[0], o[1])

    def groupnorm(self, shp):
        c, h, w = shp
        gs = [g for g in sorted({1, 2, 4, c}) if c % g == 0 and (c // g) * h * w >= 8]      # (sigma over fewer elements has a heavy lower tail: no seed keeps SIGMA_MIN in every column)
        if not gs:
            raise Infeasible("groupnorm")
        return ("groupnorm", c, self.pick(gs), self.fused(c * h * w)), shp

    def skip_map(self, shp):
        c, h, w = shp; m = int(self.rng.choice([1, 2])); entry, unb = self.exact, self.unbounded; self.relu_ok = False      # (behind a join the margin exempts no zeros)
        inner = []
        for j in range(m):
            self.unbounded = unb and j + 1 == m
            act = self.fused(c * h * w) if j + 1 < m or self.rng.random() < 0.5 else 0
            inner.append(("conv", (3, 3), c, c, act, 1, self.pick([1, "same"]), 1, 1))
        self.exact = entry and inner[-1][4] in PLATEAU; self.relu_zeros = False      # x + f(x): a plateau value of both
        return ("skip", tuple(inner)), shp

    def width(self):
        if self.split_draw:
            self.split_draw = False
            return SPLIT_WIDTH
        return int(self.rng.choice([7, 12, 16]))

    def dense(self, n, m=None):
        m = self.width() if m is None else m
        return ("dense", n, m, self.fused(m)), m

    def skip_vec(self, n, prev):
        """1-3 inner layers of Dense / LayerNorm / Dropout under the chain's adjacency (the entry counts as the layer in front), n -> n"""
        m = int(self.rng.choice([1, 2, 3])); toks, last = [], prev
        for _ in range(m):
            allowed = [t for t in NEXT.get(last, VECT) if t in ("dense", "layernorm", "dropout")]      # (behind a recurrent cell: what may follow a Dense)
            last = self.pick(allowed); toks.append(last)
        nd = toks.count("dense"); inner, cur, seen, entry, unb = [], n, 0, self.exact, self.unbounded
        for j, t in enumerate(toks):
            self.unbounded = toks[j + 1] == "layernorm" if j + 1 < m else unb
            if t == "dense":
                seen += 1
                spec, cur = self.dense(cur, n if seen == nd else int(self.rng.choice([7, 12, 16])))
            elif t == "layernorm":
                spec = ("layernorm", cur, self.fused(cur))
            else:
                p = float(self.rng.choice([0.25, 0.5]))
                spec = ("dropout", 0.25 if toks[j + 1:j + 2] == ["layernorm"] else p); self.exact = True
            inner.append(spec)
        self.exact = entry and self.exact      # x + f(x): a plateau value of both
        return ("skip", tuple(inner)), n


def _needs(tokens):
    """per position: the (h, w) the map must have BEHIND that token for the map tokens after it to fit (a pool halves; an adaptive pool takes what is left)"""
    need, out = (1, 1), [None] * len(tokens)
    for i in range(len(tokens) - 1, -1, -1):
        out[i] = need
        if tokens[i] in ("maxpool", "meanpool"):
            need = (2 * need[0], 2 * need[1])
        elif tokens[i] not in MAPT:
            need = (1, 1)
    return out, need


MAXT = ("maxpool", "adaptivemaxpool")


def _relu_ok(seg):
    """seg: the map tokens behind a layer.  Its relu may stay when a max-type pool follows DIRECTLY (max-type pools in a row hand the exemption on) and its exact zeros
    reach no further max-type pool: a Conv or GroupNorm stands in front of the next one"""
    if not seg or seg[0] not in MAXT:
        return False
    for j, x in enumerate(seg[1:], 1):
        if x in ("conv", "groupnorm"):
            return True
        if x not in MAXT:
            return not any(y in MAXT for y in seg[j:])
    return True


def instantiate(b, tokens, obs, u8=0):
    """tokens (behind the obs token, ending in the head's "dense") -> (layer specifications, nA is the caller's): shapes drawn under the need of what follows"""
    needs, _ = _needs(tokens); specs = []; shp = obs if len(obs) == 3 else None; n = None if shp else obs[0]; prev = "obs:map" if shp else "obs:vec"
    b.exact = bool(u8)
    for i, t in enumerate(tokens):
        assert t in CELLS or t in NEXT["dense" if prev in CELLS else prev], (prev, t)      # (what may follow a Dense may follow a cell)
        seg = tokens[i + 1:next((j for j in range(i + 1, len(tokens)) if tokens[j] not in MAPT), len(tokens))] if t in MAPT else []
        b.no_plateau = any(x in ("maxpool", "adaptivemaxpool") for x in seg)
        # ... but a relu DIRECTLY in front of a max-type pool stays (_relu_ok): the MaxPool margin exempts a window whose maximum is an exact 0 out of a relu
        b.relu_ok = _relu_ok(seg)
        nxt = [x for x in tokens[i + 1:i + 3] if x != "dropout"][:1]      # (a Dropout between the two only scales)
        b.unbounded = bool(nxt) and nxt[0] in ("layernorm", "groupnorm")
        if t in ("meanpool", "adaptivemeanpool", "dropout") or t in CELLS:
            b.relu_zeros = False
        if t in ("maxpool", "adaptivemaxpool") and b.exact and not b.relu_zeros:
            raise Infeasible("a max-type pool over exact values (the bytes of a u8 observation): its windows tie")
        if t in MAPT:
            if t == "conv":
                spec, shp = b.conv(shp, needs[i], not specs)
            elif t in ("maxpool", "meanpool"):
                spec, shp = b.pool(t, shp, needs[i])
            elif t in ("adaptivemaxpool", "adaptivemeanpool"):
                spec, shp = b.adaptive(t, shp, needs[i])
            elif t == "groupnorm":
                spec, shp = b.groupnorm(shp)
            elif t == "activation:map":
                spec = ("activation", b.standalone(int(np.prod(shp))))
            else:
                spec, shp = b.skip_map(shp)
        else:
            if shp is not None:
                n, shp = int(np.prod(shp)), None
            if t == "dense":
                spec, n = b.dense(n)
            elif t == "layernorm":
                spec = ("layernorm", n, b.fused(n))
            elif t == "dropout":
                p = float(b.rng.choice([0.25, 0.5]))
                spec = ("dropout", 0.25 if tokens[i + 1] == "layernorm" else p); b.exact = True      # the dropped elements are exact zeros; (half of 7 features dropped in front of a LayerNorm: sigma ~ 0 in some column)
            elif t == "activation:vec":
                spec = ("activation", b.standalone(n))
            elif t == "skip:vec":
                spec, n = b.skip_vec(n, prev)
            else:
                assert t in CELLS, t
                h = int(b.rng.choice([7, 8, 12])); spec = (t, n, h) + ((int(b.rng.choice([2, 3])),) if t == "rnn" else ()); n = h; b.exact = False
        specs.append(spec); prev = t
    return specs, n


def make(specs):
    """layer specifications -> nn layers"""
    out = []
    for s in specs:
        k = s[0]
        if k == "conv":
            _, ker, cin, cout, act, st, pad, d, g = s
            out.append(nn.Conv(ker, cin, cout, act, stride=st, pad=nn.SamePad() if pad == "same" else pad, dilation=d, groups=g))
        elif k in ("maxpool", "meanpool"):
            out.append((nn.MaxPool if k == "maxpool" else nn.MeanPool)(s[1]))
        elif k in ("adaptivemaxpool", "adaptivemeanpool"):
            glob = s[1] == (1, 1)
            out.append((nn.GlobalMaxPool() if glob else nn.AdaptiveMaxPool(s[1])) if k == "adaptivemaxpool" else (nn.GlobalMeanPool() if glob else nn.AdaptiveMeanPool(s[1])))
        elif k == "groupnorm":
            out.append(nn.GroupNorm(s[1], s[2], s[3]))
        elif k == "activation":
            out.append(AL.A(s[1]))
        elif k == "skip":
            out.append(nn.SkipConnection(nn.Chain(*make(s[1])), "+"))
        elif k == "dense":
            out.append(nn.Dense(s[1], s[2], s[3]))
        elif k == "layernorm":
            out.append(nn.LayerNorm(s[1], s[2]))
        elif k == "dropout":
            out.append(nn.Dropout(s[1]))
        elif k == "rnn":
            out.append(nn.RNN(s[1], s[2], s[3]))
        else:
            out.append({"lstm": nn.LSTM, "gru": nn.GRU}[k](s[1], s[2]))
    return out


def n_descs(specs, dueling):
    n = sum(1 + (len(s[1]) if s[0] == "skip" else 0) for s in specs)
    if dueling:
        run = 0
        for s in reversed(specs):
            if s[0] != "dense":
                break
            run += 1
        n += run
    return n


def _mk(specs, nA, dueling):
    def mk():
        chain = nn.Chain(*make(specs))
        return nn.create_dueling_network(chain) if dueling else chain
    return mk


def _case(name, specs, tokens, B, obs, nA, dueling, dq, prio, u8, T, gamma, pscale, alt=0):
    assert n_descs(specs, dueling) <= MAX_DESCS, (name, n_descs(specs, dueling))
    return types.SimpleNamespace(name=name, mk=_mk(specs, nA, dueling), B=B, obs=tuple(obs), nA=nA, dueling=dueling, dq=dq, prio=prio, u8=u8, mfma=1, T=T, seed=1, gamma=gamma, pscale=pscale,
                                 specs=tuple(specs), tokens=tuple(tokens), image=len(obs) == 3, alt=alt)


def pairs_of(tokens):
    return set(zip(tokens, tokens[1:]))


# ------------------------------------------------------------------ the generator
_PERM = np.random.default_rng(20240).permutation
_MM, _FL, _VV = ([ps[i] for i in _PERM(len(ps))] for ps in (MAP_PAIRS, FLAT_PAIRS, VEC_PAIRS))
N_IMG = N_FF - N_FF // 4      # three cases in four see an image


def _focus(seed, alt):
    """the adjacent pairs the seed's network must hold (so that every pair of PAIRS has a case whatever the dice say); alt: the alternative, where the shapes do not fit"""
    if seed % 4 != 3:
        j = seed // 4 * 3 + seed % 4; spare = len(_MM) - N_IMG      # the image cases, numbered 0 .. N_IMG - 1
        if alt == 0 and j < spare:
            second = _MM[N_IMG + j]
        elif alt == 0 and j - spare < len(_FL):
            second = _FL[j - spare]
        else:
            second = _VV[(j + alt) % len(_VV)]
        return True, j, [_MM[j], second]
    j = seed // 4
    return False, j, [_VV[j % len(_VV)], _VV[(N_FF // 4 + j + alt) % len(_VV)]]


def _tokens(rng, image, focus):
    toks, cur = [], "obs:map" if image else "obs:vec"
    order = sorted(focus, key=lambda p: (p[0] in VECT, p[1] in VECT))      # map pairs, then the flatten, then vector pairs
    for a, b in order:
        if (a, b) in pairs_of(toks):
            continue
        if cur in VECT and a in MAPT:
            continue      # behind the flatten no map pair can follow (the order above puts map pairs first; the coverage test would name a pair lost here)
        if cur != a:
            toks += route(cur, a) + [a]
        toks.append(b); cur = b
    for _ in range(int(rng.integers(0, 3))):      # up to two more tokens at random
        if sum(t in MAPT for t in toks) >= 5 and cur in MAPT:
            break
        opts = [t for t in NEXT[cur] if not (t in ("maxpool", "meanpool") and sum(x in ("maxpool", "meanpool") for x in toks) >= 2)]
        cur = opts[int(rng.integers(len(opts)))]; toks.append(cur)
    if cur in MAPT or rng.random() < 0.5 or toks[-1] != "dense":
        toks.append("dense")
    if rng.random() < 0.4:      # a longer trailing Dense run: what create_dueling_network splits
        toks.append("dense")
    return toks


def draw_at(seed, alt):
    """alternative `alt` of the feed-forward case of a seed, or None where its tokens do not fit its shapes: eight throws of the dice for the seed's own pairs before its
    second pair gives way to another"""
    image, j, focus = _focus(seed, alt // 8)
    rng = np.random.default_rng(9000 + 100 * seed + alt)
    mfma_draw = image and j % 6 == 5
    B = 32 if mfma_draw else (5, 16, 32)[j % 3]
    toks = _tokens(rng, image, focus)
    if image and mfma_draw and "conv" not in toks[:1]:
        toks = ["conv"] + toks
    _, need0 = _needs(toks)
    if image:
        if max(need0) > 9:
            return None
        c0 = int(rng.choice([1, 2, 4])); obs = (c0, int(rng.integers(max(6, need0[0]), 10)), int(rng.integers(max(6, need0[1]), 10)))
    else:
        obs = (int(rng.choice([6, 9, 12])),)
    b = _Builder(rng, B, seed, mfma_draw=mfma_draw, split_draw=(seed % 8 == 3))
    maxes = [i for i, t in enumerate(toks) if t in ("maxpool", "adaptivemaxpool")]
    u8 = int(j % 4 == 1 and not (maxes and "conv" not in toks[:maxes[0]]))      # (a max-type pool on the bytes themselves ties)
    try:
        specs, n = instantiate(b, toks, obs, u8)
    except Infeasible:
        return None
    nA = int(rng.choice([3, 4, 5])); specs[-1] = ("dense", specs[-1][1], nA, 0)
    dueling = bool(rng.random() < 0.5); prio = int(rng.random() < 0.5) if j % 5 else 0; dq = int(rng.random() < 0.6) if j % 7 else 0
    if n_descs(specs, dueling) > MAX_DESCS:
        return None
    # the glorot draw is multiplied by pscale so that the hidden layers see O(1) signals: three times where the observation is bytes / 255, twice where a pool stands first
    # (the mean of a window in front of the first learned layer)
    pscale = (3.0 if u8 else 1.0) * (2.0 if toks[0] in POOLS else 1.0)
    return _case(f"ff{seed:02d}", specs, toks, B, obs, nA, dueling, dq, prio, u8, 0, float(rng.choice([0.95, 0.99])), pscale, alt)


def draw_rec_at(seed, alt):
    """alternative `alt` of the recurrent case of a seed: [conv | dense] -> optional activation / pool -> cell -> optional tail -> Dense head"""
    rng = np.random.default_rng(9500 + seed + 1000 * alt)
    before = REC_BEFORE[seed % len(REC_BEFORE)]; after = REC_AFTER[(seed + seed // 6) % len(REC_AFTER)]
    image = before in ("conv", "activation:map", "maxpool", "adaptivemeanpool")
    toks = (["conv"] if image else ["dense"]) + ([before] if before not in ("conv", "dense") else [])
    cell = CELLS[seed % 3]; toks.append(cell)
    if after == "cell":
        toks.append(CELLS[(seed // 4) % 3])
    elif after != "dense":
        toks.append(after)
    toks.append("dense")
    B, T = (2, 4)[seed % 2], (2, 3)[(seed // 2) % 2]
    obs = (1, int(rng.integers(5, 8)), int(rng.integers(5, 8))) if image else (6,)
    b = _Builder(rng, B * T, 100 + seed)
    try:
        specs, n = instantiate(b, toks, obs)
    except Infeasible:
        return None
    nA = 3; specs[-1] = ("dense", specs[-1][1], nA, 0)
    dueling = bool((seed // 3) % 2)
    return _case(f"rec{seed:02d}", specs, toks, B, obs, nA, dueling, int(seed % 5 != 0), 0, 0, T, 0.95, 3.0, alt)


# THE NETWORK SCREEN.  A drawn network is kept only if a data seed of at most SEED_CAP passes seed_ok (twice every margin, live blocks, the one-ulp screen): a chain on which
# fp64 itself moves by a quarter tolerance under one ulp, or whose normalisation layers see sigma below the floor at every seed, says nothing about a kernel.  ALTS names,
# per case, the first alternative that passes -- found on the CPU with the reference alone, like SEEDS; test_composition_cpu re-runs every alternative in front of it.
SEED_CAP = 8
ALTS = {'ff00': 1, 'ff07': 3, 'ff08': 9, 'ff09': 4, 'ff22': 1, 'ff23': 2, 'ff28': 2, 'ff32': 2, 'ff33': 7, 'ff38': 4, 'ff42': 9, 'ff49': 19, 'ff53': 6, 'ff58': 2, 'ff60': 1, 'rec03': 1}


def _first(draw_one, seed, name):
    for alt in range(ALTS.get(name, 0), 32):
        c = draw_one(seed, alt)
        if c is not None:
            return c
    raise AssertionError(f"{name}: no alternative fits")


def draw(seed):
    """the feed-forward case of a seed: deterministic"""
    return _first(draw_at, seed, f"ff{seed:02d}")


def draw_rec(seed):
    """the recurrent case of a seed: deterministic"""
    return _first(draw_rec_at, seed, f"rec{seed:02d}")


# ------------------------------------------------------------------ Dropout masks: the engine's own law under the engine's layer index
def masks_for(net, k, B, T=0, seed=ENGINE_SEED):
    """{flat layer index: keep} of train step k (dropout_reference.keep_mask drawn under the layer's ENGINE index, skip_reference.program's numbering), or None without Dropout"""
    return SR.masks_for(net, k, B, T, seed) or None


def has_dropout(net):
    return any(l.kind == "dropout" for l in nn.all_layers(net))


# ------------------------------------------------------------------ one probe for all data rules: the union of the existing observers
def _see_input(probe, l, x, cx):
    AL.OBSERVERS["in"](probe, l, x, cx)      # the kinks of a standalone σ; the top-two gap of every MaxPool window
    if l.kind == "groupnorm":
        GR.OBSERVERS["in"](probe, l, x, cx)      # sigma of every group ("dead": the groups that are identically 0)
    elif l.kind == "adaptivemaxpool":      # AdaptiveMaxPool / GlobalMaxPool: the same gap on the window Flux's rule resolves
        (kh, sh), (kw, sw) = resolve(x.shape[2], l.oh), resolve(x.shape[3], l.ow)
        probe["pool"] = min(probe["pool"], GR._pool_gap(types.SimpleNamespace(kh=kh, kw=kw, sh=sh, sw=sw), S.kept(cx, x.detach()), cx.relu))


OBSERVERS = {"in": _see_input, "pre": AL.OBSERVERS["pre"], "sigma": LN.OBSERVERS["sigma"]}


def new_probe():
    return S.Probe(OBSERVERS, kink=np.inf, pool=np.inf, sigma=np.inf, dead=0)


def margins(c, net, p_on, p_tg, batch, k=0):
    """{kink, pool, sigma, gap, dead} of train step k in fp64: kinks and windows on s under the online parameters and the step's Dropout masks (where the derivatives are
    taken); sigma of every LayerNorm and GroupNorm over that pass and both s' passes; the gap over the columns of the network that picks the action"""
    s, sp = batch[0], batch[3]; mask = batch[5] if c.T else None
    pr = new_probe(); S.q_values(net, p_on, s, masks=masks_for(net, k, c.B, c.T), probe=pr, mask=mask)
    sig = new_probe(); q_on = S.q_values(net, p_on, sp, probe=sig, mask=mask); q_tg = S.q_values(net, p_tg, sp, probe=sig, mask=mask)
    qsel = q_on if c.dq else q_tg
    return dict(kink=pr["kink"], pool=pr["pool"], sigma=min(pr["sigma"], sig["sigma"]), dead=pr["dead"] + sig["dead"], gap=S._gap(np.concatenate(qsel) if c.T else qsel))


def holds(m, k=1.0):
    return m["kink"] > k * RELU_MARGIN and m["pool"] > k * RELU_MARGIN and m["sigma"] >= k * SIGMA_MIN and m["gap"] > k * GAP and m["dead"] == 0


def step(c, net, p_on, p_tg, batch, k=0, leg=None):
    return (S.rec_step if c.T else S.ff_step)(net, p_on, p_tg, batch, float(np.float32(c.gamma)), bool(c.dq), leg=leg, masks=masks_for(net, k, c.B, c.T))


def data(c, seed=None):
    return rec_data(c, seed) if c.T else ff_data(c, seed)


def trajectory(c, D=None, steps=STEPS, seed=None, leg=None):
    """yields (k, fp64 online parameters before step k, batch, step outputs); the parameters move by fp64 Adam"""
    D = D or data(c, seed)
    p = D.p_on.astype(np.float64); adam = Adam(p.size, lr=LRATE)
    for k in range(1 if c.T else steps):
        if c.T:
            idx, start = D.draws[k]; batch = R.sample_batch(D.ring, idx, start, c.T, c.obs)
        else:
            batch = ff_batch(c, D, D.idx[k])
        o = step(c, D.net, p, D.p_tg, batch, k, leg)
        yield k, p, batch, o
        p = adam.step(p, o["grads"])


def one_ulp(c, D, batch, rng):
    """parameters and observations moved by one fp32 ulp, relatively, each up or down at random"""
    e = float(np.finfo(np.float32).eps)
    mv = lambda x: np.asarray(x, np.float64) * (1.0 + e * rng.choice([-1.0, 1.0], np.shape(x)))
    b = list(batch); b[0], b[3] = mv(batch[0]), mv(batch[3])
    return mv(D.p_on), mv(D.p_tg), tuple(b)


def conditioning(c, D=None, seed=None):
    """the largest move of the first fp64 step, in tolerances (step_reference.distance), under one_ulp"""
    D = D or data(c, seed)
    _, p, batch, o = next(trajectory(c, D))
    p_on, p_tg, b2 = one_ulp(c, D, batch, np.random.default_rng(77))
    return max(distance(step(c, D.net, p_on, p_tg, b2), o, D.net).values())


VISIBLE = 10.0             # a layer is visible when (1 + VIS_STEP) on its parameters moves Q on s or the gradients by more than this many tolerances
VIS_STEP = 1e-3
VIS_CAP = VIS_STEP / (GRAD_RTOL + GRAD_C) + 0.01      # what a pure rescaling of a layer's own gradient amounts to at the very most, in tolerances (8.33)


def layer_slices(net):
    """{flat layer index: slice of the layer's parameters in the flat vector}"""
    out = {}
    for nm, sl in blocks(net):
        i = int("".join(ch for ch in nm.split(".")[0] if ch.isdigit()))
        out[i] = slice(out[i].start, sl.stop) if i in out else sl
    return out


def _moved(c, D, p, batch, o, scale):
    d = distance(step(c, D.net, p * scale, D.p_tg, batch), o, D.net)
    return max(d["td"] if c.T else d["q_on_s"], d["grads"])      # (a recurrent step reports no Q on s: td = Q(s, a) - y stands in its place)


HOMOGENEOUS = (0, 1, 4)      # identity, relu, leakyrelu: σ(a x) = a σ(x) for a > 0


def scale_invariant(net):
    """the flat indices of the parameter layers whose output reaches a LayerNorm / GroupNorm through scale-preserving layers ONLY -- decided from the structure, never from
    the data: the layer's own fused activation is homogeneous, and between it and the normalisation of the same chain stand nothing but Dropout layers, pools and
    Activation layers with a homogeneous σ.  Multiplying such a layer's parameters by a > 0 multiplies the normalisation's input by a, which it divides out again (up to
    its eps).  A join, a Dense, a Conv, a cell, the end of a block or of the base chain end the walk"""
    out, k = set(), [0]

    def walk(chain):
        ls = list(chain.layers)
        for i, l in enumerate(ls):
            if l.kind == "skip":
                walk(l.layers)
                continue
            if l.shapes() and l.kind not in CELLS and l.act in HOMOGENEOUS:
                for nxt in ls[i + 1:]:
                    if nxt.kind in ("layernorm", "groupnorm"):
                        out.add(k[0])
                    if not (nxt.kind in ("dropout",) + POOLS or (nxt.kind == "activation" and nxt.code in HOMOGENEOUS)):
                        break
            k[0] += 1
    for ch in S._chains(net):
        walk(ch)
    return out


def visibility(c, D, p, batch, o):
    """{flat layer index: how far the first step moves, in tolerances, when that layer's parameters are multiplied by 1 + VIS_STEP}.

    One exception BY THE LAW: a layer of scale_invariant(net) -- the uniform scaling leaves Q where it is and divides the layer's own gradient by 1.001, VIS_CAP tolerances
    at the very most whatever the data.  Uniform scaling is the one change a normalisation hides and no kernel error resembles: such a layer, and no other, is asked the
    same bound under the same factor on the FIRST HALF of each of its arrays"""
    out, blks, inv = {}, blocks(D.net), scale_invariant(D.net)
    for i, sl in layer_slices(D.net).items():
        scale = np.ones_like(p); scale[sl] = 1.0 + VIS_STEP
        seen = _moved(c, D, p, batch, o, scale)
        if seen <= VISIBLE and i in inv:
            scale = np.ones_like(p)
            for nm, b in blks:
                if b.start >= sl.start and b.stop <= sl.stop:
                    scale[b.start:b.start + max(1, (b.stop - b.start) // 2)] = 1.0 + VIS_STEP
            seen = _moved(c, D, p, batch, o, scale)
        out[i] = seen
    return out


def seed_ok(c, seed):
    """twice every margin on every step of the fp64 trajectory, no dead gradient block on the first step, the one-ulp screen, and every parameter layer visible"""
    D = data(c, seed); first = None
    for k, p, batch, o in trajectory(c, D):
        if not holds(margins(c, D.net, p, D.p_tg, batch, k), 2.0) or (k == 0 and S.dead_blocks(D.net, o["grads"])):
            return False
        first = first or (p, batch, o)
    return conditioning(c, D) < COND_BOUND and min(visibility(c, D, *first).values()) > VISIBLE


find_seed = lambda c, cap=SEED_CAP + 1: S.find_seed(c, seed_ok, cap)

# data seeds: the smallest seed that passes seed_ok, found on the CPU with this module alone (test_composition_cpu re-runs the search); a case not named here has seed 1
SEEDS = {'ff01': 3, 'ff04': 2, 'ff07': 5, 'ff16': 3, 'ff22': 5, 'ff23': 2, 'ff28': 5, 'ff30': 7, 'ff32': 7, 'ff39': 2, 'ff40': 2, 'ff53': 4, 'ff55': 5, 'ff59': 2, 'ff60': 7, 'rec00': 6, 'rec03': 6}


def _with_seed(c):
    c.seed = SEEDS.get(c.name, 1)
    return c


FF = [_with_seed(draw(s)) for s in range(N_FF)]
REC = [_with_seed(draw_rec(s)) for s in range(N_REC)]
BY_NAME = {c.name: c for c in FF + REC}

_PREPARED = {}


def prepare(c):
    """the case's data, computed once and shared; asserts the margins on the first step (the GPU test asserts them on every step, on the engine's own parameters)"""
    if c.name not in _PREPARED:
        D = data(c)
        _, p, batch, _ = next(trajectory(c, D))
        m = margins(c, D.net, p, D.p_tg, batch)
        assert holds(m), (c.name, m)
        _PREPARED[c.name] = D
    return _PREPARED[c.name]


def base_kinds(net):
    """the kinds in the base chain of a dueling network (a block's inner layers included)"""
    out = set()

    def visit(chain):
        for l in chain.layers:
            out.add(l.kind)
            if l.kind == "skip":
                visit(l.layers)
    visit(net.base)
    return out
