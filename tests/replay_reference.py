"""fp64 model of the prioritized replay and the law its sampler is held to (TEST INFRASTRUCTURE).  Shares no line with the C twin (oracle/dqn_ref.c)
or the engine: there is no tree here.  Used by tests/replay_edges_common.py.

Leaves (src/prioritized_experience_replay.jl:65-80).  A plain array of `cap` float64.  add() writes (td + eps)^alpha at (widx + i) % cap, later rows
winning; update() writes (|td| + eps)^alpha, the last occurrence of an index winning (:79); import_() sets slots 0 .. n-1 and zeroes every other slot.
An engine's float32 leaf may differ from the model's by LEAF_RTOL(alpha) = (alpha + 1) * 2^-24: one rounding of the float32 sum td + eps, which the power
(alpha <= 1) passes on scaled by alpha, and one rounding of the result; the power itself is evaluated in float64 on both sides.

Philox4x32-10 (philox4x32_10): written from the published round function (Salmon et al., SC'11), vectorised in uint64; pinned word for word to
tests/golden/philox4x32_10.json, a table printed by ATen's at::Philox4_32 (oracle/philox_fixture.cpp), by tests/test_replay_edges_cpu.py.

The stratified law.  Call `ctr`, position i of B:
    u = (word0 >> 8) * 2^-24,  word0 of Philox(key = seed, counter = {ctr lo, ctr hi, i, 0x5A4D504C})
    t = (i + u) * S / B,       S = the fp64 sum of the first `size` leaves AS THE ENGINE REPORTS THEM (leaf errors are judged separately, above)
    leaf j is acceptable iff cum[j] - d <= t < cum[j+1] + d   (cum: fp64 running sum of those leaves), and the engine's documented clamp j <= size - 1
    (tree_descend, common.h: a descent that round-off carries past the last live leaf returns size - 1) is applied to both ends of the acceptable range.
The slack d = (2 L + 4) * 2^-24 * S, L = log2(cap2), cap2 = the capacity rounded up to a power of two, is derived, not measured:
  * every stored node is a pairwise float32 sum of positive values over at most L levels: relative error at most L * 2^-24 (each level adds one rounding of
    relative size 2^-24 to a sum of positives, and errors of positives do not amplify), so every left sum the descent compares against or subtracts is off
    by at most L * 2^-24 * S in all -- the first L terms;
  * the descent subtracts at most L left sums from t, one float32 rounding each, each of at most 2^-24 * S -- the second L terms;
  * forming seg = root / B and t = (i + u) * seg costs at most 4 more roundings (the root as read, the division, the sum i + u, the product), each at most
    2^-24 * S.
A draw outside d is a finding; d is never widened.  Nothing is skipped: a target within d of a boundary has two (or more) acceptable leaves, and
sharp() reports how often -- every case must keep that under 1 % of its positions, from the reference alone.

hp.sample_distinct = 1 (…replay.jl:85, replace = false; DESIGN.md section 5, common.h::sample_distinct_fix).  Positions are visited in ascending order; a position whose
stratified leaf an earlier position already holds is redrawn on the residual priorities.  judge_distinct: the B indices are distinct; position i either holds an
acceptable stratified leaf, or -- its acceptable leaves all taken -- is judged against attempt 0 of the documented redraw: Philox lane B + i, word 3 + 1, t = u * R on
the cumulative sum of the leaves no earlier position holds, R its total, with slack d + nt * 2^-24 * S (nt = i earlier positions, one float32 subtraction of a
taken priority each, along R and along the path).  Only where R >= S / 4 (below that the float32 residual sums cancel too much for a slack stated in units of S;
such positions are counted apart, as `small_R`), and a redrawn position is left out only when its widened interval touches a taken leaf -- the case the engine's retries (attempts 1 .. 7) exist for, whose draws depend on
which side of a float32 comparison attempt 0 fell.  Every case keeps the left-out share under 5 % of its redrawn positions and states a minimum of judged
redraws; model_distinct() plays a call on the reference alone, so both are asserted before any engine exists.
"""
import json
import os

import numpy as np

TAG = 0x5A4D504C
U24 = 2.0 ** -24
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(key, counter):
    """key: (k0, k1); counter: array (..., 4) of 32-bit words -> array (..., 4) uint32.  Ten rounds: ctr' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1,
    lo(M0 c0)), the key bumped by the Weyl constants after each of the first nine."""
    c = np.asarray(counter, np.uint64) & _M32
    c0, c1, c2, c3 = (c[..., j].copy() for j in range(4))
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox_fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "philox4x32_10.json")) as f:
        return json.load(f)


def uniforms(seed, ctr, lanes, word3=TAG):
    """u of the given lanes of call `ctr`: (word0 >> 8) * 2^-24, exact in float64"""
    lanes = np.atleast_1d(np.asarray(lanes, np.uint64))
    c = np.empty((lanes.size, 4), np.uint64)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = int(ctr) & 0xFFFFFFFF, (int(ctr) >> 32) & 0xFFFFFFFF, lanes, word3 & 0xFFFFFFFF
    w0 = philox4x32_10((int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF), c)[:, 0]
    return (w0 >> np.uint32(8)).astype(np.float64) * U24


def LEAF_RTOL(alpha):
    return (float(alpha) + 1.0) * U24 * (1.0 + 1e-6)


class Replay:
    """the leaves, the ring cursor and the draw counter"""

    def __init__(self, cap, alpha, eps):
        self.cap, self.alpha, self.eps = int(cap), float(alpha), float(eps)
        self.leaves = np.zeros(self.cap, np.float64)
        self.size = self.widx = self.ctr = 0

    def priority(self, td):
        return (np.asarray(td, np.float64) + self.eps) ** self.alpha

    def add(self, td):
        p = self.priority(td)
        for i in range(max(0, p.size - self.cap), p.size):           # rows before the last `cap` are overwritten by later rows of the same call
            self.leaves[(self.widx + i) % self.cap] = p[i]
        self.widx = (self.widx + p.size) % self.cap
        self.size = min(self.cap, self.size + p.size)

    def update(self, idx, td):
        p = self.priority(np.abs(np.asarray(td, np.float64)))
        for j, v in zip(np.asarray(idx).tolist(), p.tolist()):       # in order: the last occurrence wins
            assert 0 <= j < self.size
            self.leaves[j] = v

    def import_(self, prio):
        prio = np.asarray(prio, np.float64)
        self.leaves[:] = 0.0
        self.leaves[:prio.size] = prio
        self.size, self.widx = prio.size, prio.size % self.cap

    def live(self):
        return self.leaves[:self.size].copy()


def depth(cap):
    L = 0
    while (1 << L) < cap:
        L += 1
    return L


def slack(S, cap):
    return (2 * depth(cap) + 4) * U24 * S


def _ranges(cum, t, d):
    """per target: the first and the last acceptable leaf, cum[j] - d <= t < cum[j+1] + d, clamped to the live leaves"""
    n = cum.size - 1
    lo = np.searchsorted(cum[1:], t - d, side="right")               # first j with cum[j+1] > t - d
    hi = np.searchsorted(cum[:n], t + d, side="right") - 1           # last j with cum[j] <= t + d
    return np.clip(lo, 0, n - 1), np.clip(hi, 0, n - 1)


def _margin(cum, t, idx, d):
    """distance of t from [cum[j], cum[j+1]) of the drawn leaf, in units of d (0 inside; <= 1 accepted)"""
    idx = np.asarray(idx)
    return np.maximum(np.maximum(cum[idx] - t, t - cum[idx + 1]), 0.0) / d


def strata(leaves, seed, ctr, B, cap):
    """(cum, t, d, lo, hi) of call `ctr` on the given live leaves"""
    leaves = np.asarray(leaves, np.float64)
    cum = np.concatenate([[0.0], np.cumsum(leaves)])
    S = cum[-1]
    t = (np.arange(B) + uniforms(seed, ctr, np.arange(B))) * S / B
    d = slack(S, cap)
    lo, hi = _ranges(cum, t, d)
    return cum, t, d, lo, hi


def sharp(leaves, seed, ctr, B, cap):
    """positions of call `ctr` with more than one acceptable leaf (from the reference alone)"""
    _, _, _, lo, hi = strata(leaves, seed, ctr, B, cap)
    return int((hi > lo).sum())


def judge(leaves, idx, seed, ctr, B, cap, what=""):
    """the stratified law on one call's indices.  Returns (worst margin as a fraction of d, ambiguous positions)"""
    idx = np.asarray(idx, np.int64)
    assert idx.shape == (B,) and idx.min() >= 0 and idx.max() < len(leaves), (what, idx)
    cum, t, d, lo, hi = strata(leaves, seed, ctr, B, cap)
    bad = np.nonzero((idx < lo) | (idx > hi))[0]
    assert bad.size == 0, (f"{what}: call {ctr}: position {bad[0]} drew leaf {idx[bad[0]]}, the law allows {lo[bad[0]]}..{hi[bad[0]]} "
                           f"(t = {t[bad[0]]!r}, off by {_margin(cum, t, idx, d)[bad[0]]:.3g} d; {bad.size} of {B} positions outside)")
    return float(_margin(cum, t, idx, d).max()), int((hi > lo).sum())


def judge_distinct(leaves, idx, seed, ctr, B, cap, what=""):
    """hp.sample_distinct = 1.  Returns (worst margin / its slack, ambiguous stratified positions, redrawn positions with R >= S / 4, those of them left out, redrawn
    positions with R < S / 4)"""
    leaves = np.asarray(leaves, np.float64)
    idx = np.asarray(idx, np.int64)
    n = leaves.size
    assert idx.shape == (B,) and idx.min() >= 0 and idx.max() < n, (what, idx)
    assert n < B or len(set(idx.tolist())) == B, f"{what}: call {ctr}: indices not distinct: {idx}"
    cum, t, d, lo, hi = strata(leaves, seed, ctr, B, cap)
    S = cum[-1]
    worst, redrawn, left_out, small_R = 0.0, 0, 0, 0
    for i in range(B):
        j = int(idx[i])
        taken = idx[:i]
        cand = np.arange(lo[i], hi[i] + 1)
        free = cand[~np.isin(cand, taken)]
        if j in free:                                                # its stratified leaf (or one of the acceptable ones), not held by an earlier position
            worst = max(worst, float(_margin(cum, t[i:i + 1], idx[i:i + 1], d)[0]))
            continue
        assert free.size == 0 or hi[i] > lo[i], f"{what}: call {ctr}: position {i} holds {j}; its stratified leaf {cand} is free"
        # its acceptable stratified leaves are all taken -- or (ambiguous range, partly taken) the engine's own stratified leaf was a taken one: either way
        # the position was redrawn, and the leaf it holds is judged against attempt 0 like any other redraw
        res = leaves.copy(); res[taken] = 0.0
        rc = np.concatenate([[0.0], np.cumsum(res)])
        R = rc[-1]
        if R < S / 4:
            small_R += 1
            continue
        redrawn += 1
        tr = uniforms(seed, ctr, [B + i], TAG + 1)[0] * R
        dr = d + i * U24 * S
        if (np.abs(rc[taken] - tr) <= dr).any():                     # attempt 0 may have landed on a taken leaf: the engine's retry decides, not this law
            left_out += 1
            continue
        rlo, rhi = _ranges(rc, np.array([tr]), dr)
        assert rlo[0] <= j <= rhi[0], (f"{what}: call {ctr}: redrawn position {i} holds {j}, attempt 0 of the redraw allows {rlo[0]}..{rhi[0]} "
                                       f"(t = {tr!r} of R = {R!r})")
        worst = max(worst, float(max(rc[j] - tr, tr - rc[j + 1], 0.0) / dr))
    return worst, int((hi > lo).sum()), redrawn, left_out, small_R


def model_distinct(leaves, seed, ctr, B, cap):
    """one call of hp.sample_distinct = 1 played on the reference alone (no engine, no drawn index): the stratified leaf of every position is the fp64 leaf
    that holds its target; a position whose leaf an earlier one holds is redrawn by attempt 0 on the residual.  Returns (indices, redrawn positions with
    R >= S / 4, those of them judge_distinct would leave out -- the widened attempt-0 interval touches a taken leaf --, redrawn positions with R < S / 4).
    Where attempt 0 cannot be followed (left out, or R < S / 4) the play continues with the heaviest untaken leaf: the counts are what matters here."""
    leaves = np.asarray(leaves, np.float64)
    n = leaves.size
    cum, t, d, lo, hi = strata(leaves, seed, ctr, B, cap)
    S = cum[-1]
    strat = np.clip(np.searchsorted(cum[1:], t, side="right"), 0, n - 1)
    idx, redrawn, left_out, small_R = [], 0, 0, 0
    for i in range(B):
        j = int(strat[i])
        if j in idx and n >= B:
            taken = np.array(idx, np.int64)
            res = leaves.copy(); res[taken] = 0.0
            rc = np.concatenate([[0.0], np.cumsum(res)])
            R = rc[-1]
            tr = uniforms(seed, ctr, [B + i], TAG + 1)[0] * R
            dr = d + i * U24 * S
            j = int(np.argmax(res))
            if R < S / 4:
                small_R += 1
            else:
                redrawn += 1
                if (np.abs(rc[taken] - tr) <= dr).any():
                    left_out += 1
                else:
                    j = int(np.clip(np.searchsorted(rc[1:], tr, side="right"), 0, n - 1))
        idx.append(j)
    return np.array(idx, np.int64), redrawn, left_out, small_R


def is_weights(leaves, idx, beta):
    """(size * p_j / S)^-beta in fp64 (…replay.jl:101-102)"""
    leaves = np.asarray(leaves, np.float64)
    return (leaves.size * leaves[np.asarray(idx)] / leaves.sum()) ** (-float(beta))


def huber_mean(x):
    a = np.abs(np.asarray(x, np.float64))
    q = np.minimum(a, 1.0)
    return float(np.mean(0.5 * q * q + (a - q)))


def stratum_probabilities(leaves, B):
    """q[i, j]: the probability that stratum i of B lands on leaf j -- the overlap of [cum[j], cum[j+1]) with [i, i+1) * S / B, over S / B"""
    leaves = np.asarray(leaves, np.float64)
    cum = np.concatenate([[0.0], np.cumsum(leaves)])
    seg = cum[-1] / B
    a = np.arange(B)[:, None] * seg
    ov = np.minimum(cum[None, 1:], a + seg) - np.maximum(cum[None, :-1], a)
    return np.maximum(ov, 0.0) / seg
