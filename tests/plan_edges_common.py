"""The plan table (TEST INFRASTRUCTURE): feed-forward train steps under CALLER-SUPPLIED summation plans, on the harness of tests/feedforward_edges_common.py.

The summation plan -- one (fwd_kc, dx_kc, dw_kc) triple per layer -- is a public input (dqn_engine_create, Engine(layers, hp, plan=...), every checkpoint).  It
defines what "bit-exact" means and it decides which kernel runs: every selection predicate reads the chunk count and the chunk length of a
plan entry.  The edge table of feedforward_edges_common evaluates those predicates on the default plan only; here a case is one of its cases plus an `edit`, the
map from the default plan to the plan under test, and `want` states the side of each rule the case was written for on the EDITED plan (facts()).  A case on
the wrong side fails; none is skipped.  tests/test_plan_edges_cpu.py runs the table on the C twin, tests/test_plan_edges_gpu.py on the HIP engine.

Per case: `same` -- the edit cannot change the summation order (a chunk length >= the contraction: unsplit, the bits of 0), so the twin's record must EQUAL the
default plan's; otherwise it must differ from it in at least one bit (an edit that changes no bit tests nothing).  `fwd` -- a forward case: the acting programs
read fwd_kc too, so the GPU file also runs forward() and greedy_action under the plan."""
import feedforward_edges_common as C
import ref
from feedforward_edges_common import _cv, case, mlp


def edit(**by_layer):
    """edit(l1=dict(fwd=64), l3=dict(dw=32)): the default plan with the named fields of the named layers (ABI order: base, val, adv) replaced"""
    ch = {int(k[1:]): v for k, v in by_layer.items()}

    def apply(plan):
        out = [tuple(p) for p in plan]
        for i, d in ch.items():
            assert 0 <= i < len(out) and set(d) <= {"fwd", "dx", "dw"}, (i, d, len(out))
            f, x, w = out[i]
            out[i] = (d.get("fwd", f), d.get("dx", x), d.get("dw", w))
        return out
    return apply


def whole(plan_):
    """the plan itself, whatever the default is"""
    return lambda plan: [tuple(p) for p in plan_]


def pcase(c, ed, same=False, fwd=False):
    c.name = "plan_" + c.name
    c.edit, c.same, c.fwd = ed, same, fwd
    return c


# the networks of the table (the smallest that reach the path; prio = 0 keeps a small MLP off the single-launch step)
def _f96(name, kc, want, **kw):          # Dense(96, 32) as the first layer, B = 32: the forward fwd_kc family
    return pcase(case(f"fwd_k96_kc{name}", 96, mlp(96, 32, 32, 4), 32, prio=0, want=want, **kw), edit(l0=dict(fwd=kc)), fwd=True, same=kc >= 96)


CONV = ((4, 12, 12), (4, 4, 32, 2), (3, 32, 32, 1), 32, 4)                 # conv0: K = 4 * 4 * 4 = 64, 5 x 5 positions; conv1: K = 32 * 3 * 3 = 288, 3 x 3 positions (the arena_on network)
CONV_DX33 = ((2, 14, 16), (3, 2, 16, 1), (3, 16, 32, 1), 32, 4)           # conv1: 3 x 3 / stride 1, cin = 16 (dx_cin16's network)
CONV_DX44 = ((2, 14, 16), (3, 2, 16, 1), (4, 16, 32, 2), 32, 4)           # conv1: 4 x 4 / stride 2
CONV_DW = ((4, 12, 14), (3, 4, 16, 1), (3, 16, 32, 1), 32, 4)              # conv1: 8 x 10 = 80 positions (conv_dw_b32's network)


def _dxd(name, N, kc, B, want, **kw):    # Dense(64, N) as layer 1: the dense dx_kc family
    return pcase(case(f"dx_n{N}_kc{name}", 64, mlp(64, 64, N, 4), B, prio=0, want=want, **kw), edit(l1=dict(dx=kc)))


def _dwd(name, B, kc, want, **kw):       # Dense(64, 32) first, B-long dW chains cut by dw_kc
    return pcase(case(f"dw_b{B}_kc{name}", 64, mlp(64, 32, 32, 4), B, prio=0, want=want, **kw), edit(l0=dict(dw=kc)))


FORWARD = [
    # ---- Dense(96, 32) first layer, B = 32
    _f96("64", 64, {"fwd0": "lds", "fwdS0": 2}),                                  # ragged: 64 + 32, LDS-tiled (kc % 32 == 0)
    _f96("32", 32, {"fwd0": "lds", "fwdS0": 3}, graph=0),                         # three exact chunks
    _f96("48", 48, {"fwd0": "mfma", "fwdS0": 2}),                                 # kc % 32, % 4 == 0: the direct MFMA forward
    _f96("7", 7, {"fwd0": "valu", "fwdS0": 14}, dup=True),                        # odd kc: VALU, 14 slabs, the last of 5
    _f96("95", 95, {"fwd0": "valu", "fwdS0": 2}),                                 # 95 + 1
    _f96("1", 1, {"fwd0": "valu", "fwdS0": 96}, graph=0),                         # kc = 1: S = K slabs
    _f96("96", 96, {"fwd0": "lds", "fwdS0": 1}),                                  # kc == K and kc > K: unsplit, the bits of fwd_kc = 0
    _f96("97", 97, {"fwd0": "lds", "fwdS0": 1}),
    # ---- conv first layer, K = 64
    pcase(_cv("fwd_conv0_kc32", *CONV, 32, want={"fwd0": "lds", "fwdS0": 2}), edit(l0=dict(fwd=32)), fwd=True),
    pcase(_cv("fwd_conv0_kc16", *CONV, 32, want={"fwd0": "mfma", "fwdS0": 4}), edit(l0=dict(fwd=16)), fwd=True),
    pcase(_cv("fwd_conv0_kc12", *CONV, 32, graph=0, want={"fwd0": "mfma", "fwdS0": 6}), edit(l0=dict(fwd=12)), fwd=True),      # 5 x 12 + 4
    # ---- conv second layer, K = 288
    pcase(_cv("fwd_conv1_kc96", *CONV, 32, want={"fwd1": "lds", "fwdS1": 3}), edit(l1=dict(fwd=96)), fwd=True),
    pcase(_cv("fwd_conv1_kc128", *CONV, 32, dup=True, want={"fwd1": "lds", "fwdS1": 3}), edit(l1=dict(fwd=128)), fwd=True),     # 128 + 128 + 32
    # ---- the byte arena of a u8 replay with a split first-layer forward
    pcase(_cv("fwd_arena_kc32", *CONV, 32, u8=1, want={"arena": True, "fwd0": "lds", "fwdS0": 2}), edit(l0=dict(fwd=32)), fwd=True),
    # ---- B = 128: a split forward is never the weights-resident form (fwd_wres_ok needs one chunk): the ordinary LDS-tiled launch, slabs and a reduce
    pcase(_cv("fwd_conv1_kc96_b128", *CONV, 128, want={"fwd1": "lds", "fwdS1": 3}), edit(l1=dict(fwd=96)), fwd=True),
]

HEADS = [
    # head K = 128 with two chunks of 64: no longer the 32-row rule, so head_td instead of head_cols4
    pcase(case("head_k128_kc64", 64, mlp(64, 128, 4), 32, prio=0, want={"fwdS1": 2, "head": "head_td"}), edit(l1=dict(fwd=64)), fwd=True),
    # head K = 160: 64 + 64 + 32 (the default, five chunks of 32, is DEFAULT_PLAN's head_k160)
    pcase(case("head_k160_kc64", 64, mlp(64, 160, 4), 32, prio=0, graph=0, want={"fwdS1": 3, "head": "head_td"}), edit(l1=dict(fwd=64)), fwd=True),
    pcase(case("head_k160_kc7", 64, mlp(64, 160, 4), 32, prio=0, want={"fwdS1": 23, "head": "head_td"}), edit(l1=dict(fwd=7)), fwd=True),          # 22 x 7 + 6
    # a dueling pair whose producers are split into exactly 16 and into 17 slabs: the fused reduce + head launch and its fallback (red_head_ok: S <= 16)
    pcase(case("heads_s16", 512, mlp(512, 128, 4), 32, dueling=True, want={"fwdS0": 16, "fwdS2": 16, "fwd0": "lds", "head": "red_head"}),
          edit(l0=dict(fwd=32), l2=dict(fwd=32)), fwd=True),
    pcase(case("heads_s17", 544, mlp(544, 128, 4), 32, dueling=True, want={"fwdS0": 17, "fwdS2": 17, "fwd0": "lds", "head": "head_td"}),
          edit(l0=dict(fwd=32), l2=dict(fwd=32)), fwd=True),
]

TINY = [
    # the single-launch step with chunked forwards and chunked dW on both layers: odd chunks (the scalar dW loop) and chunks of four (its 16-byte form)
    pcase(case("tiny_chunks_odd", 12, mlp(12, 24, 4), 8, want={"tiny": True}), whole([(8, 0, 3), (16, 0, 5)]), fwd=True),
    pcase(case("tiny_chunks_4", 12, mlp(12, 24, 4), 8, graph=0, want={"tiny": True}), whole([(4, 0, 4), (8, 0, 4)]), fwd=True),
    # a dx_kc that splits leaves the single launch
    pcase(case("tiny_dx_split", 12, mlp(12, 24, 4), 8, want={"tiny": False}), whole([(8, 0, 3), (16, 2, 5)])),
]

DENSE_DX = [
    _dxd("64", 96, 64, 32, {"dxmode1": 3, "dx1": "lds", "dxred1": False}),                     # ragged 64 + 32: two units of one launch
    _dxd("32", 96, 32, 32, {"dxmode1": 3, "dx1": "lds", "dxred1": False}, graph=0),            # three units
    _dxd("32", 160, 32, 32, {"dxmode1": -1, "dx1": "mfma", "dxred1": True}),                   # five chunks > U_MAX: off the units path, slabs and a reduce launch
    _dxd("48", 96, 48, 32, {"dxmode1": -1, "dx1": "mfma", "dxred1": True}, dup=True),          # kc % 32
    _dxd("48", 160, 48, 32, {"dxmode1": -1, "dx1": "mfma", "dxred1": True}, graph=0),          # ... ragged: 3 x 48 + 16
    _dxd("6", 96, 6, 32, {"dxmode1": -1, "dx1": "valu", "dxred1": True}),                      # kc % 4: VALU, 16 slabs
    _dxd("10", 96, 10, 32, {"dxmode1": -1, "dx1": "valu", "dxred1": True}),                    # ... ragged: 9 x 10 + 6
    _dxd("32_b128", 96, 32, 128, {"dxmode1": 2, "dx1": "lds", "dxred1": True}),                # B = 128: slabs plus reduce
    # a dueling join whose streams carry different dx_kc: no shared launch, the value stream adds to the advantage stream's
    pcase(_cv("dx_join_differs", (2, 14, 16), (3, 2, 16, 1), (3, 16, 32, 2), 128, 4, 32, dueling=True,
              want={"join4": "tmp", "dxkc2": 32, "dxkc4": 64, "dx4": "lds", "dx2": "mfma", "dxred2": True}), edit(l2=dict(dx=32))),
]

CONV_DX = [pcase(_cv(f"dx_conv33_tc{tc}", *CONV_DX33, 32, graph=int(tc != 2), want=w), edit(l1=dict(dx=tc))) for tc, w in (
    (1, {"dxmode1": -1, "dx1": "mfma"}),                                                       # nine chunks: conv_max_chunks > U_MAX
    (2, {"dxmode1": -1, "dx1": "mfma"}),                                                       # five
    (4, {"dxmode1": 3, "dx1": "lds"}),                                                         # three: 4 + 4 + 1
    (8, {"dxmode1": 3, "dx1": "lds"}))]                                                        # two: 8 + 1
CONV_DX += [pcase(_cv(f"dx_conv44s2_tc{tc}", *CONV_DX44, 32, dup=tc == 3, want={"dxmode1": 3, "dx1": "lds"}), edit(l1=dict(dx=tc))) for tc in (2, 3, 5)]

DENSE_DW = [
    _dwd("32", 96, 32, {"dw0": "lds", "dwS0": 3, "dwsum": "adam"}),
    _dwd("64", 96, 64, {"dw0": "lds", "dwS0": 2, "dwsum": "adam"}, graph=0),                   # ragged 64 + 32
    _dwd("40", 96, 40, {"dw0": "valu", "dwS0": 3, "dwsum": "adam"}),                           # kc % 32, and no multiple of B: VALU (40 + 40 + 16)
    _dwd("12", 36, 12, {"dw0": "valu", "dwS0": 3, "dwsum": "adam"}, dup=True),
    # a split dW on a block that is no whole number of 16-byte sets, (16 + 1) * 6 = 102 floats: the slab sum is a launch of its own
    pcase(case("dw_odd_block", 16, mlp(16, 6, 32, 4), 32, prio=0, want={"dw0": "valu", "dwS0": 2, "dwsum": "launch"}), edit(l0=dict(dw=16))),
    # a head layer's B-long chains cut at B = 128 (tail tasks of the backward launch)
    pcase(case("dw_head_b128", 64, mlp(64, 32, 4), 128, prio=0, want={"dw1": "head", "dwS1": 2, "dwsum": "adam"}), edit(l1=dict(dw=64))),
]

CONV_DW_CASES = [
    # B = 32 (LDS-tiled dW): whole positions -- one, two, all but one (ragged: 79 + 1)
    pcase(_cv("dw_conv_b32_1pos", *CONV_DW, 32, want={"dw1": "lds", "dwS1": 80}), edit(l1=dict(dw=32))),
    pcase(_cv("dw_conv_b32_2pos", *CONV_DW, 32, graph=0, want={"dw1": "lds", "dwS1": 40}), edit(l1=dict(dw=64))),
    pcase(_cv("dw_conv_b32_79pos", *CONV_DW, 32, want={"dw1": "lds", "dwS1": 2}), edit(l1=dict(dw=79 * 32))),
    # 32-sample granularity: chunks of 96 samples begin inside a position at B = 128 (106 x 96 + 64: ragged)
    pcase(_cv("dw_conv_b128_96", *CONV_DW, 128, want={"dw1": "lds", "dwS1": 107}), edit(l1=dict(dw=96))),
    # B = 48 (direct MFMA dW): multiples of B only -- two positions and three (ragged: 26 x 3 + 2); the default there is one position per chunk
    pcase(_cv("dw_conv_b48_2pos", *CONV_DW, 48, want={"dw1": "mfma", "dwS1": 40}), edit(l1=dict(dw=96))),
    pcase(_cv("dw_conv_b48_3pos", *CONV_DW, 48, dup=True, want={"dw1": "mfma", "dwS1": 27}), edit(l1=dict(dw=144))),
]

# default-plan cases the edge table does not stand on: no edit, so no "differs from the default" check
DEFAULT_PLAN = [
    # the one ragged LDS-tiled split the default plan produces at these sizes: K = 4288 -> fwd_kc = 480, nine chunks, the last one 448 long
    pcase(case("default_k4288", 4288, mlp(4288, 32, 32, 4), 32, want={"fwd0": "lds", "fwdS0": 9}), None, same=True, fwd=True),
    # the head rule at a K that is no power of two: five chunks of 32
    pcase(case("default_head_k160", 64, mlp(64, 160, 4), 32, prio=0, want={"fwdS1": 5, "head": "head_cols4"}), None, same=True, fwd=True),
]

CASES = FORWARD + HEADS + TINY + DENSE_DX + CONV_DX + DENSE_DW + CONV_DW_CASES + DEFAULT_PLAN
assert len({c.name for c in CASES}) == len(CASES)


def plan_of(c):
    """the `plan=` argument of make_handle / run_checked / replay_steps for the case"""
    return lambda layers, hp: C.case_plan(c, layers, hp)


DEFAULT = ref.default_plan
