"""GPU: the launch program is the same program.  Per network of kind_traits_cases.GPU_CASES: the launch names of one train step and of a middle step in order, the acting
program's fused_tail, and the dqn_comm_init / DQN_SIM_WORLD refusal texts, equal to what the library gave before the per-kind clauses of csrc/ were folded into the layer-kind
traits table (tests/golden/kind_traits_gpu.json, recorded on that commit, two recordings agreeing).  One engine and one or two steps per case: the file runs in seconds."""
import json
import os

import pytest

import kind_traits_cases as K

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kind_traits_gpu.json")))


def test_the_fixture_holds_the_paths_it_was_recorded_for():
    assert set(GOLD) == set(K.GPU_CASES)
    step = lambda k: GOLD[k]["step"]
    assert step("tiny") == ["tiny_step"] and "tiny_step" not in step("tiny_off") and step("lstm") == ["drqn_cols", "adam"]
    assert "red_head" in step("red_head") and "red_head" in step("red_head_dueling") and "head_cols4" in step("head_cols4") and "head_cols4" in step("cpad_head_cols4")
    for sfx in ("_ln", "_do", "_skip"):      # each of the three declines every fusion
        assert "head_td" in step("red_head" + sfx) and "head_td" in step("head_cols4" + sfx) and "head_td" in step("tiny" + sfx) and "td_huber_drqn" in step("lstm" + sfx), sfx
    for k in ("carriers", "carriers_own_level", "carriers_ln_skip"):      # the priority block is split over two carrying launches
        assert sum(n.endswith("+prio") for n in step(k)) == 2, k
    assert "bwd_join_skip2" in step("skip_join") and "bwd_join_skip2" not in step("skip_alias")
    assert {k[4:]: GOLD[k]["fused_tail"] for k in GOLD if k.startswith("act_")} == dict(dense=True, conv=True, pool=True, cpad=False, ln=False, do=False, skip=False)
    for k, layer in (("ln1_pool3", 3), ("ln1_cpad2_pool3", 2), ("pool0_cpad1", 1), ("do1_ln3", 3), ("skip2_do3", 3), ("pool1_ln3", 1)):      # the kind of highest priority is named, not the first own-level layer
        assert GOLD["refuse_" + k]["comm_init"].startswith(f"dqn_comm_init: layer {layer} is") and GOLD["refuse_" + k]["sim_world"].startswith(f"DQN_SIM_WORLD: layer {layer} is"), k


@pytest.mark.parametrize("name", sorted(K.GPU_CASES))
def test_the_program_is_the_same_program(name):
    assert K.observe_gpu(name) == GOLD[name]
