"""CPU: build_layers' refusals byte for byte and default_plan's entries number for number, against what the library decided before the per-kind clauses of csrc/ were folded
into the layer-kind traits table (tests/golden/kind_traits_cpu.json, recorded on that commit; kind_traits_cases.py has the networks).  dqn_plan_default runs both on the host."""
import json
import os

import pytest

import kind_traits_cases as K

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kind_traits_cpu.json")))


def test_the_fixture_and_the_case_table_name_the_same_cases():
    assert set(GOLD) == set(K.CPU_CASES)
    for k in ("out_pool", "out_ln", "out_do", "out_skip"):
        assert all("cannot be the network's output layer" in GOLD[k][b]["error"] for b in ("B8", "B128")), k
    refused = [k for k in GOLD if "error" in GOLD[k]["B8"]]
    for word in ("Pool", "Conv pad", "Conv with pad", "LayerNorm", "Dropout", "skip block"):      # every own-level kind's block is represented, each at least twice
        assert sum(word in GOLD[k]["B8"]["error"] for k in refused) >= (1 if word.startswith("Conv") else 2), word
    assert sum(k.startswith("plan_") for k in GOLD) >= 8 and all("plan" in GOLD[k]["B8"] and "plan" in GOLD[k]["B128"] for k in GOLD if k.startswith("plan_"))


@pytest.mark.parametrize("name", sorted(K.CPU_CASES))
def test_refusal_text_and_default_plan_are_what_they_were(name):
    assert K.observe_cpu(name) == GOLD[name]
