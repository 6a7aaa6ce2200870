"""CPU: every refusal of build_layers byte for byte, the geometry of accepted networks read back through refusal text, and their default plans number for number, against
what the library answered before build_layers was cut into one function per layer family (tests/golden/build_layers_cpu.json, recorded on that commit;
build_layers_cases.py has the descriptor lists, docs/history/build_layers.md the commit and the command).  dqn_plan_default runs build_layers on the host."""
import json
import os

import pytest

import build_layers_cases as C

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_layers_cpu.json")))


def test_the_fixture_and_the_case_table_name_the_same_cases():
    assert set(GOLD) == set(C.REFUSED) | set(C.ACCEPTED) and not set(C.REFUSED) & set(C.ACCEPTED)
    assert all("error" in GOLD[k] for k in C.REFUSED)
    assert all("plan" in GOLD[k]["B8"] and "plan" in GOLD[k]["B128"] and len(GOLD[k]["probes"]) == len(C.ACCEPTED[k][0]) for k in C.ACCEPTED)
    assert all(all(row.values()) for k in C.ACCEPTED for row in GOLD[k]["probes"])      # every probe was refused: its text is the read-back


def test_every_refusal_site_has_a_case_and_an_answer_of_its_own():
    """every site is reachable (build_layers_cases.py): one case at least per site, and at least as many distinct refusal texts as sites once the layer index is cut off"""
    assert {C.site_of(k) for k in C.REFUSED} == set(range(1, C.SITES + 1))
    by_site = {}
    for k in C.REFUSED:
        by_site.setdefault(C.site_of(k), set()).add(GOLD[k]["error"])
    assert len({min(v) for v in by_site.values()}) >= C.SITES      # a site's first text differs from every other site's: no two sites were answered by one rule
    assert len({GOLD[k]["error"] for k in C.REFUSED}) >= C.SITES


@pytest.mark.parametrize("name", sorted(C.REFUSED) + sorted(C.ACCEPTED))
def test_build_layers_answers_what_it_answered(name):
    assert C.observe(name) == GOLD[name]
