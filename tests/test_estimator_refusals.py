"""CPU: every refusal of the per-frame estimators' planners, of the TII bank's window check and of the NULL-window host forms' window
checks, by status and by its whole text: tests/golden/estimator_refusals.json holds what the library answered before the planners were
rewritten over dab-radio_amd/csrc/plan_prelude.h (tests/golden/make_golden_estimator_refusals.py wrote it and holds the table of cases,
among them calls with two faults at once: the first check in the documented order wins)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_estimator_refusals as G  # noqa: E402

INVALID_ARG = 2


@pytest.fixture(scope="module")
def golden():
    with open(G.OUT) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return G.build_drivers(tmp_path_factory.mktemp("estimator_refusals"))


@pytest.fixture(scope="module")
def library():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu.lib()


def test_the_table_names_every_refusal(golden):
    assert set(golden) == set(G.CASES) | set(G.LIB_CASES)
    for name, cases in list(G.CASES.items()) + list(G.LIB_CASES.items()):
        assert sorted(golden[name]) == sorted(G.key(kw) for kw in cases), name
        assert all(st == INVALID_ARG and text.startswith(name.replace("dabgpu_", "") + ": ") for st, text in golden[name].values()), name
    said = {text.split(": ", 1)[1].split(" ")[0] for cases in golden.values() for _, text in cases.values()}
    assert len(said) >= 15, said                                       # (distinct openings of the reasons: the table is not one refusal many times)


@pytest.mark.parametrize("planner", sorted(G.CASES))
def test_planner_refusals_keep_status_and_text(planner, golden, drivers):
    for kw in G.CASES[planner]:
        assert G.run_planner(drivers, planner, kw) == golden[planner][G.key(kw)], (planner, kw)


@pytest.mark.parametrize("fn", sorted(G.LIB_CASES))
def test_entry_point_refusals_keep_status_and_text(fn, golden, library):
    for kw in G.LIB_CASES[fn]:
        assert G.run_lib(library, fn, kw) == golden[fn][G.key(kw)], (fn, kw)
