"""CPU: what the receive-diversity planners answer (status, whole text, geometry) and every answer the three
dabgpu_diversity_combine_frames* calls and the three *_host_sync forms give without a device, by status and by whole text:
tests/golden/diversity_refusals.json holds what the library answered before the three copies of each layer above the kernel became one
(tests/golden/make_golden_diversity_refusals.py wrote it and holds the tables of cases, among them the alignment refusal of the two
optional outputs under every delegation path -- its prefix names the call that the tables given amount to, not the one that was called --
the array-null fall-through of the host forms, and calls with two faults at once: scalar before band before symbol)."""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_diversity_refusals as G  # noqa: E402

OK, INVALID_ARG = 0, 2


@pytest.fixture(scope="module")
def golden():
    with open(G.OUT) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return G.build_drivers(tmp_path_factory.mktemp("diversity_refusals"))


@pytest.fixture(scope="module")
def library():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu.lib()


def answers(golden):
    """(table, key, status, text) of every recorded case"""
    for name, cases in golden.items():
        for k, v in cases.items():
            yield (name, k, v["status"], v["error"]) if isinstance(v, dict) else (name, k, v[0], v[1])


def test_the_table_names_every_refusal(golden):
    assert set(golden) == set(G.CASES) | set(G.LIB_CASES)
    for name, cases in list(G.CASES.items()) + list(G.LIB_CASES.items()):
        assert sorted(golden[name]) == sorted(G.key(kw) for kw in cases), name
    rows = list(answers(golden))
    assert all((st == INVALID_ARG and text) or (st == OK and not text) for _, _, st, text in rows)
    refusals = [(name, k, text) for name, k, st, text in rows if st != OK]
    assert len(refusals) >= 60
    # distinct openings of the reasons (behind the prefix, the branch number left out, three words): the table is not one refusal many times
    said = {" ".join(re.sub(r"-?\d+", "#", text.split(": ", 1)[1]).split(" ")[:3]) for _, _, text in refusals}
    assert len(said) >= 12, said
    # no host form is ever accepted here, and a device call only without frames (either would go on to bind the made-up handle)
    for name, k, st, _ in rows:
        assert st != OK or name in G.CASES or (name in G.DEVICE and "nf=" not in k), (name, k)
    # a planner's prefix is its own or that of a narrower planner; an entry point's is an entry point's or a planner's
    names = [n.replace("dabgpu_", "") for n in golden]
    assert all(text.split(": ", 1)[0] in names for _, _, text in refusals)


def test_the_alignment_refusal_names_the_effective_call(golden):
    """the six delegation paths, as the library answered before the rewrite: what the tables amount to chooses the prefix"""
    sym, band = golden["dabgpu_diversity_combine_frames_symbols"], golden["dabgpu_diversity_combine_frames_banded"]
    tail = ": d_soft_scale and d_live_mask must be 4-byte aligned"
    for a in G.ALIGN:
        for table, path, prefix in ((sym, dict(syms="null"), "diversity_combine_frames_banded"),
                                    (sym, dict(syms="--", bands="a-"), "diversity_combine_frames_banded"),
                                    (sym, dict(syms="--", bands="--"), "diversity_combine_frames"),
                                    (sym, dict(syms="a-", bands="null"), "diversity_combine_frames_symbols"),
                                    (sym, dict(syms="null", bands="null"), "diversity_combine_frames"),
                                    (band, dict(bands="null"), "diversity_combine_frames"),
                                    (band, dict(bands="--"), "diversity_combine_frames"),
                                    (band, dict(), "diversity_combine_frames_banded"),
                                    (sym, dict(), "diversity_combine_frames_symbols"),
                                    (golden["dabgpu_diversity_combine_frames"], dict(), "diversity_combine_frames")):
            assert table[G.key(dict(path, **a))] == [INVALID_ARG, prefix + tail], (path, a)


@pytest.mark.parametrize("planner", sorted(G.CASES))
def test_planner_answers_keep_status_text_and_geometry(planner, golden, drivers):
    for kw in G.CASES[planner]:
        assert G.run_planner(drivers, planner, kw) == golden[planner][G.key(kw)], (planner, kw)


@pytest.mark.parametrize("fn", sorted(G.LIB_CASES))
def test_entry_point_answers_keep_status_and_text(fn, golden, library):
    for kw in G.LIB_CASES[fn]:
        assert G.run_lib(library, fn, kw) == golden[fn][G.key(kw)], (fn, kw)
