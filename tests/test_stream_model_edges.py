"""The infrastructure of tests/test_gpu_stream_bank_edges.py, pinned on the CPU so that the GPU tests cannot miss their edges unnoticed:
the parameterised L1 settings of tests/stream_model.py keep the former constants as defaults and lock on every row of the L1 table;
edge_schedule's blocks really end on window fills and frame completions and really put blocks shorter than an L1 window into the states
0, 1 and 4; and what the model returns does not depend on those cuts."""
import numpy as np
import pytest

import stream_edge_cases as EC
import stream_model as SM

# the (mode, capture format) pairs the bank tests run their exact-block-end schedules in
EDGE_FORMS = [(3, "raw_f32l"), (3, "raw_u8"), (1, "raw_u8"), (1, "raw_f32l"), (1, "raw_s16l")]


def test_l1_defaults_are_the_former_constants():
    assert SM.L1Settings() == (0.95, 100, 5, 0.35, 0.75)
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(20011) + 1j * rng.standard_normal(20011)).astype(np.complex64)
    for k, stride in ((100, 500), (100, 100), (1, 7), (129, 387), (64, 64)):
        loop = np.array([SM.l1_average(x[i:i + k]) for i in range(0, x.size - k, stride)], np.float32)
        assert np.array_equal(SM.l1_windows(x, k, stride).view(np.uint32), loop.view(np.uint32)), (k, stride)
    assert SM.l1_windows(x[:100], 100, 500).size == 0 and SM.l1_windows(x[:101], 100, 500).size == 1
    assert SM.l1_windows(x[:501], 100, 500).size == 1 and SM.l1_windows(x[:601], 100, 500).size == 2 and SM.l1_windows(x[:99], 100, 500).size == 0


@pytest.mark.parametrize("mode,name", EDGE_FORMS)
def test_edge_schedule_hits_its_targets_and_the_cut_changes_nothing(oracle, mode, name):
    case = EC.edge_case(oracle, mode, name)
    g = oracle.geometry(mode)
    hits = case["hits"]
    print(mode, name, case["blocks"], hits)
    assert hits["fill"] >= 2 and hits["frame"] >= 2, hits
    one = EC.one_block(oracle, mode, name)
    schedules = [case["blocks"]]
    if mode == 1:
        schedules.append(EC.ring_blocks(case["blocks"], g.nb_frame_samples - g.nb_null_period - g.nb_symbol_period))
        assert max(schedules[1]) <= 191400 and len(schedules[1]) > len(schedules[0])
    for blocks in schedules:
        m = EC.model(oracle, mode)
        after = EC.run_model(m, case["iq"][0], blocks)
        h = SM.edge_hits(g, blocks, after)
        assert h["fill"] >= 2 and h["frame"] >= 2, h
        assert m.position == case["iq"][0].size == sum(blocks)
        assert len(m.out_frames) == len(one.out_frames) >= 3
        for a, b in zip(m.out_frames, one.out_frames):
            assert np.array_equal(a["bits"], b["bits"])
            assert np.float32(a["fine"]).view(np.uint32) == np.float32(b["fine"]).view(np.uint32)
            assert a["offset"] == b["offset"] and a["desync"] == b["desync"]
        assert m.frames_desync == one.frames_desync and m.frames_read == one.frames_read


@pytest.mark.parametrize("mode,name", EDGE_FORMS)
def test_tiny_blocks_are_consumed_in_states_0_1_and_4(oracle, mode, name):
    case = EC.edge_case(oracle, mode, name)
    g = oracle.geometry(mode)
    blocks, after, hits = case["blocks"], case["after"], case["hits"]
    assert all(hits["tiny"][s] >= 1 for s in (0, 1, 4)), hits
    T = len(EC.TINY)
    assert tuple(blocks[:T]) == EC.TINY and all(a[0] == 0 for a in after[:T])                    # at the very start
    at = [i for i in range(1, len(blocks) - T) if tuple(blocks[i:i + T]) == EC.TINY]
    assert len(at) == 2
    i, j = at
    assert after[i - 1][:2] == (1, g.nb_null_period) and after[i - 1][3] == after[i - 2][3] + 1   # right after a frame completion
    assert all(a[0] == 1 for a in after[i:i + 3])
    assert after[j - 1][0] == 4 and all(a[0] == 4 for a in after[j:j + T])                       # in the middle of a frame
    assert 2 * g.nb_symbol_period < after[j + T - 1][2] < g.nb_frame_samples - 2 * g.nb_symbol_period
    assert sum(blocks) == case["iq"][0].size
    # the delayed neighbours run through the same blocks without an exception and consume every sample
    for e in range(1, 5):
        m = EC.model(oracle, mode)
        EC.run_model(m, case["iq"][e], blocks)
        assert m.position == sum(blocks)


@pytest.mark.parametrize("row", EC.L1_TABLE, ids=lambda r: "k%d_d%d_b%g" % (r[0], r[1], r[2]))
def test_the_model_locks_with_every_row_of_the_l1_table(oracle, row):
    forms = [(3, "raw_f32l")]
    if row[0] in (128, 129):
        forms += [(3, "raw_u8"), (3, "raw_s16l")]
    if row[0] == 129:
        forms.append((1, "raw_f32l"))
    for mode, name in forms:
        iq = EC.l1_quantised(oracle, mode, name)[1]
        blocks = EC.l1_blocks(row, iq[0].size)
        k, d = row[0], row[1]
        assert blocks[:6 if k > 1 else 5] == [b for b in (k - 1, k, k + 1, k * d, k * d + 1, k * d + k + 1) if b > 0]
        models = [EC.model(oracle, mode, row) for _ in iq]
        for m, s in zip(models, iq):
            EC.run_model(m, s, blocks)
        print(row, mode, name, [(len(m.out_frames), m.frames_desync) for m in models])
        assert len(models[0].out_frames) >= 2 and len(models[1].out_frames) >= 2
        assert len(models[2].out_frames) == 0 and models[2].frames_desync >= 1
    if row[0] == 1:
        assert models[0].frames_desync >= 2, "one-sample windows: failed synchronisations before the lock"
