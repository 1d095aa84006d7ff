"""-m gpu tests of the stream bank (dab-radio_amd/csrc/ofdm_stream.hip) at the inputs tests/test_gpu_stream_bank.py never gives it: other L1
window settings than the defaults (both branches of stream_l1_kernel, their bound k = 128 / 129, k = 1, adjacent windows, other beta and
thresholds), blocks shorter than an L1 window in every state, and blocks that end exactly with the sample that fills the correlation
window or completes a frame -- and one, two and three samples before that.  The expected side is tests/stream_model.py with the same
settings fed the same blocks; after every call the frame count, every frame's soft bits and every status field must be equal, floats
as uint32 patterns.  tests/test_stream_model_edges.py pins on the CPU that the schedules hit those edges."""
import numpy as np
import pytest

import stream_edge_cases as EC
import stream_model as SM

pytestmark = pytest.mark.gpu


def bank_cfg(dabgpu, mode, row=None):
    cfg = dabgpu.StreamCfg()
    dabgpu.lib().dabgpu_stream_cfg_default(dabgpu.C.byref(cfg))
    if row is not None:
        cfg.signal_l1_nb_samples, cfg.signal_l1_nb_decimate, cfg.signal_l1_update_beta, cfg.thresh_null_start, cfg.thresh_null_end = row
    if mode != 1:
        cfg.sync.impulse_peak_threshold_db = EC.IMPULSE_DB
    return cfg


def check_status(tag, st, models):
    for e, mo in enumerate(models):
        assert int(st["state"][e]) == mo.state, (tag, e, int(st["state"][e]), mo.state)
        assert st["signal_l1_average"][e].view(np.uint32) == np.float32(mo.signal_avg).view(np.uint32), (tag, e)
        assert st["freq_coarse"][e].view(np.uint32) == np.float32(mo.sync.freq_coarse).view(np.uint32), (tag, e)
        assert st["freq_fine"][e].view(np.uint32) == np.float32(mo.sync.freq_fine).view(np.uint32), (tag, e)
        assert int(st["fine_time_offset"][e]) == mo.fine_time_offset, (tag, e)
        assert int(st["total_frames_read"][e]) == mo.frames_read and int(st["total_frames_desync"][e]) == mo.frames_desync, (tag, e)


def check_call(tag, bank, models, blks, d_bits, nf, snaps):
    """the models take the call's blocks; frame counts, every frame's soft bits and every status field"""
    for e, mo in enumerate(models):
        before = len(mo.out_frames)
        mo.process(blks[e])
        new = mo.out_frames[before:]
        assert nf[e] == len(new), (tag, e, int(nf[e]), len(new))
        for j, fr in enumerate(new):
            assert np.array_equal(d_bits[e, j].cpu().numpy(), fr["bits"]), (tag, e, j)
        snaps[e].append(mo.snapshot())
    check_status(tag, bank.status(), models)


def report(what, g, blocks, snaps, models, k=100):
    hits = [SM.edge_hits(g, blocks, s, k) for s in snaps]
    for e, (h, mo) in enumerate(zip(hits, models)):
        print("%s stream %d: fill-ends %d frame-ends %d tiny blocks per state %s frames %d desyncs %d"
              % (what, e, h["fill"], h["frame"], h["tiny"], len(mo.out_frames), mo.frames_desync))
    return hits


def run_plain(oracle, bank, mode, name, q, iq, blocks, models, tag):
    """`blocks` of the streams q [E][n][2] (iq [E][n] to the models) through process (name None: complex float) or process_raw"""
    import dabgpu
    import torch
    g = oracle.geometry(mode)
    E, n = len(iq), iq[0].size
    max_frames = max(blocks) // (g.nb_frame_samples - g.nb_null_period - g.nb_symbol_period) + 2
    d_bits = torch.zeros((E, max_frames, g.nb_frame_bits), dtype=torch.int8, device="cuda")
    d_nf = torch.zeros(E, dtype=torch.int32, device="cuda")
    d_q = torch.from_numpy(np.array(q)).cuda()
    snaps = [[] for _ in range(E)]
    pos = 0
    for i, m in enumerate(blocks):
        d_bits.zero_()
        if name is None:
            bank.process(d_q[:, pos:pos + m].contiguous(), m, m, d_bits, max_frames, d_nf)
        else:
            bank.process_raw(d_q[:, pos:].data_ptr(), dabgpu.IQ_FORMATS.index(name), n, m, d_bits, max_frames, d_nf)
        torch.cuda.synchronize()
        check_call((tag, i, pos, m), bank, models, [s[pos:pos + m] for s in iq], d_bits, d_nf.cpu().numpy(), snaps)
        pos += m
    assert pos == n
    return snaps


L1_CASES = [(3, row, name) for row in EC.L1_TABLE for name in ([None, "raw_u8", "raw_s16l"] if row[0] in (128, 129) else [None])]
L1_CASES.append((1, EC.L1_TABLE[2], None))


@pytest.mark.parametrize("mode,row,name", L1_CASES, ids=["mode%d-k%d_d%d_b%g-%s" % (c[0], c[1][0], c[1][1], c[1][2], c[2] or "c32") for c in L1_CASES])
def test_bank_with_other_l1_settings_equals_the_model(oracle, mode, row, name):
    """one bank per row of the L1 table (tests/stream_edge_cases.py): two captures and a stream without a DAB signal; blocks of k - 1, k,
    k + 1, k * decimate, k * decimate + 1 and k * decimate + k + 1 samples (no level update; no window; one window three times; two), then
    20002 repeatedly and a ragged last one.  Rows 128 and 129 also from u8 and s16 capture bytes: both branches of stream_l1_kernel in
    their SRC != 0 instantiations"""
    import dabgpu
    ctx = dabgpu.Context(0)
    g = oracle.geometry(mode)
    q, iq = EC.l1_quantised(oracle, mode, name or "raw_f32l")
    blocks = EC.l1_blocks(row, iq[0].size)
    bank = dabgpu.StreamBank(ctx, len(iq), bank_cfg(dabgpu, mode, row), mode=mode)
    models = [EC.model(oracle, mode, row) for _ in iq]
    print("L1 row (k, decimate, beta, start, end) = %s mode %d format %s: %d blocks, first %s" % (row, mode, name or "c32", len(blocks), blocks[:6]))
    snaps = run_plain(oracle, bank, mode, name, q, iq, blocks, models, (row, mode, name))
    report("L1 k=%d" % row[0], g, blocks, snaps, models, row[0])
    assert len(models[0].out_frames) >= 2 and len(models[1].out_frames) >= 2
    assert len(models[2].out_frames) == 0 and models[2].frames_desync >= 1
    bank.close()


def edge_setup(oracle, mode, name):
    case = EC.edge_case(oracle, mode, name)
    h = case["hits"]
    print("mode %d %s schedule: %s" % (mode, name, case["blocks"]))
    assert h["fill"] >= 2 and h["frame"] >= 2 and all(h["tiny"][s] >= 1 for s in (0, 1, 4)), h
    return case


@pytest.mark.parametrize("name", [None, "raw_u8"], ids=["c32", "raw_u8"])
def test_exact_block_ends_and_tiny_blocks_mode_iii(oracle, name):
    """five streams, stream 0's blocks end with the sample that fills the correlation window / completes a frame, its neighbours' one, two
    and three samples before that; blocks of 1, 7, 99, 100 and 101 samples in the states 0, 1 and 4; complex float through process, u8
    capture bytes through process_raw"""
    import dabgpu
    ctx = dabgpu.Context(0)
    case = edge_setup(oracle, 3, name or "raw_f32l")
    bank = dabgpu.StreamBank(ctx, 5, bank_cfg(dabgpu, 3), mode=3)
    models = [EC.model(oracle, 3) for _ in range(5)]
    snaps = run_plain(oracle, bank, 3, name, case["q"], case["iq"], case["blocks"], models, ("edges", 3, name))
    hits = report("mode 3 %s" % (name or "c32"), oracle.geometry(3), case["blocks"], snaps, models)
    assert snaps[0] == case["after"] and hits[0] == case["hits"]
    assert len(models[0].out_frames) >= 3
    bank.close()


def test_a_filled_window_does_not_survive_a_reset(oracle):
    """the blocks up to the first one that ends on a window fill (state RUNNING_COARSE, nothing requested yet), a reset, the capture from
    the start again: the bank equals fresh models after every call"""
    import dabgpu
    ctx = dabgpu.Context(0)
    case = edge_setup(oracle, 3, "raw_f32l")
    g = oracle.geometry(3)
    stop = next(i for i, a in enumerate(case["after"]) if a[0] == 2 and a[1] == g.nb_null_period + g.nb_symbol_period)
    bank = dabgpu.StreamBank(ctx, 5, bank_cfg(dabgpu, 3), mode=3)
    models = [EC.model(oracle, 3) for _ in range(5)]
    run_plain(oracle, bank, 3, None, case["q"][:, :sum(case["blocks"][:stop + 1])], [s[:sum(case["blocks"][:stop + 1])] for s in case["iq"]],
              case["blocks"][:stop + 1], models, ("before reset",))
    st = bank.status()
    assert int(st["state"][0]) == 2 and int(st["total_frames_read"][0]) >= 1
    bank.reset()
    z = bank.status()
    for f in z.dtype.names:
        assert not z[f].view(np.uint32).any() if z[f].dtype == np.float32 else not z[f].any(), f
    models = [EC.model(oracle, 3) for _ in range(5)]
    snaps = run_plain(oracle, bank, 3, None, case["q"], case["iq"], case["blocks"], models, ("after reset",))
    report("after reset", g, case["blocks"], snaps, models)
    assert snaps[0] == case["after"]
    bank.close()


@pytest.mark.parametrize("name", ["raw_u8", "raw_f32l"])
def test_exact_block_ends_and_tiny_blocks_with_retained_blocks(oracle, name):
    """mode I, process_retained: every call is handed the previous call's block; a block of one or two samples meets a pending carry (the
    carried samples are copied first, the block's own reach the frame buffer through the odd / even trimming); one release in the middle
    of a frame, after which the next call is handed no block and the released block is overwritten"""
    import dabgpu
    import torch
    ctx = dabgpu.Context(0)
    case = edge_setup(oracle, 1, name)
    g = oracle.geometry(1)
    blocks, q, iq = case["blocks"], case["q"], case["iq"]
    E, cap = 5, max(blocks)
    fmt = dabgpu.IQ_FORMATS.index(name)
    max_frames = cap // 191400 + 2
    # (behind the tiny blocks in the middle of a frame, so that those meet the carry the block before them left)
    release_after = max(i for i in range(len(blocks) - 1) if case["after"][i][0] == 4 and blocks[i] >= 10000)
    assert release_after > max(i for i, b in enumerate(blocks) if b == 1)
    bank = dabgpu.StreamBank(ctx, E, bank_cfg(dabgpu, 1))
    models = [EC.model(oracle, 1) for _ in range(E)]
    bufs = [torch.zeros((E, cap, 2), dtype=torch.from_numpy(np.array(q[:1, :1])).dtype, device="cuda") for _ in range(2)]
    d_bits = torch.zeros((E, max_frames, g.nb_frame_bits), dtype=torch.int8, device="cuda")
    d_nf = torch.zeros(E, dtype=torch.int32, device="cuda")
    snaps = [[] for _ in range(E)]
    prev, pos = None, 0
    for i, m in enumerate(blocks):
        cur = bufs[i % 2]
        cur.fill_(0 if name != "raw_u8" else 7)                          # (what the call before the previous one read is gone)
        cur[:, :m] = torch.from_numpy(np.array(q[:, pos:pos + m])).cuda()
        d_bits.zero_()
        bank.process_retained(cur, fmt, cap, m, prev, d_bits, max_frames, d_nf)
        torch.cuda.synchronize()
        check_call(("retained", name, i, pos, m), bank, models, [s[pos:pos + m] for s in iq], d_bits, d_nf.cpu().numpy(), snaps)
        prev, pos = cur, pos + m
        if i == release_after:
            bank.release(prev, fmt, cap)
            torch.cuda.synchronize()
            prev.fill_(0 if name != "raw_u8" else 9)
            prev = None
    hits = report("mode 1 retained %s (release after block %d)" % (name, release_after), g, blocks, snaps, models)
    assert snaps[0] == case["after"] and hits[0] == case["hits"]
    assert len(models[0].out_frames) >= 3
    bank.close()


def test_exact_block_ends_and_tiny_blocks_in_the_ring_form(oracle):
    """mode I, s16 capture bytes, process_ring with a ring of 5 frames: the schedule's blocks cut to the 191400 samples a ring call takes
    (the exact ends stay); the slot reported after every call and the frame's bits in that slot"""
    import dabgpu
    import torch
    ctx = dabgpu.Context(0)
    name, H = "raw_s16l", 5
    case = edge_setup(oracle, 1, name)
    g = oracle.geometry(1)
    blocks = EC.ring_blocks(case["blocks"], g.nb_frame_samples - g.nb_null_period - g.nb_symbol_period)
    q, iq = case["q"], case["iq"]
    E, n = 5, iq[0].size
    fmt = dabgpu.IQ_FORMATS.index(name)
    bank = dabgpu.StreamBank(ctx, E, bank_cfg(dabgpu, 1))
    models = [EC.model(oracle, 1) for _ in range(E)]
    d_q = torch.from_numpy(np.array(q)).cuda()
    hist = torch.zeros((E, H, g.nb_frame_bits), dtype=torch.int8, device="cuda")
    slot = torch.full((E,), -7, dtype=torch.int32, device="cuda")
    snaps = [[] for _ in range(E)]
    pos = 0
    for i, m in enumerate(blocks):
        bank.process_ring(d_q[:, pos:].data_ptr(), fmt, n, m, hist, H, slot)
        torch.cuda.synchronize()
        got = slot.cpu().numpy()
        for e, mo in enumerate(models):
            before = len(mo.out_frames)
            mo.process(iq[e][pos:pos + m])
            new = mo.out_frames[before:]
            assert len(new) <= 1
            assert got[e] == ((mo.frames_read - 1) % H if new else -1), (i, pos, m, e, int(got[e]))
            if new:
                assert np.array_equal(hist[e, int(got[e])].cpu().numpy(), new[0]["bits"]), (i, pos, m, e)
            snaps[e].append(mo.snapshot())
        check_status(("ring", i, pos, m), bank.status(), models)
        pos += m
    assert pos == n
    hits = report("mode 1 ring raw_s16l", g, blocks, snaps, models)
    assert hits[0]["fill"] >= 2 and hits[0]["frame"] >= 2 and all(hits[0]["tiny"][s] >= 1 for s in (0, 1, 4)), hits[0]
    assert len(models[0].out_frames) >= 3
    bank.close()
