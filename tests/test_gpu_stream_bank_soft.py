"""-m gpu: the weighted soft bits (DABGPU_SOFT_CSI) in the stream bank, dabgpu_stream_bank_set_soft.  The bank's state machine never reads a
soft bit, so a bank under the weighted policy must find the frames its normalised twin finds, where it finds them -- frame counts and
every status field after every call are compared with a second bank left on the normalised policy and fed the same blocks -- and only
the bits differ: every completed frame equals tests/stream_soft_model.py's expectation (the oracle's transform of the frame the state
machine assembled, the numpy model's demapper), and its scale word equals softbit_model.soft_scale bit for bit.  One of the streams
has moving timing: a frame found 37 samples late has its symbol 0 split between the frame buffer and the caller's block inside the
useful part (the per-lane loader path), the others have it in the frame buffer."""
import numpy as np
import pytest

import softbit_model as SM
import stream_soft_model as SSM

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = 5
NAN_WORD = 0x7FC00000


def bits32(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def assert_status_equal(a, b, where):
    for f in a.dtype.names:
        x, y = (s[f].view(np.uint32) if s[f].dtype == np.float32 else s[f] for s in (a, b))
        assert np.array_equal(x, y), (where, f, x, y)


class Pair:
    """a bank under the weighted policy (with a scale buffer of E * slots words, NaN before every call) and its normalised twin"""

    def __init__(self, E, slots, level=64.0):
        import dabgpu
        import torch
        self.dabgpu, self.torch = dabgpu, torch
        self.ctx = dabgpu.Context(0)
        self.E, self.slots, self.level = E, slots, level
        self.norm, self.soft = dabgpu.StreamBank(self.ctx, E), dabgpu.StreamBank(self.ctx, E)
        self.scale = torch.full((E * slots,), float("nan"), dtype=torch.float32, device="cuda")
        self.soft.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, level), self.scale)
        self.bits = [torch.zeros((E, slots, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda") for _ in range(2)]
        self.nf = [torch.full((E,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]

    def clear(self):
        for b in self.bits:
            b.zero_()
        self.scale.fill_(float("nan"))

    def compare_state(self, where):
        """frame counts (or ring slots) and every status field: the policy changed nothing the state machine looks at"""
        self.torch.cuda.synchronize()
        assert self.torch.equal(self.nf[0], self.nf[1]), (where, self.nf[0].tolist(), self.nf[1].tolist())
        assert_status_equal(self.norm.status(), self.soft.status(), where)
        return self.nf[1].cpu().numpy()

    def close(self):
        self.norm.close(); self.soft.close(); self.ctx.close()


def check_call(pair, refs, models, ci, nf, where, seen_offsets):
    """every frame completed in call ci: weighted bits and scale word against the model, the twin's bits against the oracle's"""
    scale = bits32(pair.scale.cpu().numpy()).reshape(pair.E, pair.slots)
    for e in range(pair.E):
        new = refs[e][ci]
        assert nf[e] == len(new), (where, e, nf[e], len(new))
        for j, fr in enumerate(new):
            k, exp = models[e].weighted(fr, pair.level)
            assert np.array_equal(pair.bits[1][e, j].cpu().numpy(), exp), (where, e, j, fr["offset"])
            assert scale[e, j] == bits32(k), (where, e, j, scale[e, j], k)
            assert np.array_equal(pair.bits[0][e, j].cpu().numpy(), fr["bits"]), (where, e, j)
            seen_offsets.append(fr["offset"])
        assert np.all(scale[e, len(new):] == NAN_WORD), (where, e, "a scale word without a frame was written")


def assert_both_symbol0_placements(seen_offsets):
    assert any(o > 0 for o in seen_offsets), "no frame with its symbol 0 split inside the useful part (fine time offset > 0)"
    assert any(o <= 0 for o in seen_offsets), "no frame with its symbol 0 in the frame buffer (fine time offset <= 0)"


@pytest.mark.parametrize("block", [65536, 10007, 500000])
def test_float_blocks_equal_the_model_and_track_like_the_normalised_twin(oracle, block):
    import torch
    S = SSM.float_streams(oracle)
    E, n = S.shape
    ref = [SSM.run_model(oracle, ("float", e), S[e], block) for e in range(E)]
    refs, models = [r[0] for r in ref], [r[1] for r in ref]
    slots = block // 191400 + 2
    pair = Pair(E, slots)
    seen = []
    for ci, k in enumerate(range(0, n, block)):
        m = min(block, n - k)
        d_iq = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(S[:, k:k + m])).cuda())
        pair.clear()
        pair.norm.process(d_iq, m, m, pair.bits[0], slots, pair.nf[0])
        pair.soft.process(d_iq, m, m, pair.bits[1], slots, pair.nf[1])
        nf = pair.compare_state((block, k))
        check_call(pair, refs, models, ci, nf, (block, k), seen)
    assert [fr["offset"] for fr in models[SSM.MOVING].out_frames][1:] == [0, 37, -53] and models[SSM.MOVING].frames_desync == 0
    assert len(models[SSM.NOISE].out_frames) == 0 and sum(len(m.out_frames) for m in models) >= 13
    assert_both_symbol0_placements(seen)
    pair.close()


RAW_STREAMS = [1, SSM.MOVING, SSM.NOISE]


def raw_inputs(oracle, name, streams=RAW_STREAMS):
    """the float streams quantised to a capture format -> (raw bytes [E][n * sample bytes], what the readers make of them [E][n] complex)"""
    import dabgpu
    fmt = dabgpu.IQ_FORMATS.index(name)
    S = SSM.float_streams(oracle)
    n = S.shape[1] // 8 * 8
    raw = np.stack([SSM.quantise(S[e, :n], name) for e in streams])
    iq = [oracle.iq_convert(raw[i], fmt).view(np.complex64) for i in range(len(streams))]
    return fmt, n, raw, iq


@pytest.mark.parametrize("name", ["raw_u8", "raw_s8", "raw_s16l", "raw_u16l"])
def test_capture_formats_fused_loaders_and_a_converted_one(oracle, name):
    import dabgpu
    import torch
    fmt, n, raw, iq = raw_inputs(oracle, name)
    E = len(iq)
    block = 65536 + 2 if name != "raw_u16l" else 65536            # fused loaders: odd byte alignments inside the raw data
    ref = [SSM.run_model(oracle, (name, e), iq[e], block) for e in range(E)]
    refs, models = [r[0] for r in ref], [r[1] for r in ref]
    sb = dabgpu.iq_format_sample_bytes(fmt)
    d_raw = torch.from_numpy(raw).cuda()
    slots = block // 191400 + 2
    pair = Pair(E, slots)
    seen = []
    for ci, k in enumerate(range(0, n, block)):
        m = min(block, n - k)
        pair.clear()
        pair.norm.process_raw(d_raw[:, sb * k:].data_ptr(), fmt, n, m, pair.bits[0], slots, pair.nf[0])
        pair.soft.process_raw(d_raw[:, sb * k:].data_ptr(), fmt, n, m, pair.bits[1], slots, pair.nf[1])
        nf = pair.compare_state((name, k))
        check_call(pair, refs, models, ci, nf, (name, k), seen)
    assert len(seen) >= 6
    assert_both_symbol0_placements(seen)
    pair.close()


@pytest.mark.parametrize("name", ["raw_u8", "raw_f32l"])
def test_retained_blocks_equal_the_copying_form(oracle, name):
    """dabgpu_stream_bank_process_retained under the weighted policy: a frame's symbol 0 may lie in the previous block.  Bits, scale words,
    counts and status equal the copying form's (itself held to the model here), then a release and one more plain call"""
    import dabgpu
    import torch
    fmt, n, raw, iq = raw_inputs(oracle, name)
    E, block = len(iq), 250001
    sb = dabgpu.iq_format_sample_bytes(fmt)
    ref = [SSM.run_model(oracle, (name, e), iq[e], block) for e in range(E)]
    refs, models = [r[0] for r in ref], [r[1] for r in ref]
    slots = block // 191400 + 2
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    ctx = dabgpu.Context(0)
    banks = [dabgpu.StreamBank(ctx, E), dabgpu.StreamBank(ctx, E)]                 # [0] copies, [1] retained
    scale = [torch.full((E * slots,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    for b, s in zip(banks, scale):
        b.set_soft(soft, s)
    bufs = [torch.zeros((E, block * sb), dtype=torch.uint8, device="cuda") for _ in range(3)]
    bits = [torch.zeros((E, slots, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda") for _ in range(2)]
    nf = [torch.zeros(E, dtype=torch.int32, device="cuda") for _ in range(2)]
    d_raw = torch.from_numpy(raw).cuda()
    prev, frames = None, 0
    for ci, k in enumerate(range(0, n, block)):
        m = min(block, n - k)
        cur = bufs[1 + ci % 2]                                                   # the retained bank's two alternating buffers
        cur[:, :m * sb] = d_raw[:, k * sb:(k + m) * sb]
        bufs[0][:, :m * sb] = cur[:, :m * sb]
        for t in bits:
            t.zero_()
        for s in scale:
            s.fill_(float("nan"))
        banks[0].process_raw(bufs[0], fmt, block, m, bits[0], slots, nf[0])
        banks[1].process_retained(cur, fmt, block, m, prev, bits[1], slots, nf[1])
        torch.cuda.synchronize()
        bufs[0].fill_(7)                                                         # the copying bank's block is free to go
        assert torch.equal(nf[0], nf[1]) and torch.equal(bits[0], bits[1]), k
        assert np.array_equal(bits32(scale[0].cpu().numpy()), bits32(scale[1].cpu().numpy())), k
        assert_status_equal(banks[0].status(), banks[1].status(), k)
        sc = bits32(scale[1].cpu().numpy()).reshape(E, slots)
        for e in range(E):
            assert int(nf[1][e]) == len(refs[e][ci])
            for j, fr in enumerate(refs[e][ci]):
                kk, exp = models[e].weighted(fr)
                assert np.array_equal(bits[1][e, j].cpu().numpy(), exp) and sc[e, j] == bits32(kk), (name, k, e, j)
                frames += 1
        prev = cur
    assert frames >= 6
    banks[1].release(prev, fmt, block)
    m = 250000
    for b, t, c in zip(banks, bits, nf):
        bufs[0][:, :m * sb] = d_raw[:, :m * sb]
        t.zero_()
        b.process_raw(bufs[0], fmt, block, m, t, slots, c)
    torch.cuda.synchronize()
    assert torch.equal(nf[0], nf[1]) and torch.equal(bits[0], bits[1])
    for b in banks:
        b.close()
    ctx.close()


@pytest.mark.parametrize("block", [191400, 60000])
@pytest.mark.parametrize("name", ["raw_u8", "raw_f32l"])
def test_ring_form_with_retained_blocks_equals_the_copying_ring_form(oracle, name, block):
    """dabgpu_stream_bank_process_ring_retained under the weighted policy: the ring form's blocks are shorter than a frame, so a frame lies in
    the frame buffer, the previous block and the current one (60000: the bulk-copy path).  Rings, slots, scale words by ring slot and
    status equal the copying ring form's; a release at the end"""
    import dabgpu
    import torch
    fmt, n, raw, iq = raw_inputs(oracle, name)
    E, H = len(iq), 5
    sb = dabgpu.iq_format_sample_bytes(fmt)
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    ctx = dabgpu.Context(0)
    banks = [dabgpu.StreamBank(ctx, E), dabgpu.StreamBank(ctx, E)]
    scale = [torch.full((E * H,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    for b, s in zip(banks, scale):
        b.set_soft(soft, s)
    bufs = [torch.zeros((E, block * sb), dtype=torch.uint8, device="cuda") for _ in range(3)]
    hist = [torch.zeros((E, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda") for _ in range(2)]
    slot = [torch.full((E,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    d_raw = torch.from_numpy(raw).cuda()
    prev, frames = None, 0
    for ci, k in enumerate(range(0, n, block)):
        m = min(block, n - k)
        cur = bufs[1 + ci % 2]
        cur[:, :m * sb] = d_raw[:, k * sb:(k + m) * sb]
        bufs[0][:, :m * sb] = cur[:, :m * sb]
        banks[0].process_ring(bufs[0], fmt, block, m, hist[0], H, slot[0])
        banks[1].process_ring_retained(cur, fmt, block, m, prev, hist[1], H, slot[1])
        torch.cuda.synchronize()
        bufs[0].fill_(9)
        assert torch.equal(slot[0], slot[1]), (k, slot[0].tolist(), slot[1].tolist())
        assert torch.equal(hist[0], hist[1]), k
        assert np.array_equal(bits32(scale[0].cpu().numpy()), bits32(scale[1].cpu().numpy())), k
        assert_status_equal(banks[0].status(), banks[1].status(), k)
        frames += int((slot[0] >= 0).sum().item())
        prev = cur
    assert frames >= 6
    written = bits32(scale[1].cpu().numpy()).reshape(E, H) != NAN_WORD
    assert written[:2, :3].all() and not written[2].any(), "a scale word per ring slot a frame went to, none for the noise-only stream"
    banks[1].release(prev, fmt, block)
    for b in banks:
        b.close()
    ctx.close()


@pytest.mark.parametrize("name", ["raw_f32l", "raw_u8", "raw_s8", "raw_s16l"])
def test_ring_form_in_class_order(oracle, name):
    """dabgpu_stream_bank_process_ring_layout with DABGPU_BITS_MSC_CLASSED: every ring slot holds the natural-layout expectation permuted as
    dabgpu_ofdm_demod_frames_history documents; the scale words are indexed by ring slot.  Four frames into a ring of five per stream"""
    import dabgpu
    import torch
    fmt, n, raw, iq = raw_inputs(oracle, name, streams=[0, SSM.MOVING])
    E, H, block = len(iq), 5, 150001
    sb = dabgpu.iq_format_sample_bytes(fmt)
    ref = [SSM.run_model(oracle, (name, "ring", e), iq[e], block) for e in range(E)]
    refs, models = [r[0] for r in ref], [r[1] for r in ref]
    ctx = dabgpu.Context(0)
    norm, soft = dabgpu.StreamBank(ctx, E), dabgpu.StreamBank(ctx, E)
    scale = torch.full((E * H,), float("nan"), dtype=torch.float32, device="cuda")
    soft.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0), scale)
    hist = [torch.zeros((E, H, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda") for _ in range(2)]
    slot = [torch.full((E,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    d_raw = torch.from_numpy(raw).cuda()
    count, seen = [0] * E, []
    for ci, k in enumerate(range(0, n, block)):
        m = min(block, n - k)
        norm.process_ring(d_raw[:, sb * k:].data_ptr(), fmt, n, m, hist[0], H, slot[0], bits_layout=dabgpu.BITS_MSC_CLASSED)
        soft.process_ring(d_raw[:, sb * k:].data_ptr(), fmt, n, m, hist[1], H, slot[1], bits_layout=dabgpu.BITS_MSC_CLASSED)
        torch.cuda.synchronize()
        assert torch.equal(slot[0], slot[1]), k
        assert_status_equal(norm.status(), soft.status(), k)
        sl = slot[1].cpu().numpy()
        sc = bits32(scale.cpu().numpy()).reshape(E, H)
        for e in range(E):
            new = refs[e][ci]
            assert len(new) <= 1 and sl[e] == (count[e] % H if new else -1), (name, k, e)
            for fr in new:
                kk, exp = models[e].weighted(fr)
                assert np.array_equal(hist[1][e, sl[e]].cpu().numpy(), SSM.classed(exp)), (name, k, e)
                assert np.array_equal(hist[0][e, sl[e]].cpu().numpy(), SSM.classed(fr["bits"])), (name, k, e)
                assert sc[e, sl[e]] == bits32(kk), (name, k, e)
                count[e] += 1
                seen.append(fr["offset"])
    assert count == [4, 4]
    assert_both_symbol0_placements(seen)
    norm.close(); soft.close(); ctx.close()


EDGE_STREAMS = [1, SSM.MOVING]


def test_a_stream_whose_power_overflows_is_erased_and_still_tracked(oracle):
    """samples scaled by 2^60: the power of any 2048 of them is not a finite float, k = 0, every soft bit of the frame is 0 -- while level,
    NULL search and synchroniser, which never look at a soft bit, go on as in the normalised twin (whose correlations overflow too: where
    it finds its frames is its own matter, the weighted bank finds the same ones)"""
    import torch
    S = SSM.float_streams(oracle)
    big = (S[SSM.MOVING] * np.float32(2.0 ** 60)).astype(np.complex64)
    assert not np.isfinite(SM.frame_power(big[300000:300000 + SM.NB_FFT])) and SM.scale(64.0, np.float32(np.inf)) == 0.0
    streams = np.stack([big, S[SSM.MOVING]])
    block, n = 500000, S.shape[1]
    plain = SSM.run_model(oracle, ("float", SSM.MOVING), S[SSM.MOVING], block)
    slots = block // 191400 + 2
    pair = Pair(2, slots)
    erased = 0
    for ci, k in enumerate(range(0, n, block)):
        m = min(block, n - k)
        d_iq = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(streams[:, k:k + m])).cuda())
        pair.clear()
        pair.bits[1].fill_(5)
        pair.norm.process(d_iq, m, m, pair.bits[0], slots, pair.nf[0])
        pair.soft.process(d_iq, m, m, pair.bits[1], slots, pair.nf[1])
        nf = pair.compare_state(k)
        scale = bits32(pair.scale.cpu().numpy()).reshape(2, slots)
        for j in range(nf[0]):
            assert scale[0, j] == 0 and not pair.bits[1][0, j].any().item(), (k, j)
            erased += 1
        assert nf[1] == len(plain[0][ci])
        for j, fr in enumerate(plain[0][ci]):
            kk, exp = plain[1].weighted(fr)
            assert np.array_equal(pair.bits[1][1, j].cpu().numpy(), exp) and scale[1, j] == bits32(kk)
    assert erased >= 2, "the scaled stream must complete frames for the case to mean anything"
    pair.close()


@pytest.mark.parametrize("level", [1.0, 127.0])
def test_the_ends_of_the_level_range(oracle, level):
    import torch
    S = SSM.float_streams(oracle)[EDGE_STREAMS]
    block, n = 500000, S.shape[1]
    ref = [SSM.run_model(oracle, ("float", e), SSM.float_streams(oracle)[e], block) for e in EDGE_STREAMS]
    refs, models = [r[0] for r in ref], [r[1] for r in ref]
    slots = block // 191400 + 2
    pair = Pair(2, slots, level=level)
    got = pair.soft.get_soft()
    assert (got.policy, got.level) == (pair.dabgpu.SOFT_CSI, level)
    seen = []
    for ci, k in enumerate(range(0, n, block)):
        m = min(block, n - k)
        d_iq = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(S[:, k:k + m])).cuda())
        pair.clear()
        pair.norm.process(d_iq, m, m, pair.bits[0], slots, pair.nf[0])
        pair.soft.process(d_iq, m, m, pair.bits[1], slots, pair.nf[1])
        check_call(pair, refs, models, ci, pair.compare_state(k), (level, k), seen)
    assert len(seen) == 8
    pair.close()


def test_policy_switched_between_calls_and_kept_across_reset(oracle):
    """the policy belongs to the frame that completes: frames completed in a call under either policy equal that policy's expectation, in
    both directions of the switch, the scale words are written under the weighted policy only; a reset keeps the policy"""
    import dabgpu
    import torch
    S = SSM.float_streams(oracle)[EDGE_STREAMS]
    block, n = 150001, S.shape[1]
    ref = [SSM.run_model(oracle, ("float", e), SSM.float_streams(oracle)[e], block) for e in EDGE_STREAMS]
    refs, models = [r[0] for r in ref], [r[1] for r in ref]
    weighted_calls = [True, False, True, True, False, True]
    assert len(range(0, n, block)) == len(weighted_calls)
    ctx = dabgpu.Context(0)
    bank = dabgpu.StreamBank(ctx, 2)
    slots = 2
    scale = torch.zeros(2 * slots, dtype=torch.float32, device="cuda")
    bits = torch.zeros((2, slots, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
    nf = torch.zeros(2, dtype=torch.int32, device="cuda")
    done = {True: 0, False: 0}

    def run(calls, policies):
        for ci in calls:
            k = ci * block
            m = min(block, n - k)
            w = policies[ci]
            bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI if w else dabgpu.SOFT_NORMALISED, 64.0), scale)
            scale.fill_(float("nan"))
            bits.zero_()
            bank.process(torch.view_as_real(torch.from_numpy(np.ascontiguousarray(S[:, k:k + m])).cuda()), m, m, bits, slots, nf)
            torch.cuda.synchronize()
            sc = bits32(scale.cpu().numpy()).reshape(2, slots)
            for e in range(2):
                new = refs[e][ci]
                assert int(nf[e]) == len(new)
                for j, fr in enumerate(new):
                    kk, exp = models[e].weighted(fr)
                    assert np.array_equal(bits[e, j].cpu().numpy(), exp if w else fr["bits"]), (ci, e, j, w)
                    assert sc[e, j] == (bits32(kk) if w else NAN_WORD), (ci, e, j, w)
                    done[w] += 1
    run(range(len(weighted_calls)), weighted_calls)
    assert done[True] >= 2 and done[False] >= 2, done
    switches = [(a, b) for a, b in zip(weighted_calls, weighted_calls[1:])]
    assert (True, False) in switches and (False, True) in switches
    # the last call ran under the weighted policy: a reset keeps it, like the bank's configuration
    bank.reset()
    got = bank.get_soft()
    assert (got.policy, got.level) == (dabgpu.SOFT_CSI, 64.0)
    before = done[True]
    run(range(3), [True] * 3)
    assert done[True] > before
    bank.close(); ctx.close()


def test_refusals(oracle):
    import dabgpu
    import torch
    ctx = dabgpu.Context(0)
    E, slots, m = 2, 3, 300000
    bank = dabgpu.StreamBank(ctx, E)
    d_iq = torch.zeros((E, m, 2), dtype=torch.float32, device="cuda")
    bits = torch.full((E, slots, dabgpu.NB_FRAME_BITS), 3, dtype=torch.int8, device="cuda")
    nf = torch.full((E,), -7, dtype=torch.int32, device="cuda")
    # a bad level, a bad policy: refused, the bank keeps what it had
    for policy, level, text in ((dabgpu.SOFT_CSI, 0.5, "level"), (dabgpu.SOFT_CSI, 128.0, "level"), (dabgpu.SOFT_CSI, float("nan"), "level"),
                                (2, 64.0, "policy"), (-1, 64.0, "policy")):
        with pytest.raises(dabgpu.DabGpuError, match=text):
            bank.set_soft(dabgpu.SoftCfg(policy, level))
        got = bank.get_soft()
        assert (got.policy, got.level) == (dabgpu.SOFT_NORMALISED, 64.0)
    # a scale buffer too small for the call: refused before anything is launched -- no output is touched, the state does not move
    small = torch.full((E * slots - 1,), float("nan"), dtype=torch.float32, device="cuda")
    bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0), small)
    before = bank.status().copy()
    with pytest.raises(dabgpu.DabGpuError, match="scale"):
        bank.process(d_iq, m, m, bits, slots, nf)
    with pytest.raises(dabgpu.DabGpuError, match="scale"):            # the converted path: before its conversion pass too
        bank.process_raw(d_iq.view(torch.uint8), dabgpu.IQ_FORMATS.index("raw_u16l"), m, m, bits, slots, nf)
    hist = torch.full((E, 5, dabgpu.NB_FRAME_BITS), 3, dtype=torch.int8, device="cuda")
    with pytest.raises(dabgpu.DabGpuError, match="scale"):
        bank.process_ring(d_iq, dabgpu.IQ_FORMATS.index("raw_f32l"), m, 100000, hist, 5, nf)
    torch.cuda.synchronize()
    assert (bits == 3).all().item() and (hist == 3).all().item() and (nf == -7).all().item() and np.all(bits32(small.cpu().numpy()) == NAN_WORD)
    assert_status_equal(before, bank.status(), "refused call")
    # the same call fits without a scale buffer, and under the normalised policy with the small one
    bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0))
    bank.process(d_iq, m, m, bits, slots, nf)
    bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_NORMALISED, 64.0), small)
    bank.process(d_iq, m, m, bits, slots, nf)
    bank.close()
    # a bank of another transmission mode: unsupported, it keeps the normalised policy
    bank2 = dabgpu.StreamBank(ctx, 1, mode=2)
    cfg = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    st = dabgpu.lib().dabgpu_stream_bank_set_soft(bank2._h, dabgpu.C.byref(cfg), None, 0)
    assert st == ERR_UNSUPPORTED and b"mode" in dabgpu.lib().dabgpu_last_error()
    assert bank2.get_soft().policy == dabgpu.SOFT_NORMALISED
    bank2.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_NORMALISED, 64.0))
    bank2.close()
    ctx.close()


def test_1024_streams_in_two_lanes_equal_the_small_bank(oracle):
    """from 1024 streams a mode I bank runs the halves of its streams on two HIP streams: one call, four distinct captures 256 times each
    -- rows compared among equals and with a 4-stream bank, which is held to the model"""
    import dabgpu
    import torch
    fmt, n, raw, iq = raw_inputs(oracle, "raw_u8", streams=[0, 1, SSM.MOVING, SSM.NOISE])
    N, m, slots = 1024, 300000, 3
    ref = [SSM.run_model(oracle, ("raw_u8", "lanes", e), iq[e][:m], m) for e in range(4)]
    ctx = dabgpu.Context(0)
    d_small = torch.from_numpy(raw[:, :2 * m]).cuda()
    d_big = d_small.repeat(N // 4, 1).contiguous()                            # stream s = capture s mod 4
    out = {}
    for E, d in ((4, d_small), (N, d_big)):
        bank = dabgpu.StreamBank(ctx, E)
        scale = torch.full((E * slots,), float("nan"), dtype=torch.float32, device="cuda")
        bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0), scale)
        bits = torch.zeros((E, slots, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
        nf = torch.zeros(E, dtype=torch.int32, device="cuda")
        bank.process_raw(d, fmt, m, m, bits, slots, nf)
        torch.cuda.synchronize()
        out[E] = (bits, nf.cpu().numpy(), bits32(scale.cpu().numpy()).reshape(E, slots), bank.status())
        bank.close()
    b4, n4, s4, st4 = out[4]
    bN, nN, sN, stN = out[N]
    assert np.array_equal(nN, np.tile(n4, N // 4)) and np.array_equal(sN, np.tile(s4, (N // 4, 1)))
    assert torch.equal(bN.view(N // 4, 4, -1), b4.view(1, 4, -1).expand(N // 4, -1, -1))
    for f in st4.dtype.names:
        x, y = (s[f].view(np.uint32) if s[f].dtype == np.float32 else s[f] for s in (st4, stN))
        assert np.array_equal(np.tile(x, N // 4), y), f
    frames = 0
    for e in range(4):
        new = ref[e][0][0]
        assert n4[e] == len(new)
        for j, fr in enumerate(new):
            kk, exp = ref[e][1].weighted(fr)
            assert np.array_equal(b4[e, j].cpu().numpy(), exp) and s4[e, j] == bits32(kk)
            frames += 1
    assert frames >= 3
    ctx.close()
