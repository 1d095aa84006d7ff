"""-m gpu: the stream bank's DQPSK products and sync records per frame (dabgpu_stream_bank_set_products).  A weighted bank with products
writes, for every frame it completes in a frames-form call, the frame's products [75][1536] and a dabgpu_sync_state record at the
frame's bits slot.  Expected side: tests/stream_soft_model.py -- fr["dq"] (the oracle's transform of the frame the state machine
assembled, at the frequency word the demodulator used), fr["offset"], fr["coarse"], fr["freq"], and the model's scale and weighted
bits.  Every comparison is of bit patterns.  Beside the bank runs a twin: the same weighted bank without products, fed the same blocks,
whose bits, scale words, frame counts and status must be the bank's after every call.

A frame beyond the caller's capacity (it would land in the last slot) cannot be produced through the entry points: a call is refused
unless max_frames_per_stream >= n_samples / 191400 + 2, and a stream completes at most n_samples / 196608 + 1 frames in a call, so the
last two slots are never reached.  The block of 500000 samples with 4 slots is the fullest call there is (3 frames); it is checked
like every other: products, record, scale and bits of a slot belong to the same frame."""
import numpy as np
import pytest

import stream_soft_model as SSM
from test_gpu_stream_bank_soft import NAN_WORD, assert_both_symbol0_placements, assert_status_equal, bits32, raw_inputs

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_UNSUPPORTED = 2, 5
PER_FRAME = 75 * 1536
GARBAGE = 0x5A5A5A5A


def words(x):
    """complex64 / float32 array -> its uint32 words, flat"""
    return np.ascontiguousarray(x).view(np.uint32).reshape(-1)


class Bank:
    """a weighted bank with a scale buffer and, with products=True, product and record buffers of E * slots frames"""

    def __init__(self, ctx, E, slots, products=True, level=64.0):
        import dabgpu
        import torch
        self.dabgpu, self.torch, self.E, self.slots, self.level = dabgpu, torch, E, slots, level
        self.bank = dabgpu.StreamBank(ctx, E)
        self.scale = torch.full((E * slots,), float("nan"), dtype=torch.float32, device="cuda")
        self.bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, level), self.scale)
        self.bits = torch.zeros((E, slots, dabgpu.NB_FRAME_BITS), dtype=torch.int8, device="cuda")
        self.nf = torch.full((E,), -7, dtype=torch.int32, device="cuda")
        self.dq = self.rec = None
        if products:
            self.dq = torch.full((E * slots, 75, 1536, 2), float("nan"), dtype=torch.float32, device="cuda")
            self.rec = torch.full((E * slots, 6), GARBAGE, dtype=torch.int32, device="cuda")
            self.bank.set_products(self.dq, self.rec)

    def clear(self):
        self.bits.zero_()
        self.scale.fill_(float("nan"))
        if self.dq is not None:
            self.dq.fill_(float("nan"))
            self.rec.fill_(GARBAGE)                      # the call zeroes the records of all its slots itself

    def records(self):
        return self.rec.cpu().numpy().view(np.dtype(self.dabgpu.SYNC_STATE_DTYPE)).reshape(self.E, self.slots)

    def untouched_products(self, slot):
        return bool((self.dq[slot].view(self.torch.int32) == NAN_WORD).all().item())

    def close(self):
        self.bank.close()


def assert_twins_equal(a, b, where):
    """bits, scale words, frame counts and every status field of two banks"""
    a.torch.cuda.synchronize()
    assert a.torch.equal(a.nf, b.nf), (where, a.nf.tolist(), b.nf.tolist())
    assert a.torch.equal(a.bits, b.bits), where
    assert np.array_equal(bits32(a.scale.cpu().numpy()), bits32(b.scale.cpu().numpy())), where
    assert_status_equal(a.bank.status(), b.bank.status(), where)


def check_record(rec, fr, where):
    assert rec["sync_valid"] == 1 and rec["reserved"] == 0, (where, rec)
    assert rec["fine_time_offset"] == fr["offset"], (where, rec, fr["offset"])
    assert bits32(rec["freq_coarse"]) == bits32(fr["coarse"]), (where, rec, fr["coarse"])
    assert bits32(np.float32(rec["freq_coarse"]) + np.float32(rec["freq_fine"])) == bits32(fr["freq"]), (where, rec, fr["freq"])


def check_call(b, refs, models, ci, where, seen):
    """every slot of the call: a completed frame has the model's products, record, scale and weighted bits; a slot without a frame has a
    zero record and the products it had"""
    nf = b.nf.cpu().numpy()
    rec = b.records()
    scale = bits32(b.scale.cpu().numpy()).reshape(b.E, b.slots)
    for e in range(b.E):
        new = refs[e][ci]
        assert nf[e] == len(new), (where, e, nf[e], len(new))
        for j, fr in enumerate(new):
            got = b.dq[e * b.slots + j].cpu().numpy()
            assert np.array_equal(words(got), words(fr["dq"].astype(np.complex64, copy=False))), (where, e, j, "products")
            check_record(rec[e, j], fr, (where, e, j))
            k, exp = models[e].weighted(fr, b.level)
            assert np.array_equal(b.bits[e, j].cpu().numpy(), exp) and scale[e, j] == bits32(k), (where, e, j, "bits and scale of the same frame")
            seen.append(fr["offset"])
        for j in range(len(new), b.slots):
            assert not np.frombuffer(rec[e, j].tobytes(), np.uint8).any(), (where, e, j, "record of a slot without a frame")
            assert b.untouched_products(e * b.slots + j), (where, e, j, "products of a slot without a frame")
            assert scale[e, j] == NAN_WORD


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("block", [65536, 10007, 500000])
def test_float_blocks_equal_the_model_and_the_twin(oracle, ctx, block):
    import torch
    S = SSM.float_streams(oracle)
    E, n = S.shape
    ref = [SSM.run_model(oracle, ("float", e), S[e], block) for e in range(E)]
    refs, models = [r[0] for r in ref], [r[1] for r in ref]
    slots = block // 191400 + 2
    b, twin = Bank(ctx, E, slots), Bank(ctx, E, slots, products=False)
    assert b.bank.get_products()[2] == E * slots and twin.bank.get_products() == (None, None, 0)
    seen = []
    for ci, k in enumerate(range(0, n, block)):
        m = min(block, n - k)
        d_iq = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(S[:, k:k + m])).cuda())
        b.clear(); twin.clear()
        b.bank.process(d_iq, m, m, b.bits, slots, b.nf)
        twin.bank.process(d_iq, m, m, twin.bits, slots, twin.nf)
        assert_twins_equal(b, twin, (block, k))
        check_call(b, refs, models, ci, (block, k), seen)
    assert len(models[SSM.NOISE].out_frames) == 0 and len(seen) >= 13          # the noise-only stream wrote nothing (checked per call)
    assert_both_symbol0_placements(seen)
    b.close(); twin.close()


@pytest.mark.parametrize("name", ["raw_u8", "raw_s8", "raw_s16l", "raw_u16l"])
def test_capture_formats_fused_loaders_and_a_converted_one(oracle, ctx, name):
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
    b, twin = Bank(ctx, E, slots), Bank(ctx, E, slots, products=False)
    seen = []
    for ci, k in enumerate(range(0, n, block)):
        m = min(block, n - k)
        b.clear(); twin.clear()
        b.bank.process_raw(d_raw[:, sb * k:].data_ptr(), fmt, n, m, b.bits, slots, b.nf)
        twin.bank.process_raw(d_raw[:, sb * k:].data_ptr(), fmt, n, m, twin.bits, slots, twin.nf)
        assert_twins_equal(b, twin, (name, k))
        check_call(b, refs, models, ci, (name, k), seen)
    assert len(seen) >= 6
    assert_both_symbol0_placements(seen)
    b.close(); twin.close()


@pytest.mark.parametrize("name", ["raw_u8", "raw_f32l"])
def test_retained_blocks_equal_the_copying_form(oracle, ctx, name):
    """dabgpu_stream_bank_process_retained with products: a frame lies in the frame buffer, the previous block and the current block.
    Products, records, bits, scale words and status equal the copying form's (itself held to the model), then a release and one more call"""
    import dabgpu
    import torch
    fmt, n, raw, iq = raw_inputs(oracle, name)
    E, block = len(iq), 250001
    sb = dabgpu.iq_format_sample_bytes(fmt)
    ref = [SSM.run_model(oracle, (name, e), iq[e], block) for e in range(E)]
    refs, models = [r[0] for r in ref], [r[1] for r in ref]
    slots = block // 191400 + 2
    copy, kept = Bank(ctx, E, slots), Bank(ctx, E, slots)
    bufs = [torch.zeros((E, block * sb), dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_raw = torch.from_numpy(raw).cuda()
    prev, seen = None, []

    def same_products(where):
        assert torch.equal(copy.dq.view(torch.int32), kept.dq.view(torch.int32)) and torch.equal(copy.rec, kept.rec), where

    for ci, k in enumerate(range(0, n, block)):
        m = min(block, n - k)
        cur = bufs[1 + ci % 2]                                                   # the retained bank's two alternating buffers
        cur[:, :m * sb] = d_raw[:, k * sb:(k + m) * sb]
        bufs[0][:, :m * sb] = cur[:, :m * sb]
        copy.clear(); kept.clear()
        copy.bank.process_raw(bufs[0], fmt, block, m, copy.bits, slots, copy.nf)
        kept.bank.process_retained(cur, fmt, block, m, prev, kept.bits, slots, kept.nf)
        torch.cuda.synchronize()
        bufs[0].fill_(7)                                                         # the copying bank's block is free to go
        assert_twins_equal(copy, kept, (name, k))
        same_products((name, k))
        check_call(kept, refs, models, ci, (name, k), seen)
        prev = cur
    assert len(seen) >= 6
    kept.bank.release(prev, fmt, block)
    m = 250000
    for x in (copy, kept):
        bufs[0][:, :m * sb] = d_raw[:, :m * sb]
        x.clear()
        x.bank.process_raw(bufs[0], fmt, block, m, x.bits, slots, x.nf)
    assert_twins_equal(copy, kept, (name, "after the release"))
    same_products((name, "after the release"))
    copy.close(); kept.close()


def test_consumers_take_the_three_arrays_as_they_stand(oracle, ctx):
    """products + scale + records are a diversity branch: the one-branch combination reproduces the bank's own bits in every slot with a
    frame and writes zeros in the others; the estimators over (products, records) equal their host forms on the model's products, and
    report valid = 0 for slots without a frame"""
    import torch
    S = SSM.float_streams(oracle)
    E, n = S.shape
    block = 500000
    ref = [SSM.run_model(oracle, ("float", e), S[e], block) for e in range(E)]
    refs = [r[0] for r in ref]
    slots = block // 191400 + 2
    N = E * slots
    b = Bank(ctx, E, slots)
    own = torch.zeros_like(b.bits)
    slope = torch.zeros(N, dtype=torch.int64, device="cuda")
    corr = torch.zeros((N, 2), dtype=torch.float32, device="cuda")
    sym_w = torch.zeros((N, 75), dtype=torch.float32, device="cuda")
    band_w = torch.zeros((N, 128), dtype=torch.float32, device="cuda")
    mean = torch.zeros(N, dtype=torch.float32, device="cuda")
    ok = [torch.zeros(N, dtype=torch.int32, device="cuda") for _ in range(3)]
    frames = 0
    for ci, k in enumerate(range(0, n, block)):
        m = min(block, n - k)
        d_iq = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(S[:, k:k + m])).cuda())
        b.clear()
        b.bank.process(d_iq, m, m, b.bits, slots, b.nf)
        own.fill_(9)
        ctx.diversity_combine([(b.dq, b.scale, None, b.rec)], N, own)
        ctx.clock_estimate(b.dq, N, sync=b.rec, slope_in=None, gain=1.0, slope_out=slope, corr=corr, valid=ok[0])
        ctx.sym_profile(b.dq, N, sync=b.rec, symbol_weight=sym_w, valid=ok[1])
        ctx.dd_profile(b.dq, N, sync=b.rec, band_weight=band_w, mean_noise=mean, valid=ok[2])
        torch.cuda.synchronize()
        valid = [o.cpu().numpy().reshape(E, slots) for o in ok]
        for e in range(E):
            new = refs[e][ci]
            assert int(b.nf[e]) == len(new)
            for j in range(slots):
                s = e * slots + j
                if j >= len(new):
                    assert not own[e, j].any().item() and all(v[e, j] == 0 for v in valid), (k, e, j)
                    continue
                dq = new[j]["dq"].astype(np.complex64, copy=False)
                assert torch.equal(own[e, j], b.bits[e, j]), (k, e, j, "the combiner's bits are the bank's")
                _, hs, hcorr, hok = ctx.clock_track_host(dq, 0, 1.0, derotate=False)
                assert (int(slope[s]), int(valid[0][e, j])) == (hs, hok) and corr[s].cpu().numpy().tobytes() == hcorr.tobytes(), (k, e, j)
                hv, _, _, hok = ctx.sym_profile_host(dq)
                assert valid[1][e, j] == hok and np.array_equal(words(sym_w[s].cpu().numpy()), words(hv)), (k, e, j)
                hbw, hmean, hok = ctx.dd_profile_host(dq)
                assert valid[2][e, j] == hok and np.array_equal(words(band_w[s].cpu().numpy()), words(hbw)), (k, e, j)
                assert bits32(mean[s].item()) == bits32(hmean), (k, e, j)
                frames += 1
    assert frames >= 13
    b.close()


def test_1024_streams_in_two_lanes_equal_the_small_bank(oracle, ctx):
    """from 1024 streams a mode I bank runs the halves of its streams on two HIP streams, both writing global slots: one call, four
    distinct captures 256 times each -- rows compared among equals and with a 4-stream bank, which is held to the model"""
    import torch
    fmt, n, raw, iq = raw_inputs(oracle, "raw_u8", streams=[0, 1, SSM.MOVING, SSM.NOISE])
    N, m, slots = 1024, 300000, 3
    ref = [SSM.run_model(oracle, ("raw_u8", "lanes", e), iq[e][:m], m) for e in range(4)]
    d_small = torch.from_numpy(raw[:, :2 * m]).cuda()
    d_big = d_small.repeat(N // 4, 1).contiguous()                            # stream s = capture s mod 4
    small = Bank(ctx, 4, slots)
    small.bank.process_raw(d_small, fmt, m, m, small.bits, slots, small.nf)
    torch.cuda.synchronize()
    seen = []
    check_call(small, [r[0] for r in ref], [r[1] for r in ref], 0, "4 streams", seen)
    assert len(seen) >= 3
    big = Bank(ctx, N, slots)
    big.bank.process_raw(d_big, fmt, m, m, big.bits, slots, big.nf)
    torch.cuda.synchronize()
    R = N // 4

    def tiled(x4, xN):                                                        # [4 * slots, ...] against [N * slots, ...]: row of stream s = row of s mod 4
        a = x4.reshape(1, 4 * slots, -1).expand(R, -1, -1)
        return torch.equal(xN.reshape(R, 4 * slots, -1), a)

    assert tiled(small.nf.repeat_interleave(slots), big.nf.repeat_interleave(slots))
    assert tiled(small.bits, big.bits) and tiled(small.rec, big.rec)
    assert tiled(small.scale.view(torch.int32), big.scale.view(torch.int32))
    assert tiled(small.dq.view(torch.int32), big.dq.view(torch.int32))
    st4, stN = small.bank.status(), big.bank.status()
    for f in st4.dtype.names:
        x, y = (s[f].view(np.uint32) if s[f].dtype == np.float32 else s[f] for s in (st4, stN))
        assert np.array_equal(np.tile(x, R), y), f
    small.close(); big.close()


def test_refusals_touch_nothing_and_switching_off_restores_every_call(oracle, ctx):
    import dabgpu
    import torch
    L = dabgpu.lib()
    E, slots, m = 2, 3, 300000
    b = Bank(ctx, E, slots)
    bank = b.bank
    d_iq = torch.zeros((E, m, 2), dtype=torch.float32, device="cuda")
    b.bits.fill_(3)
    hist = torch.full((E, 5, dabgpu.NB_FRAME_BITS), 3, dtype=torch.int8, device="cuda")
    f32l, u16l = dabgpu.IQ_FORMATS.index("raw_f32l"), dabgpu.IQ_FORMATS.index("raw_u16l")
    before = bank.status().copy()

    def frames_forms_refused(text):
        with pytest.raises(dabgpu.DabGpuError, match=text):
            bank.process(d_iq, m, m, b.bits, slots, b.nf)
        with pytest.raises(dabgpu.DabGpuError, match=text):            # the converted path: before its conversion pass
            bank.process_raw(d_iq.view(torch.uint8), u16l, m, m, b.bits, slots, b.nf)
        with pytest.raises(dabgpu.DabGpuError, match=text):
            bank.process_retained(d_iq, f32l, m, m, None, b.bits, slots, b.nf)

    # capacity one slot short
    bank.set_products(b.dq[:E * slots - 1], b.rec[:E * slots - 1])
    assert bank.get_products()[2] == E * slots - 1
    frames_forms_refused("product frames")
    bank.set_products(b.dq, b.rec)
    # the ring forms
    for call in (lambda: bank.process_ring(d_iq, f32l, m, 100000, hist, 5, b.nf),
                 lambda: bank.process_ring(d_iq, f32l, m, 100000, hist, 5, b.nf, bits_layout=dabgpu.BITS_MSC_CLASSED),
                 lambda: bank.process_ring_retained(d_iq, f32l, m, 100000, None, hist, 5, b.nf)):
        with pytest.raises(dabgpu.DabGpuError, match="ring forms"):
            call()
    assert L.dabgpu_stream_bank_process_ring(bank._h, dabgpu._ptr(d_iq), f32l, m, 100000, dabgpu._ptr(hist), 5, dabgpu._ptr(b.nf), None) == ERR_UNSUPPORTED
    # the normalised policy; no scale buffer
    bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_NORMALISED, 64.0), b.scale)
    frames_forms_refused("DABGPU_SOFT_CSI")
    bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0))
    frames_forms_refused("scale buffer")
    bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0), b.scale)
    # misaligned buffers, only one of the two pointers: refused, the bank keeps what it had
    p_dq, p_rec = b.dq.data_ptr(), b.rec.data_ptr()
    for dq, rec, text in ((p_dq + 8, p_rec, "misaligned"), (p_dq, p_rec + 2, "misaligned"), (p_dq, None, "both"), (None, p_rec, "both")):
        st = L.dabgpu_stream_bank_set_products(bank._h, dabgpu._ptr(dq), dabgpu._ptr(rec), E * slots)
        assert st == ERR_INVALID_ARG and text.encode() in L.dabgpu_last_error(), (dq, rec, text)
        assert bank.get_products()[2] == E * slots and bank.get_products()[0] is b.dq
    torch.cuda.synchronize()
    # nothing was launched or converted: no output touched, the state did not move
    assert (b.bits == 3).all().item() and (hist == 3).all().item() and (b.nf == -7).all().item()
    assert (b.rec == GARBAGE).all().item() and all(b.untouched_products(s) for s in range(E * slots))
    assert np.all(bits32(b.scale.cpu().numpy()) == NAN_WORD)
    assert_status_equal(before, bank.status(), "refused calls")
    # a bank of another transmission mode: unsupported, it stays off
    bank2 = dabgpu.StreamBank(ctx, 1, mode=2)
    st = L.dabgpu_stream_bank_set_products(bank2._h, dabgpu._ptr(p_dq), dabgpu._ptr(p_rec), 1)
    assert st == ERR_UNSUPPORTED and b"mode" in L.dabgpu_last_error() and bank2.get_products() == (None, None, 0)
    bank2.set_products(None, None)
    bank2.close()
    # switched off, every call is what it was: the ring forms, the normalised policy, no scale buffer
    bank.set_products(None, None)
    assert bank.get_products() == (None, None, 0)
    bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0))
    bank.process_ring(d_iq, f32l, m, 100000, hist, 5, b.nf)
    bank.process(d_iq, m, m, b.bits, slots, b.nf)
    bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_NORMALISED, 64.0), b.scale)
    bank.process_raw(d_iq.view(torch.uint8), u16l, m, m, b.bits, slots, b.nf)
    torch.cuda.synchronize()
    assert (b.rec == GARBAGE).all().item(), "a bank without products writes no record"
    b.close()


def test_the_setting_survives_a_reset(oracle, ctx):
    import torch
    S = SSM.float_streams(oracle)[[1, SSM.MOVING]]
    block = 500000
    ref = [SSM.run_model(oracle, ("float", e), SSM.float_streams(oracle)[e], block) for e in (1, SSM.MOVING)]
    refs, models = [r[0] for r in ref], [r[1] for r in ref]
    slots = block // 191400 + 2
    b = Bank(ctx, 2, slots)
    d_iq = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(S[:, :block])).cuda())
    for again in (False, True):
        if again:
            b.bank.reset()
            got = b.bank.get_products()
            assert got[0] is b.dq and got[1] is b.rec and got[2] == 2 * slots
        b.clear()
        b.bank.process(d_iq, block, block, b.bits, slots, b.nf)
        b.torch.cuda.synchronize()
        seen = []
        check_call(b, refs, models, 0, ("reset", again), seen)
        assert len(seen) >= 4
    b.close()
