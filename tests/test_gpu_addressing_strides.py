"""-m gpu: strides and offsets that put the second unit (frame, ensemble, stream) past 4 GiB.  Every case has two units with different
inputs; the stride is the smallest the entry point's alignment rule allows that is >= 2^32 bytes.  Expected: the same call with the
packed stride on the same two inputs (which the other test files hold to the oracle and the models), and unit 1 against the oracle or
the host model directly where that costs little.  Buffers are tests/big_buffers.py's: untouched but for the named regions, canaries
around every output region; where the stride is exactly 2^32 a write that wrapped lands on unit 0's output and shows there.

Frame-indexed buffers have no stride: there the smallest shape that crosses is a frame count, the input is random bytes made on the
device and the last four frames must equal a four-frame call on those frames."""
import numpy as np
import pytest

import ber_model as BM
import big_buffers as BB
import blanker_model as BLM
import channel_model as CM
import channelise_model as CSM
import interferer_model as IM
import iqbal_model as QM
import resample_model as RM

pytestmark = pytest.mark.gpu

NB = 230400
S32 = 1 << 32
FRAME_SAMPLES = 196608


@pytest.fixture(scope="module")
def ctx():
    import dabgpu
    c = dabgpu.Context(0)
    yield c
    c.viterbi_set_mapping(0)
    c.close()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def noisy(oracle, bits01, rng, gain=0.45, sigma=30.0):
    s = oracle.soft_from_bits(bits01).astype(np.float32) * gain + rng.standard_normal(len(bits01)) * sigma
    return np.clip(np.rint(s), -127, 127).astype(np.int8)


def two_units(rows, stride, lead=BB.LEAD):
    """rows [2][n] (any dtype) -> a view whose unit 1 starts `stride` bytes behind unit 0"""
    rows = [np.ascontiguousarray(r).view(np.uint8).reshape(-1) for r in rows]
    view = BB.big(stride + rows[1].size + BB.CANARY_BYTES, lead=lead)          # room for a canary behind unit 1
    BB.put(view, 0, rows[0])
    BB.put(view, stride, rows[1])
    return view


def two_outputs(n_bytes, stride, fill=0x5A):
    """(view, canaries): two output regions of n_bytes, `stride` apart, filled with a pattern no result consists of"""
    view = BB.big(stride + n_bytes + BB.CANARY_BYTES)
    can = BB.Canaries()
    can.at(view, -BB.CANARY_BYTES)
    if stride % BB.WRAP >= n_bytes + BB.CANARY_BYTES:
        can.at(view, n_bytes)
        can.wrapped(view, stride)
    can.around(view, stride, n_bytes)
    BB.region(view, 0, n_bytes).fill_(fill)
    BB.region(view, stride, n_bytes).fill_(fill)
    return view, can


def units(view, stride, n_bytes):
    import torch
    return torch.stack([BB.region(view, 0, n_bytes), BB.region(view, stride, n_bytes)])


# ---- decoders ----

def test_fic_decode_frames_frame_stride(ctx, oracle):
    import dabgpu
    import torch
    rng = np.random.default_rng(9100)
    frames = rng.integers(-127, 128, (2, NB), dtype=np.int8)
    for f in range(2):
        for g in range(4):
            frames[f, 2304 * g:2304 * (g + 1)] = noisy(oracle, oracle.fic_encode_group(rng.integers(0, 256, 90, dtype=np.uint8)), rng, sigma=[0.0, 20.0, 35.0, 60.0][g] + 1e-3)
    view = two_units(frames, S32, lead=0)
    d_packed = torch.from_numpy(frames).cuda()
    rdt = np.dtype(dabgpu.RESULT_DTYPE)
    for m in (1, 2, 3, 0):
        ctx.viterbi_set_mapping(m)
        got = []
        for bits, stride in ((view, S32), (d_packed, NB)):
            d_out = torch.full((2, 4, 96), 0xC3, dtype=torch.uint8, device="cuda")
            d_res = torch.zeros((8, 16), dtype=torch.uint8, device="cuda")
            ctx.fic_decode_frames(bits, 2, d_out, d_res, frame_stride=stride)
            torch.cuda.synchronize()
            got.append((d_out.cpu().numpy(), d_res.cpu().numpy().view(rdt).reshape(2, 4)))
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), m
        for g in range(4):                                               # unit 1 against the oracle
            eb, em, ee = oracle.fic_decode_group(frames[1, 2304 * g:2304 * (g + 1)], 0)
            r = got[0][1][1, g]
            assert np.array_equal(got[0][0][1, g], eb) and int(r["crc_ok_mask"]) == em and int(r["path_error"]) == ee, (m, g)
    ctx.viterbi_set_mapping(0)
    assert not np.array_equal(got[0][0][0], got[0][0][1])
    del view
    BB.release()


@pytest.mark.parametrize("layout", [0, 1], ids=["natural", "classed"])
def test_decode_calls_and_ber_with_ensemble_strides(ctx, oracle, layout):
    """msc_decode_frames, msc_decode_ring, decode_frames and ber_frames: two ensembles, ring and output rows 2^32 bytes apart"""
    import dabgpu
    import torch
    rng = np.random.default_rng(9200 + layout)
    H, newest = 5, 3
    subs = [oracle.subchannel(3, 6, eep_level=2, eep_type=0), oracle.subchannel(100, 35, is_uep=True, uep_index=4), oracle.subchannel(800, 64, eep_level=3, eep_type=0)]
    gsubs = [dabgpu.SubChannel(s.start_address, s.length, s.is_uep, s.uep_prot_index, s.eep_prot_level, s.eep_type) for s in subs]
    n_sub = len(subs)
    cif_out = sum(oracle.subchannel_plan(s)[2] for s in subs)
    rings = rng.integers(-127, 128, (2, H, NB), dtype=np.int8)           # natural order
    for e in range(2):
        for g in range(4):
            rings[e, newest, 2304 * g:2304 * (g + 1)] = noisy(oracle, oracle.fic_encode_group(rng.integers(0, 256, 90, dtype=np.uint8)), rng)
    dev = np.stack([BM.to_classed(r) for r in rings]) if layout else rings
    ring_view = two_units(dev.reshape(2, -1), S32, lead=0)
    d_packed = torch.from_numpy(np.ascontiguousarray(dev)).cuda()
    rdt = np.dtype(dabgpu.RESULT_DTYPE)
    d_slots = torch.tensor([newest, newest], dtype=torch.int32, device="cuda")
    out_view, can = two_outputs(4 * cif_out, S32)

    def run(form, far):
        """one call, far: the 2^32 strides -> (msc bytes [2][4 cif_out], msc records, fib bytes or None, fic records or None)"""
        hist, ens_stride = (ring_view, S32) if far else (d_packed, H * NB)
        d_res = torch.zeros((2 * 4 * n_sub, 16), dtype=torch.uint8, device="cuda")
        d_fib = torch.full((2, 4, 96), 0xC3, dtype=torch.uint8, device="cuda")
        d_fres = torch.zeros((8, 16), dtype=torch.uint8, device="cuda")
        if far:
            BB.region(out_view, 0, 4 * cif_out).fill_(0x5A)
            BB.region(out_view, S32, 4 * cif_out).fill_(0x5A)
            out, out_stride = out_view, S32
        else:
            out, out_stride = torch.full((2, 4 * cif_out), 0x5A, dtype=torch.uint8, device="cuda"), 4 * cif_out
        if form == "msc_frames":
            ctx.msc_decode_frames(hist, 2, ens_stride, H, newest, gsubs, out, out_stride, d_res, bits_layout=layout)
        elif form == "msc_ring":
            ctx.msc_decode_ring(hist, 2, ens_stride, H, d_slots, gsubs, out, out_stride, d_res, bits_layout=layout)
        else:
            ctx.decode_frames(hist, 2, ens_stride, H, newest, gsubs, d_fib, d_fres, out, out_stride, d_res, bits_layout=layout)
        torch.cuda.synchronize()
        got = units(out_view, S32, 4 * cif_out) if far else out
        return got.cpu().numpy(), d_res.cpu().numpy().view(rdt), d_fib.cpu().numpy(), d_fres.cpu().numpy().view(rdt)

    last = None
    for m in (0, 1, 2, 3):
        ctx.viterbi_set_mapping(m)
        for form in ("msc_frames", "msc_ring", "decode_frames"):
            far, near = run(form, True), run(form, False)
            can.check()
            for a, b in zip(far[:2] if form != "decode_frames" else far, near):
                assert np.array_equal(a, b), (m, form)
            assert not np.array_equal(far[0][0], far[0][1]) and (far[1]["n_out_bytes"] > 0).all()
            last = far
    ctx.viterbi_set_mapping(0)
    msc_bytes, fib = last[0], last[2]
    for g in range(4):                                                   # unit 1's FIB groups against the oracle
        assert np.array_equal(fib[1, g], oracle.fic_decode_group(rings[1, newest, 2304 * g:2304 * (g + 1)], 0)[0])

    # channel BER over the same buffers: the decoded bytes as they lie in the far output rows
    bdt = np.dtype(dabgpu.BER_RESULT_DTYPE)
    d_fib = torch.from_numpy(fib).cuda()
    got = []
    for far in (True, False):
        fic_r = torch.full((2 * 4 * bdt.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        msc_r = torch.full((2 * 4 * n_sub * bdt.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        if far:
            ctx.ber_frames(ring_view, 2, S32, H, newest, gsubs, d_fib, out_view, S32, fic_r, msc_r, bits_layout=layout)
        else:
            ctx.ber_frames(d_packed, 2, H * NB, H, newest, gsubs, d_fib, torch.from_numpy(msc_bytes).cuda(), 4 * cif_out, fic_r, msc_r, bits_layout=layout)
        torch.cuda.synchronize()
        got.append((fic_r.cpu().numpy().view(bdt).reshape(2, 4), msc_r.cpu().numpy().view(bdt).reshape(2, 4, n_sub)))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    exp_fic, exp_msc = BM.ber_frames(oracle, rings[1], newest, subs, fib[1], msc_bytes[1].reshape(4, cif_out))
    assert np.array_equal(got[0][0][1], exp_fic) and np.array_equal(got[0][1][1], exp_msc)
    can.check()
    del ring_view, out_view, can
    BB.release()


# ---- demodulator forms with bits_frame_stride ----

@pytest.mark.parametrize("form", ["plain", "raw", "history-natural", "history-classed", "phase"])
def test_demodulator_bits_frame_stride(ctx, form):
    import dabgpu
    import torch
    g = torch.Generator(device="cuda").manual_seed(9300)
    u8 = dabgpu.IQ_FORMATS.index("raw_u8")
    raw = torch.randint(0, 256, (2, FRAME_SAMPLES * 2), dtype=torch.uint8, device="cuda", generator=g)
    iq = torch.randn((2, FRAME_SAMPLES, 2), dtype=torch.float32, device="cuda", generator=g)
    view, can = two_outputs(NB, S32)
    packed = torch.full((2, NB), 0x5A, dtype=torch.uint8, device="cuda")
    extra = []
    for bits, stride in ((view, S32), (packed, 0)):
        corr = torch.zeros((2, 76, 2), dtype=torch.float32, device="cuda")
        if form == "plain":
            ctx.ofdm_demod_frames(iq, bits, cp_corr=corr, n_frames=2, bits_frame_stride=stride)
        elif form == "raw":
            ctx.ofdm_demod_frames_raw(raw, u8, 2, bits, cp_corr=corr, bits_frame_stride=stride)
        elif form.startswith("history"):
            ctx.ofdm_demod_frames_history(raw, u8, 2, bits, cp_corr=corr, bits_frame_stride=stride, bits_layout=int(form.endswith("classed")))
        else:
            total = torch.zeros((2,), dtype=torch.float32, device="cuda")
            fine = torch.zeros((2,), dtype=torch.float32, device="cuda")
            ctx.ofdm_demod_phase_frames(raw, u8, 2, bits, cp_corr=corr, bits_frame_stride=stride, beta=0.5, total_phase=total, fine_freq=fine)
            extra.append(torch.cat([total, fine]))
        extra.append(corr)
    torch.cuda.synchronize()
    can.check()
    far = units(view, S32, NB)
    assert torch.equal(far, packed)
    assert not torch.equal(far[0], far[1]) and not bool((far == 0x5A).all())
    half = len(extra) // 2
    for a, b in zip(extra[:half], extra[half:]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    del view, can
    BB.release()


# ---- the six signal-path banks: in_stride and out_stride of 2^29 + 1024 samples, 4096 samples per stream ----

STRIDE_S = (1 << 29) + 1024
STRIDE_B = 8 * STRIDE_S
N = 4096


def cplx(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def bank_far_and_near(call, x, n_out, in_place=False):
    """call(d_in, in_stride_samples, d_out, out_stride_bytes) twice: rows 2^32 + 8192 bytes apart, and packed -> ([rows][n_out] complex64 far,
    the same near); the caller rewinds the bank between the two through `call`"""
    import torch
    n_in = x.shape[-1]
    if in_place:
        view = two_units(x, STRIDE_B)
        can = BB.Canaries()
        can.around(view, STRIDE_B, 8 * n_in)
        can.at(view, -BB.CANARY_BYTES)
        can.at(view, 8 * n_in)
        call(view, STRIDE_S, view, STRIDE_B)
        d_near = torch.from_numpy(x).cuda()
        call(d_near, n_in, d_near, 8 * n_in)
        torch.cuda.synchronize()
        can.check()
        far = np.stack([BB.get(view, r * STRIDE_B, 8 * n_out, np.complex64) for r in range(2)])
        near = d_near.cpu().numpy()[:, :n_out]
        del view, can
    else:
        src = two_units(x, STRIDE_B, lead=0)
        view = BB.big(STRIDE_B + 8 * n_out + BB.CANARY_BYTES)
        can = BB.Canaries()
        for r in range(2):
            BB.region(view, r * STRIDE_B, 8 * n_out).fill_(0x5A)
            can.at(view, r * STRIDE_B - BB.CANARY_BYTES)
            can.at(view, r * STRIDE_B + 8 * n_out)
        d_x = torch.from_numpy(x).cuda()
        call(src, STRIDE_S, view, STRIDE_B)
        d_near = torch.zeros((2, n_out), dtype=torch.complex64, device="cuda")
        call(d_x, n_in, d_near, 8 * n_out)
        torch.cuda.synchronize()
        can.check()
        far = np.stack([BB.get(view, r * STRIDE_B, 8 * n_out, np.complex64) for r in range(2)])
        near = d_near.cpu().numpy()
        del view, can, src
    BB.release()
    return far, near


def test_channel_bank_strides(ctx, tmp_path_factory):
    import dabgpu
    host = CM.build_host_model(tmp_path_factory.mktemp("channel_host_model"))
    x = cplx(np.random.default_rng(9400), 2, N)
    plist = [CM.params_dict(taps=((0, 1.0, 0.0), (37, 0.4, -0.3)), freq_q64=1 << 50, seed=5, noise_sigma=0.1),
             CM.params_dict(taps=((3, 0.8, 0.1), (200, -0.2, 0.5)), freq_q64=(1 << 64) - (1 << 49), start=-5, seed=6, gain=1.1, noise_sigma=0.3)]
    ch = dabgpu.Channel(ctx, [CM.to_struct(P, dabgpu.ChannelStream) for P in plist])

    def call(d_in, in_stride, d_out, out_stride):
        ch.seek(0)
        ch.apply(d_in, N, N, d_out, in_stride_samples=in_stride, wrap=True, out_stride_bytes=out_stride)
    far, near = bank_far_and_near(call, x, N)
    assert same_bits(far, near)
    assert same_bits(far[1], CM.host_apply(host, plist, x, 0, N, True)[1])
    ch.close()


def test_interferer_bank_strides_in_place(ctx, tmp_path_factory):
    import dabgpu
    host = IM.build_host_model(tmp_path_factory.mktemp("interferer_host_model"))
    shapes = [dabgpu.interferer_design(96000.0 / 2048000.0)]
    ms = [IM.Shape.from_buffer_copy(bytes(H)) for H in shapes]
    x = cplx(np.random.default_rng(9410), 2, N)
    plist = [IM.stream([IM.source(IM.TONE, amp=0.7, freq_q64=1 << 57, phase0_q64=1 << 62), IM.source(IM.BAND, amp=0.5, shape=-1)], seed=11),
             IM.stream([IM.source(IM.BAND, amp=1.3, shape=0, freq_q64=1 << 61, gate_period=700, gate_on=450, gate_offset=-13)], seed=12)]
    bank = dabgpu.Interferer(ctx, [IM.to_struct(P, dabgpu.InterfererStream) for P in plist], shapes)

    def call(d_in, in_stride, d_out, out_stride):
        bank.seek(0)
        bank.apply(d_in, N, d_out, in_stride_samples=in_stride, out_stride_bytes=out_stride)
    far, near = bank_far_and_near(call, x, N, in_place=True)
    assert same_bits(far, near)
    assert same_bits(far[1], IM.host_apply(host, plist, ms, x, 0, N)[1])
    bank.close()


def test_blanker_bank_strides(ctx, tmp_path_factory):
    import dabgpu
    host = BLM.build_host_model(tmp_path_factory.mktemp("blanker_host_model"))
    rng = np.random.default_rng(9420)
    n_in = N + 4096                                                      # the detector's look-ahead is inside the input
    x = cplx(rng, 2, n_in)
    x[0, 1500:1530] *= 40.0
    x[1, 3000:3070] *= 40.0                                              # bursts for the detector to blank
    plist = [BLM.params(start=0), BLM.params(start=5, gap=32, window=32, guard=4, threshold=2.5)]
    bank = dabgpu.Blanker(ctx, [BLM.to_struct(P, dabgpu.BlankerStream) for P in plist])

    def call(d_in, in_stride, d_out, out_stride):
        bank.seek(0)
        bank.apply(d_in, n_in, N, d_out, in_stride_samples=in_stride, out_stride_bytes=out_stride)
    far, near = bank_far_and_near(call, x, N)
    assert same_bits(far, near)
    want = BLM.host_apply(host, plist, x, 0, N)[0]
    assert same_bits(far[1], want[1]) and (far[1] == 0).any() and (far[1] != 0).any(), "the burst of stream 1 must have been blanked"
    bank.close()


def test_resampler_bank_strides(ctx, tmp_path_factory):
    import dabgpu
    host = RM.build_host_model(tmp_path_factory.mktemp("resample_host_model"))
    D, G = RM.host_design(host, 2.0), dabgpu.resample_design(2.0)
    assert np.array_equal(np.ctypeslib.as_array(G.table), np.ctypeslib.as_array(D.table))
    x = cplx(np.random.default_rng(9430), 2, N)
    plist = [RM.params_dict(RM.ONE + (1 << 47), -30, 200 << 54), RM.params_dict(RM.step_q62(2.4e6, 2.048e6), 3, 1 << 39, gain=-0.5)]
    rs = dabgpu.Resampler(ctx, [RM.to_struct(P, dabgpu.ResampleStream) for P in plist], G)

    def call(d_in, in_stride, d_out, out_stride):
        rs.seek(0)
        rs.apply(d_in, N, N, d_out, in_stride_samples=in_stride, wrap=True, out_stride_bytes=out_stride)
    far, near = bank_far_and_near(call, x, N)
    assert same_bits(far, near)
    assert same_bits(far[1], RM.host_apply(host, plist, D, x, 0, N, True)[1])
    rs.close()


def test_channeliser_bank_strides(ctx, tmp_path_factory):
    """split: two wideband streams 2^32 + 8192 bytes apart in, a channel of each as far apart out"""
    import dabgpu
    host = CSM.build_host_model(tmp_path_factory.mktemp("channelise_host_model"))
    Dm = 4
    F, G = CSM.host_design(host, Dm), dabgpu.channeliser_design(Dm)
    assert np.array_equal(np.ctypeslib.as_array(G.table), np.ctypeslib.as_array(F.table))
    x = cplx(np.random.default_rng(9440), 2, N)
    n_out = N // Dm
    chs = [CSM.channel(1 << 60, 1 << 62, 1.0, 0), CSM.channel((1 << 64) - (1 << 61), 0, -0.5, 1)]
    cb = dabgpu.Channeliser(ctx, [CSM.to_struct(c, dabgpu.ChanneliserChannel) for c in chs], 2, G, 0)

    def call(d_in, in_stride, d_out, out_stride):
        cb.seek(0)
        cb.split(d_in, N, n_out, d_out, in_stride_samples=in_stride, wrap=True, out_stride_bytes=out_stride)
    far, near = bank_far_and_near(call, x, n_out)
    assert same_bits(far, near)
    assert same_bits(far[1], CSM.host_split(host, chs, F, x, 0, 0, n_out, True)[1])
    cb.close()


def test_iq_balance_bank_strides_in_place(ctx, tmp_path_factory):
    import dabgpu
    import torch
    host = QM.build_host_model(tmp_path_factory.mktemp("iqbal_host_model"))
    rng = np.random.default_rng(9450)
    x = np.stack([QM.impair(cplx(rng, N), 0.3 * k + 0.2, 2.0 * k - 3.0, 0.1 * k - 0.2j).astype(np.complex64) for k in range(2)])
    K1, K2 = QM.front_end(0.42, 3.0)
    plist = [QM.params(mode=QM.FIXED, a=K1, b=K2, c=0.3 + 0.2j), QM.params(min_weight=1024.0, forget=1.0)]
    bank = dabgpu.IqBalance(ctx, [QM.to_struct(P, dabgpu.IqBalanceStream) for P in plist], 65536)
    # records that make stream 1's map something else than the identity, then both calls from the same state
    bank.apply(torch.from_numpy(x).cuda(), N, None, flags=QM.MEASURE, in_stride_samples=N)
    rec = QM.host_records(host, 2)
    QM.host_apply(host, plist, rec, x, 0, N, QM.MEASURE)
    states = []

    def call(d_in, in_stride, d_out, out_stride):
        bank.seek(N)
        bank.apply(d_in, N, d_out, flags=QM.APPLY, in_stride_samples=in_stride, out_stride_bytes=out_stride)
        states.append(bank.read_state().tobytes())
    far, near = bank_far_and_near(call, x, N, in_place=True)
    assert same_bits(far, near) and states[0] == states[1]
    want, _, _ = QM.host_apply(host, plist, rec, x, N, N, QM.APPLY)
    assert same_bits(far[1], want[1]) and not same_bits(far[1], x[1])
    bank.close()


# ---- frame-indexed buffers: the frame count that crosses 2^32 bytes; the last four frames against a four-frame call ----

TAIL = 4
DQ_BYTES = 75 * 1536 * 8                                                 # one frame's DQPSK products


def test_float_input_past_4_gib(ctx):
    """2731 frames of complex float reach 2^32 bytes: 2736 frames in, the soft bits of the last four"""
    import torch
    n = 2736
    frame_bytes = FRAME_SAMPLES * 8
    assert (n - TAIL) * frame_bytes >= S32
    iq = BB.big(n * frame_bytes, lead=0).view(torch.float32)
    g = torch.Generator(device="cuda").manual_seed(9500)
    for a in range(0, iq.numel(), 1 << 28):
        iq[a:a + (1 << 28)].normal_(generator=g)
    bits = torch.full((n, NB), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.ofdm_demod_frames(iq, bits, n_frames=n)
    last = iq[(n - TAIL) * FRAME_SAMPLES * 2:]
    bits4 = torch.full((TAIL, NB), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.ofdm_demod_frames(last, bits4, n_frames=TAIL)
    torch.cuda.synchronize()
    assert torch.equal(bits[n - TAIL:], bits4)
    assert not torch.equal(bits4[0], bits4[1]) and not torch.equal(bits[0], bits4[0]) and not bool((bits4 == 0x5A).all())
    del iq, last, bits
    BB.release()


def test_fft_view_past_4_gib(ctx):
    """the FFT view is 77 x 2048 complex float per frame: 3405 frames reach 2^32 bytes, 3412 from raw_u8 input"""
    import dabgpu
    import torch
    n = 3412
    fft_bytes = 77 * 2048 * 8
    assert (n - TAIL) * fft_bytes >= S32
    u8 = dabgpu.IQ_FORMATS.index("raw_u8")
    g = torch.Generator(device="cuda").manual_seed(9510)
    raw = torch.empty((n, FRAME_SAMPLES * 2), dtype=torch.uint8, device="cuda").random_(0, 256, generator=g)
    fft = BB.big(n * fft_bytes + BB.CANARY_BYTES)
    can = BB.Canaries()
    can.at(fft, -BB.CANARY_BYTES)
    can.at(fft, n * fft_bytes)
    bits = torch.empty((n, NB), dtype=torch.uint8, device="cuda")
    ctx.ofdm_demod_frames_raw(raw, u8, n, bits, fft=fft)
    fft4 = torch.full((TAIL * fft_bytes,), 0x5A, dtype=torch.uint8, device="cuda")
    bits4 = torch.empty((TAIL, NB), dtype=torch.uint8, device="cuda")
    ctx.ofdm_demod_frames_raw(raw[n - TAIL:], u8, TAIL, bits4, fft=fft4)
    torch.cuda.synchronize()
    can.check()
    assert torch.equal(BB.region(fft, (n - TAIL) * fft_bytes, TAIL * fft_bytes), fft4) and torch.equal(bits[n - TAIL:], bits4)
    assert not torch.equal(BB.region(fft, (n - TAIL) * fft_bytes - BB.WRAP, TAIL * fft_bytes), fft4) and not bool((fft4 == 0x5A).all())
    del fft, can, raw, bits
    BB.release()


def test_products_past_4_gib_and_their_consumers(ctx):
    """921 600 bytes of DQPSK products per frame: 4664 frames from raw_u8 input put frame 4660 across 2^32 bytes and 4661 .. 4663 behind it.  Then every
    consumer of products over the whole buffer, its last four records against a call on a copy of those four frames: the
    decision-directed profile, the symbol profile, the clock estimator, the combiner, and the de-rotation in place"""
    import dabgpu
    import torch
    n = 4664
    assert (n - TAIL) * DQ_BYTES < S32 < (n - TAIL + 1) * DQ_BYTES      # frame 4660 straddles 2^32, 4661 .. 4663 lie behind it
    u8 = dabgpu.IQ_FORMATS.index("raw_u8")
    g = torch.Generator(device="cuda").manual_seed(9520)
    raw = torch.empty((n, FRAME_SAMPLES * 2), dtype=torch.uint8, device="cuda").random_(0, 256, generator=g)
    dq = BB.big(n * DQ_BYTES + BB.CANARY_BYTES)
    can = BB.Canaries()
    can.at(dq, -BB.CANARY_BYTES)
    can.at(dq, n * DQ_BYTES)
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    bits = torch.full((n, NB), 0x5A, dtype=torch.uint8, device="cuda")
    scale = torch.zeros((n,), dtype=torch.float32, device="cuda")
    ctx.ofdm_demod_frames_soft(raw, u8, n, bits, soft, dqpsk=dq, soft_scale=scale)
    dq4 = torch.full((TAIL * DQ_BYTES,), 0x5A, dtype=torch.uint8, device="cuda")
    bits4 = torch.full((TAIL, NB), 0x5A, dtype=torch.uint8, device="cuda")
    scale4 = torch.zeros((TAIL,), dtype=torch.float32, device="cuda")
    ctx.ofdm_demod_frames_soft(raw[n - TAIL:], u8, TAIL, bits4, soft, dqpsk=dq4, soft_scale=scale4)
    torch.cuda.synchronize()
    can.check()
    top = BB.region(dq, (n - TAIL) * DQ_BYTES, TAIL * DQ_BYTES)
    assert torch.equal(top, dq4) and torch.equal(bits[n - TAIL:], bits4) and torch.equal(scale[n - TAIL:].view(torch.int32), scale4.view(torch.int32))
    assert not torch.equal(BB.region(dq, (n - TAIL) * DQ_BYTES - BB.WRAP, TAIL * DQ_BYTES), dq4) and not bool((dq4 == 0x5A).all())
    del raw

    def outputs(k, shapes):
        return [torch.full((k,) + shp, fill, dtype=dt, device="cuda") for shp, dt, fill in shapes]

    def same_tail(big_outs, small_outs, shapes, what):
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(big_outs, small_outs)):
            assert torch.equal(a[n - TAIL:].contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), (what, i)
            assert not torch.equal(b, torch.full_like(b, shapes[i][2])), (what, i, "nothing was written")

    f32, i64, i32 = torch.float32, torch.int64, torch.int32
    dd = [((128,), f32, -1.0), ((128,), f32, -1.0), ((), f32, -1.0), ((), i32, -1)]
    A, B = outputs(n, dd), outputs(TAIL, dd)
    for d, k, o in ((dq, n, A), (dq4, TAIL, B)):
        ctx.dd_profile(d, k, profile_out=o[0], band_weight=o[1], mean_noise=o[2], valid=o[3])
    same_tail(A, B, dd, "dd_profile")
    sy = [((75,), f32, -1.0), ((75,), f32, -1.0), ((), f32, -1.0), ((), i32, -1)]
    A, B = outputs(n, sy), outputs(TAIL, sy)
    for d, k, o in ((dq, n, A), (dq4, TAIL, B)):
        ctx.sym_profile(d, k, symbol_weight=o[0], symbol_noise=o[1], ref_noise=o[2], valid=o[3])
    same_tail(A, B, sy, "sym_profile")
    ck = [((), i64, -1), ((), i64, -1), ((2,), f32, -1.0), ((), i32, -1)]
    A, B = outputs(n, ck), outputs(TAIL, ck)
    for d, k, o in ((dq, n, A), (dq4, TAIL, B)):
        ctx.clock_estimate(d, k, slope_out=o[0], residual=o[1], corr=o[2], valid=o[3])
    same_tail(A, B, ck, "clock_estimate")
    for layout in (0, 1):
        bits.fill_(0x5A)
        bits4.fill_(0x5A)
        ctx.diversity_combine([(dq, scale)], n, bits, bits_layout=layout)
        ctx.diversity_combine([(dq4, scale4)], TAIL, bits4, bits_layout=layout)
        same_tail([bits], [bits4], [((NB,), torch.uint8, 0x5A)], f"diversity_combine layout {layout}")
    # de-rotation in place, last: slopes of +-150 ppm and 0 (a copy) in the last frames
    slope = torch.zeros((n,), dtype=i64, device="cuda")
    slope[n - TAIL:] = torch.tensor([dabgpu.clock_slope_q64(150.0), 0, dabgpu.clock_slope_q64(-150.0), dabgpu.clock_slope_q64(37.0)], dtype=i64, device="cuda")
    out4 = torch.full((TAIL * DQ_BYTES,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.clock_derotate(dq4, out4, TAIL, slope[n - TAIL:].contiguous())
    ctx.clock_derotate(dq, dq, n, slope)
    torch.cuda.synchronize()
    can.check()
    assert torch.equal(top, out4) and not torch.equal(out4, dq4)
    assert torch.equal(out4[DQ_BYTES:2 * DQ_BYTES], dq4[DQ_BYTES:2 * DQ_BYTES])
    del dq, can, top, bits
    BB.release()


def test_modulator_float_output_past_4_gib(ctx):
    """ofdm_modulate_frames, mode I, complex float out: 2736 frames, the last four against a four-frame call on their payloads"""
    import torch
    n = 2736
    frame_bytes = FRAME_SAMPLES * 8
    assert (n - TAIL) * frame_bytes >= S32
    g = torch.Generator(device="cuda").manual_seed(9530)
    payload = torch.empty((n, 75 * 1536 // 4), dtype=torch.uint8, device="cuda").random_(0, 256, generator=g)
    out = BB.big(n * frame_bytes + BB.CANARY_BYTES)
    can = BB.Canaries()
    can.at(out, -BB.CANARY_BYTES)
    can.at(out, n * frame_bytes)
    ctx.ofdm_modulate_frames(1, payload, n, out)
    out4 = torch.full((TAIL * frame_bytes,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.ofdm_modulate_frames(1, payload[n - TAIL:], TAIL, out4)
    torch.cuda.synchronize()
    can.check()
    assert torch.equal(BB.region(out, (n - TAIL) * frame_bytes, TAIL * frame_bytes), out4) and not bool((out4 == 0x5A).all())
    assert not torch.equal(BB.region(out, (n - TAIL) * frame_bytes - BB.WRAP, TAIL * frame_bytes), out4)
    del out, can, payload
    BB.release()


def test_noise_profile_on_float_input_past_4_gib(ctx):
    """the noise profile reads the NULL symbol of every frame of a float buffer: 2736 frames, the last four against a four-frame call"""
    import torch
    n = 2736
    iq = BB.big(n * FRAME_SAMPLES * 8, lead=0).view(torch.float32)
    g = torch.Generator(device="cuda").manual_seed(9540)
    for a in range(0, iq.numel(), 1 << 28):
        iq[a:a + (1 << 28)].normal_(generator=g)
    shapes = [((128,), torch.float32, -1.0), ((128,), torch.float32, -1.0), ((), torch.float32, -1.0), ((1536,), torch.float32, -1.0), ((), torch.int32, -1)]
    A = [torch.full((n,) + s, f, dtype=d, device="cuda") for s, d, f in shapes]
    B = [torch.full((TAIL,) + s, f, dtype=d, device="cuda") for s, d, f in shapes]
    for x, k, o in ((iq, n, A), (iq[(n - TAIL) * FRAME_SAMPLES * 2:], TAIL, B)):
        ctx.noise_profile(x, k, FRAME_SAMPLES, 0, profile_out=o[0], band_weight=o[1], mean_noise=o[2], carrier_power=o[3], valid=o[4])
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(A, B)):
        assert torch.equal(a[n - TAIL:].contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), i
        assert not torch.equal(b, torch.full_like(b, shapes[i][2])), (i, "nothing was written")
    assert not torch.equal(B[3][0], B[3][1])
    del iq, A
    BB.release()


def test_mode_2_float_input_past_4_gib(ctx):
    """ofdm_demod_frames_mode has no stride: 10 923 mode II frames of 49 152 samples reach 2^32 bytes; 10 928 in, the last four compared"""
    import dabgpu
    import torch
    P = dabgpu.ofdm_params(2)
    fs, fb = P["nb_frame_samples"], P["nb_frame_bits"]
    n = 10928
    assert fs == 49152 and (n - TAIL) * fs * 8 >= S32
    iq = BB.big(n * fs * 8, lead=0).view(torch.float32)
    g = torch.Generator(device="cuda").manual_seed(9550)
    for a in range(0, iq.numel(), 1 << 28):
        iq[a:a + (1 << 28)].normal_(generator=g)
    bits = torch.full((n, fb), 0x5A, dtype=torch.uint8, device="cuda")
    bits4 = torch.full((TAIL, fb), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.ofdm_demod_frames_mode(2, iq, n, bits)
    ctx.ofdm_demod_frames_mode(2, iq[(n - TAIL) * fs * 2:], TAIL, bits4)
    torch.cuda.synchronize()
    assert torch.equal(bits[n - TAIL:], bits4)
    assert not torch.equal(bits4[0], bits4[1]) and not torch.equal(bits[0], bits4[0]) and not bool((bits4 == 0x5A).all())
    del iq, bits
    BB.release()


# ---- the synchronised branch call and the stream bank ----

def test_sync_demod_frames_branch_strides(ctx):
    """two receivers whose input slices lie 2^32 bytes apart and whose soft bits lie 2^32 bytes apart, against the packed call.  The
    frames are made by the modulator on the device, the PRS P samples into each slice."""
    import dabgpu
    import torch
    P = 3200
    packed_stride = P + 1544 + FRAME_SAMPLES
    far_stride = 1 << 29                                                 # samples: 2^32 bytes
    g = torch.Generator(device="cuda").manual_seed(9560)
    payload = torch.empty((2, 75 * 1536 // 4), dtype=torch.uint8, device="cuda").random_(0, 256, generator=g)
    frames = torch.zeros((2, FRAME_SAMPLES, 2), dtype=torch.float32, device="cuda")
    ctx.ofdm_modulate_frames(1, payload, 2, frames)
    slices = torch.zeros((2, packed_stride, 2), dtype=torch.float32, device="cuda")
    slices[:, P - 2656:P - 2656 + FRAME_SAMPLES] = frames                 # NULL first: the PRS begins at sample P
    torch.cuda.synchronize()
    h = slices.cpu().numpy()
    src = two_units(h, 8 * far_stride, lead=0)
    view, can = two_outputs(NB, S32)
    soft = dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0)
    sdt = np.dtype(dabgpu.SYNC_STATE_DTYPE)
    got = []
    for iq, stride, bits, bstride in ((src, far_stride, view, S32), (slices, packed_stride, torch.full((2, NB), 0x5A, dtype=torch.uint8, device="cuda"), 0)):
        st = torch.zeros((2 * sdt.itemsize,), dtype=torch.uint8, device="cuda")
        dq = torch.full((2, 75, 1536, 2), -7.0, dtype=torch.float32, device="cuda")
        scale = torch.full((2,), -1.0, dtype=torch.float32, device="cuda")
        ctx.ofdm_sync_demod_frames_branch(iq, 2, stride, P, st, bits, soft, dq, bits_frame_stride=bstride, soft_scale=scale)
        torch.cuda.synchronize()
        got.append((st, dq, scale, units(view, S32, NB) if bits is view else bits))
    can.check()
    assert got[0][0].cpu().numpy().view(sdt)["sync_valid"].tolist() == [1, 1]
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    assert not torch.equal(got[0][3][0], got[0][3][1]) and not bool((got[0][3] == 0x5A).all())
    del src, view, can
    BB.release()


@pytest.fixture(scope="module")
def bank_streams(oracle):
    """two unsynchronised float streams of four frames each (tests/stream_soft_model.py's, shared with the stream bank's own tests)"""
    import stream_soft_model as SSM
    S = SSM.float_streams(oracle)[:2]
    n = S.shape[1] // 8 * 8
    return np.ascontiguousarray(S[:, :n]), n


def run_stream_bank(ctx, d_iq, stride, n, slots, bits, scale, dq=None, rec=None):
    """a weighted two-stream bank over the whole block in one frames-form call -> frame counts [2]"""
    import dabgpu
    import torch
    bank = dabgpu.StreamBank(ctx, 2)
    bank.set_soft(dabgpu.SoftCfg(dabgpu.SOFT_CSI, 64.0), scale)
    if dq is not None:
        bank.set_products(dq, rec)
    nf = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    bank.process(d_iq, stride, n, bits, slots, nf)
    torch.cuda.synchronize()
    bank.close()
    return nf.cpu().numpy()


def test_stream_bank_stream_stride(ctx, bank_streams):
    """stream_stride_samples = 2^29: the second stream's samples begin 2^32 bytes behind the first's"""
    import torch
    x, n = bank_streams
    slots = n // 191400 + 2
    src = two_units(x, 8 << 29, lead=0)
    d_x = torch.from_numpy(x).cuda()
    got = []
    for d_iq, stride in ((src, 1 << 29), (d_x, n)):
        bits = torch.full((2, slots, NB), 0x5A, dtype=torch.uint8, device="cuda")
        scale = torch.full((2 * slots,), -1.0, dtype=torch.float32, device="cuda")
        got.append((run_stream_bank(ctx, d_iq, stride, n, slots, bits, scale), bits, scale))
    assert got[0][0].tolist() == got[1][0].tolist() and min(got[0][0]) >= 2, got[0][0]
    assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2].view(torch.int32), got[1][2].view(torch.int32))
    assert not torch.equal(got[0][1][0, 0], got[0][1][1, 0])
    del src
    BB.release()


def test_stream_bank_bits_past_4_gib(ctx, bank_streams):
    """max_frames = 18642: the second stream's bits slots begin 18642 * 230400 >= 2^32 bytes behind the first's, its scale words at
    [18642 + slot]; against a bank with the smallest max_frames the call takes"""
    import torch
    x, n = bank_streams
    slots, far = n // 191400 + 2, 18642
    d_x = torch.from_numpy(x).cuda()
    view = BB.big(2 * far * NB)
    can = BB.Canaries()
    can.at(view, -BB.CANARY_BYTES)
    can.at(view, far * NB - BB.CANARY_BYTES)                            # the end of stream 0's slots, never reached
    BB.region(view, 0, slots * NB).fill_(0x5A)
    BB.region(view, far * NB, slots * NB).fill_(0x5A)                   # (a wrapped write of stream 1 lands in stream 0's slots: compared)
    scale_far = torch.full((2 * far,), -1.0, dtype=torch.float32, device="cuda")
    nf_far = run_stream_bank(ctx, d_x, n, n, far, view, scale_far)
    bits = torch.full((2, slots, NB), 0x5A, dtype=torch.uint8, device="cuda")
    scale = torch.full((2 * slots,), -1.0, dtype=torch.float32, device="cuda")
    nf = run_stream_bank(ctx, d_x, n, n, slots, bits, scale)
    can.check()
    assert nf_far.tolist() == nf.tolist() and min(nf) >= 2, nf
    for s in range(2):
        k = int(nf[s])
        assert torch.equal(BB.region(view, s * far * NB, k * NB), bits[s, :k].reshape(-1)), s
        assert torch.equal(scale_far[s * far:s * far + k].view(torch.int32), scale[s * slots:s * slots + k].view(torch.int32)), s
    del view, can
    BB.release()


def test_stream_bank_products_past_4_gib(ctx, bank_streams):
    """products on, max_frames = 4661: the second stream's products begin 4661 * 921600 >= 2^32 bytes behind the first's, its records at
    [4661 + slot]; against a bank with the smallest max_frames"""
    import torch
    x, n = bank_streams
    slots, far = n // 191400 + 2, 4661
    assert far * DQ_BYTES >= S32
    d_x = torch.from_numpy(x).cuda()
    dq_far = BB.big(2 * far * DQ_BYTES, lead=BB.LEAD // 2)
    can = BB.Canaries()
    can.at(dq_far, -BB.CANARY_BYTES, lead=BB.LEAD // 2)
    can.at(dq_far, far * DQ_BYTES - BB.CANARY_BYTES)
    rec_far = torch.full((2 * far, 6), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    bits_far = torch.empty((2, far, NB), dtype=torch.uint8, device="cuda")
    scale_far = torch.full((2 * far,), -1.0, dtype=torch.float32, device="cuda")
    nf_far = run_stream_bank(ctx, d_x, n, n, far, bits_far, scale_far, dq_far, rec_far)
    dq = torch.full((2 * slots * DQ_BYTES,), 0x5A, dtype=torch.uint8, device="cuda")
    rec = torch.full((2 * slots, 6), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    bits = torch.full((2, slots, NB), 0x5A, dtype=torch.uint8, device="cuda")
    scale = torch.full((2 * slots,), -1.0, dtype=torch.float32, device="cuda")
    nf = run_stream_bank(ctx, d_x, n, n, slots, bits, scale, dq, rec)
    can.check()
    assert nf_far.tolist() == nf.tolist() and min(nf) >= 2, nf
    for s in range(2):
        k = int(nf[s])
        assert torch.equal(BB.region(dq_far, s * far * DQ_BYTES, k * DQ_BYTES), dq[s * slots * DQ_BYTES:(s * slots + k) * DQ_BYTES]), s
        assert torch.equal(rec_far[s * far:s * far + k], rec[s * slots:s * slots + k]) and torch.equal(bits_far[s, :k], bits[s, :k]), s
        assert not bool((dq[s * slots * DQ_BYTES:(s * slots + 1) * DQ_BYTES] == 0x5A).all())
    del dq_far, can, bits_far
    BB.release()


# ---- DAB+ and packet mode, both directions, and the channel encoder ----

def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    for u, i in ((np.uint64, np.int64), (np.uint32, np.int32), (np.uint16, np.int16)):
        if a.dtype == u:
            a = a.view(i)
    if a.dtype.fields is not None:
        a = a.view(np.uint8)
    return torch.from_numpy(a).cuda()


@pytest.mark.parametrize("far", ["stream_offsets", "superframes"])
def test_dabplus_bank_offsets_and_superframe_stride(ctx, oracle, far):
    """two DAB+ streams of one super frame each.  stream_offsets: stream 1's logical frames begin 2^32 bytes into the frames buffer;
    superframes: superframe_stride = 2^32 with one super frame per stream puts stream 1's slot there.  Against the packed call, and
    stream 1's record and bytes against the oracle's AAC_Frame_Processor"""
    import dabgpu
    import dabplus_model as M
    import torch
    rng = np.random.default_rng(9600)
    sizes, F = [96, 192], 5
    max_n = max(sizes)
    sfs = [M.make_superframe(oracle, rng, n)[0] for n in sizes]
    sfs[1] = M.corrupt(rng, sfs[1], {0: 2, 3: 4})                       # errors for the outer code to correct
    rows = np.zeros((2, F, max_n), np.uint8)
    for s, n in enumerate(sizes):
        rows[s, :, :n] = sfs[s].reshape(5, n)
    rdt = np.dtype(dabgpu.SUPERFRAME_RESULT_DTYPE)
    d_n = dev(np.array(sizes, np.int32))
    got = []
    for is_far in (True, False):
        far_in, far_out = is_far and far == "stream_offsets", is_far and far == "superframes"
        frames = two_units(rows.reshape(2, -1), S32, lead=0) if far_in else torch.from_numpy(rows).cuda()
        d_off = dev(np.array([0, S32 if far_in else F * max_n], np.uint64))
        can = None
        if far_out:
            d_sf, can = two_outputs(5 * max_n, S32, fill=0xC3)
        else:
            d_sf = torch.full((2, 5 * max_n), 0xC3, dtype=torch.uint8, device="cuda")
        d_res = torch.zeros((2, rdt.itemsize), dtype=torch.uint8, device="cuda")
        d_cnt = torch.full((2, 4), -9, dtype=torch.int32, device="cuda")
        bank = dabgpu.DabPlusBank(ctx, 2)
        bank.process(frames, d_off, max_n, d_n, F, d_sf, S32 if far_out else 5 * max_n, d_res, 1, d_cnt)
        torch.cuda.synchronize()
        bank.close()
        if can is not None:
            can.check()
        sf = units(d_sf, S32, 5 * max_n) if far_out else d_sf
        got.append((sf.cpu().numpy(), d_res.cpu().numpy().view(rdt).reshape(2), d_cnt.cpu().numpy()))
        del frames, d_sf, can
        BB.release()
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b)
    assert got[0][2][:, 0].tolist() == [1, 1]
    proc = oracle.AacFrameProcessor()
    for f in range(F):
        rc, o, sf_o = proc.process(rows[1, f, :sizes[1]])
    assert o["superframe_done"] and o["header_valid"] and np.array_equal(got[0][0][1, :5 * sizes[1]], sf_o)
    r = got[0][1][1]
    assert int(r["header_valid"]) == 1 and int(r["rs_corrected"]) == int(o["rs_corrected"]) > 0 and int(r["frame_index"]) == F - 1


def test_dabplus_tx_stream_offsets(ctx):
    """DabPlusTx.encode into a payload whose second stream begins 2^32 bytes in: the packed call and the model's bytes"""
    import dabgpu
    import dabplus_tx_model as T
    import torch
    rng = np.random.default_rng(9610)
    streams = []
    for n, d in ((72, 0x13), (768, 0x6F)):
        lens = T.split_lengths(rng, d, n, "random")
        streams.append((n, [(d, [rng.integers(0, 256, l, dtype=np.uint8) for l in lens])]))
    au, offs, lens, desc, fbytes = T.pack_call(streams)
    stride = 1536
    args = [dev(x) for x in (au, offs, lens, desc, fbytes)]
    view, can = two_outputs(5 * stride, S32, fill=0xC3)
    packed = torch.full((2, 5 * stride), 0xC3, dtype=torch.uint8, device="cuda")
    st = [torch.full((2, 1), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    tx = dabgpu.DabPlusTx(ctx)
    tx.encode(2, 1, *args, view, dev(np.array([0, S32], np.uint64)), stride, st[0])
    tx.encode(2, 1, *args, packed, dev(np.array([0, 5 * stride], np.uint64)), stride, st[1])
    torch.cuda.synchronize()
    can.check()
    far = units(view, S32, 5 * stride)
    assert torch.equal(far, packed) and torch.equal(st[0], st[1]) and not st[0].cpu().numpy().any()
    n, (d, aus) = streams[1][0], streams[1][1][0]
    frames, status = T.encode(d, aus, n)
    got = far[1].cpu().numpy().reshape(5, stride)
    assert status == 0 and np.array_equal(got[:, :n], np.asarray(frames).reshape(5, n)) and (got[:, n:] == 0xC3).all()
    del view, can
    BB.release()


def packet_streams(rng, K):
    import packet_fec_model as M
    streams = []
    for (L, fb, start), address in (((48, 192, 24 * 3), 77), ((96, 384, 24 * 9), 901)):
        lens = [int(v) for v in rng.integers(0, 500, 40)]
        groups = [rng.integers(0, 256, v, dtype=np.uint8) for v in lens]
        st, ent, first, consumed, _, _ = M.layout(lens, address, L, fb, start, 1, K)
        assert st == 0 and consumed > 2
        streams.append(dict(groups=groups, ent=ent, first=first, address=address, fb=fb, start=start, bytes=M.encode(groups, ent, first, address)))
    return streams


def test_packet_tx_stream_offsets(ctx):
    """PacketTx.encode into a payload whose second stream begins 2^32 bytes in: the packed call and the model's bytes"""
    import dabgpu
    import packet_fec_model as M
    import torch
    K = 2
    streams = packet_streams(np.random.default_rng(9620), K)
    data, goffs, gbase, table, first = M.pack_tx_call([(s["groups"], s["ent"], s["first"]) for s in streams])
    stride = 384 + 8
    rows = max((s["start"] % s["fb"] + K * M.RING + s["fb"] - 1) // s["fb"] for s in streams)
    total = rows * stride
    args = [dev(data), dev(goffs), dev(gbase), dev(table), table.shape[1], dev(first), dev(np.array([s["address"] for s in streams], np.uint16)),
            dev(np.array([s["fb"] for s in streams], np.uint32)), dev(np.array([s["start"] for s in streams], np.uint64))]
    view, can = two_outputs(total, S32, fill=0xC3)
    packed = torch.full((2, total), 0xC3, dtype=torch.uint8, device="cuda")
    st = [torch.full((2, K), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    tx = dabgpu.PacketTx(ctx)
    tx.encode(2, K, *args, view, dev(np.array([0, S32], np.uint64)), stride, st[0])
    tx.encode(2, K, *args, packed, dev(np.array([0, total], np.uint64)), stride, st[1])
    torch.cuda.synchronize()
    can.check()
    far = units(view, S32, total)
    assert torch.equal(far, packed) and torch.equal(st[0], st[1]) and not st[0].cpu().numpy().any()
    s = streams[1]
    exp = np.full(total, 0xC3, np.uint8)
    k = s["start"] + np.arange(s["bytes"].size, dtype=np.int64)
    exp[(k // s["fb"] - s["start"] // s["fb"]) * stride + k % s["fb"]] = s["bytes"]
    assert np.array_equal(far[1].cpu().numpy(), exp)
    del view, can
    BB.release()


@pytest.mark.parametrize("far", ["stream_offsets", "packets"])
def test_packet_bank_offsets_and_packet_stride(ctx, far):
    """two packet-mode streams with FEC.  stream_offsets: stream 1's logical frames begin 2^32 bytes in; packets: packet_stride = 2^32
    puts stream 1's packets there.  Against the packed call, and stream 1's counts and packets against the model's processor"""
    import dabgpu
    import packet_fec_model as M
    import torch
    K = 3
    streams = packet_streams(np.random.default_rng(9630), K)
    fbs = [s["fb"] for s in streams]
    stride = max(fbs)
    logical = [M.to_logical_frames(s["bytes"], s["fb"], s["start"]) for s in streams]
    F = min(f.shape[0] for f in logical)
    rows = np.zeros((2, F, stride), np.uint8)
    for i, f in enumerate(logical):
        rows[i, :, :fbs[i]] = f[:F]
    rdt, fdt = np.dtype(dabgpu.PACKET_RECORD_DTYPE), np.dtype(dabgpu.PACKET_FEC_FRAME_DTYPE)
    pk_bytes = M.RING + F * stride
    max_rec, max_fec = pk_bytes // 24 + 1, F * stride // M.RING + 2
    got = []
    for is_far in (True, False):
        far_in, far_out = is_far and far == "stream_offsets", is_far and far == "packets"
        frames = two_units(rows.reshape(2, -1), S32, lead=0) if far_in else torch.from_numpy(rows).cuda()
        d_off = dev(np.array([0, S32 if far_in else F * stride], np.uint64))
        can = None
        if far_out:
            d_pk, can = two_outputs(pk_bytes, S32, fill=0xC3)
        else:
            d_pk = torch.full((2, pk_bytes), 0xC3, dtype=torch.uint8, device="cuda")
        d_rec = torch.full((2, max_rec * rdt.itemsize), 0xC3, dtype=torch.uint8, device="cuda")
        d_fec = torch.full((2, max_fec * fdt.itemsize), 0xC3, dtype=torch.uint8, device="cuda")
        d_cnt = torch.full((2, 4), -9, dtype=torch.int32, device="cuda")
        bank = dabgpu.PacketBank(ctx, 2)
        bank.process(frames, d_off, stride, dev(np.array(fbs, np.uint32)), F, d_pk, S32 if far_out else pk_bytes, d_rec, max_rec, d_fec, max_fec, d_cnt)
        torch.cuda.synchronize()
        bank.close()
        if can is not None:
            can.check()
        pk = units(d_pk, S32, pk_bytes) if far_out else d_pk
        got.append((pk.cpu().numpy(), d_rec.cpu().numpy(), d_fec.cpu().numpy(), d_cnt.cpu().numpy()))
        del frames, d_pk, can
        BB.release()
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b)
    exp = M.run_frames(list(logical[1][:F]))
    assert got[0][3][1].tolist() == exp["counts"] and exp["counts"][0] > 10 and exp["counts"][2] >= 1
    assert np.array_equal(got[0][0][1, :exp["packets"].size], exp["packets"])


def test_tx_bank_encode_frames_frame_stride(ctx):
    """TxBank.encode_frames, two ensembles of one frame, frame_stride = 2^32: the second ensemble's frame bits lie there.  (The payload
    itself is [n][F][4][cif_in_bytes] without a stride: the ABI gives no way to place its rows.)"""
    import dabgpu
    import torch
    subs = [dabgpu.SubChannel(0, 48, False, 0, 2, 0), dabgpu.SubChannel(100, 35, True, 4, 0, 0), dabgpu.SubChannel(800, 64, False, 0, 3, 0)]
    bank = dabgpu.TxBank(ctx, 2, subs)
    g = torch.Generator(device="cuda").manual_seed(9640)
    fib = torch.empty((2, 1, 4, 3, 30), dtype=torch.uint8, device="cuda").random_(0, 256, generator=g)
    pay = torch.empty((2, 1, 4, bank.cif_in_bytes), dtype=torch.uint8, device="cuda").random_(0, 256, generator=g)
    view, can = two_outputs(28800, S32)
    packed = torch.full((2, 28800), 0x5A, dtype=torch.uint8, device="cuda")
    bank.encode_frames(fib, pay, 1, view, frame_stride=S32)
    bank.reset()
    bank.encode_frames(fib, pay, 1, packed)
    torch.cuda.synchronize()
    can.check()
    far = units(view, S32, 28800)
    assert torch.equal(far, packed) and not torch.equal(far[0], far[1]) and not bool((far == 0x5A).all())
    bank.close()
    del view, can
    BB.release()
