"""-m gpu: the grow-only buffers of the banks, sessions and receivers.  Every case has one form: object A runs a sequence of calls whose
shapes grow, so that its buffers are reallocated in the middle of the sequence; object B is first grown by one call at the largest shape,
put back to its start (reset / seek(0)), and runs the same sequence with buffers that never move.  Every output of A equals B's byte for
byte.  The shapes are the smallest at which two different capacities occur."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def signal(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


@pytest.fixture(scope="module")
def gpu():
    import dabgpu
    ctx = dabgpu.Context(0)
    yield dabgpu, ctx
    ctx.close()


# ---- signal banks: one stream or channel, n_out = 256, then 4096 ----
def _signal_bank_case(make, call):
    x = signal(1024, 5)
    a, b = make(), make()
    try:
        call(b, x, 4096)                                   # B: both host-form buffers at their largest
        b.seek(0)
        for n_out in (256, 4096):
            ya, yb = call(a, x, n_out), call(b, x, n_out)
            assert ya.shape[-1] == n_out and np.isfinite(ya).all() and np.any(ya != 0)
            assert same(ya, yb), n_out
    finally:
        a.close()
        b.close()


def test_channel_host_form_grows(gpu):
    dabgpu, ctx = gpu
    streams = [dabgpu.channel_stream(taps=((0, 1.0, 0.0), (3, 0.25, -0.5)), cycles_per_sample=1.0e-3, seed=7, noise_sigma=0.1)]
    _signal_bank_case(lambda: dabgpu.Channel(ctx, streams), lambda bank, x, n: bank.apply_host(x, n, wrap=True))


def test_resampler_host_form_grows(gpu):
    dabgpu, ctx = gpu
    params = [dabgpu.resample_stream(dabgpu.resample_step(ppm=37.0), offset=0.25)]
    _signal_bank_case(lambda: dabgpu.Resampler(ctx, params), lambda bank, x, n: bank.apply_host(x, n, wrap=True))


def test_channeliser_host_forms_grow(gpu):
    dabgpu, ctx = gpu
    chs = [dabgpu.channeliser_channel(dabgpu.channeliser_freq(250.0e3, 4.096e6))]
    _signal_bank_case(lambda: dabgpu.Channeliser(ctx, chs, 1, 2), lambda bank, x, n: bank.split_host(x, n, wrap=True))
    _signal_bank_case(lambda: dabgpu.Channeliser(ctx, chs, 1, 2), lambda bank, x, n: bank.combine_host(x, n, wrap=True))


# ---- channel encoder: one ensemble, one small sub-channel, 1 frame, then 3 ----
@pytest.mark.parametrize("form", ["encode", "transmit"])
def test_tx_bank_host_forms_grow(gpu, form):
    dabgpu, ctx = gpu
    subs = [dabgpu.SubChannel(0, 6, 0, 0, 2, 0)]
    rng = np.random.default_rng(11)
    a, b = dabgpu.TxBank(ctx, 1, subs), dabgpu.TxBank(ctx, 1, subs)
    try:
        fib = rng.integers(0, 256, (1, 3, 4, 3, 30), dtype=np.uint8)
        pay = rng.integers(0, 256, (1, 3, 4, a.cif_in_bytes), dtype=np.uint8)
        run = (lambda bank, f: bank.encode_frames_host(fib[:, :f], pay[:, :f], f)) if form == "encode" else \
              (lambda bank, f: bank.transmit_frames_host(fib[:, :f], pay[:, :f], f))
        run(b, 3)                                          # B: frame bits, FIB, payload and output buffers at their largest
        b.reset()
        ctx.synchronize()
        for f in (1, 3):
            ya, yb = run(a, f), run(b, f)
            assert ya.shape[1] == f and np.any(ya != 0)
            assert same(ya, yb), f
    finally:
        a.close()
        b.close()


# ---- stream bank: mode III, one stream, a format without a fused loader; 4096 samples, then 65536 ----
def test_stream_bank_raw_scratch_and_windows_grow(gpu):
    import torch
    dabgpu, ctx = gpu
    g = dabgpu.ofdm_params(3)
    fs, fb = g["nb_frame_samples"], g["nb_frame_bits"]
    rng = np.random.default_rng(3)
    frames = ctx.ofdm_modulate_frames_host(3, rng.integers(0, 256, (3, fb // 8), dtype=np.uint8), 3, layout=dabgpu.TX_PAYLOAD_FRAME_BITS).reshape(-1)
    x = np.concatenate([0.01 * signal(1500, 4), frames / np.abs(frames).max()])
    s16 = np.round(np.stack([x.real, x.imag], axis=1) * 20000.0).astype(">i2")             # big endian: converted through the bank's scratch
    fmt = dabgpu.IQ_FORMATS.index("raw_s16b")
    d_raw = torch.from_numpy(s16.view(np.uint8).reshape(-1)).cuda()
    cfg = dabgpu.stream_cfg_default()
    cfg.sync.impulse_peak_threshold_db = 8.0
    blocks = (4096, 65536, 65536)
    max_frames = max(blocks) // (fs - g["nb_null_period"] - g["nb_symbol_period"]) + 2
    a, b = dabgpu.StreamBank(ctx, 1, cfg, mode=3), dabgpu.StreamBank(ctx, 1, cfg, mode=3)

    def run(bank, at, n):
        bits = torch.zeros((1, max_frames, fb), dtype=torch.int8, device="cuda")
        nf = torch.zeros(1, dtype=torch.int32, device="cuda")
        bank.process_raw(d_raw[4 * at:], fmt, n, n, bits, max_frames, nf)
        torch.cuda.synchronize()
        return bits.cpu().numpy(), nf.cpu().numpy(), bank.status()

    try:
        run(b, 0, max(blocks))                             # B: the conversion scratch and the L1-window table at their largest
        b.reset()
        at, total = 0, 0
        for n in blocks:
            (bits_a, nf_a, st_a), (bits_b, nf_b, st_b) = run(a, at, n), run(b, at, n)
            assert same(nf_a, nf_b) and same(bits_a, bits_b) and st_a.tobytes() == st_b.tobytes(), (at, n)
            at += n
            total += int(nf_a[0])
        assert total >= 1 and int(st_a["total_frames_read"][0]) == total      # (the comparison was of frames, not of empty buffers)
    finally:
        a.close()
        b.close()


# ---- frame session: one short sub-channel, a frame; three sub-channels, a frame ----
def test_frame_session_result_blocks_grow(gpu):
    dabgpu, _ = gpu
    one = [dabgpu.SubChannel(0, 6, 0, 0, 2, 0)]
    three = [dabgpu.SubChannel(0, 6, 0, 0, 2, 0), dabgpu.SubChannel(64, 48, 0, 0, 2, 0), dabgpu.SubChannel(200, 52, 1, 20, 0, 0)]
    rng = np.random.default_rng(17)
    frames = rng.integers(-127, 128, (2, dabgpu.NB_FRAME_BITS), dtype=np.int8)
    a, b = dabgpu.FrameSession(0), dabgpu.FrameSession(0)

    def results(ses, subs, gen):
        out = [ses.fetch_fib_group(gen, grp) for grp in range(4)]
        out += [ses.fetch_cif(gen, sc, cif) for sc in subs for cif in range(4)]
        assert all(r is not None for r in out)
        return [np.concatenate([np.asarray(part).reshape(-1).astype(np.uint64) for part in r]) for r in out]

    try:
        # B: the device block and a slot's pinned block at their largest.  The frame is all zeros, which is what a new session's history
        # holds: the time de-interleaver of the frames below reads the same soft bits in both sessions
        b.set_subchannels(three)
        b.push_frame(np.zeros(dabgpu.NB_FRAME_BITS, np.int8))
        for subs, bits in ((one, frames[0]), (three, frames[1])):
            a.set_subchannels(subs)
            b.set_subchannels(subs)
            ga, gb = a.push_frame(bits), b.push_frame(bits)
            assert gb == ga + 1
            ra, rb = results(a, subs, ga), results(b, subs, gb)
            assert len(ra) == 4 + 4 * len(subs) and all(same(p, q) for p, q in zip(ra, rb)), len(subs)
    finally:
        a.close()
        b.close()


# ---- receivers: the display views are asked for only after frames have run without them ----
class _Frame(C.Structure):
    _fields_ = [("generation", C.c_uint64), ("bits", C.c_void_p), ("n_bits", C.c_size_t), ("freq_fine", C.c_float), ("total_phase", C.c_float),
                ("fft", C.c_void_p), ("dqpsk", C.c_void_p)]


@pytest.mark.parametrize("form", ["private", "banked"])
def test_receiver_views_asked_for_late(gpu, form):
    dabgpu, _ = gpu
    L = dabgpu.lib()
    L.dabgpu_receiver_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.dabgpu_receiver_create_banked.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.dabgpu_receiver_destroy.argtypes = [C.c_void_p]
    L.dabgpu_receiver_stage.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.dabgpu_receiver_reset.argtypes = [C.c_void_p]
    L.dabgpu_receiver_submit_frame.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.dabgpu_receiver_wait_frame.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    n_fft_view = (dabgpu.NB_FRAME_SYMBOLS + 1) * dabgpu.NB_FFT * 2
    n_dq_view = (dabgpu.NB_FRAME_SYMBOLS - 1) * 1536 * 2
    x = signal(dabgpu.NB_NULL_PERIOD + dabgpu.NB_FRAME_SAMPLES, 23)

    def make():
        rx = C.c_void_p()
        if form == "banked":
            dabgpu.check(L.dabgpu_receiver_create_banked(C.byref(rx), 0), "dabgpu_receiver_create_banked")
        else:
            dabgpu.check(L.dabgpu_receiver_create(C.byref(rx), 0, 1, None, None), "dabgpu_receiver_create")
        return rx

    def frame(rx, k, views):
        h, cap = C.c_void_p(), C.c_size_t()
        dabgpu.check(L.dabgpu_receiver_stage(rx, C.byref(h), C.byref(cap)), "dabgpu_receiver_stage")
        stage = np.ctypeslib.as_array(C.cast(h, C.POINTER(C.c_float)), shape=(2 * cap.value,)).view(np.complex64)
        stage[:x.size] = np.roll(x, 1000 * k)
        gen, fr = C.c_uint64(), _Frame()
        dabgpu.check(L.dabgpu_receiver_submit_frame(rx, dabgpu.NB_NULL_PERIOD, 0.9, views, 0, C.byref(gen)), "dabgpu_receiver_submit_frame")
        dabgpu.check(L.dabgpu_receiver_wait_frame(rx, gen.value, C.byref(fr)), "dabgpu_receiver_wait_frame")
        out = [np.ctypeslib.as_array(C.cast(fr.bits, C.POINTER(C.c_int8)), shape=(fr.n_bits,)).copy(),
               np.array([fr.freq_fine, fr.total_phase], np.float32)]
        if views:
            assert fr.fft and fr.dqpsk
            out.append(np.ctypeslib.as_array(C.cast(fr.fft, C.POINTER(C.c_float)), shape=(n_fft_view,)).copy())
            out.append(np.ctypeslib.as_array(C.cast(fr.dqpsk, C.POINTER(C.c_float)), shape=(n_dq_view,)).copy())
        return out

    a, b = make(), make()
    try:
        frame(b, 9, 1)                                     # B: the device views and a slot's pinned views exist from the start
        dabgpu.check(L.dabgpu_receiver_reset(b), "dabgpu_receiver_reset")
        for k, views in enumerate((0, 0, 1, 1, 0, 1)):
            ra, rb = frame(a, k, views), frame(b, k, views)
            assert len(ra) == (4 if views else 2) and np.any(ra[0] != 0)
            assert all(same(p, q) for p, q in zip(ra, rb)), (k, views)
    finally:
        L.dabgpu_receiver_destroy(a)
        L.dabgpu_receiver_destroy(b)
