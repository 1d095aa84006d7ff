"""Test infrastructure: the expected side of the stream bank's weighted soft bits (dabgpu_stream_bank_set_soft).  StreamSoftModel is
tests/stream_model.py's state machine -- the policy changes nothing it looks at -- that also keeps, for every completed frame, the
196608 assembled samples and the frequency word the demodulator used, float32(coarse + fine) before the update.  From those the
weighted frame is composed as tests/softbit_loop.py::cpu_soft_bits composes it: the oracle's transform at that frequency,
softbit_model.dqpsk, softbit_model.soft_scale over samples 504 .. 2551 of the frame, softbit_model.frame_bits.  The same composition
with the normalised demapper must give the oracle's own soft bits: that is asserted for every frame.

Also the inputs shared by the CPU and the device tests: the streams of tests/test_gpu_stream_bank.py (its builders are imported, not
copied) plus one whose timing moves, so that a frame is found 37 samples late (its symbol 0 then ends in the caller's block, the
boundary inside the useful part) and one 53 samples early."""
import numpy as np

import softbit_loop as SL
import softbit_model as SM
import stream_model

F32 = np.float32
FRAME = 196608
_BINS = SL.carrier_bins()


class StreamSoftModel(stream_model.StreamModel):
    def __init__(self, oracle, mode=1):
        assert mode == 1
        super().__init__(oracle, mode)
        self.frame_mapper = oracle.mapper()

    def read_symbols(self, buf):
        f = F32(F32(self.sync.freq_coarse) + F32(self.sync.freq_fine))          # (a completing frame updates the fine word below)
        before = len(self.out_frames)
        take = super().read_symbols(buf)
        if len(self.out_frames) > before:
            fr = self.out_frames[-1]
            fr["samples"] = self.frame.copy()                                   # still the assembled frame when read_symbols returns
            fr["freq"] = f
            r = self.O.demod_frame(fr["samples"], f, want_fft=True)
            X = r["fft"].reshape(77, 2048)[:76, _BINS]
            fr["dq"] = SM.dqpsk(X[:-1], X[1:])
            assert np.array_equal(r["bits"], fr["bits"]) and np.array_equal(SM.frame_bits(fr["dq"], self.frame_mapper), fr["bits"]), \
                "the composition's normalised soft bits are the oracle's"
        return take

    def scale(self, fr, level=64.0):
        return SM.soft_scale(fr["samples"][SM.NB_CP:SM.NB_CP + SM.NB_FFT], level)

    def weighted(self, fr, level=64.0):
        """(k, the frame's 230400 weighted soft bits in the natural layout); computed once per level"""
        key = ("weighted", float(level))
        if key not in fr:
            k = self.scale(fr, level)
            fr[key] = (k, SM.frame_bits(fr["dq"], self.frame_mapper, k))
        return fr[key]


def classed(bits):
    """natural layout -> DABGPU_BITS_MSC_CLASSED (dabgpu_ofdm_demod_frames_history): inside every CIF row of 55296 soft bits, bit i sits at
    (i mod 16) * 3456 + i / 16; the FIC part stays"""
    out = np.array(bits, copy=True)
    for c in range(4):
        row = bits[9216 + 55296 * c:9216 + 55296 * (c + 1)]
        out[9216 + 55296 * c:9216 + 55296 * (c + 1)] = row.reshape(3456, 16).T.reshape(-1)
    return out


def moving_stream(oracle, make_stream):
    """make_stream(oracle, 1, 5, 1.8e-3, 1234, 3.0) with 37 samples duplicated inside its third frame and 53 removed inside its fourth: the
    frames after the edits are found at fine time offsets +37 and -53"""
    s = make_stream(oracle, 1, 5, 1.8e-3, 1234, 3.0)
    a, b = 21234 + 2 * FRAME + 100, 21234 + 3 * FRAME + 100
    return np.concatenate([s[:a + 37], s[a:b], s[b + 53:]])


N_FLOAT = (21234 + 4 * FRAME + 4000) // 7 * 7 - 1           # the moving stream's four frames; not a multiple of 7: a ragged last block
_cache = {}


def float_streams(oracle):
    """the three signal streams of test_stream_bank_matches_stream_model (zeros behind their end), the moving stream, the noise-only stream"""
    if "float" not in _cache:
        from test_gpu_stream_bank import make_stream, noise_with_dips
        base = [make_stream(oracle, 1, 4, 1.8e-3, 1234, 3.0), make_stream(oracle, 2, 4, -7.3e-3, 77, 6.0),
                make_stream(oracle, 3, 4, 2.0e-4, 2551, 1.0, dropout=(215000, 235000)), moving_stream(oracle, make_stream),
                noise_with_dips(4, streams_len=850000)]
        out = np.zeros((len(base), N_FLOAT), np.complex64)
        for e, s in enumerate(base):
            out[e, :min(s.size, N_FLOAT)] = s[:N_FLOAT]
        _cache["float"] = out
    return _cache["float"]


MOVING, NOISE = 3, 4


def quantise(x, name):
    """complex float [n] -> capture bytes of format `name`, as tests/test_gpu_stream_bank.py quantises its streams"""
    v = np.stack([x.real, x.imag], axis=-1).reshape(-1)
    v = v / np.abs(v).max()
    if name == "raw_f32l":
        return np.ascontiguousarray(np.stack([x.real, x.imag], axis=-1).reshape(-1).astype("<f4")).view(np.uint8)
    if name == "raw_u8":
        return np.clip(np.rint(v * 127.0 + 127.5), 0, 255).astype(np.uint8)
    if name == "raw_s8":
        return np.clip(np.rint(v * 127.0), -128, 127).astype(np.int8).view(np.uint8)
    if name == "raw_s16l":
        return np.clip(np.rint(v * 30000.0), -32768, 32767).astype("<i2").view(np.uint8)
    assert name == "raw_u16l"
    return (np.clip(np.rint(v * 30000.0), -32768, 32767).astype(np.int32) + 32768).astype("<u2").view(np.uint8)


# ---- the closed loop of tests/softbit_loop.py through the unsynchronised state machine ----
LOOP_POINTS = [(10.0, 1), (10.0, 7)]          # (SNR dB, fading seed): all five frames are found, no desync
LOOP_BLOCK = 65536


def loop_stream(rx):
    """the received transmission behind a lead-in of its own signal, so that the level is established before the first NULL symbol"""
    return np.concatenate([rx[2693:2693 + 30000], rx]).astype(np.complex64)


def loop_counts(oracle, frames_normalised, frames_weighted, fib, pay, nb):
    """{policy: (FIB CRCs of 60, wrong bytes of the EEP 3-A sub-channel)} from the five frames' soft bits of either policy"""
    return {SM.SOFT_NORMALISED: SL.count(oracle, frames_normalised, fib, pay, nb), SM.SOFT_CSI: SL.count(oracle, frames_weighted, fib, pay, nb)}


def loop_cpu_point(oracle, host, iq, fib, pay, nb, snr_db, seed):
    """one operating point on the CPU -> (the stream, the model after it, the counts); once per point"""
    key = ("loop", snr_db, seed)
    if key not in _cache:
        stream = loop_stream(SL.received(host, iq, snr_db, seed))
        calls, m = run_model(oracle, key, stream, LOOP_BLOCK)
        frames = m.out_frames
        counts = None
        if len(frames) == 5:
            counts = loop_counts(oracle, [fr["bits"] for fr in frames], [m.weighted(fr, SL.LEVEL)[1] for fr in frames], fib, pay, nb)
        _cache[key] = (stream, m, counts)
    return _cache[key]


def run_model(oracle, key, samples, block):
    """the model over `samples` in blocks of `block` -> (per call: the frames completed in it, the model); once per key"""
    key = (key, block)
    if key not in _cache:
        m = StreamSoftModel(oracle)
        calls = []
        for k in range(0, samples.size, block):
            before = len(m.out_frames)
            m.process(samples[k:k + block])
            calls.append(m.out_frames[before:])
        _cache[key] = (calls, m)
    return _cache[key]
