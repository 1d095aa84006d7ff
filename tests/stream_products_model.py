"""Test infrastructure: the expected side of the stream bank's DQPSK products (dabgpu_stream_bank_set_products) and the closed loop
behind them.  The products, the record and the scale of a completed frame are tests/stream_soft_model.py's: fr["dq"], the record words
fr["coarse"], fr["offset"] and fr["freq"] = float32(coarse + fine before the frame's phase update), and StreamSoftModel.scale(fr).

The closed loop is tests/clock_loop.py's transmission -- five mode I frames, the static two-path channel, noise, a sampling-clock error
applied by the resampler's host model -- received by the UNSYNCHRONISED state machine: the stream behind stream_soft_model.loop_stream's
lead-in, fed in blocks of 65536 to StreamSoftModel.  Behind every completed frame the clock tracker's float32 host model
(tests/clock_model.py, HostModel: one estimator pass, gain 1, the state carried per stream) reads the frame's products and de-rotates
them by the slope it has just updated; the weighted soft bits (softbit_model.frame_bits at the frame's scale) of the products as they
came ("plain") and of the de-rotated ones ("tracked") go to the oracle's FIC and MSC decoders (Loop.count)."""
import numpy as np

import clock_model as CK
import softbit_loop as SL
import softbit_model as SM
import stream_soft_model as SSM

POINTS = [(12.0, 200.0), (12.0, -200.0), (15.0, 0.0)]         # (SNR dB, clock error ppm)
BLOCK = SSM.LOOP_BLOCK
N_FRAMES = 5
PATHS = ("plain", "tracked")
_cache = {}


def record_words(fr):
    """what the frame's dabgpu_sync_state record must say, as comparable words: (fine_time_offset, freq_coarse bits, float32(coarse + fine) bits)"""
    return int(fr["offset"]), int(np.float32(fr["coarse"]).view(np.uint32)), int(np.float32(fr["freq"]).view(np.uint32))


def loop_input(loop, snr_db, ppm):
    """the stream of one operating point as the unsynchronised receiver is fed it; once per point"""
    key = ("input", float(snr_db), float(ppm))
    if key not in _cache:
        _cache[key] = SSM.loop_stream(loop.stream(snr_db, ppm))
    return _cache[key]


def track_frames(loop, products):
    """the tracker over one stream's frames in order -> (de-rotated products, slope words after each frame)"""
    model = CK.HostModel(loop.clock_lib)
    out, slopes = [], []
    for dq in products:
        v, _ = model.track(dq)
        out.append(v)
        slopes.append(int(model.slope))
    return out, slopes


def counts_of(loop, products, derotated, scales):
    """{path: (FIB CRCs of 60, wrong bytes of the EEP 3-A sub-channel)} from five frames' products on either path and their scales"""
    assert len(products) == len(derotated) == len(scales) == N_FRAMES
    return {"plain": loop.count([SM.frame_bits(d, loop.mapper, k) for d, k in zip(products, scales)]),
            "tracked": loop.count([SM.frame_bits(d, loop.mapper, k) for d, k in zip(derotated, scales)])}


def cpu_point(oracle, loop, snr_db, ppm):
    """one operating point on the CPU -> dict(stream, model, calls, counts or None, slopes, ppm); once per point"""
    key = ("point", float(snr_db), float(ppm))
    if key not in _cache:
        stream = loop_input(loop, snr_db, ppm)
        calls, m = SSM.run_model(oracle, key, stream, BLOCK)
        frames = m.out_frames
        derotated, slopes = track_frames(loop, [fr["dq"] for fr in frames])
        counts = None
        if len(frames) == N_FRAMES:
            counts = counts_of(loop, [fr["dq"] for fr in frames], derotated, [m.scale(fr, SL.LEVEL) for fr in frames])
        _cache[key] = dict(stream=stream, model=m, calls=calls, counts=counts, slopes=slopes, ppm=[CK.ppm_of(s) for s in slopes])
    return _cache[key]
