"""Inputs shared by the device tests of the weighted soft bits (tests/test_gpu_softbits*.py): the transmission of tests/channel_loop.py
through the two-path host model of the channel at 15 dB, built once per process, and what the tests expect of a call -- the scale from
the numpy model over the frame's phase reference window, the soft bits from the numpy model over the DQPSK view of the NORMALISED
call (a view tests/test_gpu_ofdm.py pins to the oracle)."""
import numpy as np

import channel_loop as CL
import channel_model as CM
import demod_model as DM
import softbit_model as SM

NB_FRAME_SAMPLES, NB_FRAME_BITS = 196608, 230400
FORMATS = ["raw_f32l", "raw_u8", "raw_s8", "raw_s16l"]
_cache = {}


def received(oracle, tmp_dir):
    """the received stream (complex64) and what was sent: (rx, fib, pay, nb)"""
    if "rx" not in _cache:
        host = CM.build_host_model(tmp_dir)
        fib, pay, nb = CL.inputs(oracle)
        iq = CL.oracle_iq(oracle, fib, pay)
        _cache["rx"] = (CM.host_apply(host, [CL.params(iq, CL.SNR_DB)], iq, 0, CL.N_OUT, False)[0], fib, pay, nb)
    return _cache["rx"]


def frame_at(rx, j, timing=CL.TIMING):
    a = 2656 + j * NB_FRAME_SAMPLES + timing
    return rx[a:a + NB_FRAME_SAMPLES].copy()


def float_frames(rx):
    """six frames at the known position: as received; scaled by 2^-70 (the scale is near the top of the float range, the products near
    its bottom) and by 2^60 (the power overflows); one NaN sample inside the phase reference window; one outside it (symbol 39);
    scaled by 2^-80 (the power vanishes)"""
    f = np.stack([frame_at(rx, j) for j in (0, 1, 2, 3, 4, 0)])
    f[5] *= np.float32(2.0 ** -80)
    f[1] *= np.float32(2.0 ** -70)
    f[2] *= np.float32(2.0 ** 60)
    f[3, 504 + 1000] = complex(np.nan, 0.25)
    f[4, 39 * 2552 + 504 + 468] = complex(0.5, np.nan)
    return f


def capture_frames(rx, fmt_name):
    """the same transmission in a capture format: three frames at full scale, at a tenth of it and clipping; and a frame of zeros
    (for the signed formats: zero power)"""
    if fmt_name == "raw_f32l":
        f = float_frames(rx)
        return f.view(np.float32).reshape(len(f), NB_FRAME_SAMPLES, 2), f
    peak = float(np.abs(np.stack([frame_at(rx, j) for j in range(3)]).view(np.float32)).max())
    raws = [DM.encode_capture(frame_at(rx, j), fmt_name, peak * s) for j, s in enumerate((1.0, 10.0, 0.25))]
    raws.append(DM.encode_capture(np.zeros(NB_FRAME_SAMPLES, np.complex64), fmt_name, 1.0))
    raw = np.stack(raws)
    dec = np.stack([DM.decode_capture(r, fmt_name) for r in raw])
    dt = DM.CAPTURE[fmt_name][0]
    return raw.view(dt).reshape(len(raw), NB_FRAME_SAMPLES, 2), dec


def expected_scale(decoded_frames, level):
    return np.array([SM.soft_scale(f[SM.NB_CP:SM.NB_CP + SM.NB_FFT], level) for f in decoded_frames], np.float32)


def expected_bits(dqpsk_view, scales, mapper):
    """[n][75][1536] products of the normalised call, the frames' scales -> [n][230400] soft bits, natural layout"""
    return np.stack([SM.frame_bits(d, mapper, k) for d, k in zip(dqpsk_view, scales)])
