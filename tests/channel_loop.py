"""The closed loop transmitter -> channel -> receiver, shared by its CPU form (tests/test_channel_closed_loop.py: oracle composition and
modulator -> host model -> oracle receive chain) and its device form (tests/test_gpu_channel_loop.py: TxBank -> channel kernel -> the
product's synchronisation, demodulator and decoders).  One ensemble, mode I, 5 frames = 20 CIFs (the time interleaver needs 16): an
EEP 3-A and a UEP sub-channel; two paths, the second 200 samples late at -6 dB (inside the 504-sample guard interval), a carrier
offset of 0.05 of a carrier spacing (50 Hz), the signal 37 samples late, white noise at SNR_DB.  The fraction is small because the
receiver demodulates its first frame before its fine-frequency loop has an estimate: on the CPU (oracle chain) 0.02 and 0.05 of a
spacing deliver all 60 FIB CRCs of the five frames at 15 and 12 dB, 0.1 delivers 56 / 51, 0.2 loses frame 0 whole -- a property of
the receive chain, the same on the device by the parity contract."""
import numpy as np

import channel_model as CM
import tx_encode_cases as T

N_FRAMES = 5
P = 700                                   # samples in front of the expected PRS position in a receiver slice
STRIDE = P + 1544 + 196608
TIMING = 37
CFO_CYCLES = 0.05 / 2048                   # cycles per sample
SNR_DB = 15.0                             # chosen on the CPU: tests/test_channel_closed_loop.py delivers every byte here AND 3 dB below
SUBS = [dict(start=0, length=48, is_uep=0, uep_index=0, eep_level=2, eep_type=0),
        dict(start=200, length=52, is_uep=1, uep_index=20, eep_level=0, eep_type=0)]
SEED = 5900


def inputs(oracle):
    nb = sum(oracle.subchannel_plan(T.o_sub(oracle, d))[2] for d in SUBS)
    fib, pay = T.random_input(np.random.default_rng(SEED), 1, N_FRAMES, nb)
    return fib, pay, nb


def oracle_iq(oracle, fib, pay):
    """the oracle's transmitter: composition of the frame bits, then its modulator; NULL-first, back to back"""
    frames = T.expected_frames(oracle, SUBS, fib[0], pay[0])
    return np.concatenate([oracle.modulate_frame(np.unpackbits(f, bitorder="little")) for f in frames]).astype(np.complex64)


def sigma_for(iq, snr_db):
    """noise_sigma per component: mean signal power of the two-path sum = (1 + 0.25) x the transmission's, over snr, halved"""
    p = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2)) * (1.0 + TAP2 ** 2)
    return float(np.sqrt(p / (2.0 * 10.0 ** (snr_db / 10.0))))


TAP2 = 0.5                                # -6 dB


def params(iq, snr_db=SNR_DB):
    return CM.params_dict(taps=[(0, 1.0, 0.0), (200, TAP2, 0.0)], freq_q64=int(round(CFO_CYCLES * 2 ** 64)), start=TIMING, seed=0xDAB,
                          noise_sigma=sigma_for(iq, snr_db))


N_OUT = N_FRAMES * 196608 + 4096


def slices_of(rx):
    """the receiver's view: frame j from P samples before where its PRS would start without the timing offset"""
    s = np.zeros((N_FRAMES, STRIDE), np.complex64)
    for j in range(N_FRAMES):
        a = 2656 + j * 196608 - P
        seg = rx[a:a + STRIDE]
        s[j, :seg.size] = seg
    return s


def check_delivery(exp, fib, pay, nb, oracle):
    """exp = oracle.receive_frames(...) after N_FRAMES frames: sync, every FIB CRC, the last frame's FIB bodies and sub-channel bytes"""
    assert exp["sync_failed"] == 0
    assert exp["state"].fine_time_offset == TIMING
    assert exp["fib_crc_ok"] == 12 * N_FRAMES
    for g in range(4):
        for i in range(3):
            assert np.array_equal(exp["fib"][g, 32 * i:32 * i + 30], fib[0, N_FRAMES - 1, g, i])
    cifs = pay.reshape(4 * N_FRAMES, nb)
    for c in range(4):
        assert np.array_equal(exp["msc"][c], cifs[4 * (N_FRAMES - 1) + c - 15]), f"CIF {c}"
