"""The closed loop that shows what the weighted soft bits buy, shared by its CPU form (tests/test_softbit_closed_loop.py) and its device
form (tests/test_gpu_softbits_loop.py): the transmission of tests/channel_loop.py (five mode I frames, an EEP 3-A and a UEP
sub-channel) through the fading channel of tests/channel_fading_loop.py -- `tu6`, all six taps Rayleigh at 10 Hz, the signal 37
samples late -- without a carrier offset, at an SNR below the fading loop's operating point.  What is counted: FIB CRCs of the five
frames (60) and wrong bytes of the EEP 3-A sub-channel's five logical frames that the time interleaver has delivered by then."""
import numpy as np

import channel_fading_loop as FL
import channel_fading_model as FM
import channel_loop as CL
import channel_model as CM
import softbit_model as SM
import tx_encode_cases as T

LEVEL = 64.0
# (SNR dB, fading seed) at which the reference's soft bits do not deliver and the weighted ones do (tests/test_softbit_closed_loop.py)
POINTS = [(10.0, 2), (8.0, 0)]


def params(iq, snr_db):
    p = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
    return CM.params_dict(taps=FL.tu6_taps(), freq_q64=0, start=CL.TIMING, seed=0xDAB, noise_sigma=float(np.sqrt(p / (2.0 * 10.0 ** (snr_db / 10.0)))))


def received(host, iq, snr_db, fading_seed):
    P = params(iq, snr_db)
    return FM.host_apply(host, [P], [FL.table(P, fading_seed)], iq, 0, CL.N_OUT, False)[0]


def frames_of(rx):
    return np.stack([rx[2656 + j * 196608 + CL.TIMING:2656 + j * 196608 + CL.TIMING + 196608] for j in range(CL.N_FRAMES)])


def cpu_soft_bits(oracle, frame, policy, mapper, bins):
    """one frame cut at the known position -> its 230400 soft bits: the oracle's transform, the numpy model's soft bits"""
    r = oracle.demod_frame(frame, 0.0, want_fft=True)
    if policy == SM.SOFT_NORMALISED:
        return r["bits"], r
    X = r["fft"].reshape(77, 2048)[:76, bins]
    k = SM.soft_scale(frame[SM.NB_CP:SM.NB_CP + SM.NB_FFT], LEVEL)
    return SM.frame_bits(SM.dqpsk(X[:-1], X[1:]), mapper, k), r


def carrier_bins():
    c = np.arange(1536)
    return np.where(c < 768, c - 768, c - 768 + 1) % 2048


def count(oracle, frame_bits, fib, pay, nb):
    """soft bits of the five frames [5][230400] -> (FIB CRCs that pass, of 60; wrong bytes of the EEP 3-A sub-channel's delivered logical frames)"""
    sub = T.o_sub(oracle, CL.SUBS[0])
    n_bytes = oracle.subchannel_plan(sub)[2]
    cifs = pay.reshape(4 * CL.N_FRAMES, nb)[:, :n_bytes]
    de = oracle.Deinterleaver(sub.length * 8)
    crc, wrong, delivered = 0, 0, 0
    for j in range(CL.N_FRAMES):
        b = frame_bits[j]
        for g in range(4):
            _, mask, _ = oracle.fic_decode_group(b[2304 * g:2304 * (g + 1)])
            crc += bin(mask).count("1")
        for c in range(4):
            cif = b[9216 + 55296 * c:9216 + 55296 * (c + 1)]
            de.consume(cif[sub.start_address * 64:(sub.start_address + sub.length) * 64])
            out = de.deinterleave()
            if out is None:
                continue
            got, _ = oracle.msc_decode_logical(sub, out)
            wrong += int((got != cifs[4 * j + c - 15]).sum())
            delivered += 1
    assert delivered == 4 * CL.N_FRAMES - 15
    return crc, wrong


def cpu_point(oracle, host, iq, fib, pay, nb, snr_db, seed, policies=(SM.SOFT_NORMALISED, SM.SOFT_CSI)):
    """{policy: (FIB CRCs, wrong bytes)} of one operating point"""
    frames = frames_of(received(host, iq, snr_db, seed))
    m, bins = oracle.mapper(), carrier_bins()
    return {p: count(oracle, [cpu_soft_bits(oracle, f, p, m, bins)[0] for f in frames], fib, pay, nb) for p in policies}
