"""The fading closed loop, shared by its CPU form (tests/test_channel_fading_closed_loop.py) and its device form
(tests/test_gpu_channel_fading_loop.py): the loop of tests/channel_loop.py -- imported, not edited: five mode I frames, EEP 3-A plus a UEP
sub-channel, the signal 37 samples late, 0.05 carrier spacings of offset -- with the two static paths replaced by the `tu6` preset, all six
taps Rayleigh at DOPPLER_HZ.  The operating point was chosen on the CPU (DESIGN.md 4.18 has the table of seeds x SNR): the lowest SNR on a
1 dB grid at which the fading seeds 0..7 all deliver 60 of 60 FIB CRCs and the transmitted bytes, both there and 3 dB below."""
import numpy as np

import channel_fading_model as FM
import channel_loop as CL
import channel_model as CM

DOPPLER_HZ = 10.0
DOPPLER_CYCLES = DOPPLER_HZ / 2.048e6
SNR_DB = 19.0
FADING_SEED = 0
# dabgpu_channel_profile("tu6"): 0, 0.2, 0.5, 1.6, 2.3, 5.0 us at 2.048 MHz, -3, 0, -2, -6, -8, -10 dB, unit total power
TU6_DELAYS = [0, 0, 1, 3, 5, 10]
TU6_DB = [-3.0, 0.0, -2.0, -6.0, -8.0, -10.0]


def tu6_taps():
    p = 10.0 ** (np.array(TU6_DB) / 10.0)
    return [(d, float(np.float32(np.sqrt(a))), 0.0) for d, a in zip(TU6_DELAYS, p / p.sum())]


def params(iq, snr_db=SNR_DB):
    """unit total tap power and unit mean gain power: the mean signal power after the channel is the transmission's"""
    p = float(np.mean(np.abs(iq.astype(np.complex128)) ** 2))
    return CM.params_dict(taps=tu6_taps(), freq_q64=int(round(CL.CFO_CYCLES * 2 ** 64)), start=CL.TIMING, seed=0xDAB,
                          noise_sigma=float(np.sqrt(p / (2.0 * 10.0 ** (snr_db / 10.0)))))


def table(P, seed=FADING_SEED):
    return FM.plan_stream(P, DOPPLER_CYCLES, seed, 0, [FM.FADING] * len(P["taps"]))


def delivered(exp, fib, pay, nb):
    """what the operating point is chosen by: synchronised, 60 of 60 FIB CRCs, the last frame's FIB bodies and sub-channel bytes"""
    if exp["sync_failed"] != 0 or exp["fib_crc_ok"] != 12 * CL.N_FRAMES:
        return False
    ok = all(np.array_equal(exp["fib"][g, 32 * i:32 * i + 30], fib[0, CL.N_FRAMES - 1, g, i]) for g in range(4) for i in range(3))
    cifs = pay.reshape(4 * CL.N_FRAMES, nb)
    return ok and all(np.array_equal(exp["msc"][c], cifs[4 * (CL.N_FRAMES - 1) + c - 15]) for c in range(4))
