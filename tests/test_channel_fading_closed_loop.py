"""CPU: the fading closed loop of tests/channel_fading_loop.py without the device -- oracle transmitter -> fading host model (`tu6`, all
taps Rayleigh at 10 Hz) -> oracle receive chain -- at the operating point and 3 dB below it, fading seed 0: 60 of 60 FIB CRCs and the
transmitted bytes at both.  The operating point is the lowest SNR on a 1 dB grid at which the seeds 0..7 all deliver at that SNR and 3 dB
below it (FIB CRCs of 60 per seed; * = a sub-channel byte of the last frame wrong although every CRC passed):

    SNR dB   seed 0    1    2    3    4    5    6    7
      10      58*   48*  43*  52*  60*  60*  48*  37*
      11      60    56*  49*  58*  60*  60*  48*  46*
      12      60    57*  52*  59*  60*  60*  48*  57*
      13      60    58*  56*  59*  60*  60*  50*  60*
      14      60    60*  59*  60*  60*  60*  54*  60
      15      60    60*  59*  60*  60*  60   57*  60
      16..22  60    60   60   60   60   60   60   60      every seed delivers
    -> 19 dB (19 and 16 deliver for every seed).  A fade takes the instantaneous SNR below the mean, hence 4 dB more than the static loop's 15."""
import numpy as np
import pytest

import channel_fading_loop as FL
import channel_fading_model as FM
import channel_loop as CL
import tx_encode_cases as T


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return FM.build_host_model(tmp_path_factory.mktemp("channel_fading_host_model"))


@pytest.mark.parametrize("snr_db", [FL.SNR_DB, FL.SNR_DB - 3.0])
def test_fading_host_model_through_the_oracle_chain_delivers_every_byte(oracle, host, snr_db):
    fib, pay, nb = CL.inputs(oracle)
    iq = CL.oracle_iq(oracle, fib, pay)
    P = FL.params(iq, snr_db)
    assert abs(sum(re * re + im * im for _, re, im in P["taps"]) - 1) < 1e-6
    measured = 10 * np.log10(np.mean(np.abs(iq) ** 2) / (2 * P["noise_sigma"] ** 2))
    assert abs(measured - snr_db) < 1e-6
    rx = FM.host_apply(host, [P], [FL.table(P)], iq, 0, CL.N_OUT, False)[0]
    exp = oracle.receive_frames(CL.slices_of(rx), CL.STRIDE, CL.P, CL.N_FRAMES, [T.o_sub(oracle, d) for d in CL.SUBS])
    print(f"SNR {snr_db} dB: sigma {P['noise_sigma']:.5f}, fine time offset {exp['state'].fine_time_offset}, "
          f"frequency words {exp['state'].freq_coarse:.3e} {exp['state'].freq_fine:.3e}, FIB CRCs {exp['fib_crc_ok']}")
    assert exp["sync_failed"] == 0 and exp["fib_crc_ok"] == 12 * CL.N_FRAMES
    assert CL.TIMING <= exp["state"].fine_time_offset <= CL.TIMING + max(FL.TU6_DELAYS)      # (the strongest path of the moment, not always the first)
    assert FL.delivered(exp, fib, pay, nb)
