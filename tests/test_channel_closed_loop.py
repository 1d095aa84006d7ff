"""CPU: the closed loop of tests/channel_loop.py without the device -- oracle transmitter -> host model of the channel -> oracle receive
chain -- at the noise level the GPU test uses and 3 dB below it: every FIB CRC passes and the sub-channel bytes are the transmitted
ones at both, so the GPU test's expectation has margin and does not rest on the code under test."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CM
import tx_encode_cases as T


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return CM.build_host_model(tmp_path_factory.mktemp("channel_host_model"))


@pytest.mark.parametrize("snr_db", [CL.SNR_DB, CL.SNR_DB - 3.0])
def test_host_model_through_the_oracle_chain_delivers_every_byte(oracle, host, snr_db):
    fib, pay, nb = CL.inputs(oracle)
    iq = CL.oracle_iq(oracle, fib, pay)
    rx = CM.host_apply(host, [CL.params(iq, snr_db)], iq, 0, CL.N_OUT, False)[0]
    measured = 10 * np.log10(np.mean(np.abs(iq) ** 2) * 1.25 / (2 * CL.sigma_for(iq, snr_db) ** 2))
    assert abs(measured - snr_db) < 1e-6
    exp = oracle.receive_frames(CL.slices_of(rx), CL.STRIDE, CL.P, CL.N_FRAMES, [T.o_sub(oracle, d) for d in CL.SUBS])
    print(f"SNR {snr_db} dB: sigma {CL.sigma_for(iq, snr_db):.5f}, fine time offset {exp['state'].fine_time_offset}, "
          f"frequency words {exp['state'].freq_coarse:.3e} {exp['state'].freq_fine:.3e}, FIB CRCs {exp['fib_crc_ok']}")
    CL.check_delivery(exp, fib, pay, nb, oracle)
