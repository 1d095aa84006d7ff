"""CPU: the closed loops of tests/resample_loop.py without the device -- oracle transmitter -> host models of the channel and of the
resampler -> oracle receive chain -- at the channel loop's noise level and 3 dB below it: no sync failure, every FIB CRC, the transmitted
FIB bodies and sub-channel bytes, and the fine time offset of EVERY frame where T(m) puts it, +-1 sample (a drifting clock moves it, which
the channel loop's own check, pinned to 37, would refuse).  So the GPU test's expectation has margin and does not rest on the code under
test.  The ladder of clock errors behind CLOCK_PPM: DESIGN.md 4.19."""
import pytest

import channel_loop as CL
import channel_model as CM
import resample_loop as RL
import resample_model as RM


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample_loop_host_models")
    return CM.build_host_model(d), RM.build_host_model(d)


@pytest.mark.parametrize("snr_db", [CL.SNR_DB, CL.SNR_DB - 3.0])
def test_the_top_of_the_ladder_delivers_and_the_tests_run_at_half_of_it(oracle, hosts, snr_db):
    """the rung that CLOCK_PPM is half of, run here: the largest error of the ladder still delivers everything at both noise levels (the
    whole ladder: resample_loop.sweep, recorded in DESIGN.md 4.19)"""
    top = max(RL.LADDER_PPM)
    bad, offsets, exp = RL.run_clock(oracle, hosts[0], hosts[1], top, snr_db)
    print(f"{top} ppm at {snr_db} dB: fine time offsets {offsets}, FIB CRCs {exp['fib_crc_ok']}")
    assert not bad, bad
    assert RL.CLOCK_PPM == top / 2


@pytest.mark.parametrize("snr_db", [CL.SNR_DB, CL.SNR_DB - 3.0])
def test_clock_error_through_the_oracle_chain_delivers_every_byte(oracle, hosts, snr_db):
    bad, offsets, exp = RL.run_clock(oracle, hosts[0], hosts[1], RL.CLOCK_PPM, snr_db)
    print(f"{RL.CLOCK_PPM} ppm at {snr_db} dB: fine time offsets {offsets}, FIB CRCs {exp['fib_crc_ok']}")
    assert not bad, bad
    assert offsets[0] - offsets[-1] >= 38                                    # the drift is there: 4 frames x 9.83 samples


@pytest.mark.parametrize("snr_db", [CL.SNR_DB, CL.SNR_DB - 3.0])
def test_up_to_2400000_and_back_down_delivers_every_byte(oracle, hosts, snr_db):
    bad, offsets, exp = RL.run_updown(oracle, hosts[0], hosts[1], snr_db)
    print(f"2.048 -> 2.4 -> 2.048 MS/s at {snr_db} dB: fine time offsets {offsets}, FIB CRCs {exp['fib_crc_ok']}")
    assert not bad, bad
