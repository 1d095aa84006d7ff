"""CPU: the closed loop of tests/channelise_loop.py without the device -- oracle transmitter -> host models of the channel, the combiner
and the channeliser -> oracle receive chain -- at the channel loop's noise level and 3 dB below it, with a neighbour 1.712 MHz to either
side: no sync failure, fine time offset 37 in every frame, every FIB CRC, the transmitted FIB bodies and sub-channel bytes.  So the GPU
test's expectation has margin and does not rest on the code under test.  The ladder of neighbour levels behind ADJACENT_DB: DESIGN.md 4.20."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CHM
import channelise_loop as XL
import channelise_model as CM


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("channelise_loop_host_models")
    return CHM.build_host_model(d), CM.build_host_model(d)


@pytest.mark.parametrize("snr_db", [CL.SNR_DB, CL.SNR_DB - 3.0])
def test_the_top_of_the_ladder_delivers_and_the_tests_run_10_db_under_it(oracle, hosts, snr_db):
    """the top rung of the ladder, run here: it still delivers everything at both noise levels (the whole ladder: channelise_loop.sweep,
    recorded in DESIGN.md 4.20)"""
    top = max(XL.LADDER_DB)
    assert XL.ADJACENT_DB == top - 10.0
    bad, offsets, exp, _, _ = XL.run(oracle, hosts[0], hosts[1], top, snr_db)
    print(f"neighbours {top} dB up at {snr_db} dB: fine time offsets {offsets}, FIB CRCs {exp['fib_crc_ok']}")
    assert not bad, bad


@pytest.mark.parametrize("snr_db", [CL.SNR_DB, CL.SNR_DB - 3.0])
def test_neighbours_through_the_oracle_chain_deliver_every_byte(oracle, hosts, snr_db):
    bad, offsets, exp, wide, back = XL.run(oracle, hosts[0], hosts[1], XL.ADJACENT_DB, snr_db)
    print(f"neighbours {XL.ADJACENT_DB} dB up at {snr_db} dB: fine time offsets {offsets}, FIB CRCs {exp['fib_crc_ok']}")
    assert not bad, bad
    # the neighbours are there: the capture carries 2 x 1000 times the wanted block's power
    p_wide, p_back = float(np.mean(np.abs(wide) ** 2)) * XL.D, float(np.mean(np.abs(back) ** 2))
    assert p_wide > 1500.0 * p_back


def test_the_alias_only_edges_do_not_survive_that_level(oracle, hosts):
    """cutoff 0.5 of the block rate, the resampler's kind of filter: the neighbour's lowest 336 kHz pass the transition band and land beside
    the wanted carriers at full strength -- why the channeliser's default is the sharper design"""
    bad, offsets, exp, _, _ = XL.run(oracle, hosts[0], hosts[1], XL.ADJACENT_DB, CL.SNR_DB, XL.ALIAS_ONLY_EDGES)
    print(f"alias-only edges, neighbours {XL.ADJACENT_DB} dB up at {CL.SNR_DB} dB: {bad}, FIB CRCs {exp['fib_crc_ok']}")
    assert bad
