"""CPU: the closed loop of tests/iqbal_loop.py without the device -- oracle transmitter -> host models of the channel, the combiner, the front
end, the IQ balance and the channeliser -> oracle receive chain -- at the channel loop's noise level and 3 dB below it, with one neighbour
30 dB up at the wanted block's mirror frequency and a front end that rejects it by 29 dB.  Uncorrected the loop delivers at most 15 of 60
FIBs; corrected (prime + correct) it delivers every FIB CRC, FIB body and sub-channel byte with offset 37 in every frame; with no
impairment the corrector changes no delivered byte.  So the GPU test's expectation has margin and does not rest on the code under test.
The ladder of neighbour levels behind the operating point: DESIGN.md 4.32."""
import numpy as np
import pytest

import channel_loop as CL
import channel_model as CHM
import channelise_model as CM
import iqbal_loop as QL
import iqbal_model as IM


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("iqbal_loop_host_models")
    return CHM.build_host_model(d), CM.build_host_model(d), IM.build_host_model(d)


def test_the_operating_point_is_the_one_the_issue_names():
    K1, K2 = IM.front_end(QL.GAIN_DB, QL.PHASE_DEG)
    assert abs(IM.irr_db(K1, K2) - 29.0) < 0.1 and QL.ADJACENT_DB == max(QL.LADDER_DB) == 30.0


@pytest.mark.parametrize("snr_db", [CL.SNR_DB, CL.SNR_DB - 3.0])
def test_uncorrected_the_image_takes_the_block_and_corrected_every_byte_arrives(oracle, hosts, snr_db):
    bad, exp, _ = QL.run(oracle, hosts, QL.ADJACENT_DB, snr_db, impaired=True, corrected=False)
    print(f"uncorrected at {snr_db} dB: {exp['fib_crc_ok']} of 60 FIB CRCs, {bad}")
    assert exp["fib_crc_ok"] <= QL.UNCORRECTED_CAP, "the impairment no longer breaks the uncorrected loop: the contrast has gone"
    bad, exp, rec = QL.run(oracle, hosts, QL.ADJACENT_DB, snr_db, impaired=True, corrected=True)
    K1, K2 = IM.front_end(QL.GAIN_DB, QL.PHASE_DEG)
    w = complex(rec["w_re"][0], rec["w_im"][0])
    print(f"corrected at {snr_db} dB: {exp['fib_crc_ok']} of 60 FIB CRCs, {bad}; residual image rejection {IM.irr_db(*IM.residual(K1, K2, w)):.1f} dB, "
          f"DC error {abs(complex(rec['d_re'][0], rec['d_im'][0]) - QL.DC):.2e}")
    assert not bad, bad
    assert rec["valid"][0] == 1 and rec["tiles_used"][0] == QL.N_WIDE // IM.TILE and rec["tiles_skipped"][0] == 0


@pytest.mark.parametrize("snr_db", [CL.SNR_DB, CL.SNR_DB - 3.0])
def test_without_an_impairment_the_corrector_changes_no_delivered_byte(oracle, hosts, snr_db):
    bad0, exp0, _ = QL.run(oracle, hosts, QL.ADJACENT_DB, snr_db, impaired=False, corrected=False)
    bad1, exp1, rec = QL.run(oracle, hosts, QL.ADJACENT_DB, snr_db, impaired=False, corrected=True)
    assert not bad0 and not bad1, (bad0, bad1)                               # the reference chain alone meets the conditions too
    assert np.array_equal(exp0["fib"], exp1["fib"]) and np.array_equal(exp0["msc"], exp1["msc"]) and exp0["fib_crc_ok"] == exp1["fib_crc_ok"]
    assert abs(complex(rec["w_re"][0], rec["w_im"][0])) < 1e-3               # a perfect front end: 60 dB or better is left as it is
