"""CPU: the banded path driven by the library's own interferer, end to end on the CPU models (tests/interferer_loop.py): the transmission
of tests/channel_loop.py -> channel host model with white noise -> interferer host model -> synchroniser and demodulator oracle ->
noise-profile and banded-combiner host models -> decoders.  The band source has DESIGN 4.27's geometry: 96 kHz wide, 300 carrier spacings
above the centre.  The operating point, SNR 12 dB and I / S = 0 dB, comes from the CPU sweep DESIGN 4.28 records (SNR 6 .. 15 dB, I / S
none, -12 .. +6 dB): with 3 dB to either side of both, the banded path delivers every FIB (CRC) and every transmitted byte at both alphas
and the plain weighted soft bits on the same samples deliver fewer than half the FIBs.  (At SNR 6 dB the channel alone already loses a
FIB; at I / S = +6 dB the synchroniser refuses two frames of five.)  Bursts -- white noise on for 100 us every 10 ms -- at I / S = 17 dB
while on, and 3 dB either side, do not break the synchroniser; the sweep shows them costing about a quarter of the FIBs whatever the soft
bits, since the band weights know nothing of time."""
import pytest

import channel_loop as CL
import interferer_loop as IL

SNR_POINT, IS_POINT = IL.SNR_DB, IL.POINT_DB
BURST_POINT = IL.BURST_DB


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    return IL.Loop(oracle, tmp_path_factory.mktemp("interferer_loop"))


@pytest.mark.parametrize("snr_db,is_db", [(SNR_POINT, IS_POINT), (SNR_POINT - 3, IS_POINT), (SNR_POINT + 3, IS_POINT), (SNR_POINT, IS_POINT - 3),
                                          (SNR_POINT, IS_POINT + 3)])
def test_banded_path_delivers_where_plain_soft_bits_do_not(loop, snr_db, is_db):
    plain = loop.plain(snr_db, is_db)
    banded = {a: loop.banded(snr_db, is_db, a) for a in IL.ALPHAS}
    print(f"SNR {snr_db} dB, I / S {is_db} dB: plain {plain}, banded {banded}")
    assert loop.branch(snr_db, is_db)["valid"].all()                   # no frame refused: the difference is the weights'
    for a in IL.ALPHAS:
        assert banded[a] == IL.DELIVERED                                # every FIB (CRC), no wrong byte
    assert plain[0] < 6 * CL.N_FRAMES                                   # fewer than half of the 60 FIBs


def test_without_an_interferer_both_deliver(loop):
    for snr_db in (SNR_POINT - 3, SNR_POINT, SNR_POINT + 3):
        assert loop.plain(snr_db, None) == IL.DELIVERED
        for a in IL.ALPHAS:
            assert loop.banded(snr_db, None, a) == IL.DELIVERED


@pytest.mark.parametrize("is_db", [BURST_POINT - 3, BURST_POINT, BURST_POINT + 3])
def test_bursts_do_not_break_the_synchroniser(loop, is_db):
    """the sweep at SNR 12 dB: every frame synchronised up to 20 dB (at 23 dB one of five is refused); FIBs delivered, of 60, printed: the
    sweep does not show a margin for a claim on them beyond "some are lost, most arrive" """
    b = loop.branch(SNR_POINT, is_db, "burst")
    plain, banded = loop.plain(SNR_POINT, is_db, "burst"), loop.banded(SNR_POINT, is_db, 0.25, "burst")
    print(f"bursts at I / S {is_db} dB: plain {plain}, banded {banded}")
    assert b["valid"].all()
    assert plain[0] >= 6 * CL.N_FRAMES and banded[0] >= 6 * CL.N_FRAMES
