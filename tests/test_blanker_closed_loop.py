"""CPU: the impulse blanker in the closed loop of the CPU models (tests/blanker_loop.py): tests/interferer_loop.py's transmission, channel
and burst source -- white noise on 205 of every 20480 samples -- then the blanker's float32 host model at the default parameters, then the
unchanged receiver with plain weighted soft bits.  DESIGN.md 4.29 holds the table these assertions come from: with the blanker every FIB
(CRC) and every byte arrives and every frame synchronises at I / S 11 .. 23 dB, where the unblanked stream loses 6 .. 25 FIBs of 60 (and
one frame of five at 23 dB); without an interferer nothing is flagged and nothing changes; a steady band source gets a few blocks in a
thousand flagged (narrowband noise has a slow envelope), which is the documented limit."""
import pytest

import blanker_loop as BL
import channel_loop as CL

SNR_POINT = BL.SNR_DB


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    return BL.Loop(oracle, tmp_path_factory.mktemp("blanker_loop"))


@pytest.mark.parametrize("snr_db,is_db", [(SNR_POINT, 11.0), (SNR_POINT, 14.0), (SNR_POINT, 17.0), (SNR_POINT, 20.0), (SNR_POINT, 23.0),
                                          (SNR_POINT - 3, 17.0), (SNR_POINT + 3, 17.0)])
def test_blanked_bursts_cost_nothing(loop, snr_db, is_db):
    plain, blanked = loop.plain(snr_db, is_db, "burst"), loop.blanked(snr_db, is_db, "burst")
    _, _, n, total = loop.blanked_stream(snr_db, is_db, "burst")
    print(f"SNR {snr_db} dB, bursts at I / S {is_db} dB: unblanked {plain}, blanked {blanked}, {n} of {total} blocks blanked")
    assert blanked == BL.DELIVERED                                          # every FIB (CRC), no wrong byte
    assert loop.blanked_branch(snr_db, is_db, "burst")["valid"].all()       # every frame synchronised
    assert plain[0] < 12 * CL.N_FRAMES                                      # the unblanked stream delivers fewer than the 60 FIBs
    assert n <= 0.02 * total                                                # 1 % of the samples in bursts: at most 2 % of the blocks


@pytest.mark.parametrize("snr_db", [SNR_POINT - 6, SNR_POINT - 3, SNR_POINT + 3])
def test_without_an_interferer_nothing_is_flagged(loop, snr_db):
    y, m, n, total = loop.blanked_stream(snr_db, None)
    assert n == 0 and not m.any() and total == 30848
    assert y.tobytes() == loop.stream(snr_db, None).tobytes()
    assert loop.blanked(snr_db, None) == loop.plain(snr_db, None)


def test_steady_band_source_false_alarms_stay_below_one_percent(loop):
    """the limit DESIGN.md 4.29 documents: the share is printed and held below 1 % of the blocks; the band at I / S 0 dB delivers no FIB
    through the plain soft bits either way (the banded combiner is the defence there), and the counts are held to what the model finds"""
    plain, blanked = loop.plain(SNR_POINT, 0.0, "band"), loop.blanked(SNR_POINT, 0.0, "band")
    _, _, n, total = loop.blanked_stream(SNR_POINT, 0.0, "band")
    print(f"steady band at I / S 0 dB: {n} of {total} blocks blanked ({100.0 * n / total:.2f} %), unblanked {plain}, blanked {blanked}")
    assert n < 0.01 * total
    # what the committed model finds: no FIB either way, and the wrong bytes of the sub-channel move from 449 to 462 --
    # the blanker neither rescues this case nor costs a FIB in it
    assert n == 114
    assert plain == (0, 449) and blanked == (0, 462)
