"""CPU: what the estimated weights buy, end to end (tests/noise_loop.py): the transmission of tests/channel_loop.py through its static
two-path channel, heard by two branches whose noise differs by 9 dB, combined by the numpy model of csrc/diversity_core.h with unit
weights, with the weights the estimator's host model takes from each frame's NULL window, and with the true weights 1 / (2 sigma^2) of
the channels.  The operating point was chosen on the CPU by the sweep DESIGN 4.26 records (3 .. 14 dB): at 7 dB of branch A, and 1 dB
either side, the estimated weights deliver every FIB and byte, unit weights lose most of them, and the estimated weights count exactly
what the true ones count."""
import pytest

import channel_loop as CL
import noise_loop as NL

POINT_DB = NL.POINT_DB


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    return NL.Loop(oracle, tmp_path_factory.mktemp("noise_loop"))


@pytest.mark.parametrize("snr_db", [POINT_DB - 1.0, POINT_DB, POINT_DB + 1.0])
def test_estimated_weights_deliver_where_unit_weights_do_not(loop, snr_db):
    alone, unit = loop.single(snr_db, "A"), loop.pair(snr_db, "unit")
    est, true = loop.pair(snr_db, "estimated"), loop.pair(snr_db, "true")
    print(f"{snr_db} dB: A alone {alone}, unit {unit}, estimated {est}, true {true}")
    for name in ("A", "B"):
        assert loop.branch(snr_db, name)["valid"].all()                # no frame refused: the difference is the weights'
    assert est == NL.DELIVERED                                          # (a)
    assert unit[0] < 12 * CL.N_FRAMES and unit[1] > 0                   # (b)
    assert est == true                                                  # (c)


def test_estimated_weights_follow_the_channels(loop):
    """the estimates behind the weights: each branch's noise within five of the model's deviations of its channel's 2 sigma^2 in every
    frame, so the weights' ratio is the 9 dB that was put in"""
    import numpy as np
    import noise_model as NM
    for name in ("A", "B"):
        b = loop.branch(POINT_DB, name)
        ratio = b["noise"] / (2.0 * loop.sigma(POINT_DB, name) ** 2)
        assert (np.abs(ratio - 1.0) < 5.0 * NM.relative_deviation()).all(), (name, ratio)
    a, b = loop.branch(POINT_DB, "A"), loop.branch(POINT_DB, "B")
    # the ratio of two independent estimates: sqrt 2 of one estimate's deviation, five of those
    assert (np.abs(a["w"] / b["w"] / 10.0 ** (NL.EXTRA_DB / 10.0) - 1.0) < 5.0 * 2.0 ** 0.5 * NM.relative_deviation()).all()


def test_never_worse_than_unit_weights(loop):
    """over the swept points the estimated pair never counts fewer FIBs or more wrong bytes than the unit-weight pair"""
    for snr_db in (3.0, 5.0, 9.0, 11.0, 14.0):
        unit, est = loop.pair(snr_db, "unit"), loop.pair(snr_db, "estimated")
        assert est[0] >= unit[0] and est[1] <= unit[1], (snr_db, unit, est)
