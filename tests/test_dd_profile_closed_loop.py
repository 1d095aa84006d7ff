"""CPU: what the decision-directed profile buys, end to end (tests/dd_profile_loop.py): the loop of tests/noise_profile_loop.py with its
band interferer gated off around every NULL symbol.  At SNR 12 dB with I / S of -3, 0 and +3 dB, and at SNR 9 dB with I / S 0 dB (the
points were measured again with these models: DESIGN 4.30), the banded combiner with the decision-directed weights delivers all 60 FIBs
and every byte at both alphas, where the same combiner with the NULL-based weights and the plain weighted soft bits deliver at most 15
FIBs (13 is the most seen).  With the interferer left on through the NULL both profiles deliver; without an interferer at 7 dB all three
paths deliver."""
import numpy as np
import pytest

import dd_profile_loop as DL


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    return DL.Loop(oracle, tmp_path_factory.mktemp("dd_profile_loop"))


@pytest.mark.parametrize("snr_db,is_db", DL.POINTS)
def test_decision_directed_weights_deliver_under_a_gated_interferer(loop, snr_db, is_db):
    assert loop.branch(snr_db, is_db)["valid"].all()                   # no frame refused: the difference is the weights'
    for a in DL.ALPHAS:
        c = loop.counts(snr_db, is_db, True, a)
        print(f"SNR {snr_db} dB, I / S {is_db} dB, gated, alpha {a}: {c}")
        assert c["dd"] == DL.DELIVERED
        assert c["null"][0] <= DL.FAIL_CAP and c["null"][1] > 0
        assert c["plain"][0] <= DL.FAIL_CAP and c["plain"][1] > 0


def test_both_profiles_deliver_when_the_null_hears_the_interferer(loop):
    for a in DL.ALPHAS:
        c = loop.counts(*DL.UNGATED, False, a)
        print(f"SNR {DL.UNGATED[0]} dB, I / S {DL.UNGATED[1]} dB, ungated, alpha {a}: {c}")
        assert c["dd"] == DL.DELIVERED and c["null"] == DL.DELIVERED and c["plain"][0] <= DL.FAIL_CAP


def test_without_an_interferer_the_weighting_costs_nothing(loop):
    assert loop.branch(DL.CLEAN_SNR_DB, None)["valid"].all()
    for a in DL.ALPHAS:
        assert loop.counts(DL.CLEAN_SNR_DB, None, True, a) == {p: DL.DELIVERED for p in ("plain", "null", "dd")}
    w = loop.branch(DL.CLEAN_SNR_DB, None)["dd"][1.0]
    assert (w.max(axis=1) / w.min(axis=1) < 2.0).all()                 # nearly flat: the two-path channel's ripple through the bias at low SNR


def test_profile_follows_the_interferer_and_the_null_does_not(loop):
    """the weights behind the counts at the operating point: bands 85 .. 91 lie wholly under the interferer (places 1019.3 .. 1115.3 of the
    1536).  The decision-directed noise of those bands is tens of times that of the bands clear of it; the NULL-based one, which hears a
    gated interferer's silence, is not even twice."""
    b = loop.branch(12.0, 0.0)
    inside, clear = np.arange(86, 91), np.r_[0:80, 97:128]
    for j in range(5):
        dd, null = 1.0 / b["dd"][1.0][j], 1.0 / b["w"][1.0][j]
        assert dd[inside].min() > 20.0 * np.median(dd[clear]), j
        assert np.median(null[inside]) < 2.0 * np.median(null[clear]), j
