"""CPU: what the symbol weights buy, end to end (tests/sym_profile_loop.py): the loop of tests/dd_profile_loop.py under a white burst of
three OFDM symbols every 60000 samples.  At SNR 12 dB with I / S of +3, +6 and +9 dB, and at SNR 9 dB with I / S +6 dB (the points were
measured again with these float32 models: DESIGN 4.31), the symbol-weighted combiner delivers every byte of the sub-channel, on top of
the plain weighted soft bits and on top of the decision-directed band weights, where either of those alone loses 25 bytes and more; the
FIBs under the bursts are lost on every path (the FIC is not time-interleaved).  Without a burst all paths deliver and no row falls below
0.8; at I / S +12 dB, where the synchroniser refuses a frame, the weights do no worse than plain."""
import numpy as np
import pytest

import sym_profile_loop as L


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    return L.Loop(oracle, tmp_path_factory.mktemp("sym_profile_loop"))


@pytest.mark.parametrize("snr_db,is_db", L.POINTS)
def test_symbol_weights_deliver_under_a_white_burst(loop, snr_db, is_db):
    b = loop.branch(snr_db, is_db)
    c = loop.counts(snr_db, is_db)
    print(f"SNR {snr_db} dB, I / S {is_db} dB: {c}; smallest weight {b['v'].min():.4f}, rows below 0.5: {(b['v'] < 0.5).sum(axis=1).tolist()}")
    assert b["valid"].all() and b["sym_ok"].all()                      # no frame refused: the difference is the weights'
    assert c["plain+sym"][1] == 0 and c["dd+sym"][1] == 0
    assert c["plain+sym"][0] >= c["plain"][0] and c["dd+sym"][0] >= c["plain"][0]
    assert c["plain"][1] >= L.CONTRAST and c["dd"][1] >= L.CONTRAST


def test_without_a_burst_the_weighting_costs_nothing(loop):
    b = loop.branch(L.CLEAN_SNR_DB, None)
    c = loop.counts(L.CLEAN_SNR_DB, None)
    print(f"SNR {L.CLEAN_SNR_DB} dB, no burst: {c}; smallest weight {b['v'].min():.4f}")
    assert b["valid"].all() and b["sym_ok"].all()
    assert c == {p: L.DELIVERED for p in L.PATHS}
    assert b["v"].min() > 0.8 and ((b["v"] == 1).sum(axis=1) >= 38).all()


def test_the_documented_limit(loop):
    """I / S +12 dB: the synchroniser refuses a frame and the count is bounded by that; the weights do no worse than plain"""
    c = loop.counts(*L.LIMIT)
    print(f"SNR {L.LIMIT[0]} dB, I / S {L.LIMIT[1]} dB: {c}; valid {loop.branch(*L.LIMIT)['valid'].tolist()}")
    for p in ("plain+sym", "dd+sym"):
        assert c[p][0] >= c["plain"][0] and c[p][1] <= c["plain"][1]


def test_weights_follow_the_bursts(loop):
    """the weights behind the counts at SNR 12 dB, I / S +6 dB: a row whose two symbols both lie wholly under a burst weighs less than a
    fifth, and more than half of each frame's rows keep weight 1"""
    b = loop.branch(12.0, 6.0)
    g = L.gate(L.CL.N_OUT)
    for j in range(L.CL.N_FRAMES):
        prs = j * 196608 + 2656                                        # the frame's phase reference symbol in the stream, within the timing offset
        inside = [s for s in range(75) if g[prs + s * 2552 - 100:prs + (s + 2) * 2552 + 100].all()]      # product s: symbols s and s + 1
        assert len(inside) >= 2, (j, inside)
        assert (b["v"][j][inside] < 0.2).all(), (j, inside, b["v"][j][inside])
        assert (b["v"][j] == 1).sum() >= 38
