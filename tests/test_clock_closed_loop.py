"""CPU: what the clock tracker buys, end to end (tests/clock_loop.py): the loop of tests/resample_loop.py with a sampling-clock error
applied by the resampler's host model, the tracker's float32 host model behind every frame's demodulation, the state carried over the
five frames, one pass per frame, gain 1.  At (SNR 12 dB, 150 ppm), (12, 200), (12, -200), (15, 200) and (9, 150) the de-rotated products
deliver all 60 FIB CRCs and every byte where the plain weighted bits lose 76, 687, 638, 649 and 213 bytes (measured with these float32
models; the tracked ppm of the five frames are in DESIGN 4.33).  Without a clock error both paths deliver.  At (9 dB, 200 ppm) and
(12 dB, 400 ppm), the documented limits, the tracked path still loses bytes (3 and 54 against 775 and 948) and does no worse than plain.
The tracked ppm in frames 2 to 4 at (12 dB, 200 ppm) stays within twice the worst deviation seen over eight noise seeds (4.36 ppm)."""
import numpy as np
import pytest

import clock_loop as L


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    return L.Loop(oracle, tmp_path_factory.mktemp("clock_loop"))


@pytest.mark.parametrize("snr_db,ppm", L.POINTS)
def test_tracked_products_deliver_under_a_clock_error(loop, snr_db, ppm):
    b = loop.branch(snr_db, ppm)
    c = loop.counts(snr_db, ppm)
    print(f"SNR {snr_db} dB, {ppm} ppm: {c}; tracked {[round(float(x), 1) for x in b['ppm']]} ppm")
    assert b["valid"].all() and b["clock_ok"].all()                    # no frame refused: the difference is the de-rotation's
    assert c["tracked"] == L.DELIVERED
    assert c["plain"][1] >= L.CONTRAST and c["plain"][0] <= c["tracked"][0]
    assert (np.sign(b["ppm"]) == np.sign(ppm)).all()                   # a stream made with +X tracks to +X
    # |what is left| shrinks over the first frames: the state is carried
    assert abs(ppm - b["ppm"][1]) < abs(ppm - b["ppm"][0]) < abs(ppm)


@pytest.mark.parametrize("snr_db,ppm", L.CLEAN)
def test_without_a_clock_error_the_tracking_costs_nothing(loop, snr_db, ppm):
    b = loop.branch(snr_db, ppm)
    c = loop.counts(snr_db, ppm)
    print(f"SNR {snr_db} dB, no clock error: {c}; tracked {[round(float(x), 1) for x in b['ppm']]} ppm")
    assert b["valid"].all() and b["clock_ok"].all()
    assert c == {p: L.DELIVERED for p in L.PATHS}
    assert np.abs(b["ppm"]).max() < L.ACCURACY_BOUND_PPM


@pytest.mark.parametrize("snr_db,ppm", L.LIMITS)
def test_the_documented_limits(loop, snr_db, ppm):
    c = loop.counts(snr_db, ppm)
    print(f"SNR {snr_db} dB, {ppm} ppm: {c}; tracked {[round(float(x), 1) for x in loop.branch(snr_db, ppm)['ppm']]} ppm")
    assert c["tracked"][0] >= c["plain"][0] and c["tracked"][1] <= c["plain"][1]


def test_accuracy_of_the_tracked_ppm(loop):
    snr_db, ppm = L.ACCURACY_POINT
    worst = 0.0
    for seed in L.ACCURACY_SEEDS:
        b = loop.branch(snr_db, ppm, seed=seed)
        dev = max(abs(float(b["ppm"][j]) - ppm) for j in L.ACCURACY_FRAMES)
        print(f"seed {seed:#x}: tracked {[round(float(x), 2) for x in b['ppm']]} ppm, worst of frames 2 to 4 {dev:.2f}")
        assert b["valid"].all() and b["clock_ok"].all()
        worst = max(worst, dev)
    print(f"worst deviation {worst:.2f} ppm; measured {L.ACCURACY_MEASURED_PPM}, bound {L.ACCURACY_BOUND_PPM}")
    assert worst <= L.ACCURACY_BOUND_PPM
