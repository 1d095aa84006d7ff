"""CPU: the consumers of DQPSK products behind the UNSYNCHRONISED state machine (tests/stream_products_model.py): clock_loop.Loop.stream
at (SNR, sampling-clock error) -> stream_soft_model.loop_stream's lead-in -> StreamSoftModel in blocks of 65536 -> the clock tracker's
host model over fr["dq"], state carried, gain 1 -> softbit_model.frame_bits at the frame's scale -> the oracle's FIC and MSC decoders.
This is the expected side of tests/test_gpu_stream_products_loop.py and fixes what the stream bank's products
(dabgpu_stream_bank_set_products) must deliver: its job is to show that the tracker works on frames the state machine assembled itself,
not cut at a known position.

At every point the model finds all five frames without a desync.  At +-200 ppm the tracked path delivers strictly more FIB CRCs and
strictly fewer wrong bytes than the plain weighted bits; without a clock error the two paths count the same.  The test prints the counts
and the tracked ppm after each frame (DESIGN 4.34 tabulates them)."""
import pytest

import clock_loop as L
import stream_products_model as SPM


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    return L.Loop(oracle, tmp_path_factory.mktemp("stream_products_loop"))


@pytest.mark.parametrize("snr_db,ppm", SPM.POINTS)
def test_tracker_behind_the_unsynchronised_receiver(oracle, loop, snr_db, ppm):
    p = SPM.cpu_point(oracle, loop, snr_db, ppm)
    m = p["model"]
    print(f"SNR {snr_db} dB, {ppm} ppm: {len(m.out_frames)} frames, {m.frames_desync} desyncs, offsets {[fr['offset'] for fr in m.out_frames]}")
    assert len(m.out_frames) == SPM.N_FRAMES == 5 and m.frames_desync == 0
    plain, tracked = p["counts"]["plain"], p["counts"]["tracked"]
    print(f"SNR {snr_db} dB, {ppm} ppm: plain {plain}, tracked {tracked} (FIB CRCs of 60, wrong bytes); tracked ppm {[round(x, 1) for x in p['ppm']]}")
    if ppm != 0.0:
        assert tracked[0] > plain[0], "more FIB CRCs on the de-rotated products"
        assert tracked[1] < plain[1], "fewer wrong bytes on the de-rotated products"
    else:
        assert tracked == plain, "without a clock error the tracking costs nothing"
