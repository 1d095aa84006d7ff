"""CPU: the closed loop of tests/softbit_loop.py -- oracle transmitter -> fading host model (`tu6`, six Rayleigh taps at 10 Hz, timing 37,
no carrier offset) -- through the UNSYNCHRONISED state machine: the received samples behind a lead-in of their own signal, fed in blocks
of 65536 to tests/stream_soft_model.py (level, NULL search, synchroniser, fine-frequency loop; the frame as the state machine assembles
it, not cut at a known position), soft bits of either policy composed from the oracle's transform, the oracle's FIC and MSC decoders.
This is the expected side of tests/test_gpu_stream_bank_soft_loop.py: it fails without the stream bank's weighted policy only in the sense
that its device twin does; its job is to fix the expectations.

At both points the model completes all five frames without a desync.  Counted: FIB CRCs of 60 / wrong bytes of the EEP 3-A
sub-channel's five delivered logical frames, measured with this construction:

    point              normalised   weighted
    (10 dB, seed 1)    (44, 26)     (59, 8)
    (10 dB, seed 7)    (38, 64)     (54, 0)

(Points at which a stream loses its first frame exist too -- (10 dB, seed 2) and (8 dB, seed 0), 4 and 3 frames -- and are not used for
delivery counts.)"""
import pytest

import channel_fading_model as FM
import channel_loop as CL
import softbit_model as SM
import stream_soft_model as SSM


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    host = FM.build_host_model(tmp_path_factory.mktemp("stream_soft_loop_host_model"))
    fib, pay, nb = CL.inputs(oracle)
    return host, CL.oracle_iq(oracle, fib, pay), fib, pay, nb


@pytest.mark.parametrize("snr_db,seed", SSM.LOOP_POINTS)
def test_weighted_soft_bits_through_the_unsynchronised_receiver(oracle, loop, snr_db, seed):
    host, iq, fib, pay, nb = loop
    stream, model, counts = SSM.loop_cpu_point(oracle, host, iq, fib, pay, nb, snr_db, seed)
    print(f"{snr_db} dB, fading seed {seed}: {len(model.out_frames)} frames, {model.frames_desync} desyncs, offsets {[fr['offset'] for fr in model.out_frames]}")
    assert len(model.out_frames) == CL.N_FRAMES == 5 and model.frames_desync == 0
    norm, csi = counts[SM.SOFT_NORMALISED], counts[SM.SOFT_CSI]
    print(f"{snr_db} dB, fading seed {seed}: normalised {norm}, weighted {csi} (FIB CRCs of 60, wrong bytes)")
    assert csi[0] > norm[0], "more FIB CRCs under the weighted policy"
    assert csi[1] < norm[1], "fewer wrong bytes under the weighted policy"
