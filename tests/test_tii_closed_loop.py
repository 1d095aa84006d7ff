"""CPU closed loop of TII (include/dabgpu.h, "TII"): the oracle's transmitter with a NULL symbol made by tests/tii_model.py -> the channel
of tests/channel_model.py (a second path 200 samples late at -6 dB, a carrier offset of 3.05 carrier spacings, 37 samples late, noise)
-> the oracle's synchroniser, frame by frame as a receiver runs it (coarse frequency, fine time, demodulator, fine-frequency update)
-> the float32 host model of the detector, fed with the record the synchroniser leaves after each frame.

What the loop shows about the synchroniser's record (the reference's arithmetic, ofdm_demodulator.cpp:438-467 and :829-840): on
acquisition the coarse estimate is a weighted mean of three bins (-3.0x spacings here) and the fine word takes the remainder through
fmodf(., 0.505 spacings), which is no rounding to the nearest carrier: it leaves up to half a spacing in it (3.0x -> 0.49).  The record of
the FIRST frame after acquisition is therefore up to half a carrier spacing off; the fine-frequency update (beta 0.9) has it within
0.05 spacings after that frame and within 0.005 after the next.  A NULL symbol transformed half a spacing off puts a third of every
pair's power into the neighbouring combs, so the detector must not be fed the first frame after an acquisition
(DABGPU_TII_SETTLE_FRAMES = 1).  The tests below pin both halves: the settled loop is exact, the unsettled frame is what lights the
neighbours.

SNR here = power of the received frame (both paths, mean over the data symbols) over the noise power.  TII_MIN_SNR_DB is the lowest SNR
of a 1 dB grid at which this chain was exact for 16 noise seeds (tools-free sweep: `python tests/test_tii_closed_loop.py`); the tests
run 3 dB above it."""
import numpy as np
import pytest

import channel_model as CM
import tii_model as M

S, NULL = 196608, 2656
P = 3200                                     # a frame's PRS is expected P samples into its slice; its NULL period begins at P - NULL
STRIDE = P + 1544 + S
LEAD = 4096                                  # silence before the first frame, so that its slice begins inside the stream
LATE, CFO = 37, 3.05 / 2048
TXS = [(11, 5, 1.0), (40, 17, 0.5), (33, 17, 0.7)]
# three transmitters, two of them on comb 17: one clean record and the union of the two main ids (a fourth would be needed for a second
# clean record; the definition gives exactly these two)
EXPECTED = [(5, 11, M.TABLE[11]), (17, -1, M.TABLE[40] | M.TABLE[33])]
SETTLE = 1                                   # DABGPU_TII_SETTLE_FRAMES
TII_MIN_SNR_DB = 9.0                         # the sweep's result (see sweep() and DESIGN.md 4.17)
TEST_SNR_DB = TII_MIN_SNR_DB + 3.0


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("tii_host_model"))


@pytest.fixture(scope="module")
def chan(tmp_path_factory):
    return CM.build_host_model(tmp_path_factory.mktemp("tii_channel_model"))


_tx = {}


def transmitted(oracle, tii_frames, n_frames=4):
    """n_frames frames of the oracle's modulator back to back (NULL first), the NULL periods of `tii_frames` replaced by the model's; and
    the power of a data sample"""
    key = (tuple(tii_frames), n_frames)
    if key not in _tx:
        rng = np.random.default_rng(7100)
        x = np.concatenate([oracle.modulate_frame(rng.integers(0, 2, oracle.NB_FRAME_BITS).astype(np.uint8)) for _ in range(n_frames)])
        power = float(np.mean(np.abs(x[NULL:S].astype(np.complex128)) ** 2))
        null = M.null_period(oracle.prs_fft(), TXS)
        # amp = 1 is the per-carrier power of a data carrier: the model's unnormalised inverse transform against the oracle's scaling
        prs_bin = np.abs(oracle.fft_n(x[NULL + 504:NULL + 504 + 2048])[1])
        null = (null * (prs_bin / 2048.0)).astype(np.complex64)
        for f in tii_frames:
            x[f * S:f * S + NULL] = null
        _tx[key] = (x, power)
    return _tx[key]


def received(oracle, chan, tii_frames, snr_db, seed, n_frames=4, signal=True):
    x, power = transmitted(oracle, tii_frames, n_frames)
    sigma = float(np.sqrt(1.25 * power / 10.0 ** (snr_db / 10.0) / 2.0))
    prm = CM.params_dict(taps=[(0, 1.0, 0.0), (200, 0.5, 0.0)], freq_q64=int(round(CFO * 2 ** 64)), start=LATE, seed=seed,
                         gain=1.0 if signal else 0.0, noise_sigma=sigma)
    x = np.concatenate([np.zeros(LEAD, np.complex64), x])
    return CM.host_apply(chan, [prm], x, 0, x.size + STRIDE, False)[0]


def run_loop(oracle, host, rx, n_frames=4, settle=SETTLE, threshold=2.16):
    """the receiver's frame loop; the detector sees every frame from `settle` frames after the acquisition on, with the synchroniser's
    record as it stands after that frame.  Returns (records of the last decision, the net offsets in carrier spacings, the model)"""
    conj_ref, time_ref = oracle.sync_refs()
    st = oracle.SyncState(0.0, 0.0, 0, 0, 0, 0)
    m = M.HostModel(host, oracle, threshold)
    nets, locked = [], 0
    for j in range(n_frames):
        sl = rx[LEAD + j * S + NULL - P:LEAD + j * S + NULL - P + STRIDE]
        prs_sym = sl[P:P + 2048]
        oracle.coarse_freq_sync(prs_sym, st, None, time_ref)
        f = np.float32(np.float32(st.freq_coarse) + np.float32(st.freq_fine))
        ok, off, _ = oracle.fine_time_sync(prs_sym, f, None, conj_ref)
        if not ok:
            st = oracle.SyncState(0.0, 0.0, 0, 0, 0, 0)
            locked = 0
            nets.append(None)
            continue
        r = oracle.demod_frame(sl[P + off:P + off + S], f)
        st.freq_fine = float(oracle.update_fine_freq(st.freq_fine, r["total_phase"]))
        net = np.float32(np.float32(st.freq_coarse) + np.float32(st.freq_fine))
        nets.append(float(net) * 2048)
        if locked >= settle:
            m.process(sl, P - NULL + off, net)
        locked += 1
    return m.decide(), nets, m


def test_closed_loop_through_the_synchroniser(oracle, host, chan):
    """four frames, TII in frames 1 and 3, three transmitters: exactly the clean record and the union record"""
    rx = received(oracle, chan, (1, 3), TEST_SNR_DB, 0x7101)
    rec, nets, m = run_loop(oracle, host, rx)
    print("net offsets after each frame (carrier spacings):", nets, "records:", rec)
    assert m.frames == 3
    assert M.records_as_tuples(rec) == EXPECTED, rec
    # the record after the first frame is the coarse estimate's remainder away; after the second the loop is settled
    assert 0.2 < abs(nets[0] + 3.05) <= 0.52 and all(abs(n + 3.05) < 0.06 for n in nets[1:]), nets


def test_the_frame_after_acquisition_is_what_lights_the_neighbours(oracle, host, chan):
    """TII in every frame at 20 dB: fed from the first frame on the decision carries the combs next to the transmitters' (the record is
    0.45 spacings off in that frame), fed from the second frame on it is exact"""
    rx = received(oracle, chan, (0, 1, 2, 3), 20.0, 0x7102)
    rec, nets, _ = run_loop(oracle, host, rx, settle=1)
    assert M.records_as_tuples(rec) == EXPECTED, rec
    rec0, _, _ = run_loop(oracle, host, rx, settle=0)
    print("unsettled:", rec0)
    subs = {int(r["sub_id"]) for r in rec0}
    assert {5, 17} < subs and subs <= {4, 5, 6, 16, 17, 18}, rec0


def test_noise_alone_through_the_loop(oracle, host, chan):
    """64 seeds: the transmitter's frames at the test SNR without any TII, and noise without a transmitter -- no record either way"""
    for seed in range(64):
        rx = received(oracle, chan, (), TEST_SNR_DB, 0x7200 + seed, n_frames=3)
        rec, nets, m = run_loop(oracle, host, rx, n_frames=3)
        assert m.frames == 2 and len(rec) == 0, (seed, rec)
    # no transmitter at all: the synchroniser never locks, a caller with a fixed position feeds the detector all the same
    m = M.HostModel(host, oracle, 2.16)
    for seed in range(64):
        rx = received(oracle, chan, (), 0.0, 0x7300 + seed, n_frames=1, signal=False)
        m.reset()
        for f in range(2):
            m.process(rx, 4000 * f, np.float32(-CFO))
        assert len(m.decide()) == 0, seed


def test_exact_over_16_seeds_at_the_test_snr(oracle, host, chan):
    for seed in range(16):
        rec, _, _ = run_loop(oracle, host, received(oracle, chan, (1, 3), TEST_SNR_DB, 0x7400 + seed))
        assert M.records_as_tuples(rec) == EXPECTED, (seed, rec)


def sweep(oracle, host, chan, grid=range(-6, 16)):
    """SNR (dB) -> number of the 16 seeds at which the chain is exact; the lowest SNR from which every higher one is exact too"""
    table = {}
    for snr in grid:
        table[snr] = sum(M.records_as_tuples(run_loop(oracle, host, received(oracle, chan, (1, 3), float(snr), 0x7400 + s))[0]) == EXPECTED
                         for s in range(16))
    lowest = min(s for s in grid if all(table[t] == 16 for t in grid if t >= s))
    return table, lowest


if __name__ == "__main__":
    import os
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(M.ROOT, "oracle"))
    import oracle as O
    O.build()
    tmp = tempfile.mkdtemp()
    print(sweep(O, M.build_host_model(tmp), CM.build_host_model(tmp)))
