"""The closed loop that shows what receive diversity buys, shared by its CPU form (tests/test_diversity_closed_loop.py) and its device
form (tests/test_gpu_diversity_loop.py): the transmission of tests/channel_loop.py (five mode I frames, an EEP 3-A and a UEP
sub-channel) heard by several receivers, each through its own realisation of the fading channel of tests/softbit_loop.py -- `tu6`, six
Rayleigh taps at 10 Hz, the signal 37 samples late, no carrier offset -- and its own noise.  A branch is named by its fading seed; its
noise seed is fixed with it (no two branches share one).  Every branch runs the receiver's own per-frame sequence -- coarse frequency
synchronisation, fine time synchronisation, demodulation at the position and offset found, fine-frequency update -- so that a frame
the synchroniser refuses is a dead branch of that frame, exactly as on the device.  Counted: FIB CRCs of the five frames (60) and wrong
bytes of the EEP 3-A sub-channel's five delivered logical frames."""
import numpy as np

import channel_fading_loop as FL
import channel_fading_model as FM
import channel_loop as CL
import channel_model as CM
import diversity_model as DM
import softbit_loop as SL
import softbit_model as SM

LEVEL = SL.LEVEL
# fading seed of a branch -> its noise seed
NOISE_SEED = {1: 0xDAB, 7: 0xDAB + 1, 3: 0xDAB + 2, 6: 0xDAB + 3}
# (SNR dB, the two branches) at which neither branch delivers alone and the pair delivers everything -- also 1 dB below and 1 dB above
POINTS = [(6.0, (3, 6)), (6.0, (1, 3))]
DELIVERED = (12 * CL.N_FRAMES, 0)


def params(iq, snr_db, fading_seed):
    p = SL.params(iq, snr_db)
    p["seed"] = NOISE_SEED[fading_seed]
    return p


def received(host, iq, snr_db, fading_seed):
    P = params(iq, snr_db, fading_seed)
    return FM.host_apply(host, [P], [FL.table(P, fading_seed)], iq, 0, CL.N_OUT, False)[0]


def receive_branch(oracle, rx):
    """the receiver's per-frame sequence over the five slices of one branch (oracle/dab_oracle_chain.c, dab_receive_frames, with the
    weighted policy's scale in place of the soft bits): -> dict(dq [5][75][1536] products in carrier order, k [5], valid [5])"""
    slices = CL.slices_of(rx)
    state = oracle.SyncState(0.0, 0.0, 0, 0, 0, 0)
    conj_ref, time_ref = oracle.sync_refs()
    bins = SL.carrier_bins()
    dq = np.zeros((CL.N_FRAMES, 75, 1536), np.complex64)
    k, valid = np.zeros(CL.N_FRAMES, np.float32), np.zeros(CL.N_FRAMES, np.int32)
    for j in range(CL.N_FRAMES):
        prs = slices[j, CL.P:CL.P + 2048]
        oracle.coarse_freq_sync(prs, state, prs_time_ref=time_ref)
        f = np.float32(np.float32(state.freq_coarse) + np.float32(state.freq_fine))
        ok, off, _ = oracle.fine_time_sync(prs, f, prs_fft_conj=conj_ref)
        if not ok:                                                     # the receiver resets (ofdm_demodulator.cpp:529-532)
            state.freq_coarse, state.freq_fine, state.is_found_coarse = 0.0, 0.0, 0
            continue
        frame = slices[j, CL.P + off:CL.P + off + 196608]
        r = oracle.demod_frame(frame, f, want_fft=True)
        state.freq_fine = float(oracle.update_fine_freq(state.freq_fine, r["total_phase"]))
        X = r["fft"].reshape(77, 2048)[:76, bins]
        dq[j] = SM.dqpsk(X[:-1], X[1:])
        k[j] = SM.soft_scale(frame[SM.NB_CP:SM.NB_CP + SM.NB_FFT], LEVEL)
        valid[j] = 1
    return dict(dq=dq, k=k, valid=valid)


def branch_bits(branch, mapper):
    """the branch's own weighted soft bits [5][230400]; a refused frame stays an erasure"""
    return [SM.frame_bits(branch["dq"][j], mapper, branch["k"][j]) if branch["valid"][j] else np.zeros(DM.NB_FRAME_BITS, np.int8)
            for j in range(CL.N_FRAMES)]


def combined_bits(branches, mapper, weights=None):
    """the frames of several branches combined by the numpy model of csrc/diversity_core.h"""
    return [DM.combine_frame([b["dq"][j] for b in branches], [b["k"][j] for b in branches], mapper, weights, [b["valid"][j] for b in branches])[0]
            for j in range(CL.N_FRAMES)]


class Loop:
    """the transmission once; branches are received once per (SNR, fading seed) and kept"""

    def __init__(self, oracle, tmp_dir):
        self.oracle = oracle
        self.host = FM.build_host_model(tmp_dir)
        self.fib, self.pay, self.nb = CL.inputs(oracle)
        self.iq = CL.oracle_iq(oracle, self.fib, self.pay)
        self.mapper = oracle.mapper()
        self._branches = {}

    def branch(self, snr_db, seed):
        key = (float(snr_db), seed)
        if key not in self._branches:
            self._branches[key] = receive_branch(self.oracle, received(self.host, self.iq, snr_db, seed))
        return self._branches[key]

    def count(self, bits):
        return SL.count(self.oracle, bits, self.fib, self.pay, self.nb)

    def single(self, snr_db, seed):
        return self.count(branch_bits(self.branch(snr_db, seed), self.mapper))

    def combined(self, snr_db, seeds):
        return self.count(combined_bits([self.branch(snr_db, s) for s in seeds], self.mapper))

    def refused(self, snr_db, seeds):
        return int(sum((self.branch(snr_db, s)["valid"] == 0).sum() for s in seeds))
