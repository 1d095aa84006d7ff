"""The closed loop that shows what the estimated weights buy, for tests/test_noise_closed_loop.py: the transmission of tests/channel_loop.py
(five mode I frames, an EEP 3-A and a UEP sub-channel) through its static two-path channel, heard by two branches with noise seeds of
their own, branch B's noise 9 dB above branch A's.  Each slice holds the whole NULL in front of its frame (CL.slices_of does not): the
PRS is expected P samples into it, the NULL at P - 2656.  Every branch runs the receiver's own per-frame sequence (coarse frequency,
fine time, demodulation, fine-frequency update), as in tests/diversity_loop.py; the weight of a frame comes from the float32 host
model of the estimator (tests/noise_model.py) on that frame's NULL window at the offset the synchroniser found and the frequency of
the record after the frame's fine-frequency update, which is what the device call behind a branch's demodulation reads.
Counted: FIB CRCs of the five frames (60) and wrong bytes of the EEP 3-A sub-channel's five delivered logical frames."""
import numpy as np

import channel_loop as CL
import channel_model as CM
import diversity_model as DM
import noise_model as NM
import softbit_loop as SL
import softbit_model as SM

LEVEL = SL.LEVEL
P = 2656 + 700
STRIDE = P + 1544 + 196608
EXTRA_DB = 9.0                             # branch B's noise above branch A's
NOISE_SEED = {"A": 0xDAB, "B": 0xDAB + 17}
DELIVERED = (12 * CL.N_FRAMES, 0)
POINT_DB = 7.0                             # SNR of branch A; chosen on the CPU by the sweep DESIGN 4.26 records, tested with 1 dB either side


def params(iq, snr_db, branch):
    p = CL.params(iq, snr_db - (EXTRA_DB if branch == "B" else 0.0))
    p["seed"] = NOISE_SEED[branch]
    return p


def slices_of(rx):
    """frame j from P samples before where its PRS would start without the timing offset; frame 0's slice begins in front of the stream"""
    s = np.zeros((CL.N_FRAMES, STRIDE), np.complex64)
    for j in range(CL.N_FRAMES):
        a = 2656 + j * 196608 - P
        lo = max(a, 0)
        seg = rx[lo:a + STRIDE]
        s[j, lo - a:lo - a + seg.size] = seg
    return s


def receive_branch(oracle, noise_model, rx):
    """-> dict(dq [5][75][1536], k [5], valid [5], w [5] estimated weights, noise [5], snr [5])"""
    slices = slices_of(rx)
    state = oracle.SyncState(0.0, 0.0, 0, 0, 0, 0)
    conj_ref, time_ref = oracle.sync_refs()
    bins = SL.carrier_bins()
    n = CL.N_FRAMES
    out = dict(dq=np.zeros((n, 75, 1536), np.complex64), k=np.zeros(n, np.float32), valid=np.zeros(n, np.int32), w=np.zeros(n, np.float32),
               noise=np.zeros(n, np.float32), snr=np.zeros(n, np.float32))
    for j in range(n):
        prs = slices[j, P:P + 2048]
        oracle.coarse_freq_sync(prs, state, prs_time_ref=time_ref)
        f = np.float32(np.float32(state.freq_coarse) + np.float32(state.freq_fine))
        ok, off, _ = oracle.fine_time_sync(prs, f, prs_fft_conj=conj_ref)
        if not ok:
            state.freq_coarse, state.freq_fine, state.is_found_coarse = 0.0, 0.0, 0
            continue
        frame = slices[j, P + off:P + off + 196608]
        r = oracle.demod_frame(frame, f, want_fft=True)
        state.freq_fine = float(oracle.update_fine_freq(state.freq_fine, r["total_phase"]))
        X = r["fft"].reshape(77, 2048)[:76, bins]
        out["dq"][j] = SM.dqpsk(X[:-1], X[1:])
        out["k"][j] = SM.soft_scale(frame[SM.NB_CP:SM.NB_CP + SM.NB_FFT], LEVEL)
        out["valid"][j] = 1
        # the estimator sits behind the demodulation: it rotates by the record as that call left it, fine-frequency update included
        f_after = np.float32(np.float32(state.freq_coarse) + np.float32(state.freq_fine))
        rec, _ = noise_model.estimate(slices[j], P - 2656 + off, f_after)
        out["w"][j], out["noise"][j], out["snr"][j] = rec["weight"], rec["noise_power"], rec["snr"]
    return out


class Loop:
    """the transmission once; a branch is received once per (SNR, name) and kept"""

    def __init__(self, oracle, tmp_dir):
        self.oracle = oracle
        self.host = CM.build_host_model(tmp_dir)
        self.noise_model = NM.HostModel(NM.build_host_model(tmp_dir), oracle)
        self.fib, self.pay, self.nb = CL.inputs(oracle)
        self.iq = CL.oracle_iq(oracle, self.fib, self.pay)
        self.mapper = oracle.mapper()
        self._branches = {}

    def sigma(self, snr_db, name):
        return params(self.iq, snr_db, name)["noise_sigma"]

    def branch(self, snr_db, name):
        key = (float(snr_db), name)
        if key not in self._branches:
            rx = CM.host_apply(self.host, [params(self.iq, snr_db, name)], self.iq, 0, CL.N_OUT, False)[0]
            self._branches[key] = receive_branch(self.oracle, self.noise_model, rx)
        return self._branches[key]

    def count(self, bits):
        return SL.count(self.oracle, bits, self.fib, self.pay, self.nb)

    def single(self, snr_db, name):
        b = self.branch(snr_db, name)
        return self.count([SM.frame_bits(b["dq"][j], self.mapper, b["k"][j]) if b["valid"][j] else np.zeros(DM.NB_FRAME_BITS, np.int8)
                           for j in range(CL.N_FRAMES)])

    def pair(self, snr_db, weights):
        """weights: "unit", "estimated" or "true" (1 / (2 noise_sigma^2) of each branch's channel)"""
        br = [self.branch(snr_db, n) for n in ("A", "B")]
        bits = []
        for j in range(CL.N_FRAMES):
            if weights == "unit":
                w = None
            elif weights == "estimated":
                w = [b["w"][j] for b in br]
            else:
                w = [np.float32(1.0 / (2.0 * self.sigma(snr_db, n) ** 2)) for n in ("A", "B")]
            bits.append(DM.combine_frame([b["dq"][j] for b in br], [b["k"][j] for b in br], self.mapper, w, [b["valid"][j] for b in br])[0])
        return self.count(bits)
