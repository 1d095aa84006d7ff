"""The closed loop that shows what the band weights buy, for tests/test_noise_profile_closed_loop.py and its device form: the
transmission of tests/channel_loop.py (five mode I frames, an EEP 3-A and a UEP sub-channel) through its static two-path channel at
SNR_DB, with a narrowband interferer added to the received stream: band-limited Gaussian noise WIDTH carriers wide (white noise with
every bin of its transform outside the band cleared), centred OFFSET carrier spacings from the centre, of total power I relative to the
signal power S that tests/channel_loop.py's SNR refers to.  The receiver is the per-frame sequence of tests/noise_loop.py; behind each
frame's demodulation the noise profile (the float32 host model of tests/noise_profile_model.py) reads that frame's NULL at the offset
the synchroniser found and the frequency of the record after the fine-frequency update, with the previous frame's profile as its
state.  Plain: the demodulator's weighted soft bits.  Banded: the banded combiner over the one branch with that frame's band weights.
Counted: FIB CRCs of the five frames (60) and wrong bytes of the EEP 3-A sub-channel's five delivered logical frames."""
import numpy as np

import channel_loop as CL
import channel_model as CM
import diversity_model as DM
import noise_loop as NL
import noise_profile_model as PM
import softbit_loop as SL
import softbit_model as SM

LEVEL = SL.LEVEL
P, STRIDE = NL.P, NL.STRIDE
SNR_DB = 9.0
WIDTH = 96
OFFSET = {"A": 300.3, "B": -420.7}         # carrier spacings above the centre: each branch its own interferer
POINT_DB = 0.0                             # I / S of the operating point, tested with 3 dB either side (the sweep: DESIGN 4.27)
ALPHAS = (1.0, 0.25)
DELIVERED = NL.DELIVERED
JAM_SEED = {"A": 0xDAB + 101, "B": 0xDAB + 102}


def signal_power(iq):
    """S: the mean power of the two-path sum, as tests/channel_loop.py's sigma_for takes it"""
    return float(np.mean(np.abs(iq.astype(np.complex128)) ** 2)) * (1.0 + CL.TAP2 ** 2)


def interferer(n, offset, width, power, seed):
    """n samples of Gaussian noise confined to `width` carrier spacings around `offset` spacings, mean power `power`"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    X = np.fft.fft(x)
    f = np.fft.fftfreq(n) * 2048.0                                                     # in carrier spacings
    X[np.abs(f) > width / 2.0] = 0.0
    x = np.fft.ifft(X) * np.exp(2j * np.pi * (offset / 2048.0) * np.arange(n))
    return x * np.sqrt(power / np.mean(np.abs(x) ** 2))


def receive_branch(oracle, profile_model, rx, alphas=ALPHAS, exclude=None):
    """-> dict(dq [5][75][1536], k [5], valid [5], w {alpha: [5][128]}, mean {alpha: [5]}, null [5] NULL position, freq [5]): NL.receive_branch
    with the profile in the estimator's place"""
    slices = NL.slices_of(rx)
    state = oracle.SyncState(0.0, 0.0, 0, 0, 0, 0)
    conj_ref, time_ref = oracle.sync_refs()
    bins = SL.carrier_bins()
    n = CL.N_FRAMES
    out = dict(dq=np.zeros((n, 75, 1536), np.complex64), k=np.zeros(n, np.float32), valid=np.zeros(n, np.int32), null=np.zeros(n, np.int64),
               freq=np.zeros(n, np.float32), w={a: np.zeros((n, 128), np.float32) for a in alphas}, mean={a: np.zeros(n, np.float32) for a in alphas},
               slices=slices)
    prof = {a: np.zeros(128, np.float32) for a in alphas}
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
        # the profile sits behind the demodulation: it rotates by the record as that call left it, fine-frequency update included
        out["freq"][j] = np.float32(np.float32(state.freq_coarse) + np.float32(state.freq_fine))
        out["null"][j] = P - 2656 + off
        for a in alphas:
            p = profile_model.profile(slices[j], int(out["null"][j]), out["freq"][j], exclude, prof[a], a)
            prof[a] = p["profile"]
            out["w"][a][j], out["mean"][a][j] = p["band_weight"], p["mean_noise"]
    return out


class Loop:
    """the transmission once; a branch is received once per (I / S, name) and kept.  I / S = None: no interferer"""

    def __init__(self, oracle, tmp_dir):
        self.oracle = oracle
        self.host = CM.build_host_model(tmp_dir)
        self.profile_model = PM.HostModel(PM.build_host_model(tmp_dir), oracle)
        self.fib, self.pay, self.nb = CL.inputs(oracle)
        self.iq = CL.oracle_iq(oracle, self.fib, self.pay)
        self.mapper = oracle.mapper()
        self.S = signal_power(self.iq)
        self._clean, self._branches = {}, {}

    def stream(self, is_db, name, width=WIDTH):
        """the received stream of a branch: the channel at SNR_DB with the branch's noise seed, plus its interferer"""
        if name not in self._clean:
            p = CL.params(self.iq, SNR_DB)
            p["seed"] = NL.NOISE_SEED[name]
            self._clean[name] = CM.host_apply(self.host, [p], self.iq, 0, CL.N_OUT, False)[0]
        rx = self._clean[name]
        if is_db is None:
            return rx
        jam = interferer(rx.size, OFFSET[name], width, self.S * 10.0 ** (is_db / 10.0), JAM_SEED[name])
        return (rx + jam).astype(np.complex64)

    def branch(self, is_db, name, width=WIDTH):
        key = (None if is_db is None else float(is_db), name, width)
        if key not in self._branches:
            self._branches[key] = receive_branch(self.oracle, self.profile_model, self.stream(is_db, name, width))
        return self._branches[key]

    def count(self, bits):
        return SL.count(self.oracle, bits, self.fib, self.pay, self.nb)

    def plain(self, is_db, name="A", width=WIDTH):
        b = self.branch(is_db, name, width)
        return self.count([SM.frame_bits(b["dq"][j], self.mapper, b["k"][j]) if b["valid"][j] else np.zeros(DM.NB_FRAME_BITS, np.int8)
                           for j in range(CL.N_FRAMES)])

    def banded_bits(self, is_db, names=("A",), alpha=1.0, width=WIDTH):
        br = [self.branch(is_db, n, width) for n in names]
        return [PM.combine_frame([b["dq"][j] for b in br], [b["k"][j] for b in br], self.mapper, None, [b["valid"][j] for b in br],
                                 [b["w"][alpha][j] for b in br])[0] for j in range(CL.N_FRAMES)]

    def banded(self, is_db, names=("A",), alpha=1.0, width=WIDTH):
        return self.count(self.banded_bits(is_db, names, alpha, width))

    def plain_pair(self, is_db, names=("A", "B")):
        """the scalar combiner with unit weights over the branches"""
        br = [self.branch(is_db, n) for n in names]
        return self.count([DM.combine_frame([b["dq"][j] for b in br], [b["k"][j] for b in br], self.mapper, None, [b["valid"][j] for b in br])[0]
                           for j in range(CL.N_FRAMES)])
