"""The closed loop that shows what the symbol weights buy, for tests/test_sym_profile_closed_loop.py and its device form: the loop of
tests/dd_profile_loop.py (five mode I frames through the static two-path channel, EEP 3-A sub-channel, 60 FIBs) with a WHITE BURST in the
band interferer's place: complex Gaussian noise of power I relative to the signal power S (PCG64 seed 777) behind the integer gate of the
library's interferer bank (include/dabgpu.h, "Interferer": on iff ((m - gate_offset) mod gate_period) < gate_on) with period 60000
samples, on for 7656 samples (three OFDM symbols), offset 20000: three or four bursts a frame, none of which the blanker, the NULL profile
or the decision-directed profile can answer.  Behind each frame's demodulation the symbol noise profile (the float32 host model of
tests/sym_profile_model.py) reads that frame's DQPSK products; the symbol-weighted combiner (the compiled rule of
tests/diversity_symbols_model.py) takes its weights on top of the plain weighted soft bits ("csi": one branch, no band table) and on top
of the decision-directed band weights ("banded-dd").  Counted: FIB CRCs of the five frames (60) and wrong bytes of the EEP 3-A
sub-channel's five delivered logical frames."""
import numpy as np

import channel_loop as CL
import channel_model as CM
import dd_profile_loop as DL
import dd_profile_model as DD
import diversity_model as DM
import diversity_symbols_model as DS
import noise_loop as NL
import noise_profile_loop as PL
import noise_profile_model as PM
import softbit_loop as SL
import softbit_model as SM
import sym_profile_model as SP

GATE_PERIOD, GATE_ON, GATE_OFFSET = 60000, 7656, 20000
BURST_SEED = 777
ALPHA = 1.0                                            # the decision-directed profile's: no smoothing, as the bursts have none
DELIVERED = PL.DELIVERED
CONTRAST = 25                                          # wrong bytes the paths without symbol weights show at least, at every point
# (SNR dB, I / S dB): the points at which the symbol weights deliver every byte and the paths without them lose 50 and more
POINTS = ((12.0, 3.0), (12.0, 6.0), (12.0, 9.0), (9.0, 6.0))
LIMIT = (12.0, 12.0)                                   # the documented limit: a frame is refused, the weights do no worse than plain
CLEAN_SNR_DB = DL.CLEAN_SNR_DB
PATHS = ("plain", "dd", "plain+sym", "dd+sym")


def gate(n):
    """bool [n]: sample m of the received stream hears the burst"""
    return ((np.arange(n, dtype=np.int64) - GATE_OFFSET) % GATE_PERIOD) < GATE_ON


def burst(n, power):
    """n samples of white complex Gaussian noise of mean power `power` behind the gate"""
    rng = np.random.Generator(np.random.PCG64(BURST_SEED))
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(power / 2.0)
    return x * gate(n)


def symbol_weights(sym_model, branch):
    """(v [5][75], q [5][75], ok [5]) from the branch's products of its valid frames; the estimator keeps no state"""
    v, q = np.zeros((CL.N_FRAMES, 75), np.float32), np.zeros((CL.N_FRAMES, 75), np.float32)
    ok = np.zeros(CL.N_FRAMES, np.int32)
    for j in range(CL.N_FRAMES):
        if branch["valid"][j]:
            p = sym_model.profile(branch["dq"][j])
            v[j], q[j], ok[j] = p["symbol_weight"], p["symbol_noise"], p["valid"]
    return v, q, ok


class Loop:
    """the transmission once; a stream is received once per (SNR, I / S) and kept.  I / S = None: no burst"""

    def __init__(self, oracle, tmp_dir):
        self.oracle = oracle
        self.host = CM.build_host_model(tmp_dir)
        self.profile_model = PM.HostModel(PM.build_host_model(tmp_dir), oracle)
        self.dd_model = DD.HostModel(DD.build_host_model(tmp_dir))
        self.sym_lib = SP.build_host_model(tmp_dir)
        self.sym_model = SP.HostModel(self.sym_lib)
        self.fib, self.pay, self.nb = CL.inputs(oracle)
        self.iq = CL.oracle_iq(oracle, self.fib, self.pay)
        self.mapper = oracle.mapper()
        self.S = PL.signal_power(self.iq)
        self._clean, self._branches = {}, {}

    def stream(self, snr_db, is_db):
        if snr_db not in self._clean:
            p = CL.params(self.iq, snr_db)
            p["seed"] = NL.NOISE_SEED["A"]
            self._clean[snr_db] = CM.host_apply(self.host, [p], self.iq, 0, CL.N_OUT, False)[0]
        rx = self._clean[snr_db]
        return rx if is_db is None else (rx + burst(rx.size, self.S * 10.0 ** (is_db / 10.0))).astype(np.complex64)

    def branch(self, snr_db, is_db):
        key = (float(snr_db), None if is_db is None else float(is_db))
        if key not in self._branches:
            b = PL.receive_branch(self.oracle, self.profile_model, self.stream(snr_db, is_db), alphas=(ALPHA,))
            b["dd"] = DL.dd_weights(self.dd_model, b, (ALPHA,))
            b["v"], b["q"], b["sym_ok"] = symbol_weights(self.sym_model, b)
            self._branches[key] = b
        return self._branches[key]

    def count(self, bits):
        return SL.count(self.oracle, bits, self.fib, self.pay, self.nb)

    def bits(self, snr_db, is_db, path):
        """the five frames' soft bits: "plain" (the demodulator's weighted bits), "dd" (banded, decision-directed weights), and either with
        "+sym": the symbol-weighted combiner over the one branch"""
        b = self.branch(snr_db, is_db)
        out = []
        for j in range(CL.N_FRAMES):
            if not b["valid"][j]:
                out.append(np.zeros(DM.NB_FRAME_BITS, np.int8))
                continue
            band = [b["dd"][ALPHA][j]] if path.startswith("dd") else None
            if path == "plain":
                out.append(SM.frame_bits(b["dq"][j], self.mapper, b["k"][j]))
            elif path == "dd":
                out.append(PM.combine_frame([b["dq"][j]], [b["k"][j]], self.mapper, None, [1], band)[0])
            else:
                out.append(DS.host_combine_frame(self.sym_lib, [b["dq"][j]], [b["k"][j]], None, [1], band, [b["v"][j]])[0])
        return out

    def counts(self, snr_db, is_db, paths=PATHS):
        return {p: self.count(self.bits(snr_db, is_db, p)) for p in paths}
