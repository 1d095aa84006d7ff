"""The closed loop that shows what the decision-directed profile buys, for tests/test_dd_profile_closed_loop.py and its device form: the
loop of tests/noise_profile_loop.py (five mode I frames through the static two-path channel, a band interferer 96 carriers wide at 300.3
spacings) with the interferer GATED off around every NULL symbol: the integer gate of the library's interferer bank (include/dabgpu.h,
"Interferer": on iff ((m - gate_offset) mod gate_period) < gate_on) with the frame's period, off from 1000 samples in front of each NULL
of the transmission to 1000 samples behind it.  The NULL symbol then shows the noise floor alone, the NULL-based profile comes out flat,
and the banded combiner fails as the plain weighted soft bits do; the decision-directed profile reads the same frame's DQPSK products
(the float32 host model of tests/dd_profile_model.py), its state carried from frame to frame, and the combiner takes its weights
unchanged.  Counted: FIB CRCs of the five frames (60) and wrong bytes of the EEP 3-A sub-channel's five delivered logical frames."""
import numpy as np

import channel_loop as CL
import channel_model as CM
import dd_profile_model as DD
import diversity_model as DM
import noise_loop as NL
import noise_profile_loop as PL
import noise_profile_model as PM
import softbit_loop as SL
import softbit_model as SM

P, STRIDE, LEVEL = PL.P, PL.STRIDE, PL.LEVEL
GATE_PERIOD = 196608
GATE_MARGIN = 1000
GATE_OFFSET = 2656 + GATE_MARGIN                       # the gate opens this far into every frame of the transmission ...
GATE_ON = GATE_PERIOD - 2656 - 2 * GATE_MARGIN         # ... and closes 1000 samples in front of the next NULL
ALPHAS = PL.ALPHAS
DELIVERED = PL.DELIVERED
FAIL_CAP = 15                                          # FIB CRCs of 60 the paths without the new weights may deliver at a gated point
# (SNR dB, I / S dB): the operating point with 3 dB either side, and 3 dB less SNR at the point (the sweep: DESIGN 4.30)
POINTS = ((12.0, -3.0), (12.0, 0.0), (12.0, 3.0), (9.0, 0.0))
UNGATED = (12.0, 0.0)
CLEAN_SNR_DB = 7.0


def gate(n):
    """bool [n]: sample m of the received stream hears the interferer"""
    return ((np.arange(n, dtype=np.int64) - GATE_OFFSET) % GATE_PERIOD) < GATE_ON


def dd_weights(dd_model, branch, alphas=ALPHAS):
    """{alpha: [5][128]} band weights from the branch's products, the state carried across its valid frames"""
    w = {a: np.zeros((CL.N_FRAMES, 128), np.float32) for a in alphas}
    for a in alphas:
        prof = np.zeros(128, np.float32)
        for j in range(CL.N_FRAMES):
            if not branch["valid"][j]:
                continue
            p = dd_model.profile(branch["dq"][j], None, prof, a)
            prof, w[a][j] = p["profile"], p["band_weight"]
    return w


class Loop:
    """the transmission once; a stream is received once per (SNR, I / S, gated) and kept.  I / S = None: no interferer"""

    def __init__(self, oracle, tmp_dir):
        self.oracle = oracle
        self.host = CM.build_host_model(tmp_dir)
        self.profile_model = PM.HostModel(PM.build_host_model(tmp_dir), oracle)
        self.dd_model = DD.HostModel(DD.build_host_model(tmp_dir))
        self.fib, self.pay, self.nb = CL.inputs(oracle)
        self.iq = CL.oracle_iq(oracle, self.fib, self.pay)
        self.mapper = oracle.mapper()
        self.S = PL.signal_power(self.iq)
        self._clean, self._branches = {}, {}

    def jam(self, n, is_db, gated):
        x = PL.interferer(n, PL.OFFSET["A"], PL.WIDTH, self.S * 10.0 ** (is_db / 10.0), PL.JAM_SEED["A"])
        return x * gate(n) if gated else x

    def stream(self, snr_db, is_db, gated=True):
        if snr_db not in self._clean:
            p = CL.params(self.iq, snr_db)
            p["seed"] = NL.NOISE_SEED["A"]
            self._clean[snr_db] = CM.host_apply(self.host, [p], self.iq, 0, CL.N_OUT, False)[0]
        rx = self._clean[snr_db]
        return rx if is_db is None else (rx + self.jam(rx.size, is_db, gated)).astype(np.complex64)

    def branch(self, snr_db, is_db, gated=True):
        key = (float(snr_db), None if is_db is None else float(is_db), bool(gated))
        if key not in self._branches:
            b = PL.receive_branch(self.oracle, self.profile_model, self.stream(snr_db, is_db, gated))
            b["dd"] = dd_weights(self.dd_model, b)
            self._branches[key] = b
        return self._branches[key]

    def count(self, bits):
        return SL.count(self.oracle, bits, self.fib, self.pay, self.nb)

    def bits(self, snr_db, is_db, gated=True, path="dd", alpha=1.0):
        """the five frames' soft bits: path "plain" (the demodulator's weighted bits), "null" (banded, NULL-based weights), "dd" (banded,
        decision-directed weights)"""
        b = self.branch(snr_db, is_db, gated)
        out = []
        for j in range(CL.N_FRAMES):
            if not b["valid"][j]:
                out.append(np.zeros(DM.NB_FRAME_BITS, np.int8))
            elif path == "plain":
                out.append(SM.frame_bits(b["dq"][j], self.mapper, b["k"][j]))
            else:
                w = b["dd"][alpha][j] if path == "dd" else b["w"][alpha][j]
                out.append(PM.combine_frame([b["dq"][j]], [b["k"][j]], self.mapper, None, [1], [w])[0])
        return out

    def counts(self, snr_db, is_db, gated=True, alpha=1.0):
        return {p: self.count(self.bits(snr_db, is_db, gated, p, alpha)) for p in ("plain", "null", "dd")}
