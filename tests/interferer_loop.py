"""The closed loop that drives the banded path from the library's own interferer, for tests/test_interferer_closed_loop.py and its device
form: the transmission of tests/channel_loop.py (five mode I frames, an EEP 3-A and a UEP sub-channel) through its static two-path channel
with white noise at an SNR, then the interferer's host model (tests/interferer_model.py, interferer_core.h under g++) on the received
stream, then the receiver of tests/noise_profile_loop.py: synchroniser and demodulator oracle per frame, the noise profile's float32 host
model on that frame's NULL, and either the demodulator's weighted soft bits (plain) or the banded combiner over the one branch (banded).
The band source has DESIGN 4.27's geometry: 96 kHz wide (96 carrier spacings), 300 kHz (300 spacings) above the centre; its power, while
on, is I relative to the signal power S that tests/channel_loop.py's SNR refers to.  The burst source is white noise gated on for
BURST_ON of every BURST_PERIOD samples.  Counted: FIB CRCs of the five frames (60) and wrong bytes of the EEP 3-A sub-channel's five
delivered logical frames."""
import numpy as np

import channel_loop as CL
import channel_model as CM
import diversity_model as DM
import interferer_model as IM
import noise_loop as NL
import noise_profile_loop as PL
import noise_profile_model as PM
import softbit_loop as SL
import softbit_model as SM

SNR_DB = 12.0                              # the operating point, with 3 dB either side, from the sweep of DESIGN 4.28
POINT_DB = 0.0                             # I / S of the band source
WIDTH_HZ, OFFSET_HZ = 96000.0, 300000.0
ALPHAS = PL.ALPHAS
DELIVERED = PL.DELIVERED
JAM_SEED = 0xDAB + 201
BURST_PERIOD, BURST_ON, BURST_OFFSET = 20480, 205, -1000        # 10 ms apart, 100 us long (1 % of the time), ignition-like
BURST_DB = 17.0                            # I / S of a burst while it is on


def q64(hz):
    return int(round(hz / 2.048e6 * 2 ** 64)) & IM.M64


def band_stream(S, is_db):
    return IM.stream([IM.source(IM.BAND, amp=np.sqrt(S * 10.0 ** (is_db / 10.0)), shape=0, freq_q64=q64(OFFSET_HZ))], seed=JAM_SEED)


def burst_stream(S, is_db):
    return IM.stream([IM.source(IM.BAND, amp=np.sqrt(S * 10.0 ** (is_db / 10.0)), shape=-1, gate_period=BURST_PERIOD, gate_on=BURST_ON,
                                gate_offset=BURST_OFFSET)], seed=JAM_SEED)


class Loop:
    """the transmission once; a stream is received once per (SNR, I / S, kind) and kept.  I / S = None: no interferer"""

    def __init__(self, oracle, tmp_dir):
        import dabgpu
        self.oracle = oracle
        self.host = CM.build_host_model(tmp_dir)
        self.ihost = IM.build_host_model(tmp_dir)
        self.profile_model = PM.HostModel(PM.build_host_model(tmp_dir), oracle)
        self.fib, self.pay, self.nb = CL.inputs(oracle)
        self.iq = CL.oracle_iq(oracle, self.fib, self.pay)
        self.mapper = oracle.mapper()
        self.S = PL.signal_power(self.iq)
        self.shape = IM.Shape.from_buffer_copy(bytes(dabgpu.interferer_design(WIDTH_HZ / 2.048e6)))
        self._clean, self._branches = {}, {}

    def channel_params(self, snr_db):
        p = CL.params(self.iq, snr_db)
        p["seed"] = NL.NOISE_SEED["A"]
        return p

    def interferer_params(self, is_db, kind):
        return band_stream(self.S, is_db) if kind == "band" else burst_stream(self.S, is_db)

    def stream(self, snr_db, is_db, kind="band"):
        if snr_db not in self._clean:
            self._clean[snr_db] = CM.host_apply(self.host, [self.channel_params(snr_db)], self.iq, 0, CL.N_OUT, False)[0]
        rx = self._clean[snr_db]
        if is_db is None:
            return rx
        return IM.host_apply(self.ihost, [self.interferer_params(is_db, kind)], [self.shape], rx, 0, rx.size)[0]

    def branch(self, snr_db, is_db, kind="band"):
        key = (float(snr_db), None if is_db is None else float(is_db), kind)
        if key not in self._branches:
            self._branches[key] = PL.receive_branch(self.oracle, self.profile_model, self.stream(snr_db, is_db, kind))
        return self._branches[key]

    def count(self, bits):
        return SL.count(self.oracle, bits, self.fib, self.pay, self.nb)

    def plain(self, snr_db, is_db, kind="band"):
        b = self.branch(snr_db, is_db, kind)
        return self.count([SM.frame_bits(b["dq"][j], self.mapper, b["k"][j]) if b["valid"][j] else np.zeros(DM.NB_FRAME_BITS, np.int8)
                           for j in range(CL.N_FRAMES)])

    def banded(self, snr_db, is_db, alpha=1.0, kind="band"):
        b = self.branch(snr_db, is_db, kind)
        return self.count([PM.combine_frame([b["dq"][j]], [b["k"][j]], self.mapper, None, [b["valid"][j]], [b["w"][alpha][j]])[0]
                           for j in range(CL.N_FRAMES)])
