"""The closed loop that shows what the clock tracker buys, for tests/test_clock_closed_loop.py and its device form: the loop of
tests/resample_loop.py -- five mode I frames, both sub-channels, the static two-path channel, carrier offset, noise, then the resampler's
host model applying a sampling-clock error of `ppm` -- received by tests/noise_profile_loop.py's receive_branch.  Behind each frame's
demodulation the tracker (the float32 host model of tests/clock_model.py: one estimator pass per frame, gain 1, the state carried over
the five frames) reads that frame's DQPSK products and de-rotates them by the slope it has just updated; the soft bits are the plain
weighted ones (tests/softbit_model.py, frame_bits) on either side.  Counted: FIB CRCs of the five frames (60) and wrong bytes of the
EEP 3-A sub-channel's five delivered logical frames.

Sign: the resampler's `ppm` is dabgpu_simulate_transmitter --clock-ppm's (step = 1 + ppm 1e-6 input samples per output sample), and a
stream made with +X tracks to +X."""
import numpy as np

import channel_loop as CL
import channel_model as CM
import clock_model as CK
import noise_profile_loop as PL
import resample_model as RM
import resample_loop as RL
import softbit_loop as SL
import softbit_model as SM

EXTRA = 1024                                           # samples the resampler may read beyond the channel loop's output (400 ppm: 400)
CONTRAST = 25                                          # wrong bytes the plain path shows at least, at every contrast point
# (SNR dB, ppm): the tracked path delivers all 60 FIB CRCs and every byte, the plain path loses CONTRAST bytes and more
POINTS = ((12.0, 150.0), (12.0, 200.0), (12.0, -200.0), (15.0, 200.0), (9.0, 150.0))
CLEAN = ((15.0, 0.0), (9.0, 0.0))                      # no clock error: both paths deliver, the tracking costs nothing
LIMITS = ((9.0, 200.0), (12.0, 400.0))                 # documented limits: the tracked path does no worse than plain on either count
DELIVERED = (60, 0)
ACCURACY_POINT = (12.0, 200.0)
ACCURACY_SEEDS = tuple(0xDAB + i for i in range(8))    # the channel's noise seeds
ACCURACY_FRAMES = (2, 3, 4)
# worst |tracked - truth| over ACCURACY_SEEDS in frames 2 to 4 at ACCURACY_POINT, measured with this float32 loop; the
# tests hold twice that, since eight seeds do not show the tail
ACCURACY_MEASURED_PPM = 4.36                           # seeds 0xDAB .. 0xDB2: 1.40 3.20 4.31 4.36 2.80 3.28 2.90 2.21
ACCURACY_BOUND_PPM = 2.0 * ACCURACY_MEASURED_PPM
PATHS = ("plain", "tracked")


class Loop:
    """the transmission once; a stream is received once per (SNR, ppm, seed) and kept"""

    def __init__(self, oracle, tmp_dir):
        self.oracle = oracle
        self.host = CM.build_host_model(tmp_dir)
        self.rs_host = RM.build_host_model(tmp_dir)
        self.clock_lib = CK.build_host_model(tmp_dir)
        self.fib, self.pay, self.nb = CL.inputs(oracle)
        self.iq = CL.oracle_iq(oracle, self.fib, self.pay)
        self.mapper = oracle.mapper()
        self._branches = {}

    def stream(self, snr_db, ppm, seed=None):
        p = CL.params(self.iq, snr_db)
        if seed is not None:
            p["seed"] = seed
        rx = CM.host_apply(self.host, [p], self.iq, 0, CL.N_OUT + EXTRA, False)[0]
        P = RL.clock_params(ppm)
        D = RM.host_design(self.rs_host, RM.design_max_step(P["step_q62"]))
        return RM.host_apply(self.rs_host, [P], D, rx, 0, CL.N_OUT, False)[0]

    def branch(self, snr_db, ppm, seed=None):
        """receive_branch's dict, plus the tracker's: v [5][75][1536] de-rotated products, ppm [5] tracked after each frame,
        slope [5], residual [5], clock_ok [5]"""
        key = (float(snr_db), float(ppm), seed)
        if key not in self._branches:
            b = PL.receive_branch(self.oracle, None, self.stream(snr_db, ppm, seed), alphas=())
            model = CK.HostModel(self.clock_lib)
            b["v"] = np.zeros_like(b["dq"])
            b["slope"], b["residual"] = np.zeros(CL.N_FRAMES, np.int64), np.zeros(CL.N_FRAMES, np.int64)
            b["ppm"], b["clock_ok"] = np.zeros(CL.N_FRAMES), np.zeros(CL.N_FRAMES, np.int32)
            for j in range(CL.N_FRAMES):
                if b["valid"][j]:                      # a refused frame leaves stale products behind: the state waits
                    b["v"][j], e = model.track(b["dq"][j])
                    b["residual"][j], b["clock_ok"][j] = e["residual"], e["valid"]
                b["slope"][j], b["ppm"][j] = model.slope, CK.ppm_of(model.slope)
            self._branches[key] = b
        return self._branches[key]

    def count(self, bits):
        return SL.count(self.oracle, bits, self.fib, self.pay, self.nb)

    def bits(self, snr_db, ppm, path, seed=None):
        b = self.branch(snr_db, ppm, seed)
        dq = b["dq"] if path == "plain" else b["v"]
        return [SM.frame_bits(dq[j], self.mapper, b["k"][j]) if b["valid"][j] else np.zeros(SM.NB_DATA_SYMBOLS * SM.NB_SYM_BITS, np.int8)
                for j in range(CL.N_FRAMES)]

    def counts(self, snr_db, ppm, paths=PATHS, seed=None):
        return {p: self.count(self.bits(snr_db, ppm, p, seed)) for p in paths}
