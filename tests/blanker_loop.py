"""The closed loop of the impulse blanker, for tests/test_blanker_closed_loop.py and its device form: tests/interferer_loop.py's
transmission, channel and interferer (bursts: white noise on for 205 of every 20480 samples; band: DESIGN 4.27's steady 96 kHz source), then
the blanker's float32 host model (tests/blanker_model.py, blanker_core.h under g++) at the default parameters over the whole received
stream, then interferer_loop's unchanged receiver with the demodulator's plain weighted soft bits.  Counted as there: FIB CRCs of the five
frames (60) and wrong bytes of the EEP 3-A sub-channel; beside them the blocks the blanker zeroed, of all."""
import numpy as np

import blanker_model as BM
import channel_loop as CL
import diversity_model as DM
import interferer_loop as IL
import noise_profile_loop as PL
import softbit_model as SM

SNR_DB = IL.SNR_DB
DELIVERED = IL.DELIVERED
PARAMS = BM.params()


class Loop(IL.Loop):
    """interferer_loop's loop with the blanker between the interferer and the receiver; a blanked stream is received once and kept"""

    def __init__(self, oracle, tmp_dir):
        super().__init__(oracle, tmp_dir)
        self.bhost = BM.build_host_model(tmp_dir)
        self._blanked, self._blanked_branches = {}, {}

    def blanked_stream(self, snr_db, is_db, kind="burst", params=PARAMS):
        """(the blanked stream, its mask words, blocks blanked, blocks in all)"""
        key = (float(snr_db), None if is_db is None else float(is_db), kind, tuple(sorted(params.items())))
        if key not in self._blanked:
            rx = self.stream(snr_db, is_db, kind)
            y, m = BM.host_apply(self.bhost, [params], rx, 0, rx.size)
            self._blanked[key] = (y[0], m[0], BM.popcount(m[0]), (rx.size + BM.LEN - 1) // BM.LEN)
        return self._blanked[key]

    def blanked_branch(self, snr_db, is_db, kind="burst", params=PARAMS):
        key = (float(snr_db), None if is_db is None else float(is_db), kind, tuple(sorted(params.items())))
        if key not in self._blanked_branches:
            self._blanked_branches[key] = PL.receive_branch(self.oracle, self.profile_model, self.blanked_stream(snr_db, is_db, kind, params)[0])
        return self._blanked_branches[key]

    def blanked(self, snr_db, is_db, kind="burst", params=PARAMS):
        """(FIBs delivered, wrong bytes) of the blanked stream through the plain weighted soft bits"""
        b = self.blanked_branch(snr_db, is_db, kind, params)
        return self.count([SM.frame_bits(b["dq"][j], self.mapper, b["k"][j]) if b["valid"][j] else np.zeros(DM.NB_FRAME_BITS, np.int8)
                           for j in range(CL.N_FRAMES)])
