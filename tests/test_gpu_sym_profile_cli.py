"""-m gpu: the symbol weights through the tools.  A channel-coded capture made by dabgpu_simulate_transmitter through the two-path channel
of tests/channel_loop.py at SNR 12 dB with the white burst of tests/sym_profile_loop.py (--interferer white:6 behind --interferer-gate
60000:7656:20000: three OFDM symbols of I / S = +6 dB every 60000 samples) through dabgpu_radio_cli: with --soft-bits csi --symbol-weights
every sub-channel byte that was sent arrives, with --soft-bits csi alone at least 25 bytes are wrong -- the contrast of the loop (measured: 0
against 986 of 2496).  On top of --soft-bits banded-dd the flag takes 995 wrong bytes to 2 (measured; the loop's own operating point has 0),
so there the path is only held below the 25.  On a capture without a burst the flag costs nothing.  The flag's option rules."""
import os
import subprocess

import numpy as np
import pytest

import channel_loop as CL
import sym_profile_loop as L
import tx_encode_cases as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_simulate_transmitter")
RADIO = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_radio_cli")
SUB_ARGS = ["--subchannel", "0:48:eep3-A", "--subchannel", "200:52:uep20"]      # tests/channel_loop.py's SUBS
N_FRAMES = 8
SNR_DB, IS_DB = 12.0, 6.0


def sim(*args):
    res = subprocess.run([SIM] + [str(a) for a in args], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]


def radio(capture, out_dir, *extra):
    res = subprocess.run([RADIO, "-i", str(capture), "--radio-fib-output", str(out_dir / "fib.bin"), "--radio-msc-output", str(out_dir / "sub_"),
                          "--radio-subchannel", "0,48,3,A", "--ofdm-block-size", "65536"] + [str(a) for a in extra], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    return (out_dir / "fib.bin").read_bytes(), (out_dir / "sub_0.bin").read_bytes(), res.stderr.decode()


def wrong_bytes(got, cifs, n0):
    """the sub-channel bytes delivered against what was sent: the tool may spend a frame or two acquiring, and the last frame may not be
    delivered -- the fewest wrong bytes over the runs of frames a .. b - 1 that give this many bytes (the 15 CIFs the time
    de-interleaver holds back taken off)"""
    got = np.frombuffer(got, np.uint8)
    best = None
    for a in range(3):
        for b in (N_FRAMES - 1, N_FRAMES):
            want = cifs[4 * a:4 * b - 15].reshape(-1)
            if want.size == got.size and want.size > 0:
                w = int((want != got).sum())
                best = w if best is None else min(best, w)
    assert best is not None, (got.size, n0)
    return best


def test_capture_with_a_white_burst_through_the_radio(oracle, tmp_path):
    fib, pay, nb = CL.inputs(oracle)
    n0 = oracle.subchannel_plan(T.o_sub(oracle, CL.SUBS[0]))[2]
    fib.tofile(tmp_path / "fib_in.bin"); pay.tofile(tmp_path / "pay_in.bin")
    # the files are read cyclically: frame j carries the payload of frame j mod 5
    cifs = np.concatenate([pay[0].reshape(4 * CL.N_FRAMES, nb)[:, :n0]] * 2)[:4 * N_FRAMES]
    common = [*SUB_ARGS, "--fib-file", tmp_path / "fib_in.bin", "--payload-file", tmp_path / "pay_in.bin", "--frames", N_FRAMES, "--snr-db", SNR_DB,
              "--noise-seed", 9, "--tap", "0:1:0", "--tap", f"200:{CL.TAP2}:0"]
    burst = ["--interferer", f"white:{IS_DB:.0f}", "--interferer-gate", f"{L.GATE_PERIOD}:{L.GATE_ON}:{L.GATE_OFFSET}", "--interferer-seed", L.BURST_SEED]
    for name, extra in (("clean", []), ("burst", burst)):
        sim(*common, *extra, "-o", tmp_path / f"{name}.u8")
        (tmp_path / name).mkdir()
    # without a burst: the flag costs nothing
    for policy in ("csi", "banded-dd"):
        _, msc, log = radio(tmp_path / "clean.u8", tmp_path / "clean", "--soft-bits", policy, "--symbol-weights")
        assert wrong_bytes(msc, cifs, n0) == 0 and "frames_kept=0" in log, (policy, log[-500:])
    # under the burst: the contrast of the loop, on top of the plain weighted bits and on top of the decision-directed band weights
    for policy in ("csi", "banded-dd"):
        fib_w, msc_w, log_w = radio(tmp_path / "burst.u8", tmp_path / "burst", "--soft-bits", policy, "--symbol-weights")
        fib_p, msc_p, log_p = radio(tmp_path / "burst.u8", tmp_path / "burst", "--soft-bits", policy)
        with_flag, without = wrong_bytes(msc_w, cifs, n0), wrong_bytes(msc_p, cifs, n0)
        print(f"{policy}: wrong bytes with --symbol-weights {with_flag} of {len(msc_w)}, without {without} of {len(msc_p)}; FIBs {len(fib_w) // 30} and "
              f"{len(fib_p) // 30}; {log_w.strip().splitlines()[-1]}")
        assert "symbols: frames_weighted=" in log_w and "frames_kept=0" in log_w and "symbols:" not in log_p
        assert without >= L.CONTRAST and len(fib_w) >= len(fib_p)
        # csi is the pass mark: every byte.  On top of banded-dd (the tool's alpha 0.25, 8-bit samples, seven delivered frames: not the loop's
        # operating point, where that path delivers every byte too) 2 of 2496 bytes were wrong when this was measured, against 995 without the
        # flag; asserted there is only that the path stays below the threshold that marks a path without the weights
        assert with_flag == 0 if policy == "csi" else with_flag < L.CONTRAST


def test_option_rules(tmp_path):
    np.zeros(8192, np.uint8).tofile(tmp_path / "iq.u8")
    for extra, text in ((["--symbol-weights"], b"--symbol-weights needs --soft-bits csi, banded or banded-dd"),
                        (["--soft-bits", "normalised", "--symbol-weights"], b"the normalised policy divides"),
                        (["--soft-bits", "csi", "--symbol-weights", "--configuration", "dab"], b"--soft-bits needs the OFDM stage")):
        res = subprocess.run([RADIO, "-i", str(tmp_path / "iq.u8")] + extra, capture_output=True, timeout=60)
        assert res.returncode != 0 and text in res.stderr, (extra, res.stderr[-500:])
    for policy in ("csi", "banded", "banded-dd"):
        res = subprocess.run([RADIO, "-i", str(tmp_path / "iq.u8"), "--soft-bits", policy, "--symbol-weights"], capture_output=True, timeout=60)
        assert res.returncode == 0 and b"symbols: frames_weighted=0 frames_kept=0" in res.stderr, (policy, res.stderr[-500:])
