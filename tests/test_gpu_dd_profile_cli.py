"""-m gpu: the decision-directed profile through the tools.  A channel-coded capture made by dabgpu_simulate_transmitter with the gated
band interferer of tests/dd_profile_loop.py (96 kHz of Gaussian noise 300.3 kHz above the centre, I / S = 0 dB while on, silent from 1000
samples in front of every NULL symbol to 1000 behind it, SNR 12 dB) through dabgpu_radio_cli: with --soft-bits banded-dd every FIB of the
delivered frames and every sub-channel byte that was sent arrives; with --soft-bits banded, whose profile hears the interferer's silence,
and with --soft-bits csi fewer FIBs arrive.  On a capture without an interferer both banded paths deliver what was sent."""
import os
import subprocess

import numpy as np
import pytest

import channel_loop as CL
import dd_profile_loop as DL
import noise_profile_loop as PL
import tx_encode_cases as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_simulate_transmitter")
RADIO = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_radio_cli")
SUB_ARGS = ["--subchannel", "0:48:eep3-A", "--subchannel", "200:52:uep20"]      # tests/channel_loop.py's SUBS
N_FRAMES = 8
SNR_DB, IS_DB = DL.UNGATED


def sim(*args):
    res = subprocess.run([SIM] + [str(a) for a in args], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]


def radio(capture, out_dir, *extra):
    res = subprocess.run([RADIO, "-i", str(capture), "--radio-fib-output", str(out_dir / "fib.bin"), "--radio-msc-output", str(out_dir / "sub_"),
                          "--radio-subchannel", "0,48,3,A", "--ofdm-block-size", "65536"] + [str(a) for a in extra], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    return (out_dir / "fib.bin").read_bytes(), (out_dir / "sub_0.bin").read_bytes(), res.stderr.decode()


def sent_between(fib, cifs, a, b):
    """what a receiver that delivers the frames a .. b - 1 hands out: their FIBs and the sub-channel's CIFs 4 a .. 4 b less the 15 the time
    de-interleaver holds back"""
    return fib[a:b].tobytes(), cifs[4 * a:4 * b - 15].tobytes()


def test_capture_with_a_gated_interferer_through_the_radio(oracle, tmp_path):
    fib, pay, nb = CL.inputs(oracle)
    n0 = oracle.subchannel_plan(T.o_sub(oracle, CL.SUBS[0]))[2]
    fib.tofile(tmp_path / "fib_in.bin"); pay.tofile(tmp_path / "pay_in.bin")
    # the files are read cyclically: frame j carries the FIBs and the payload of frame j mod 5
    fibs = np.concatenate([fib[0].reshape(CL.N_FRAMES, -1)] * 2)[:N_FRAMES]
    cifs = np.concatenate([pay[0].reshape(4 * CL.N_FRAMES, nb)[:, :n0]] * 2)[:4 * N_FRAMES]
    common = [*SUB_ARGS, "--fib-file", tmp_path / "fib_in.bin", "--payload-file", tmp_path / "pay_in.bin", "--frames", N_FRAMES, "--snr-db", SNR_DB,
              "--noise-seed", 9]
    jam = ["--interferer", f"band:{PL.OFFSET['A'] * 1000.0:.0f}:{PL.WIDTH * 1000}:{IS_DB:.0f}",
           "--interferer-gate", f"{DL.GATE_PERIOD}:{DL.GATE_ON}:{DL.GATE_OFFSET}", "--interferer-seed", 77]
    for name, extra in (("clean", []), ("gated", jam)):
        sim(*common, *extra, "-o", tmp_path / f"{name}.u8")
        (tmp_path / name).mkdir()
    # the tool may spend a frame or two acquiring, and the last frame is not delivered: no NULL follows it in the file
    expected = [sent_between(fibs, cifs, a, b) for a in range(3) for b in (N_FRAMES - 1, N_FRAMES)]
    # without an interferer: both profiles deliver what was sent
    for policy in ("banded", "banded-dd"):
        got_fib, got_msc, log = radio(tmp_path / "clean.u8", tmp_path / "clean", "--soft-bits", policy)
        assert (got_fib, got_msc) in expected and "frames_kept_csi=0" in log, (policy, log[-500:])
    # gated: the decision-directed weights deliver everything that was sent, the NULL-based ones and the plain weighted bits do not
    dd_fib, dd_msc, log = radio(tmp_path / "gated.u8", tmp_path / "gated", "--soft-bits", "banded-dd", "--alpha", 0.25)
    print(f"banded-dd: {len(dd_fib) // 30} FIBs, {len(dd_msc) // n0} CIFs; {log.strip().splitlines()[-3:]}")
    assert (dd_fib, dd_msc) in expected and "frames_kept_csi=0" in log
    for policy in ("banded", "csi"):
        raw_fib, raw_msc, log = radio(tmp_path / "gated.u8", tmp_path / "gated", "--soft-bits", policy)
        print(f"{policy}: {len(raw_fib) // 30} FIBs; {log.strip().splitlines()[-2:]}")
        assert len(raw_fib) < len(dd_fib) and raw_msc != dd_msc, policy


def test_option_rules(tmp_path):
    np.zeros(8192, np.uint8).tofile(tmp_path / "iq.u8")
    for extra, text in ((["--soft-bits", "banded-d"], b"normalised, csi, banded or banded-dd"), (["--soft-bits", "banded-dd", "--alpha", "0"], b"--alpha"),
                        (["--soft-bits", "banded-dd", "--ofdm-block-size", "193953"], b"193952"), (["--soft-bits", "csi", "--alpha", "0.5"], b"--alpha needs"),
                        (["--soft-bits", "banded-dd", "--configuration", "dab"], b"--soft-bits needs the OFDM stage")):
        res = subprocess.run([RADIO, "-i", str(tmp_path / "iq.u8")] + extra, capture_output=True, timeout=60)
        assert res.returncode != 0 and text in res.stderr, (extra, res.stderr[-500:])
