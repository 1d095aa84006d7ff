"""-m gpu: the clock tracker through the tools.  A channel-coded capture made by dabgpu_simulate_transmitter through the two-path channel of
tests/channel_loop.py at SNR 12 dB with --clock-ppm 200, through dabgpu_radio_cli: with --soft-bits csi --track-clock --clock-report the FIB
bodies and the sub-channel bytes that were sent arrive, and the reported ppm settles within the bound of tests/clock_loop.py around +200;
the same capture without --track-clock loses FIBs.  With --clock-ppm 0 the tracked run delivers what was sent (it cannot equal an
untracked run byte for byte: the state takes small non-zero values).  The flag's option rules."""
import os
import re
import subprocess

import numpy as np
import pytest

import channel_loop as CL
import clock_loop as L
import tx_encode_cases as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_simulate_transmitter")
RADIO = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_radio_cli")
SUB_ARGS = ["--subchannel", "0:48:eep3-A", "--subchannel", "200:52:uep20"]      # tests/channel_loop.py's SUBS
N_FRAMES = 8
SNR_DB, PPM = 12.0, 200.0


def sim(*args):
    res = subprocess.run([SIM] + [str(a) for a in args], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]


def radio(capture, out_dir, *extra):
    res = subprocess.run([RADIO, "-i", str(capture), "--radio-fib-output", str(out_dir / "fib.bin"), "--radio-msc-output", str(out_dir / "sub_"),
                          "--radio-subchannel", "0,48,3,A", "--ofdm-block-size", "65536"] + [str(a) for a in extra], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    return (out_dir / "fib.bin").read_bytes(), (out_dir / "sub_0.bin").read_bytes(), res.stderr.decode(), res.stdout.decode()


def wrong_bytes(got, cifs):
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
    assert best is not None, got.size
    return best


def reported(stdout):
    return [(int(m.group(1)), float(m.group(2)), int(m.group(3))) for m in re.finditer(r"^clock frame=(\d+) ppm=(-?[\d.]+) valid=(\d)$", stdout, re.M)]


def test_capture_with_a_clock_error_through_the_radio(oracle, tmp_path):
    fib, pay, nb = CL.inputs(oracle)
    n0 = oracle.subchannel_plan(T.o_sub(oracle, CL.SUBS[0]))[2]
    fib.tofile(tmp_path / "fib_in.bin"); pay.tofile(tmp_path / "pay_in.bin")
    # the files are read cyclically: frame j carries the payload of frame j mod 5
    cifs = np.concatenate([pay[0].reshape(4 * CL.N_FRAMES, nb)[:, :n0]] * 2)[:4 * N_FRAMES]
    sent_fibs = {bytes(r) for r in fib.reshape(-1, 30)}
    common = [*SUB_ARGS, "--fib-file", tmp_path / "fib_in.bin", "--payload-file", tmp_path / "pay_in.bin", "--frames", N_FRAMES, "--snr-db", SNR_DB,
              "--noise-seed", 9, "--tap", "0:1:0", "--tap", f"200:{CL.TAP2}:0"]
    for name, ppm in (("clean", 0), ("drift", PPM)):
        sim(*common, "--clock-ppm", ppm, "-o", tmp_path / f"{name}.u8")
        (tmp_path / name).mkdir()
    # a clock error of 200 ppm: tracked, everything that was sent arrives
    fib_t, msc_t, log_t, out_t = radio(tmp_path / "drift.u8", tmp_path / "drift", "--soft-bits", "csi", "--track-clock", "--clock-report")
    rep = reported(out_t)
    print(f"tracked: {len(fib_t) // 30} FIBs, {len(msc_t)} bytes; reported {[(f, p, v) for f, p, v in rep]}; {log_t.strip().splitlines()[-1]}")
    assert len(rep) >= N_FRAMES - 3 and all(v == 1 for _, _, v in rep) and "clock: frames_tracked=" in log_t and "frames_kept=0" in log_t
    assert wrong_bytes(msc_t, cifs) == 0
    got_fibs = [fib_t[i:i + 30] for i in range(0, len(fib_t), 30)]
    assert len(got_fibs) >= 12 * (N_FRAMES - 3) and all(f in sent_fibs for f in got_fibs)
    assert all(abs(p - PPM) <= L.ACCURACY_BOUND_PPM for _, p, _ in rep[2:]), rep                       # a stream made with +X tracks to +X
    # the same capture untracked loses FIBs
    fib_p, msc_p, log_p, out_p = radio(tmp_path / "drift.u8", tmp_path / "drift", "--soft-bits", "csi")
    print(f"untracked: {len(fib_p) // 30} FIBs, {len(msc_p)} bytes")
    assert len(fib_p) < len(fib_t) and "clock:" not in log_p and not reported(out_p)
    # on top of the band weights the flag works the same way
    fib_b, msc_b, log_b, _ = radio(tmp_path / "drift.u8", tmp_path / "drift", "--soft-bits", "banded-dd", "--track-clock")
    assert wrong_bytes(msc_b, cifs) == 0 and len(fib_b) >= len(fib_t) - 12
    # without a clock error: the tracked run is checked on what was sent
    fib_c, msc_c, log_c, out_c = radio(tmp_path / "clean.u8", tmp_path / "clean", "--soft-bits", "csi", "--track-clock", "0.5", "--clock-report")
    rep = reported(out_c)
    print(f"no clock error: {len(fib_c) // 30} FIBs; reported {[p for _, p, _ in rep]}")
    assert wrong_bytes(msc_c, cifs) == 0 and all(bytes(fib_c[i:i + 30]) in sent_fibs for i in range(0, len(fib_c), 30)) and len(fib_c) >= 12 * (N_FRAMES - 3)
    assert all(v == 1 and abs(p) <= L.ACCURACY_BOUND_PPM for _, p, v in rep)


def test_option_rules(tmp_path):
    np.zeros(8192, np.uint8).tofile(tmp_path / "iq.u8")
    for extra, text in ((["--track-clock"], b"--track-clock needs --soft-bits csi, banded or banded-dd"),
                        (["--soft-bits", "normalised", "--track-clock"], b"no products to de-rotate"),
                        (["--soft-bits", "csi", "--track-clock", "0"], b"--track-clock: a gain above 0, up to 1"),
                        (["--soft-bits", "csi", "--track-clock", "1.5"], b"--track-clock: a gain above 0, up to 1"),
                        (["--soft-bits", "csi", "--clock-report"], b"--clock-report needs --track-clock"),
                        (["--soft-bits", "csi", "--track-clock", "--configuration", "dab"], b"--soft-bits needs the OFDM stage")):
        res = subprocess.run([RADIO, "-i", str(tmp_path / "iq.u8")] + extra, capture_output=True, timeout=60)
        assert res.returncode != 0 and text in res.stderr, (extra, res.stderr[-500:])
    for policy in ("csi", "banded", "banded-dd"):
        res = subprocess.run([RADIO, "-i", str(tmp_path / "iq.u8"), "--soft-bits", policy, "--track-clock", "0.5", "--symbol-weights"], capture_output=True, timeout=60)
        assert res.returncode == 0 and b"clock: frames_tracked=0 frames_kept=0 ppm=0.000" in res.stderr, (policy, res.stderr[-500:])
