"""-m gpu: the impulse blanker through the tools.  A channel-coded capture made by dabgpu_simulate_transmitter with the burst source of
tests/interferer_loop.py (white noise on 205 of every 20480 samples, I / S = 17 dB while on, SNR 12 dB) through dabgpu_radio_cli: with
--blank every FIB of the delivered frames and every sub-channel byte that was sent arrives and the tool prints its blanked share; without
the option fewer FIBs arrive.  On a capture made without an interferer the outputs without the option are what was sent, as before, no
blanker line is printed, and with the option nothing is blanked and the same bytes arrive."""
import os
import re
import subprocess

import numpy as np
import pytest

import channel_loop as CL
import interferer_loop as IL
import tx_encode_cases as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_simulate_transmitter")
RADIO = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_radio_cli")
SUB_ARGS = ["--subchannel", "0:48:eep3-A", "--subchannel", "200:52:uep20"]      # tests/channel_loop.py's SUBS
N_FRAMES = 8


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


def test_capture_with_bursts_through_the_radio(oracle, tmp_path):
    fib, pay, nb = CL.inputs(oracle)
    n0 = oracle.subchannel_plan(T.o_sub(oracle, CL.SUBS[0]))[2]
    fib.tofile(tmp_path / "fib_in.bin"); pay.tofile(tmp_path / "pay_in.bin")
    # the files are read cyclically: frame j carries the FIBs and the payload of frame j mod 5
    fibs = np.concatenate([fib[0].reshape(CL.N_FRAMES, -1)] * 2)[:N_FRAMES]
    cifs = np.concatenate([pay[0].reshape(4 * CL.N_FRAMES, nb)[:, :n0]] * 2)[:4 * N_FRAMES]
    common = [*SUB_ARGS, "--fib-file", tmp_path / "fib_in.bin", "--payload-file", tmp_path / "pay_in.bin", "--frames", N_FRAMES, "--snr-db", IL.SNR_DB,
              "--noise-seed", 9]
    bursts = ["--interferer", f"white:{IL.BURST_DB:.0f}", "--interferer-gate", f"{IL.BURST_PERIOD}:{IL.BURST_ON}", "--interferer-seed", 77]
    for name, extra in (("clean", []), ("bursts", bursts)):
        sim(*common, *extra, "-o", tmp_path / f"{name}.u8")
        (tmp_path / name).mkdir()
    # the tool may spend a frame or two acquiring, and the last frame is not delivered: no NULL follows it in the file
    expected = [sent_between(fibs, cifs, a, b) for a in range(3) for b in (N_FRAMES - 1, N_FRAMES)]
    # without an interferer and without the option: what it was
    got_fib, got_msc, log = radio(tmp_path / "clean.u8", tmp_path / "clean")
    assert (got_fib, got_msc) in expected and "blank blocks" not in log
    same_fib, same_msc, log = radio(tmp_path / "clean.u8", tmp_path / "clean", "--blank")
    assert (same_fib, same_msc) == (got_fib, got_msc)
    assert re.search(r"^blank blocks=0 of %d$" % (N_FRAMES * 196608 // 32), log, re.M), log[-500:]
    # bursts: with the blanker everything that was sent, without it fewer FIBs
    blk_fib, blk_msc, log = radio(tmp_path / "bursts.u8", tmp_path / "bursts", "--blank")
    m = re.search(r"^blank blocks=(\d+) of (\d+)$", log, re.M)
    print(f"--blank: {len(blk_fib) // 30} FIBs, {len(blk_msc) // n0} CIFs; {log.strip().splitlines()[-3:]}")
    assert (blk_fib, blk_msc) in expected
    assert m and int(m.group(2)) == N_FRAMES * 196608 // 32 and 0.01 * int(m.group(2)) < int(m.group(1)) < 0.02 * int(m.group(2))
    again, _, log = radio(tmp_path / "bursts.u8", tmp_path / "bursts", "--blank", 2.5)
    assert again == blk_fib
    raw_fib, raw_msc, log = radio(tmp_path / "bursts.u8", tmp_path / "bursts")
    print(f"no blanker: {len(raw_fib) // 30} FIBs; {log.strip().splitlines()[-2:]}")
    assert len(raw_fib) < len(blk_fib) and "blank blocks" not in log


def test_blank_option_rules(tmp_path):
    np.zeros(8192, np.uint8).tofile(tmp_path / "iq.u8")
    for extra, text in ((["--blank", "1"], b"--blank: a threshold above 1"), (["--blank", "2000"], b"--blank: a threshold above 1"),
                        (["--blank", "--transmission-mode", "2"], b"transmission mode 1 only"),
                        (["--blank", "--configuration", "dab"], b"--blank needs the OFDM stage"),
                        (["--blank", "abc"], b"unknown argument 'abc'"), (["--blank", "--tii", "--ofdm-block-size", "193921"], b"193920"),
                        (["--blank", "2.5", "--soft-bits", "banded", "--ofdm-block-size", "193952"], b"193920"),
                        (["--blank", "--snr", "--ofdm-block-size", "98304"], b"98272")):
        res = subprocess.run([RADIO, "-i", str(tmp_path / "iq.u8")] + extra, capture_output=True, timeout=60)
        assert res.returncode != 0 and text in res.stderr, (extra, res.stderr[-500:])
