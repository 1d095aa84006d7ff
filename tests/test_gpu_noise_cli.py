"""-m gpu: the noise estimate through the command-line tools.  dabgpu_simulate_transmitter --snr-db S into dabgpu_radio_cli --snr: one line
per settled frame, `snr frame=N noise=... signal=... snr_db=...`, whose snr_db lies around S inside a tolerance derived below; the first
frame after the acquisition is skipped; without --snr the tool writes what it writes with it, less those lines.

What S becomes on the way.  The transmitter's noise_sigma is sqrt(P / (2 * 10^(S / 10))) per component against P = 1536, the mean power
per sample of a symbol, which is what SIGNAL / NOISE of the printed line estimates.  The capture is 8-bit: the scale is
4 / 1536 * 127.5 = 0.332 steps per unit, a symbol's power 1536 * 0.332^2 = 169.3 steps^2 per sample, and the truncating quantiser adds white
noise of 1 / 12 per component, 1 / 6 steps^2 per sample, to the channel's: the receiver sees 10 log10(169.3 / (169.3 / 10^(S/10) + 1 / 6)),
0.043 dB below S at 10 dB.  The quantiser's mean of half a step is a carrier at the centre, outside every comb; it adds at most
|0.5 + 0.5 j|^2 = 0.5 steps^2 to the symbol's power, 0.3 % or 0.013 dB, which the tolerance carries as an allowance.

One frame's deviation.  NOISE has the estimator's derived relative deviation d_N = 0.0319 (tests/noise_model.py).  SIGNAL is the mean of
|s + n|^2 over 2048 samples less NOISE; the symbol's own power over its useful part is exact (Parseval), the cross term and the noise's
own power give a relative variance of (2 / snr + 1 / snr^2) / 2048, and NOISE enters once more with d_N / snr.  snr_db is 10 / ln 10
times the relative error of the ratio; five such deviations per frame, and five over sqrt(n) for the mean of n frames."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import noise_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_simulate_transmitter")
RX = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_radio_cli")
SNR_DB = 10.0
FRAMES = 20
LINE = re.compile(r"snr frame=(\d+) noise=(\S+) signal=(\S+) snr_db=(\S+)$")


def expected_db(s_db):
    symbol = 1536.0 * (4.0 / 1536.0 * 127.5) ** 2
    return 10.0 * math.log10(symbol / (symbol / 10.0 ** (s_db / 10.0) + 1.0 / 6.0))


def deviation_db(s_db):
    snr = 10.0 ** (s_db / 10.0)
    d_n = M.relative_deviation()
    return 10.0 / math.log(10.0) * math.sqrt(d_n ** 2 + (2.0 / snr + 1.0 / snr ** 2) / 2048.0 + (d_n / snr) ** 2)


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    iq = tmp_path_factory.mktemp("noise_cli") / "tx.u8"
    res = subprocess.run([TX, "--snr-db", str(SNR_DB), "--frames", str(FRAMES), "-o", str(iq)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    return iq


def receive(iq, out, *options):
    res = subprocess.run([RX, "-i", str(iq), "--configuration", "ofdm", "--ofdm-enable-output", "--ofdm-output", str(out), *options],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    return res.stdout


def test_printed_snr_lies_around_the_transmitters(capture, tmp_path):
    stdout = receive(capture, tmp_path / "bits.bin", "--snr")
    got = [LINE.match(l) for l in stdout.splitlines() if l.startswith("snr ")]
    assert all(got) and len(got) >= FRAMES - 5, stdout
    frames = [int(m.group(1)) for m in got]
    db = np.array([float(m.group(4)) for m in got])
    noise, signal = np.array([float(m.group(2)) for m in got]), np.array([float(m.group(3)) for m in got])
    want, dev, allowance = expected_db(SNR_DB), deviation_db(SNR_DB), 10.0 * math.log10(1.0 + 0.5 / 169.3)
    print(f"frames {frames}\nsnr_db {db.tolist()}\nexpected {want:.3f} dB, one frame's deviation {dev:.3f} dB, mean {db.mean():.3f}, sample deviation {db.std():.3f}")
    assert frames[0] >= 2 and frames == sorted(set(frames))                       # the first frame after the acquisition is skipped; one line per frame
    assert abs(want - (SNR_DB - 0.043)) < 0.001
    assert (np.abs(db - want) < 5.0 * dev + allowance).all()
    assert abs(db.mean() - want) < 5.0 * dev / math.sqrt(len(db)) + allowance
    assert np.allclose(10.0 * np.log10(signal / noise), db, atol=0.006)            # the line is consistent with itself (two decimals)


def test_without_the_option_the_tool_does_what_it_did(capture, tmp_path):
    plain = receive(capture, tmp_path / "plain.bin")
    with_snr = receive(capture, tmp_path / "snr.bin", "--snr")
    assert "snr " not in plain
    assert [l for l in with_snr.splitlines() if not l.startswith("snr ")] == plain.splitlines()
    assert (tmp_path / "plain.bin").read_bytes() == (tmp_path / "snr.bin").read_bytes() and (tmp_path / "plain.bin").stat().st_size > 0
    # ... and beside --tii the decision lines are those of --tii alone
    tii = receive(capture, tmp_path / "tii.bin", "--tii")
    both = receive(capture, tmp_path / "both.bin", "--tii", "--snr")
    assert [l for l in both.splitlines() if not l.startswith("snr ")] == tii.splitlines()
    for bad in (["--snr", "--ofdm-block-size", "2551"], ["--snr", "--ofdm-block-size", "98305"], ["--snr", "--input-rate", "2400000"]):
        res = subprocess.run([RX, "-i", str(capture), "--configuration", "ofdm", *bad], capture_output=True, text=True, timeout=120)
        assert res.returncode != 0 and "--snr" in res.stderr, (bad, res.stderr)
