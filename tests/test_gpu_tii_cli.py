"""-m gpu: TII through the command-line tools.  dabgpu_simulate_transmitter --tii 11:5 --tii 40:17:0.5 at the test SNR of the closed loop
(tests/test_tii_closed_loop.py: 3 dB above the lowest exact SNR) into dabgpu_radio_cli --tii: every decision line names those two pairs
and no other -- without a carrier offset, and with 3.05 carrier spacings of it, where the line would carry the neighbouring combs if the
tool fed its decoder the first frame after the acquisition.  Without --tii the transmitter's bytes are what they were; frames between
the TII frames keep their zeros."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_tii_closed_loop import TEST_SNR_DB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_simulate_transmitter")
RX = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_radio_cli")
S, NULL = 196608, 2656


@pytest.mark.parametrize("cfo_hz", [0, 3050])
def test_transmitter_to_receiver(tmp_path, cfo_hz):
    iq = tmp_path / "tx.u8"
    res = subprocess.run([TX, "--tii", "11:5", "--tii", "40:17:0.5", "--snr-db", str(TEST_SNR_DB), "--cfo-hz", str(cfo_hz), "--frames", "20", "-o", str(iq)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([RX, "-i", str(iq), "--configuration", "ofdm", "--tii"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    print(res.stdout, res.stderr)
    lines = [l for l in res.stdout.splitlines() if l.startswith("tii ")]
    assert len(lines) >= 2, (res.stdout, res.stderr)
    for l in lines:
        pairs = [t.rsplit("/", 1)[0] for t in l.split(":", 1)[1].split()]
        assert pairs == ["11:5", "40:17"], l
    assert re.match(r"tii frames=8 ", lines[0]) and re.match(r"tii frames=16 ", lines[1])


def test_transmitter_options(tmp_path):
    run = lambda *a: subprocess.run([TX] + list(a), capture_output=True, timeout=120)
    plain = np.frombuffer(run("--frames", "2").stdout, np.uint8).reshape(2, S, 2)
    tii = run("--frames", "3", "--tii", "11:5")
    assert tii.returncode == 0, tii.stderr
    got = np.frombuffer(tii.stdout, np.uint8).reshape(3, S, 2)
    assert np.array_equal(got[1], plain[0]) and np.array_equal(got[:, NULL:], np.broadcast_to(plain[0, NULL:], (3, S - NULL, 2)))
    assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0, :NULL], plain[0, :NULL])
    for bad in (["--tii", "70:0"], ["--tii", "0:24"], ["--tii", "1:1"] * 5, ["--tii", "1:1", "--seed", "3"], ["--tii", "1:1", "-m", "2"]):
        res = run("--frames", "1", *bad)
        assert res.returncode == 1 and res.stdout == b"", bad
