"""-m gpu: dabgpu_radio_cli --soft-bits.  A capture of the closed loop of tests/softbit_loop.py at its first operating point (10 dB, fading
seed 2: the reference's soft bits lose FIBs there, the weighted ones deliver all 60) is written as complex float and received by the
tool: with --soft-bits csi every FIB of the frames it delivers is a transmitted one and none is missing; with the default policy FIBs
are lost.  An unknown policy name and a level outside [1, 127] are refused."""
import os
import subprocess

import numpy as np
import pytest

import channel_fading_model as FM
import channel_loop as CL
import softbit_loop as SL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dab-radio_amd", "host", "apps", "dabgpu_radio_cli")


def run(capture, out, *extra):
    res = subprocess.run([CLI, "-i", str(capture), "--ofdm-input-mode", "raw_f32l", "--radio-fib-output", str(out)] + [str(a) for a in extra],
                         capture_output=True, timeout=300)
    return res


def test_csi_delivers_the_transmitted_fibs_at_the_weighted_operating_point(oracle, tmp_path):
    host = FM.build_host_model(tmp_path)
    fib, pay, nb = CL.inputs(oracle)
    iq = CL.oracle_iq(oracle, fib, pay)
    snr_db, seed = SL.POINTS[0]
    rx = SL.received(host, iq, snr_db, seed)
    # (a NULL symbol's worth of the stream is repeated in front so that the tool's power-dip search has its run-in)
    np.concatenate([rx[:2656], rx]).astype(np.complex64).tofile(tmp_path / "iq.c32")
    res = run(tmp_path / "iq.c32", tmp_path / "fib_csi.bin", "--soft-bits", "csi", "--soft-level", 64)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    got = (tmp_path / "fib_csi.bin").read_bytes()
    sent = fib[0].reshape(CL.N_FRAMES, -1)
    print(f"csi: {len(got) // 30} FIBs")
    # the tool delivers every frame, or every frame but the one it acquires on: all of their FIBs, in order
    assert got in (sent.tobytes(), sent[1:].tobytes())
    res = run(tmp_path / "iq.c32", tmp_path / "fib_norm.bin")
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    norm = (tmp_path / "fib_norm.bin").read_bytes()
    print(f"normalised: {len(norm) // 30} FIBs")
    assert len(norm) < len(got)
    res = run(tmp_path / "iq.c32", tmp_path / "fib_n2.bin", "--soft-bits", "normalised")
    assert res.returncode == 0 and (tmp_path / "fib_n2.bin").read_bytes() == norm


def test_unknown_policy_and_bad_level_are_refused(tmp_path):
    np.zeros(4096, np.complex64).tofile(tmp_path / "iq.c32")
    res = run(tmp_path / "iq.c32", tmp_path / "f.bin", "--soft-bits", "llr")
    assert res.returncode != 0 and b"unknown soft-bit policy 'llr'" in res.stderr
    for level in ("0.5", "128", "nan"):
        res = run(tmp_path / "iq.c32", tmp_path / "f.bin", "--soft-bits", "csi", "--soft-level", level)
        assert res.returncode != 0 and b"level" in res.stderr, (level, res.stderr[-500:])
    for extra in (["--soft-level", "64"], ["--soft-bits", "normalised", "--soft-level", "64"]):      # a level without the policy it belongs to
        res = run(tmp_path / "iq.c32", tmp_path / "f.bin", *extra)
        assert res.returncode != 0 and b"--soft-level needs --soft-bits csi" in res.stderr, (extra, res.stderr[-500:])
