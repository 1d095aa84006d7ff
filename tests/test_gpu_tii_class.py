"""-m gpu: the C++ classes of TII (dab-radio_amd/host/ofdm) through tests/cpp/tii_class_harness (built by build()).
OFDM_Modulator::SetTII: additive -- frames without a list are the frames of before, a frame with one equals the library's host form bit
for bit, a refused list throws and leaves the list in force.  TII_Decoder: accumulators behind its records equal the float32 host model
of tests/tii_model.py bit for bit, the first call after construction and after Reset() is not accumulated (DABGPU_TII_SETTLE_FRAMES)."""
import os
import subprocess

import numpy as np
import pytest

import tii_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "tii_class_harness")
S, NULL = 196608, 2656


def test_modulator_setter(tmp_path):
    import dabgpu
    rng = np.random.default_rng(8100)
    payload = rng.integers(0, 256, (1, 75 * 384), dtype=np.uint8)
    payload.tofile(tmp_path / "payload.bin")
    res = subprocess.run([EXE, "mod", str(tmp_path / "payload.bin"), str(tmp_path / "out.c64")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert "refused" in res.stdout and "main id 70" in res.stdout
    got = np.fromfile(tmp_path / "out.c64", np.complex64).reshape(4, S)
    ctx = dabgpu.Context(0)
    plain = ctx.ofdm_modulate_frames_host(1, payload, 1)[0]
    tii = ctx.ofdm_modulate_frames_tii_host(1, payload, 1, [[(11, 5, 1.0), (40, 17, 0.5)]])[0]
    ctx.close()
    u = lambda a: a.view(np.uint32)
    assert np.array_equal(u(got[0]), u(plain)) and np.array_equal(u(got[2]), u(plain)) and not plain[:NULL].any()
    assert np.array_equal(u(got[1]), u(tii)) and np.array_equal(u(got[3]), u(tii)) and np.abs(tii[:NULL]).max() > 0


def test_decoder_equals_the_host_model(oracle, tmp_path):
    host = M.build_host_model(tmp_path)
    prs = oracle.prs_fft()
    x = M.null_period(prs, [(11, 5, 1.0), (40, 17, 0.5), (33, 17, 0.7)])
    rng = np.random.default_rng(8200)
    n, w, fto, cfo = 6, 4000, 37, 3.05 / 2048
    win = np.zeros((n, w), np.complex64)
    for k in range(n):
        s = np.zeros(w, np.complex128)
        s[fto:fto + NULL] += x
        s *= np.exp(2j * np.pi * cfo * np.arange(w))
        s += 1.5 * (rng.standard_normal(w) + 1j * rng.standard_normal(w))
        win[k] = s
    win.tofile(tmp_path / "win.c64")
    freq = np.float32(-cfo)
    res = subprocess.run([EXE, "dec", str(tmp_path / "win.c64"), str(n), str(w), repr(float(freq)), str(fto), "3", str(tmp_path / "out.bin")],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert "frames 2" in res.stdout                                  # windows 4 and 5 since the Reset() before window 3
    out = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(n, 8 + 24 * 16)
    m = M.HostModel(host, oracle, 2.16)
    union = M.TABLE[40] | M.TABLE[33]
    for k in range(n):
        ok, cnt = out[k, :8].view(np.int32)
        if k in (0, 3):                                             # the settle frame after construction / Reset(): not accumulated
            assert ok == 0 and cnt == -1
            if k == 3:
                m.reset()
            continue
        m.process(win[k], fto, freq)
        exp = m.decide()
        assert ok == 1 and cnt == len(exp)
        got = out[k, 8:].view(np.int32).reshape(24, 4)[:cnt]           # main_id, sub_id, mask, strength bits
        assert np.array_equal(got[:, 0], exp["main_id"]) and np.array_equal(got[:, 1], exp["sub_id"])
        assert np.array_equal(got[:, 2].view(np.uint32), exp["mask"]) and np.array_equal(got[:, 3].view(np.uint32), exp["strength"].view(np.uint32))
    assert [(int(r[1]), int(r[0]), int(r[2])) for r in got] == [(5, 11, M.TABLE[11]), (17, -1, union)]
    # a span that does not hold the window: the class's exception
    res = subprocess.run([EXE, "dec", str(tmp_path / "win.c64"), str(n), str(w), "0", "1500", "-1", str(tmp_path / "out2.bin")],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "TII_Decoder" in res.stderr
