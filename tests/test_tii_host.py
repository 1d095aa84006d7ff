"""CPU: the TII host logic of dab-radio_amd/csrc/dabgpu_host_logic.cpp at its edges -- dabgpu_tii_carriers, dabgpu_tii_validate, the
entry points' refusals before any device call -- and the same functions fuzzed on their own under ASan + UBSan
(tests/cpp/tii_host_fuzz.cpp)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import tii_model as M

ROOT = M.ROOT
CSRC = M.CSRC
INVALID_ARG = 2


@pytest.fixture(scope="module")
def dabgpu():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu


def test_carriers_at_the_edges(dabgpu):
    L = dabgpu.lib()
    out = np.zeros(32, np.int32)
    assert L.dabgpu_tii_carriers(0, 0, out.ctypes.data) == 0 and out[0] == -768 + 48 * 4 and out[-1] == 385 + 48 * 7 + 1
    assert L.dabgpu_tii_carriers(69, 23, out.ctypes.data) == 0 and out[0] == -768 + 46 and out[-1] == 385 + 46 + 48 * 3 + 1
    assert max(dabgpu.tii_carriers(0, 23)) == 768 and min(dabgpu.tii_carriers(69, 0)) == -768
    for p, c, text in ((70, 0, "main id 70"), (-1, 0, "main id -1"), (0, 24, "sub id 24"), (0, -1, "sub id -1")):
        assert L.dabgpu_tii_carriers(p, c, out.ctypes.data) == INVALID_ARG and text.encode() in L.dabgpu_last_error()
    assert L.dabgpu_tii_carriers(0, 0, None) == INVALID_ARG
    assert C.sizeof(C.c_float) * 2 == np.dtype(dabgpu.TII_TX_DTYPE).itemsize == 8 and np.dtype(dabgpu.TII_RECORD_DTYPE).itemsize == 16


def test_list_validation(dabgpu):
    L = dabgpu.lib()
    ok = [[], [(0, 0, 0.0)], [(69, 23, -3.0e38), (0, 0, 1.0), (69, 0, 1e-30), (0, 23, 2.0)]]
    dabgpu.tii_validate(*dabgpu.tii_lists(ok))
    for bad, text in (([[(70, 0, 1.0)]], "frame 0: transmitter 0: main id 70"), ([[], [(1, 1, 1.0), (0, 24, 1.0)]], "frame 1: transmitter 1: sub id 24"),
                      ([[(1, 1, 1.0)] * 5], "5 transmitters"), ([[(1, 1, float("nan"))]], "amp is not finite"),
                      ([[(1, 1, float("-inf"))]], "amp is not finite")):
        with pytest.raises(dabgpu.DabGpuError) as err:
            dabgpu.tii_validate(*dabgpu.tii_lists(bad))
        assert text in str(err.value)
    lists, counts = dabgpu.tii_lists([[(200, 200, float("nan"))]])
    counts[0] = 0                                                            # entries beyond the count are not read
    dabgpu.tii_validate(lists, counts)
    assert L.dabgpu_tii_validate(None, counts.ctypes.data, 1) == INVALID_ARG
    assert L.dabgpu_tii_validate(None, None, 5) == 0 and L.dabgpu_tii_validate(lists.ctypes.data, counts.ctypes.data, 0) == 0


def test_entry_points_check_before_any_device_call(dabgpu):
    """no device here: a call that reached one would fail differently (or crash on the fake handles)"""
    L = dabgpu.lib()
    fake = C.c_void_p(0x1000)
    h = C.c_void_p()
    pl = np.zeros(75 * 384, np.uint8)
    out = np.zeros(196608, np.complex64)
    f32 = dabgpu.IQ_FORMATS.index("raw_f32l")
    for bad, text in (([[(70, 0, 1.0)]], b"main id 70"), ([[(0, 24, 1.0)]], b"sub id 24"), ([[(1, 1, 1.0)] * 5], b"5 transmitters")):
        lists, counts = dabgpu.tii_lists(bad)
        assert L.dabgpu_ofdm_modulate_frames_tii_host_sync(fake, 1, pl.ctypes.data, 0, 1, None, 0.0, out.ctypes.data, f32, lists.ctypes.data,
                                                           counts.ctypes.data) == INVALID_ARG and text in L.dabgpu_last_error()
    lists, counts = dabgpu.tii_lists([[(1, 1, 1.0)]])
    for mode in (2, 3, 4):
        assert L.dabgpu_ofdm_modulate_frames_tii_host_sync(fake, mode, pl.ctypes.data, 0, 1, None, 0.0, out.ctypes.data, f32, lists.ctypes.data,
                                                           counts.ctypes.data) == INVALID_ARG and b"mode I only" in L.dabgpu_last_error()
        assert L.dabgpu_ofdm_modulate_frames_tii(fake, mode, fake, 0, 1, None, 0.0, fake, f32, None, fake, fake) == INVALID_ARG
        assert b"mode I only" in L.dabgpu_last_error()
    assert L.dabgpu_ofdm_modulate_frames_tii(None, 1, fake, 0, 1, None, 0.0, fake, f32, None, fake, fake) == INVALID_ARG
    assert L.dabgpu_ofdm_modulate_frames_tii(fake, 1, fake, 0, 1, None, 0.0, C.c_void_p(0x1008), f32, None, fake, fake) == INVALID_ARG
    assert L.dabgpu_tii_bank_create(None, 1, None, C.byref(h)) == INVALID_ARG
    assert L.dabgpu_tii_bank_create(fake, 1, None, None) == INVALID_ARG
    assert L.dabgpu_tii_bank_create(fake, 0, None, C.byref(h)) == INVALID_ARG and b"0 receivers" in L.dabgpu_last_error()
    assert L.dabgpu_tii_bank_create(fake, (1 << 20) + 1, None, C.byref(h)) == INVALID_ARG
    cfg = np.array([np.nan, 0], np.float32)
    assert L.dabgpu_tii_bank_create(fake, 1, cfg.ctypes.data, C.byref(h)) == INVALID_ARG and b"threshold" in L.dabgpu_last_error()
    assert L.dabgpu_tii_bank_reset(None, None) == INVALID_ARG
    assert L.dabgpu_tii_bank_process(None, fake, 4199, 0, None, None, 0, None, None, None) == INVALID_ARG
    assert L.dabgpu_tii_bank_process_host_sync(None, fake, 2656, 0, 0.0, 0, 0, None, None) == INVALID_ARG
    assert L.dabgpu_tii_bank_read(None, None, None, None) == INVALID_ARG
    L.dabgpu_tii_bank_destroy(None)


def test_host_logic_fuzzed_under_asan_and_ubsan(tmp_path):
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(p) or not os.path.exists(p):
        pytest.skip("libasan.so is not installed with this gcc")
    exe = tmp_path / "tii_host_fuzz"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "tii_host_fuzz.cpp"),
                          os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    for seed in (1, 2):
        res = subprocess.run([str(exe), "40000", str(seed)], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
        assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
        out = json.loads(res.stdout.strip().splitlines()[-1])
        assert out["failed_checks"] == 0
        keys = ("carriers_ok", "carriers_main_low", "carriers_main_high", "carriers_sub_low", "carriers_sub_high", "lists_ok", "lists_count",
                "lists_main", "lists_sub", "lists_amp", "mask_pattern", "mask_other")
        assert min(out[k] for k in keys) > 100, {k: out[k] for k in keys if out[k] <= 100}
