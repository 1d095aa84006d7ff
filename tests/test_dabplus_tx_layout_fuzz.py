"""CPU: dabgpu_dabplus_superframe_layout (dab-radio_amd/csrc/dabgpu_host_logic.cpp) built on its own under ASan + UBSan and fuzzed
(tests/cpp/dabplus_tx_layout_fuzz.cpp), the way tests/test_host_sanitizers.py builds the rest of the device-free library code."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")


def test_layout_function_fuzzed_under_asan_and_ubsan(tmp_path):
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(p) or not os.path.exists(p):
        pytest.skip("libasan.so is not installed with this gcc")
    exe = tmp_path / "dabplus_tx_layout_fuzz"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "dabplus_tx_layout_fuzz.cpp"),
                          os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    for seed in (1, 2):
        res = subprocess.run([str(exe), "200000", str(seed)], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
        assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
        out = json.loads(res.stdout.strip().splitlines()[-1])
        assert out["failed_checks"] == 0
        # both sides of every decision were reached
        assert min(out["status0"], out["status1"], out["status2"], out["status3"]) > 100, out
