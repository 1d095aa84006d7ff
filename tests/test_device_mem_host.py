"""CPU: the owners of device memory, pinned memory, events and streams (dab-radio_amd/csrc/device_mem.h) as a stand-alone program
(tests/cpp/device_mem_host.cpp, its own main) against a counting stand-in for the runtime (tests/cpp/hip_stub), built with
-fsanitize=address,undefined -- leak detection on -- and run directly: creates and releases balance through scopes, moves and regrows,
the grow-only step, every partial failure of a create function, a seeded random walk."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")


def test_owner_program_under_sanitizers(tmp_path):
    exe = tmp_path / "device_mem_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "device_mem_host.cpp"), "-o", str(exe)], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    for steps, seed in ((4000, 1), (4000, 20261020)):
        res = subprocess.run([str(exe), str(steps), str(seed)], capture_output=True, timeout=600, env=env)
        assert res.returncode == 0, (res.stdout.decode()[-500:], res.stderr.decode()[-3000:])
        out = json.loads(res.stdout.decode().strip().splitlines()[-1])
        assert out["failed_checks"] == 0 and out["steps"] == steps and out["checks"] > steps
        assert out["made"] == out["released"] > 500
