"""CPU: the planner of the decision-directed noise profile (dabgpu_dd_profile_plan, dab-radio_amd/csrc/dabgpu_host_logic.cpp): every
refusal by its reason, the edges of n_frames, alignment, alpha and the state's overlap, the geometry.  tests/cpp/dd_profile_plan_fuzz.cpp
restates the rules and fuzzes them, and runs the host forms, under ASan + UBSan as a program of its own."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
INVALID_ARG = 2
LDS = 6144 + 8


def build_driver(out_dir, flags=()):
    exe = out_dir / "dd_profile_plan_fuzz"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          os.path.join(ROOT, "tests", "cpp", "dd_profile_plan_fuzz.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("dd_profile_plan"))


def plan(exe, mode=1, dq=0x1000000, n_frames=3, alpha=0.25, sync=0, exclude=0, pin=0, pout=0, weight=0x50000, mean=0, noise=0, amp=0, valid=0,
         null_out=0):
    args = [mode, dq, n_frames, repr(float(alpha)), sync, exclude, pin, pout, weight, mean, noise, amp, valid, null_out]
    res = subprocess.run([str(exe), "plan"] + [a if isinstance(a, str) else str(int(a)) for a in args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout)


def test_geometry(driver):
    assert plan(driver) == dict(status=0, error="", grid=3, threads=256, lds_bytes=LDS)
    assert plan(driver, n_frames=1)["grid"] == 1 and plan(driver, n_frames=1 << 24)["grid"] == 1 << 24
    base = plan(driver, n_frames=67)
    for kw in (dict(sync=0x60000), dict(exclude=0x71000), dict(pin=0x800000, pout=0x800000), dict(pin=0x800000, pout=0x900000),
               dict(mean=0x80104, noise=0x90008, amp=0x98008, valid=0xA0004), dict(dq=0x1000010), dict(alpha=1.0)):
        assert plan(driver, n_frames=67, **kw) == base, kw
    import dabgpu
    g = dabgpu.dd_profile_plan(0x1000000, 5, band_weight=0x50000)
    assert (g.grid, g.threads, g.lds_bytes) == (5, 256, LDS)
    with pytest.raises(dabgpu.DabGpuError, match="alpha"):
        dabgpu.dd_profile_plan(0x1000000, 5, band_weight=0x50000, alpha=0.0)


def test_refusals_name_their_reason(driver):
    state = 3 * 512
    for kw, text in ((dict(mode=0), "mode"), (dict(mode=2), "mode"), (dict(mode=3), "mode"), (dict(mode=4), "mode"), (dict(mode=-1), "mode"),
                     (dict(n_frames=0), "n_frames"), (dict(n_frames=(1 << 24) + 1), "n_frames"),
                     (dict(dq=0), "null products"), (dict(dq=0x1000008), "16-byte"), (dict(dq=0x1000004), "16-byte"), (dict(dq=0x1000001), "16-byte"),
                     (dict(sync=0x60002), "4-byte"), (dict(exclude=0x71002), "4-byte"), (dict(pin=0x800003), "4-byte"), (dict(pout=0x900001), "4-byte"),
                     (dict(weight=0x50001), "4-byte"), (dict(mean=0x80202), "4-byte"), (dict(valid=0xA0002), "4-byte"),
                     (dict(noise=0x90004), "8-byte"), (dict(noise=0x90001), "8-byte"), (dict(amp=0x98004), "8-byte"), (dict(amp=0x98006), "8-byte"),
                     (dict(alpha=0.0), "alpha"), (dict(alpha=-0.25), "alpha"), (dict(alpha=1.0000001), "alpha"), (dict(alpha=float("nan")), "alpha"),
                     (dict(alpha=float("inf")), "alpha"),
                     (dict(pin=0x800000, pout=0x800004), "overlap"), (dict(pin=0x800000, pout=0x800000 + state - 4), "overlap"),
                     (dict(pin=0x800000 + state - 4, pout=0x800000), "overlap"),
                     (dict(weight=0), "no output"), (dict(weight=0, pin=0x800000, exclude=0x71000, sync=0x60000), "no output"),
                     (dict(null_out=1), "null result")):
        p = plan(driver, **kw)
        assert p["status"] == INVALID_ARG and text in p["error"], (kw, p)
        if not kw.get("null_out"):
            assert p["grid"] == 0 and p["threads"] == 0 and p["lds_bytes"] == 0                 # a refusal leaves no geometry behind
    # the edges on the accepting side; every output alone is an output
    for kw in (dict(n_frames=1 << 24), dict(dq=0x1000010), dict(alpha=1.0), dict(alpha=1e-30),
               dict(pin=0x800000, pout=0x800000), dict(pin=0x800000, pout=0x800000 + state), dict(pin=0x800000 + state, pout=0x800000),
               dict(weight=0, pout=0x80000), dict(weight=0, mean=0x80000), dict(weight=0, noise=0x80000), dict(weight=0, amp=0x80000),
               dict(weight=0, valid=0x80000)):
        assert plan(driver, **kw)["status"] == 0, kw


def check_counters(out):
    assert out["failed_checks"] == 0 and out["checked"] == out["accepted"] + out["refused"]
    assert out["accepted"] > 0 and all(r > 0 for r in out["reasons"]) and len(out["reasons"]) == 9, out


def test_rules_fuzzed(driver):
    res = subprocess.run([str(driver), "fuzz", "200000", "7"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    check_counters(json.loads(res.stdout.strip().splitlines()[-1]))
    res = subprocess.run([str(driver), "frames"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and json.loads(res.stdout)["failed_checks"] == 0, (res.stdout[-2000:], res.stderr[-4000:])


def test_planner_fuzzed_under_asan_and_ubsan(tmp_path):
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(p) or not os.path.exists(p):
        pytest.skip("libasan.so is not installed with this gcc")
    exe = build_driver(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for seed in (1, 2):
        res = subprocess.run([str(exe), "fuzz", "200000", str(seed)], capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
        check_counters(json.loads(res.stdout.strip().splitlines()[-1]))
    res = subprocess.run([str(exe), "frames"], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    assert plan(exe)["status"] == 0
