"""CPU: the two planners of the sampling-clock tracker (dabgpu_clock_estimate_plan, dabgpu_clock_derotate_plan,
dab-radio_amd/csrc/dabgpu_host_logic.cpp): every refusal by its reason, the edges of n_frames, alignment, gain and overlap, the geometry.
tests/cpp/clock_plan_fuzz.cpp restates the rules and fuzzes them, and runs the host forms, under ASan + UBSan as a program of its own."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
INVALID_ARG = 2
ESTIMATE_LDS, DEROTATE_LDS = 48, 12288
FRAME_BYTES = 75 * 1536 * 8


def build_driver(out_dir, flags=()):
    exe = out_dir / "clock_plan_fuzz"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          os.path.join(ROOT, "tests", "cpp", "clock_plan_fuzz.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("clock_plan"))


def run_json(exe, args):
    res = subprocess.run([str(exe)] + [a if isinstance(a, str) else str(int(a)) for a in args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout)


def eplan(exe, mode=1, dq=0x1000000, n_frames=3, sync=0, slope_in=0, gain="1.0", slope_out=0x50000, residual=0, corr=0, valid=0, null_out=0):
    return run_json(exe, ["eplan", mode, dq, n_frames, sync, slope_in, str(gain), slope_out, residual, corr, valid, null_out])


def dplan(exe, mode=1, src=0x1000000, dst=0x1000000, n_frames=3, sync=0, slope=0x50000, spb=0, null_out=0):
    return run_json(exe, ["dplan", mode, src, dst, n_frames, sync, slope, spb, null_out])


def test_estimator_geometry(driver):
    assert eplan(driver) == dict(status=0, error="", grid=3, threads=256, lds_bytes=ESTIMATE_LDS)
    assert eplan(driver, n_frames=1)["grid"] == 1 and eplan(driver, n_frames=1 << 24)["grid"] == 1 << 24
    base = eplan(driver, n_frames=67)
    for kw in (dict(sync=0x60004), dict(slope_in=0x70008), dict(slope_in=0x50000), dict(residual=0x90008, corr=0x98004, valid=0xA0004), dict(dq=0x1000010),
               dict(gain="0.25"), dict(gain="1e-30")):
        assert eplan(driver, n_frames=67, **kw) == base, kw
    import dabgpu
    g = dabgpu.clock_estimate_plan(0x1000000, 5, slope_out=0x50000)
    assert (g.grid, g.threads, g.lds_bytes) == (5, 256, ESTIMATE_LDS)
    with pytest.raises(dabgpu.DabGpuError, match="16-byte"):
        dabgpu.clock_estimate_plan(0x1000008, 5, slope_out=0x50000)
    with pytest.raises(dabgpu.DabGpuError, match="mode"):
        dabgpu.clock_estimate_plan(0x1000000, 5, slope_out=0x50000, mode=2)
    with pytest.raises(dabgpu.DabGpuError, match="gain"):
        dabgpu.clock_estimate_plan(0x1000000, 5, slope_out=0x50000, gain=1.5)


def test_estimator_refusals_name_their_reason(driver):
    for kw, text in ((dict(mode=0), "mode"), (dict(mode=2), "mode"), (dict(mode=3), "mode"), (dict(mode=4), "mode"), (dict(mode=-1), "mode"),
                     (dict(n_frames=0), "n_frames"), (dict(n_frames=(1 << 24) + 1), "n_frames"),
                     (dict(dq=0), "null products"), (dict(dq=0x1000008), "16-byte"), (dict(dq=0x1000004), "16-byte"), (dict(dq=0x1000001), "16-byte"),
                     (dict(slope_in=0x70004), "8-byte"), (dict(slope_out=0x50004), "8-byte"), (dict(residual=0x90001), "8-byte"),
                     (dict(sync=0x60002), "4-byte"), (dict(corr=0x98002), "4-byte"), (dict(valid=0xA0003), "4-byte"),
                     (dict(gain="0"), "gain"), (dict(gain="-0.5"), "gain"), (dict(gain="1.0000001"), "gain"), (dict(gain="nan"), "gain"),
                     (dict(gain="inf"), "gain"),
                     (dict(slope_in=0x50008), "overlap"), (dict(slope_in=0x50000 - 16), "overlap"), (dict(slope_in=0x50000 + 16), "overlap"),
                     (dict(slope_out=0), "no output"), (dict(slope_out=0, sync=0x60000, slope_in=0x70000), "no output"),
                     (dict(null_out=1), "null result")):
        p = eplan(driver, **kw)
        assert p["status"] == INVALID_ARG and text in p["error"], (kw, p)
        if not kw.get("null_out"):
            assert p["grid"] == 0 and p["threads"] == 0 and p["lds_bytes"] == 0                 # a refusal leaves no geometry behind
    # the edges on the accepting side; every output alone is an output; the state in place, or just clear of it
    for kw in (dict(n_frames=1 << 24), dict(dq=0x1000010), dict(gain="1"), dict(gain="1e-45"), dict(slope_out=0, residual=0x80000),
               dict(slope_out=0, corr=0x80004), dict(slope_out=0, valid=0x80004), dict(slope_in=0x50000), dict(slope_in=0x50000 - 24),
               dict(slope_in=0x50000 + 24)):
        assert eplan(driver, **kw)["status"] == 0, kw


def test_derotator_planner(driver):
    base = dplan(driver)
    assert base["status"] == 0 and base["threads"] == 256 and base["lds_bytes"] == DEROTATE_LDS and base["grid"] == 3 * base["runs_per_frame"]
    assert base["symbols_per_block"] * base["runs_per_frame"] >= 75 > base["symbols_per_block"] * (base["runs_per_frame"] - 1)
    for spb, runs in ((1, 75), (5, 15), (7, 11), (38, 2), (74, 2), (75, 1)):
        g = dplan(driver, spb=spb, n_frames=67)
        assert (g["symbols_per_block"], g["runs_per_frame"], g["grid"]) == (spb, runs, 67 * runs)
    # symbols_per_block = 0: short runs for a small batch, 25 from 86 frames on, and the largest batch still fits a grid
    assert dplan(driver, n_frames=1)["runs_per_frame"] == 25 and dplan(driver, n_frames=86)["symbols_per_block"] == 25
    assert dplan(driver, n_frames=4096)["grid"] == 3 * 4096 and dplan(driver, n_frames=1 << 24)["grid"] == 3 << 24
    out_of_place = dplan(driver, dst=0x1000000 + 3 * FRAME_BYTES)
    assert out_of_place == base and dplan(driver, dst=0x1000000 - 3 * FRAME_BYTES) == base                  # just clear of the input
    for kw, text in ((dict(mode=0), "mode"), (dict(mode=2), "mode"), (dict(n_frames=0), "n_frames"), (dict(n_frames=(1 << 24) + 1), "n_frames"),
                     (dict(src=0), "null products"), (dict(dst=0), "null products"), (dict(src=0x1000008, dst=0x1000008), "16-byte"),
                     (dict(dst=0x2000004), "16-byte"),
                     (dict(dst=0x1000000 + 16), "overlap"), (dict(dst=0x1000000 + 3 * FRAME_BYTES - 16), "overlap"),
                     (dict(dst=0x1000000 - 3 * FRAME_BYTES + 16), "overlap"),
                     (dict(slope=0), "null slope"), (dict(slope=0x50004), "8-byte"), (dict(sync=0x60002), "4-byte"),
                     (dict(spb=76), "symbols_per_block"), (dict(spb=-1), "symbols_per_block"), (dict(null_out=1), "null result")):
        p = dplan(driver, **kw)
        assert p["status"] == INVALID_ARG and text in p["error"], (kw, p)
        if not kw.get("null_out"):
            assert p["grid"] == 0 and p["threads"] == 0 and p["lds_bytes"] == 0 and p["symbols_per_block"] == 0 and p["runs_per_frame"] == 0
    import dabgpu
    g = dabgpu.clock_derotate_plan(0x1000000, 0x1000000, 4, 0x50000, symbols_per_block=15)
    assert (g.symbols_per_block, g.runs_per_frame, g.grid, g.threads, g.lds_bytes) == (15, 5, 20, 256, DEROTATE_LDS)
    with pytest.raises(dabgpu.DabGpuError, match="overlap"):
        dabgpu.clock_derotate_plan(0x1000000, 0x1000010, 4, 0x50000)


def check_counters(out):
    assert out["failed_checks"] == 0 and out["checked"] == out["accepted"] + out["refused"] == out["derotate_accepted"] + out["derotate_refused"]
    assert out["accepted"] > 0 and all(r > 0 for r in out["reasons"]) and len(out["reasons"]) == 9, out
    assert out["derotate_accepted"] > 0 and all(r > 0 for r in out["derotate_reasons"]) and len(out["derotate_reasons"]) == 9, out


def test_rules_fuzzed(driver):
    res = subprocess.run([str(driver), "fuzz", "200000", "7"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    check_counters(json.loads(res.stdout.strip().splitlines()[-1]))
    res = subprocess.run([str(driver), "frames"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and json.loads(res.stdout)["failed_checks"] == 0, (res.stdout[-2000:], res.stderr[-4000:])


def test_planners_fuzzed_under_asan_and_ubsan(tmp_path):
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
    assert eplan(exe)["status"] == 0 and dplan(exe)["status"] == 0
