"""CPU: the receive-diversity planner (dabgpu_diversity_plan, dab-radio_amd/csrc/dabgpu_host_logic.cpp): every refusal by its reason,
the edges of every fact, the choice of the run length, and that grid x run length visits every (frame, symbol) exactly once.
tests/cpp/diversity_plan_fuzz.cpp restates the rules and fuzzes them under ASan + UBSan as a program of its own."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
INVALID_ARG = 2
FRAME_BITS = 230400


def build_driver(out_dir, flags=()):
    exe = out_dir / "diversity_plan_fuzz"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          os.path.join(ROOT, "tests", "cpp", "diversity_plan_fuzz.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("diversity_plan"))


def plan(exe, n_branches=2, n_frames=3, layout=0, spb=0, stride=0, bits=0x30000, dqpsk=0x10000, scale=0x20000, weight=0, sync=0, null_table=0,
         null_out=0, last_only=0):
    args = [n_branches, n_frames, layout, spb, stride, bits, dqpsk, scale, weight, sync, null_table, null_out, last_only]
    res = subprocess.run([str(exe), "plan"] + [str(int(a)) for a in args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout)


def test_geometry_and_the_choice_of_the_run_length(driver):
    p = plan(driver, n_frames=1024)
    assert p == dict(status=0, error="", symbols_per_block=25, runs_per_frame=3, grid=3072, threads=256, lds_bytes=6144)
    # small batches take shorter runs, so that the launch still spreads over the chip: the demodulator's rule
    assert plan(driver, n_frames=1)["runs_per_frame"] == 25 and plan(driver, n_frames=1)["symbols_per_block"] == 3
    assert plan(driver, n_frames=3)["grid"] == 3 * plan(driver, n_frames=3)["runs_per_frame"] >= 60
    assert plan(driver, n_frames=85)["runs_per_frame"] > 3 and plan(driver, n_frames=86)["runs_per_frame"] == 3
    # a run length that is given is taken as it is
    for spb in (1, 7, 25, 38, 74, 75):
        p = plan(driver, n_frames=5, spb=spb)
        assert p["symbols_per_block"] == spb and p["runs_per_frame"] == -(-75 // spb) and p["grid"] == 5 * p["runs_per_frame"]
    # nothing else enters the geometry
    base = plan(driver, n_frames=40, spb=7)
    for kw in (dict(layout=1), dict(stride=8 * FRAME_BITS), dict(weight=0x50000), dict(sync=0x60000), dict(n_branches=8), dict(n_branches=1)):
        assert plan(driver, n_frames=40, spb=7, **kw) == base
    assert plan(driver, n_frames=0)["status"] == 0 and plan(driver, n_frames=0)["grid"] == 0
    assert plan(driver, n_frames=1 << 24, spb=1)["grid"] == 75 << 24


def test_refusals_name_their_reason(driver):
    for kw, text in ((dict(n_branches=0), "n_branches"), (dict(n_branches=9), "n_branches"), (dict(n_branches=-1), "n_branches"),
                     (dict(n_frames=(1 << 24) + 1), "n_frames"), (dict(layout=2), "bits_layout"), (dict(layout=-1), "bits_layout"),
                     (dict(spb=-1), "symbols_per_block"), (dict(spb=76), "symbols_per_block"),
                     (dict(stride=FRAME_BITS - 16), "bits_frame_stride"), (dict(stride=FRAME_BITS + 8), "bits_frame_stride"), (dict(stride=16), "bits_frame_stride"),
                     (dict(bits=0), "d_bits"), (dict(bits=0x30008), "d_bits"),
                     (dict(dqpsk=0), "no products"), (dict(scale=0), "no scales"), (dict(dqpsk=0x10008), "16-byte"),
                     (dict(scale=0x20002), "4-byte"), (dict(weight=0x50001), "4-byte"), (dict(sync=0x60002), "4-byte"),
                     (dict(n_branches=8, dqpsk=0, last_only=1), "branch 7"), (dict(n_branches=3, scale=0x20001, last_only=1), "branch 2"),
                     (dict(null_table=1), "null"), (dict(null_out=1), "null")):
        p = plan(driver, **kw)
        assert p["status"] == INVALID_ARG and text in p["error"], (kw, p)
        if not kw.get("null_out"):
            assert p["grid"] == 0 and p["threads"] == 0 and p["symbols_per_block"] == 0        # a refusal leaves no geometry behind
    for kw in (dict(n_branches=1), dict(n_branches=8), dict(n_frames=1 << 24), dict(spb=75), dict(spb=1), dict(stride=FRAME_BITS), dict(stride=FRAME_BITS + 16),
               dict(layout=1), dict(weight=0x50004, sync=0x60004)):
        assert plan(driver, **kw)["status"] == 0, kw


@pytest.mark.parametrize("n_frames", [1, 3, 86, 700])
def test_grid_and_run_length_cover_every_symbol_exactly_once(driver, n_frames):
    for spb in (0, 1, 2, 7, 24, 25, 26, 37, 38, 74, 75):
        res = subprocess.run([str(driver), "cover", str(n_frames), str(spb)], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        out = json.loads(res.stdout)
        assert out["status"] == 0 and out["cells"] == 75 * n_frames == out["once"] and out["outside"] == 0, (spb, out)
        assert out["grid"] == n_frames * out["runs_per_frame"]


def check_counters(out):
    assert out["failed_checks"] == 0 and out["checked"] == out["accepted"] + out["refused"]
    assert out["accepted"] > 0 and out["chosen"] > 0 and all(r > 0 for r in out["reasons"]) and len(out["reasons"]) == 9, out


def test_rules_fuzzed(driver):
    res = subprocess.run([str(driver), "fuzz", "200000", "7"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    check_counters(json.loads(res.stdout.strip().splitlines()[-1]))


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
    for args in (("cover", "86", "0"), ("cover", "5", "7"), ("plan", "9", "3", "0", "0", "0", "196608", "65536", "131072", "0", "0")):
        res = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
