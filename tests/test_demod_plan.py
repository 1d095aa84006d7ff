"""CPU: the demodulation planner (dabgpu_host_plan_demod, dab-radio_amd/csrc/dabgpu_host_logic.cpp) -- which kernel one demodulator launch runs,
over what grid, with how much LDS, and where the phase tail goes.  tests/cpp/demod_plan_driver.cpp enumerates every combination of the facts
of a call against the launch rules, restated there from their description; a few plans are worked by hand here.  The same driver runs under
ASan + UBSan in tests/test_host_sanitizers.py."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
MODE1, GENERIC, WAVE, WAVE3 = range(4)
TAIL_NONE, TAIL_FUSED, TAIL_LAUNCH = range(3)


def build_driver(tmp_path, flags=()):
    exe = tmp_path / "demod_plan_driver"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          os.path.join(ROOT, "tests", "cpp", "demod_plan_driver.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


def check_every_combination(exe, env=None):
    res = subprocess.run([str(exe), "all"], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    out = json.loads(res.stdout.strip().splitlines()[-1])
    # modes 0..5 x loaders -1..4 x 8 boolean facts x 2 switches x mode I on the size-generic kernel x 11 run lengths x 4 batch sizes
    assert out["checked"] == 6 * 6 * 2 ** 11 * 11 * 4 and out["failed_checks"] == 0
    # both sides of every decision were reached
    for k in ("bad_mode", "bad_loader", "classed_views", "bank_sync_stride", "mode1", "generic", "wave", "wave3", "tail_none", "tail_fused", "tail_launch", "raise_lds"):
        assert out[k] > 1000, (k, out[k])
    assert out["refused"] < out["checked"] and out["mode1"] + out["generic"] + out["wave"] + out["wave3"] == out["checked"] - out["refused"]
    assert out["bad_mode"] == out["checked"] // 3                              # modes 0 and 5 of six
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("demod_plan"))


def plan(exe, mode, src=0, desc=0, fft=0, dqpsk=0, sync=0, stride=0, total_phase=0, fine_freq=0, classed=0, spb=0, n_frames=1, generic_mode1=0,
         sw_generic=0, sw_single=0):
    args = [mode, src, desc, fft, dqpsk, sync, stride, total_phase, fine_freq, classed, spb, n_frames, generic_mode1, sw_generic, sw_single]
    res = subprocess.run([str(exe), "plan"] + [str(int(a)) for a in args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout)


def test_every_combination_of_the_facts_follows_the_launch_rules(driver):
    check_every_combination(driver)


def test_plans_worked_by_hand(driver):
    # mode I, 1024 frames of complex float, soft bits only: three runs of 25 symbols, one workgroup each
    p = plan(driver, 1, n_frames=1024)
    assert p == {"status": 0, "family": MODE1, "variant": 0, "symbols_per_block": 25, "chunks": 3, "grid": 3072, "threads": 256, "lds_bytes": 0,
                 "raise_lds_limit": 0, "tail": TAIL_NONE, "fine_stride": 1}
    # a whole frame per workgroup fuses the phase tail; three runs launch it; the display views never fuse
    assert plan(driver, 1, spb=75, fine_freq=1, n_frames=2)["tail"] == TAIL_FUSED
    assert plan(driver, 1, spb=25, total_phase=1, n_frames=2)["tail"] == TAIL_LAUNCH
    assert plan(driver, 1, spb=75, total_phase=1, dqpsk=1)["tail"] == TAIL_LAUNCH
    p = plan(driver, 1, spb=1, n_frames=2)
    assert (p["chunks"], p["grid"]) == (75, 150)
    assert plan(driver, 1, spb=76)["symbols_per_block"] == 25 and plan(driver, 1, spb=-1)["symbols_per_block"] == 25
    # sync records: they carry the fine-frequency word (six floats apart), so the tail runs without either output being given
    p = plan(driver, 1, sync=1, stride=1, spb=75)
    assert (p["tail"], p["fine_stride"]) == (TAIL_FUSED, 6)
    # variants: s16 loader (3) of a bank round in class order = ((3 * 2 + 1) * 3 + 2); u8 with views = ((1 * 2 + 0) * 3 + 1); a bank has no tail
    assert plan(driver, 1, src=3, desc=1, classed=1)["variant"] == 23
    assert plan(driver, 1, src=1, fft=1)["variant"] == 7
    assert plan(driver, 1, src=2, desc=1, total_phase=1, spb=75)["tail"] == TAIL_NONE
    # modes II-IV: one wavefront per run, four runs per workgroup; mode III two symbols per wavefront
    p = plan(driver, 2, n_frames=3)
    assert (p["family"], p["symbols_per_block"], p["chunks"], p["grid"], p["threads"], p["lds_bytes"]) == (WAVE, 19, 4, 3, 256, 0)
    p = plan(driver, 3, n_frames=3)
    assert (p["family"], p["chunks"], p["grid"]) == (WAVE3, 8, 6)
    assert plan(driver, 3, sw_single=1)["family"] == WAVE and plan(driver, 4, src=2, desc=1)["variant"] == 3
    assert plan(driver, 3, spb=152)["chunks"] == 1 and plan(driver, 3, spb=153)["symbols_per_block"] == 19
    # the FFT view or the switch keeps them on the size-generic kernel: 128 threads for FFT 512 / 256, (period + 3 FFTs) * 8 + 2048 bytes
    p = plan(driver, 2, fft=1, n_frames=3)
    assert (p["family"], p["grid"], p["threads"], p["lds_bytes"], p["raise_lds_limit"]) == (GENERIC, 12, 128, (638 + 3 * 512) * 8 + 2048, 0)
    p = plan(driver, 4, sw_generic=1)
    assert (p["family"], p["threads"], p["lds_bytes"]) == (GENERIC, 256, (1276 + 3 * 1024) * 8 + 2048)
    # mode I on the size-generic kernel is the one launch above 48 KB; the switch alone does not move mode I there
    p = plan(driver, 1, generic_mode1=1, n_frames=2)
    assert (p["family"], p["symbols_per_block"], p["grid"], p["lds_bytes"], p["raise_lds_limit"]) == (GENERIC, 19, 8, 71616, 1)
    assert plan(driver, 1, sw_generic=1)["family"] == MODE1
    # 2^24 frames of mode III, one symbol per run: 2 550 136 832 workgroups, no wrap
    assert plan(driver, 3, fft=1, spb=1, n_frames=1 << 24)["grid"] == 152 << 24
    assert plan(driver, 3, spb=1, n_frames=1 << 24)["grid"] == 38 << 24


def test_refusals_name_their_reason(driver):
    for kw, text in ((dict(mode=0), "invalid transmission mode 0"), (dict(mode=5), "invalid transmission mode 5"),
                     (dict(mode=1, src=4), "no loader 4"), (dict(mode=1, src=-1, desc=1), "no loader -1"),
                     (dict(mode=1, classed=1, fft=1), "class order"), (dict(mode=1, classed=1, dqpsk=1), "class order"),
                     (dict(mode=1, desc=1, sync=1), "bank round"), (dict(mode=1, desc=1, stride=1), "bank round")):
        p = plan(driver, **kw)
        assert p["status"] == 2 and text in p["error"], (kw, p)
    # the other kernels refuse nothing more: the loader is not looked at without descriptors and runs as s16 (variant 4) when unknown with
    # them, and the mode I kernel's facts are not theirs
    assert plan(driver, 2, src=4)["variant"] == 0 and plan(driver, 2, src=4, desc=1)["variant"] == 4 and plan(driver, 3, src=-1, desc=1)["variant"] == 4
    assert plan(driver, 4, classed=1, fft=1, desc=1, sync=1)["status"] == 0
