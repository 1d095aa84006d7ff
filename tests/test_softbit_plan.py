"""CPU: the soft-decision policy in the demodulation planner (dabgpu_host_plan_demod, dab-radio_amd/csrc/dabgpu_host_logic.cpp).  The weighted
policy's kernels are numbered behind the 24 there were -- 24 + loader * 3 + layout --, the old numbers stay, and the planner refuses
the policy for modes II-IV, for a bank round (frame descriptors) and for a level outside [1, 127], each with its reason.
tests/cpp/softbit_plan_driver.cpp enumerates the combinations against the rules restated there and fuzzes them under ASan + UBSan as a
program of its own."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
INVALID_ARG = 2
NORMALISED, CSI = 0, 1


def build_driver(out_dir, flags=()):
    exe = out_dir / "softbit_plan_driver"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          os.path.join(ROOT, "tests", "cpp", "softbit_plan_driver.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("softbit_plan"))


def plan(exe, mode=1, src=0, desc=0, fft=0, dqpsk=0, sync=0, classed=0, spb=0, n_frames=1, generic_mode1=0, policy=CSI, level=64.0):
    args = [mode, src, desc, fft, dqpsk, sync, classed, spb, n_frames, generic_mode1, policy]
    res = subprocess.run([str(exe), "plan"] + [str(int(a)) for a in args] + [repr(float(level))], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout)


def test_new_variant_numbers_and_the_old_ones(driver):
    for src in range(4):
        assert plan(driver, src=src)["variant"] == 24 + 3 * src                            # soft bits only
        assert plan(driver, src=src, dqpsk=1)["variant"] == 24 + 3 * src + 1               # + display views
        assert plan(driver, src=src, fft=1, dqpsk=1)["variant"] == 24 + 3 * src + 1
        assert plan(driver, src=src, classed=1)["variant"] == 24 + 3 * src + 2             # class order
        # the normalised policy keeps the numbers it had: ((loader * 2 + bank) * 3 + layout)
        for desc in (0, 1):
            for layout, kw in enumerate((dict(), dict(fft=1), dict(classed=1))):
                assert plan(driver, src=src, desc=desc, policy=NORMALISED, **kw)["variant"] == (src * 2 + desc) * 3 + layout
    assert plan(driver, src=3, desc=1, classed=1, policy=NORMALISED)["variant"] == 23
    assert plan(driver, src=3, classed=1)["variant"] == 35                                  # the last of 36
    # the level does not enter a normalised plan, whatever it is
    assert plan(driver, policy=NORMALISED, level=1000.0) == plan(driver, policy=NORMALISED, level=64.0)
    # run length, grid and phase tail are those of the normalised call
    for kw in (dict(n_frames=1024), dict(spb=75, sync=1, n_frames=4), dict(spb=1, n_frames=2), dict(spb=38, sync=1)):
        a, b = plan(driver, **kw), plan(driver, policy=NORMALISED, **kw)
        assert a["status"] == 0 and {k: a[k] for k in a if k != "variant"} == {k: b[k] for k in b if k != "variant"}
    assert plan(driver, spb=75, sync=1)["tail"] == 1 and plan(driver, spb=25, sync=1)["tail"] == 2


def test_refusals_name_their_reason(driver):
    for kw, text in ((dict(mode=2), "mode I"), (dict(mode=3), "mode I"), (dict(mode=4), "mode I"), (dict(mode=1, generic_mode1=1), "mode I"),
                     (dict(desc=1), "bank"), (dict(desc=1, classed=1, src=2), "bank"),
                     (dict(level=0.5), "level"), (dict(level=127.5), "level"), (dict(level=float("nan")), "level"), (dict(level=float("inf")), "level"),
                     (dict(level=-64.0), "level"), (dict(policy=2), "policy"), (dict(policy=-1), "policy"),
                     (dict(classed=1, fft=1), "class order"), (dict(src=4), "no loader")):
        p = plan(driver, **kw)
        assert p["status"] == INVALID_ARG and text in p["error"], (kw, p)
    for level in (1.0, 127.0):
        assert plan(driver, level=level)["status"] == 0
    # modes II-IV with the normalised policy are what they were
    assert plan(driver, mode=2, policy=NORMALISED, level=0.0)["status"] == 0


def test_configuration_check_of_the_entry_points(driver):
    def cfg(policy, level):
        res = subprocess.run([str(driver), "cfg", str(policy), repr(float(level))], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stderr
        return json.loads(res.stdout)
    assert cfg(0, 64)["status"] == 0 and cfg(1, 1)["status"] == 0 and cfg(1, 127)["status"] == 0
    assert cfg(0, 64)["null"] == INVALID_ARG
    for policy, level, text in ((2, 64, "policy"), (-1, 64, "policy"), (1, 0.999, "level"), (0, 128, "level"), (1, float("nan"), "level")):
        c = cfg(policy, level)
        assert c["status"] == INVALID_ARG and text in c["error"], (policy, level, c)


def check_counters(out):
    assert out["failed_checks"] == 0
    assert out["checked"] == out["refused"] + out["normalised"] + out["weighted"]
    for k in ("earlier", "normalised", "weighted", "bad_policy", "not_mode1", "bank", "bad_level"):
        assert out[k] > 0, (k, out)
    assert all(v > 0 for v in out["variants"]) and len(out["variants"]) == 12


def test_every_combination_follows_the_rules(driver):
    res = subprocess.run([str(driver), "all"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["checked"] == 6 * 6 * 2 ** 9 * 4 * 9 * 3
    check_counters(out)


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
    res = subprocess.run([str(exe), "all"], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
