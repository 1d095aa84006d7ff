"""CPU: the stream bank's weighted soft bits in the demodulation planner (dabgpu_host_plan_demod, dab-radio_amd/csrc/dabgpu_host_logic.cpp).
A call with frame descriptors under DABGPU_SOFT_CSI is still refused with "bank" in the reason (tests/test_softbit_plan.py): the bank round
states `bank_soft`, and only then the planner answers with one of the eight kernels 36 + loader * 2 + (class order).  Without the fact
every plan and every refusal text is what it was before the fact existed; tests/cpp/bank_soft_plan_driver.cpp restates that planner in
full and the fact's rules from their description, enumerates the product of the facts and fuzzes them under ASan + UBSan as a program
of its own."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
INVALID_ARG = 2
NORMALISED, CSI = 0, 1


def build_driver(out_dir, flags=()):
    exe = out_dir / "bank_soft_plan_driver"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          os.path.join(ROOT, "tests", "cpp", "bank_soft_plan_driver.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("bank_soft_plan"))


def plan(exe, mode=1, src=0, desc=1, fft=0, dqpsk=0, sync=0, stride=0, classed=0, spb=19, n_frames=4, generic_mode1=0, policy=CSI, level=64.0, bank_soft=1):
    args = [mode, src, desc, fft, dqpsk, sync, stride, classed, spb, n_frames, generic_mode1, policy]
    res = subprocess.run([str(exe), "plan"] + [str(int(a)) for a in args] + [repr(float(level)), str(int(bank_soft))], capture_output=True, text=True,
                         timeout=60)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout)


def test_the_eight_variant_numbers(driver):
    seen = []
    for src in range(4):
        for classed in (0, 1):
            p = plan(driver, src=src, classed=classed)
            assert p["status"] == 0 and p["family"] == 0 and p["variant"] == 36 + 2 * src + classed, (src, classed, p)
            seen.append(p["variant"])
    assert seen == list(range(36, 44))
    for level in (1.0, 127.0):
        assert plan(driver, level=level)["variant"] == 36


def test_the_rest_of_the_plan_is_the_normalised_bank_rounds(driver):
    for kw in (dict(), dict(n_frames=1024), dict(n_frames=2048, src=1, classed=1), dict(spb=0, src=3), dict(spb=75, src=2), dict(spb=1, n_frames=3)):
        a, b = plan(driver, **kw), plan(driver, policy=NORMALISED, bank_soft=0, **kw)
        assert a["status"] == 0 and b["status"] == 0
        assert {k: a[k] for k in a if k != "variant"} == {k: b[k] for k in b if k != "variant"}, kw
        assert a["tail"] == 0                                        # a bank round runs its own phase kernel
    p = plan(driver, n_frames=1024)
    assert (p["symbols_per_block"], p["chunks"], p["grid"], p["threads"]) == (19, 4, 4096, 256)


def test_refusals_name_their_reason(driver):
    for kw, text in ((dict(fft=1), "a bank round has no display views under the weighted policy"),
                     (dict(dqpsk=1), "a bank round has no display views under the weighted policy"),
                     (dict(desc=0), "bank_soft"), (dict(policy=NORMALISED), "bank_soft"), (dict(desc=0, policy=NORMALISED), "bank_soft"),
                     (dict(mode=2), "mode I"), (dict(mode=3), "mode I"), (dict(mode=4), "mode I"), (dict(generic_mode1=1), "mode I"),
                     (dict(level=0.5), "level"), (dict(level=127.5), "level"), (dict(level=float("nan")), "level"),
                     (dict(policy=2), "policy"), (dict(policy=-1), "policy"),
                     (dict(classed=1, fft=1), "class order"), (dict(src=4), "no loader"), (dict(sync=1), "bank round"), (dict(stride=1), "bank round")):
        p = plan(driver, **kw)
        assert p["status"] == INVALID_ARG and text in p["error"], (kw, p)


def test_without_the_fact_the_refusal_and_its_text_are_unchanged(driver):
    for kw in (dict(), dict(classed=1, src=2), dict(fft=1)):
        p = plan(driver, bank_soft=0, **kw)
        assert p == {"status": INVALID_ARG, "error": "ofdm_demod: the weighted soft bits have no stream-bank loader (frame descriptors)"}, (kw, p)
    assert plan(driver, desc=0, bank_soft=0)["variant"] == 24
    assert plan(driver, policy=NORMALISED, bank_soft=0, src=3, classed=1)["variant"] == 23


def check_counters(out, fuzz=False):
    assert out["failed_checks"] == 0
    assert out["checked"] == out["as_before"] + out["no_desc"] + out["normalised"] + out["bad_policy"] + out["not_mode1"] + out["views"] + out["bad_level"] + out["weighted"]
    for k in ("as_before", "as_before_refused", "as_before_bank", "no_desc", "normalised", "bad_policy", "not_mode1", "views", "bad_level", "weighted"):
        assert out[k] > 0, (k, out)
    assert all(v > 0 for v in out["variants"]) and len(out["variants"]) == 8


def test_every_combination_follows_the_rules(driver):
    res = subprocess.run([str(driver), "all"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["checked"] == 6 * 6 * 2 ** 12 * 4 * 6 * 4 * 2
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
        check_counters(json.loads(res.stdout.strip().splitlines()[-1]), fuzz=True)
