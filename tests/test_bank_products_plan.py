"""CPU: the stream bank's DQPSK products in the demodulation planner (dabgpu_host_plan_demod, dab-radio_amd/csrc/dabgpu_host_logic.cpp).
A weighted bank round that asks for a display view is still refused with "a bank round has no display views under the weighted policy"
(tests/test_bank_soft_plan.py): the round states `bank_products`, a fact of its own, and only then the planner answers with one of the
four kernels 44 + loader, which store the products at the descriptor's bits slot.  Without the fact every plan and every refusal text is
what it was before the fact existed; tests/cpp/bank_products_plan_driver.cpp restates that planner in full and the fact's rules from
their description, enumerates the product of the facts and fuzzes them under ASan + UBSan as a program of its own."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
INVALID_ARG = 2
NORMALISED, CSI = 0, 1
NO_VIEWS = "ofdm_demod: a bank round has no display views under the weighted policy"


def build_driver(out_dir, flags=()):
    exe = out_dir / "bank_products_plan_driver"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          os.path.join(ROOT, "tests", "cpp", "bank_products_plan_driver.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("bank_products_plan"))


def plan(exe, mode=1, src=0, desc=1, fft=0, dqpsk=0, sync=0, stride=0, classed=0, spb=19, n_frames=4, generic_mode1=0, policy=CSI, level=64.0, bank_soft=1,
         bank_products=1):
    args = [mode, src, desc, fft, dqpsk, sync, stride, classed, spb, n_frames, generic_mode1, policy]
    res = subprocess.run([str(exe), "plan"] + [str(int(a)) for a in args] + [repr(float(level)), str(int(bank_soft)), str(int(bank_products))],
                         capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout)


def test_the_four_variant_numbers_behind_the_44_that_exist(driver):
    assert [plan(driver, src=src)["variant"] for src in range(4)] == [44, 45, 46, 47]
    for src in range(4):
        p = plan(driver, src=src)
        assert p["status"] == 0 and p["family"] == 0, (src, p)
    for level in (1.0, 127.0):
        assert plan(driver, level=level)["variant"] == 44
    # the existing numbers do not move
    assert [plan(driver, src=src, classed=c, bank_products=0)["variant"] for src in range(4) for c in (0, 1)] == list(range(36, 44))
    assert plan(driver, desc=0, bank_soft=0, bank_products=0)["variant"] == 24
    assert plan(driver, policy=NORMALISED, bank_soft=0, bank_products=0, src=3, classed=1)["variant"] == 23


def test_the_geometry_is_the_bank_rounds(driver):
    for kw in (dict(), dict(n_frames=1024), dict(n_frames=2048, src=1), dict(spb=0, src=3), dict(spb=75, src=2), dict(spb=1, n_frames=3)):
        a, b, c = plan(driver, **kw), plan(driver, bank_products=0, **kw), plan(driver, policy=NORMALISED, bank_soft=0, bank_products=0, **kw)
        assert a["status"] == 0 and b["status"] == 0 and c["status"] == 0
        for other in (b, c):
            assert {k: a[k] for k in a if k != "variant"} == {k: other[k] for k in other if k != "variant"}, kw
        assert a["tail"] == 0                                        # a bank round runs its own phase kernel
    p = plan(driver, n_frames=1024)
    assert (p["symbols_per_block"], p["chunks"], p["grid"], p["threads"]) == (19, 4, 4096, 256)


def test_refusals_name_their_reason(driver):
    for kw, text in ((dict(bank_soft=0), "bank_soft"), (dict(bank_soft=0, policy=NORMALISED), "bank_soft"), (dict(bank_soft=0, desc=0), "bank_soft"),
                     (dict(classed=1), "classed"), (dict(fft=1), "fft"), (dict(dqpsk=1), "dqpsk"), (dict(fft=1, dqpsk=1), "fft"),
                     (dict(desc=0), "bank_soft"), (dict(policy=NORMALISED), "bank_soft"),
                     (dict(mode=2), "mode I"), (dict(mode=3), "mode I"), (dict(mode=4), "mode I"), (dict(generic_mode1=1), "mode I"),
                     (dict(level=0.5), "level"), (dict(level=127.5), "level"), (dict(level=float("nan")), "level"),
                     (dict(policy=2), "policy"), (dict(policy=-1), "policy"),
                     (dict(classed=1, fft=1), "class order"), (dict(src=4), "no loader"), (dict(sync=1), "bank round"), (dict(stride=1), "bank round")):
        p = plan(driver, **kw)
        assert p["status"] == INVALID_ARG and text in p["error"], (kw, p)
    for kw in (dict(bank_soft=0), dict(classed=1), dict(fft=1), dict(dqpsk=1)):
        assert "bank_products" in plan(driver, **kw)["error"], kw


def test_without_the_fact_the_pinned_refusal_and_its_text_are_unchanged(driver):
    for kw in (dict(fft=1), dict(dqpsk=1), dict(fft=1, dqpsk=1, src=2)):
        assert plan(driver, bank_products=0, **kw) == {"status": INVALID_ARG, "error": NO_VIEWS}, kw
    p = plan(driver, bank_soft=0, bank_products=0)
    assert p == {"status": INVALID_ARG, "error": "ofdm_demod: the weighted soft bits have no stream-bank loader (frame descriptors)"}


def check_counters(out):
    assert out["failed_checks"] == 0
    parts = ("as_before", "no_bank_soft", "classed", "fft", "dqpsk", "bad_policy", "not_mode1", "bad_level", "products")
    assert out["checked"] == sum(out[k] for k in parts)
    for k in parts + ("as_before_refused", "as_before_views", "as_before_weighted_bank"):
        assert out[k] > 0, (k, out)
    assert all(v > 0 for v in out["variants"]) and len(out["variants"]) == 4 and sum(out["variants"]) == out["products"]


def test_every_combination_follows_the_rules(driver):
    res = subprocess.run([str(driver), "all"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["checked"] == 6 * 6 * 2 ** 13 * 4 * 4 * 2 * 2
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
