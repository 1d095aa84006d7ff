"""CPU: the planners of the noise profile and of the banded combiner (dabgpu_noise_profile_plan, dabgpu_diversity_plan_banded,
dab-radio_amd/csrc/dabgpu_host_logic.cpp): every refusal by its reason, the edges of stride, offset, alpha and the state's overlap, the
geometry.  tests/cpp/noise_profile_plan_fuzz.cpp restates the rules and fuzzes them, and runs the host forms, under ASan + UBSan as a
program of its own."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
INVALID_ARG = 2
NULL = 2656
LDS = 18432 + 8192 + 8


def build_driver(out_dir, flags=()):
    exe = out_dir / "noise_profile_plan_fuzz"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          os.path.join(ROOT, "tests", "cpp", "noise_profile_plan_fuzz.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("noise_profile_plan"))


def plan(exe, mode=1, iq=0x10000, n_frames=3, stride=200000, off=700, alpha=0.25, states=0, freq=0, exclude=0, pin=0, pout=0, weight=0x50000, mean=0,
         power=0, valid=0, null_out=0):
    args = [mode, iq, n_frames, stride, off, repr(float(alpha)), states, freq, exclude, pin, pout, weight, mean, power, valid, null_out]
    res = subprocess.run([str(exe), "plan"] + [a if isinstance(a, str) else str(int(a)) for a in args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout)


def banded(exe, n=2, n_frames=3, bits=0x100000, stride=0, layout=0, spb=0, dqpsk0=0x2000000, scale0=0x300000, weight0=0, band0=0x400000, band1=0x500000,
           null_bands=0):
    args = [n, n_frames, bits, stride, layout, spb, dqpsk0, scale0, weight0, band0, band1, null_bands]
    res = subprocess.run([str(exe), "banded"] + [str(int(a)) for a in args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout)


def test_geometry(driver):
    assert plan(driver) == dict(status=0, error="", grid=3, threads=256, lds_bytes=LDS)
    assert plan(driver, n_frames=1)["grid"] == 1 and plan(driver, n_frames=1 << 24)["grid"] == 1 << 24
    base = plan(driver, n_frames=65)
    for kw in (dict(states=0x60000), dict(freq=0x70000), dict(exclude=0x71000), dict(pin=0x800000, pout=0x800000), dict(pin=0x800000, pout=0x900000),
               dict(mean=0x80100, power=0x90000, valid=0xA0000), dict(iq=0x10008), dict(off=0), dict(stride=1 << 40), dict(alpha=1.0)):
        assert plan(driver, n_frames=65, **kw) == base, kw
    import dabgpu
    g = dabgpu.noise_profile_plan(0x10000, 5, 200000, 700, band_weight=0x50000)
    assert (g.grid, g.threads, g.lds_bytes) == (5, 256, LDS)
    with pytest.raises(dabgpu.DabGpuError, match="alpha"):
        dabgpu.noise_profile_plan(0x10000, 5, 200000, 700, band_weight=0x50000, alpha=0.0)


def test_refusals_name_their_reason(driver):
    state = 3 * 512
    for kw, text in ((dict(mode=0), "mode"), (dict(mode=2), "mode"), (dict(mode=3), "mode"), (dict(mode=4), "mode"), (dict(mode=-1), "mode"),
                     (dict(n_frames=0), "n_frames"), (dict(n_frames=(1 << 24) + 1), "n_frames"),
                     (dict(iq=0), "null samples"), (dict(iq=0x10004), "8-byte"), (dict(iq=0x10001), "8-byte"),
                     (dict(states=0x60002), "4-byte"), (dict(freq=0x70001), "4-byte"), (dict(exclude=0x71002), "4-byte"), (dict(pin=0x800003), "4-byte"),
                     (dict(pout=0x900001), "4-byte"), (dict(weight=0x50001), "4-byte"), (dict(mean=0x80202), "4-byte"), (dict(power=0x90001), "4-byte"),
                     (dict(valid=0xA0002), "4-byte"),
                     (dict(stride=700 + NULL - 1), "stream_stride_samples"), (dict(stride=0), "stream_stride_samples"),
                     (dict(states=0x60000, stride=700 + NULL + 1542), "stream_stride_samples"),
                     (dict(stride=(1 << 40) + 1), "stream_stride_samples"), (dict(off=(1 << 40) + 1, stride=1 << 40), "stream_stride_samples"),
                     (dict(alpha=0.0), "alpha"), (dict(alpha=-0.25), "alpha"), (dict(alpha=1.0000001), "alpha"), (dict(alpha=float("nan")), "alpha"),
                     (dict(alpha=float("inf")), "alpha"),
                     (dict(pin=0x800000, pout=0x800004), "overlap"), (dict(pin=0x800000, pout=0x800000 + state - 4), "overlap"),
                     (dict(pin=0x800000 + state - 4, pout=0x800000), "overlap"),
                     (dict(weight=0), "no output"), (dict(weight=0, pin=0x800000, exclude=0x71000), "no output"), (dict(null_out=1), "null result")):
        p = plan(driver, **kw)
        assert p["status"] == INVALID_ARG and text in p["error"], (kw, p)
        if not kw.get("null_out"):
            assert p["grid"] == 0 and p["threads"] == 0 and p["lds_bytes"] == 0                 # a refusal leaves no geometry behind
    # the edges on the accepting side; every output alone is an output
    for kw in (dict(stride=700 + NULL), dict(states=0x60000, stride=700 + NULL + 1543), dict(off=0, stride=NULL), dict(n_frames=1 << 24),
               dict(off=(1 << 40) - NULL, stride=1 << 40), dict(iq=0x10008), dict(alpha=1.0), dict(alpha=1e-30),
               dict(pin=0x800000, pout=0x800000), dict(pin=0x800000, pout=0x800000 + state), dict(pin=0x800000 + state, pout=0x800000),
               dict(weight=0, pout=0x80000), dict(weight=0, mean=0x80000), dict(weight=0, power=0x80000), dict(weight=0, valid=0x80000)):
        assert plan(driver, **kw)["status"] == 0, kw


def test_banded_planner(driver):
    ok = banded(driver)
    assert ok == dict(status=0, error="", symbols_per_block=ok["symbols_per_block"], runs_per_frame=ok["runs_per_frame"],
                      grid=3 * ok["runs_per_frame"], threads=256, lds_bytes=6144 + 64)
    plain = banded(driver, null_bands=1)
    assert plain["status"] == 0 and plain["lds_bytes"] == 6144 and plain["grid"] == ok["grid"]
    assert banded(driver, band0=0, band1=0)["lds_bytes"] == 6144                               # an array of NULLs: the scalar call
    assert banded(driver, band0=0)["lds_bytes"] == 6144 + 64 and banded(driver, n=1, band0=0)["lds_bytes"] == 6144
    assert banded(driver, weight0=0x600000, band0=0)["status"] == 0                           # a scalar weight beside another branch's table
    assert banded(driver, weight0=0x600000, null_bands=1)["status"] == 0
    assert banded(driver, n=8, n_frames=1024)["grid"] == 3072
    for kw, text in ((dict(weight0=0x600000), "both a band table and d_weight"), (dict(band0=0x400002), "band weights must be 4-byte"),
                     (dict(band1=0x500001), "band weights must be 4-byte"),
                     (dict(n=0), "n_branches"), (dict(n=9), "n_branches"), (dict(n_frames=(1 << 24) + 1), "n_frames"), (dict(layout=2), "bits_layout"),
                     (dict(spb=76), "symbols_per_block"), (dict(spb=-1), "symbols_per_block"), (dict(stride=230384), "bits_frame_stride"),
                     (dict(stride=230408), "bits_frame_stride"), (dict(bits=0), "d_bits"), (dict(bits=0x100008), "d_bits"),
                     (dict(dqpsk0=0), "no products or no scales"), (dict(scale0=0), "no products or no scales"), (dict(dqpsk0=0x2000008), "16-byte"),
                     (dict(scale0=0x300002), "4-byte"), (dict(weight0=0x600001, band0=0), "4-byte")):
        p = banded(driver, **kw)
        assert p["status"] == INVALID_ARG and text in p["error"], (kw, p)
        assert p["grid"] == 0 and p["threads"] == 0 and p["lds_bytes"] == 0 and p["symbols_per_block"] == 0


def check_counters(out):
    assert out["failed_checks"] == 0 and out["checked"] == out["accepted"] + out["refused"] == out["banded_accepted"] + out["banded_refused"]
    assert out["accepted"] > 0 and all(r > 0 for r in out["reasons"]) and len(out["reasons"]) == 9, out
    assert out["banded_accepted"] > 0 and all(r > 0 for r in out["banded_reasons"]) and len(out["banded_reasons"]) == 11, out


def test_rules_fuzzed(driver):
    res = subprocess.run([str(driver), "fuzz", "200000", "7"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    check_counters(json.loads(res.stdout.strip().splitlines()[-1]))
    res = subprocess.run([str(driver), "bands"], capture_output=True, text=True, timeout=600)
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
    res = subprocess.run([str(exe), "bands"], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    assert plan(exe)["status"] == 0 and banded(exe)["status"] == 0
