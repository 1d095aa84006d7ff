"""CPU: the planners of the symbol noise profile and of the symbol-weighted combiner (dabgpu_sym_profile_plan,
dabgpu_diversity_plan_symbols, dab-radio_amd/csrc/dabgpu_host_logic.cpp): every refusal by its reason, the edges of n_frames and
alignment, the geometry.  tests/cpp/sym_profile_plan_fuzz.cpp restates the rules and fuzzes them, and runs the host form, under ASan +
UBSan as a program of its own."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
INVALID_ARG = 2
LDS = 3600 + 900 + 12
DIVERSITY_LDS, DIVERSITY_TABLED_LDS = 6144, 6144 + 64


def build_driver(out_dir, flags=()):
    exe = out_dir / "sym_profile_plan_fuzz"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          os.path.join(ROOT, "tests", "cpp", "sym_profile_plan_fuzz.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("sym_profile_plan"))


def run_json(exe, args):
    res = subprocess.run([str(exe)] + [a if isinstance(a, str) else str(int(a)) for a in args], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout)


def plan(exe, mode=1, dq=0x1000000, n_frames=3, sync=0, weight=0x50000, noise=0, ref=0, valid=0, null_out=0):
    return run_json(exe, ["plan", mode, dq, n_frames, sync, weight, noise, ref, valid, null_out])


def dplan(exe, n_branches=2, n_frames=3, bits=0x700000, stride=0, layout=0, spb=0, dq=0x100000, scale=0x200000, weight=0, sync=0, band=0, sym=0x600000,
          tables=2):
    return run_json(exe, ["dplan", n_branches, n_frames, bits, stride, layout, spb, dq, scale, weight, sync, band, sym, tables])


def test_geometry(driver):
    assert plan(driver) == dict(status=0, error="", grid=3, threads=256, lds_bytes=LDS)
    assert plan(driver, n_frames=1)["grid"] == 1 and plan(driver, n_frames=1 << 24)["grid"] == 1 << 24
    base = plan(driver, n_frames=67)
    for kw in (dict(sync=0x60000), dict(noise=0x90004, ref=0x98004, valid=0xA0004), dict(dq=0x1000010), dict(weight=0x50004)):
        assert plan(driver, n_frames=67, **kw) == base, kw
    import dabgpu
    g = dabgpu.sym_profile_plan(0x1000000, 5, symbol_weight=0x50000)
    assert (g.grid, g.threads, g.lds_bytes) == (5, 256, LDS)
    with pytest.raises(dabgpu.DabGpuError, match="16-byte"):
        dabgpu.sym_profile_plan(0x1000008, 5, symbol_weight=0x50000)
    with pytest.raises(dabgpu.DabGpuError, match="mode"):
        dabgpu.sym_profile_plan(0x1000000, 5, symbol_weight=0x50000, mode=2)


def test_refusals_name_their_reason(driver):
    for kw, text in ((dict(mode=0), "mode"), (dict(mode=2), "mode"), (dict(mode=3), "mode"), (dict(mode=4), "mode"), (dict(mode=-1), "mode"),
                     (dict(n_frames=0), "n_frames"), (dict(n_frames=(1 << 24) + 1), "n_frames"),
                     (dict(dq=0), "null products"), (dict(dq=0x1000008), "16-byte"), (dict(dq=0x1000004), "16-byte"), (dict(dq=0x1000001), "16-byte"),
                     (dict(sync=0x60002), "4-byte"), (dict(weight=0x50001), "4-byte"), (dict(noise=0x90002), "4-byte"), (dict(ref=0x98003), "4-byte"),
                     (dict(valid=0xA0002), "4-byte"),
                     (dict(weight=0), "no output"), (dict(weight=0, sync=0x60000), "no output"),
                     (dict(null_out=1), "null result")):
        p = plan(driver, **kw)
        assert p["status"] == INVALID_ARG and text in p["error"], (kw, p)
        if not kw.get("null_out"):
            assert p["grid"] == 0 and p["threads"] == 0 and p["lds_bytes"] == 0                 # a refusal leaves no geometry behind
    # the edges on the accepting side; every output alone is an output
    for kw in (dict(n_frames=1 << 24), dict(dq=0x1000010), dict(weight=0, noise=0x80000), dict(weight=0, ref=0x80000), dict(weight=0, valid=0x80000)):
        assert plan(driver, **kw)["status"] == 0, kw


def test_combiner_planner(driver):
    base = dplan(driver)
    assert base["status"] == 0 and base["threads"] == 256 and base["lds_bytes"] == DIVERSITY_TABLED_LDS and base["grid"] == 3 * base["runs_per_frame"]
    # no symbol table at all: the banded planner's answer, and without a band table the scalar one's
    assert dplan(driver, tables=0)["lds_bytes"] == DIVERSITY_LDS and dplan(driver, sym=0)["lds_bytes"] == DIVERSITY_LDS
    assert dplan(driver, tables=1, band=0x500000)["lds_bytes"] == DIVERSITY_TABLED_LDS
    assert dplan(driver, tables=3, band=0x500000)["lds_bytes"] == DIVERSITY_TABLED_LDS
    assert dplan(driver, tables=3, band=0, weight=0x300000)["status"] == 0               # a scalar weight beside a symbol table is fine
    for spb, runs in ((1, 75), (5, 15), (75, 1)):
        g = dplan(driver, spb=spb, n_frames=67)
        assert (g["symbols_per_block"], g["runs_per_frame"], g["grid"]) == (spb, runs, 67 * runs)
    for kw, text in ((dict(n_branches=0), "n_branches"), (dict(n_branches=9), "n_branches"), (dict(n_frames=(1 << 24) + 1), "n_frames"),
                     (dict(layout=2), "bits_layout"), (dict(spb=76), "symbols_per_block"), (dict(spb=-1), "symbols_per_block"),
                     (dict(stride=230384), "bits_frame_stride"), (dict(stride=230408), "bits_frame_stride"),
                     (dict(bits=0), "d_bits"), (dict(bits=0x700008), "d_bits"), (dict(dq=0), "no products"), (dict(scale=0), "no products"),
                     (dict(dq=0x100008), "d_dqpsk"), (dict(scale=0x200002), "4-byte"), (dict(weight=0x300001), "4-byte"), (dict(sync=0x400002), "4-byte"),
                     (dict(tables=3, band=0x500002), "band weights"), (dict(tables=3, band=0x500000, weight=0x300000), "both a band table"),
                     (dict(sym=0x600002), "symbol weights"), (dict(sym=0x600001), "symbol weights"), (dict(tables=3, band=0x500000, sym=0x600003), "symbol weights")):
        p = dplan(driver, **kw)
        assert p["status"] == INVALID_ARG and text in p["error"], (kw, p)
        assert p["grid"] == 0 and p["threads"] == 0 and p["lds_bytes"] == 0
    import dabgpu
    g = dabgpu.diversity_plan_symbols([(0x100000, 0x200000)], 4, 0x700000, None, [0x600000])
    assert (g.threads, g.lds_bytes) == (256, DIVERSITY_TABLED_LDS)
    assert dabgpu.diversity_plan_symbols([(0x100000, 0x200000)], 4, 0x700000, None, None).lds_bytes == DIVERSITY_LDS
    with pytest.raises(dabgpu.DabGpuError, match="symbol weights"):
        dabgpu.diversity_plan_symbols([(0x100000, 0x200000)], 4, 0x700000, None, [0x600002])
    with pytest.raises(ValueError, match="symbol_weights"):
        dabgpu.diversity_plan_symbols([(0x100000, 0x200000)], 4, 0x700000, None, [0x600000, None])


def check_counters(out):
    assert out["failed_checks"] == 0 and out["checked"] == out["accepted"] + out["refused"] == out["combiner_accepted"] + out["combiner_refused"]
    assert out["accepted"] > 0 and all(r > 0 for r in out["reasons"]) and len(out["reasons"]) == 6, out
    assert out["combiner_accepted"] > 0 and all(r > 0 for r in out["combiner_reasons"]) and len(out["combiner_reasons"]) == 12, out


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
    assert plan(exe)["status"] == 0 and dplan(exe)["status"] == 0
