"""CPU: the interferer's planner and argument checks (dabgpu_interferer_plan, dabgpu_interferer_bank_* before any device call;
dab-radio_amd/csrc/dabgpu_host_logic.cpp): every refusal and every acceptance at its edge, NULL handles, and the planner fuzzed on its own,
plain and under ASan + UBSan, as a stand-alone program (tests/cpp/interferer_plan_fuzz.cpp)."""
import ctypes as C
import json
import os
import subprocess

import pytest

import interferer_model as IM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
INVALID_ARG = 2
WIDTHS = (0.3, 96000.0 / 2048000.0, 2.0 ** -7, 0.6)             # L = 2, 16, 64, 1


@pytest.fixture(scope="module")
def dabgpu():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu


@pytest.fixture(scope="module")
def shapes(dabgpu):
    return [dabgpu.interferer_design(w) for w in WIDTHS]


def plan(dabgpu, plist, shapes=()):
    return dabgpu.interferer_plan([IM.to_struct(P, dabgpu.InterfererStream) for P in plist], shapes)


def slot(L):
    return 64 * L + 8 * (1024 // L + 18)


def test_acceptances_at_their_edges(dabgpu, shapes):
    assert C.sizeof(dabgpu.InterfererSource) == 56 and C.sizeof(dabgpu.InterfererStream) == 240 and C.sizeof(dabgpu.InterfererShape) == 4160
    assert C.sizeof(IM.Stream) == 240 and C.sizeof(IM.Shape) == 4160
    none = {"block_samples": 1024, "band_slots": 0, "slot_bytes": 0, "lds_bytes": 0}
    assert plan(dabgpu, [IM.stream()]) == none                              # no source at all
    assert plan(dabgpu, [IM.stream([IM.source(IM.TONE, amp=3.0e38), IM.source(IM.BAND, amp=1.0, shape=-1)])], shapes) == none     # tones and white: no LDS
    assert plan(dabgpu, [IM.stream([IM.source(IM.BAND, amp=0.0, shape=1)])], shapes) == none                    # amp = 0 costs nothing
    worst = max(slot(L) for L in (2, 16, 64, 1))
    assert worst == slot(1) == 8400
    assert plan(dabgpu, [IM.stream([IM.source(IM.BAND, amp=1.0, shape=1)])], shapes) == {"block_samples": 1024, "band_slots": 1, "slot_bytes": worst, "lds_bytes": worst}
    assert plan(dabgpu, [IM.stream([IM.source(IM.BAND, amp=1.0, shape=1)])], shapes[:3])["slot_bytes"] == slot(2)
    four = IM.stream([IM.source(IM.BAND, amp=1.0, shape=i) for i in range(4)])
    assert plan(dabgpu, [IM.stream(), four], shapes)["lds_bytes"] == 4 * worst
    edge = IM.source(IM.TONE, amp=0.0, gate_period=(1 << 64) - 1, gate_on=(1 << 64) - 1, gate_offset=(1 << 62) - 1, freq_q64=(1 << 64) - 1)
    assert plan(dabgpu, [IM.stream([edge, dict(edge, gate_offset=-(1 << 62) + 1, gate_on=0), dict(edge, gate_period=0, gate_on=0)], seed=(1 << 64) - 1)]) == none
    off = IM.source(IM.OFF, amp=float("nan"), shape=99, gate_period=1, gate_on=2, gate_offset=1 << 62)
    assert plan(dabgpu, [IM.stream([off])]) == none                          # an OFF source is not read


def test_every_refusal(dabgpu, shapes):
    L = dabgpu.lib()
    nan, inf = float("nan"), float("inf")
    tone = IM.source(IM.TONE, amp=1.0)
    bad = [
        ([], "0 streams"),
        ([IM.stream(), IM.stream([tone, dict(tone, kind=3)])], "stream 1: source 1: kind 3"),
        ([IM.stream([dict(tone, kind=-1)])], "source 0: kind -1"),
        ([IM.stream([dict(tone, amp=nan)])], "amp is not finite"),
        ([IM.stream([dict(tone, amp=inf)])], "amp is not finite"),
        ([IM.stream([dict(tone, amp=-1e-30)])], "amp is negative"),
        ([IM.stream([dict(tone, gate_period=7, gate_on=8)])], "gate_on 8 above gate_period 7"),
        ([IM.stream([dict(tone, gate_period=0, gate_on=1)])], "gate_on 1 above gate_period 0"),
        ([IM.stream([dict(tone, gate_offset=1 << 62)])], "gate_offset"),
        ([IM.stream([dict(tone, gate_offset=-(1 << 62))])], "gate_offset"),
        ([IM.stream([IM.source(IM.BAND, amp=1.0, shape=4)])], "shape 4 of 4"),
        ([IM.stream([IM.source(IM.BAND, amp=1.0, shape=-2)])], "shape -2 of 4"),
    ]
    for plist, text in bad:
        with pytest.raises(dabgpu.DabGpuError) as err:
            plan(dabgpu, plist, shapes)
        assert text in str(err.value), (text, str(err.value))
    with pytest.raises(dabgpu.DabGpuError) as err:
        plan(dabgpu, [IM.stream([IM.source(IM.BAND, amp=1.0, shape=0)])])    # a shape index without a shape
    assert "shape 0 of 0" in str(err.value)
    five = IM.to_struct(IM.stream(), dabgpu.InterfererStream)
    for n, text in ((5, "5 sources"), (-1, "-1 sources")):
        five.n_sources = n
        with pytest.raises(dabgpu.DabGpuError) as err:
            dabgpu.interferer_plan([five])
        assert text in str(err.value)
    one = (dabgpu.InterfererStream * 1)(IM.to_struct(IM.stream([tone]), dabgpu.InterfererStream))
    sh = (dabgpu.InterfererShape * 4)(*shapes)
    assert L.dabgpu_interferer_plan(None, 1, None, 0, None) == INVALID_ARG and b"null parameters" in L.dabgpu_last_error()
    assert L.dabgpu_interferer_plan(one, 1, None, 1, None) == INVALID_ARG and b"null parameters / shapes" in L.dabgpu_last_error()
    assert L.dabgpu_interferer_plan(one, (1 << 20) + 1, None, 0, None) == INVALID_ARG and b"1048577 streams" in L.dabgpu_last_error()
    assert L.dabgpu_interferer_plan(one, 1, sh, 5, None) == INVALID_ARG and b"5 shapes" in L.dabgpu_last_error()
    assert L.dabgpu_interferer_plan(one, 1, sh, -1, None) == INVALID_ARG and b"-1 shapes" in L.dabgpu_last_error()
    assert L.dabgpu_interferer_plan(one, 1, sh, 4, None) == 0 and L.dabgpu_interferer_plan(one, 1, None, 0, None) == 0
    for interp, text in ((0, b"interp 0"), (3, b"interp 3"), (128, b"interp 128")):
        broken = (dabgpu.InterfererShape * 1)(dabgpu.interferer_design(0.3))
        broken[0].interp = interp
        assert L.dabgpu_interferer_plan(one, 1, broken, 1, None) == INVALID_ARG and text in L.dabgpu_last_error()
    broken = (dabgpu.InterfererShape * 1)(dabgpu.interferer_design(0.3))
    broken[0].taps[31] = nan
    assert L.dabgpu_interferer_plan(one, 1, broken, 1, None) == INVALID_ARG and b"tap 31 is not finite" in L.dabgpu_last_error()
    broken[0].taps[31], broken[0].taps[32] = 0.0, nan                        # (the first tap the shape does not use)
    assert L.dabgpu_interferer_plan(one, 1, broken, 1, None) == 0


def test_bank_entry_points_check_before_any_device_call(dabgpu, shapes):
    """no device here: a call that reached one would fail differently (or crash on the fake handles)"""
    L = dabgpu.lib()
    h = C.c_void_p()
    one = (dabgpu.InterfererStream * 1)(IM.to_struct(IM.stream([IM.source(IM.TONE, amp=1.0)]), dabgpu.InterfererStream))
    fake = C.c_void_p(0x1000)
    assert L.dabgpu_interferer_bank_create(None, 1, one, None, 0, C.byref(h)) == INVALID_ARG
    assert L.dabgpu_interferer_bank_create(fake, 1, one, None, 0, None) == INVALID_ARG
    assert L.dabgpu_interferer_bank_create(fake, 0, one, None, 0, C.byref(h)) == INVALID_ARG
    assert L.dabgpu_interferer_bank_create(fake, 1, None, None, 0, C.byref(h)) == INVALID_ARG
    assert L.dabgpu_interferer_bank_create(fake, 1, one, None, 2, C.byref(h)) == INVALID_ARG
    bad = (dabgpu.InterfererStream * 1)(IM.to_struct(IM.stream([IM.source(IM.TONE, amp=-1.0)]), dabgpu.InterfererStream))
    assert L.dabgpu_interferer_bank_create(fake, 1, bad, None, 0, C.byref(h)) == INVALID_ARG and b"interferer_bank_create: stream 0: source 0: amp is negative" in L.dabgpu_last_error()
    assert L.dabgpu_interferer_bank_set_params(None, one, None) == INVALID_ARG
    assert L.dabgpu_interferer_bank_seek(None, 0, None) == INVALID_ARG
    assert L.dabgpu_interferer_bank_seek(fake, 1 << 62, None) == INVALID_ARG and b"2^62" in L.dabgpu_last_error()
    assert L.dabgpu_interferer_bank_apply(None, fake, 0, 1, fake, 10, 0, 1.0, None) == INVALID_ARG and b"null bank" in L.dabgpu_last_error()
    assert L.dabgpu_interferer_bank_apply_host_sync(None, fake, 0, 1, fake, 10, 0, 1.0) == INVALID_ARG
    L.dabgpu_interferer_bank_destroy(None)


def build_fuzzer(tmp_path, sanitize):
    exe = tmp_path / ("interferer_plan_fuzz_san" if sanitize else "interferer_plan_fuzz")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    res = subprocess.run(["g++", "-std=c++17"] + flags + ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                                                          os.path.join(ROOT, "tests", "cpp", "interferer_plan_fuzz.cpp"),
                                                          os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


def check_fuzz_output(res):
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["failed_checks"] == 0
    # both sides of every decision were reached: acceptance and refusal, and of each refusal its low and its high edge
    two_sided = ("n_streams", "n_shapes", "null_lists", "interp", "n_sources", "kind", "gate_on", "gate_offset", "shape_index", "amp_not_finite",
                 "amp_negative", "tap_value")
    keys = ["accepted", "tones_only", "banded", "fits_no", "fits_yes", "apply_ok_a", "apply_ok_b", "apply_no_input", "apply_in_place"]
    keys += [k + e for k in two_sided for e in ("_low", "_high")]
    keys += [k + e for k in ("apply_format", "apply_in_stride", "apply_out_stride", "apply_align", "apply_in_place") for e in ("_a", "_b")]
    keys += ["apply_n_out_a", "apply_null_out_a", "apply_scale_a", "apply_grid_a"]
    assert min(out[k] for k in keys) > 100, {k: out[k] for k in keys if out[k] <= 100}
    assert out["designs_ok"] > 100 and out["designs_refused"] > 100


def test_planner_fuzzed_plain(tmp_path):
    exe = build_fuzzer(tmp_path, False)
    check_fuzz_output(subprocess.run([str(exe), "60000", "1"], capture_output=True, text=True, timeout=600))


def test_planner_fuzzed_under_asan_and_ubsan(tmp_path):
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(p) or not os.path.exists(p):
        pytest.skip("libasan.so is not installed with this gcc")
    exe = build_fuzzer(tmp_path, True)
    for seed in (1, 2):
        check_fuzz_output(subprocess.run([str(exe), "60000", str(seed)], capture_output=True, text=True, timeout=600,
                                         env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")))
