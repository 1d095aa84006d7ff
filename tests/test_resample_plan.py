"""CPU: the resampler's planner and argument checks (dabgpu_resample_plan, dabgpu_resample_step_q62 / _step, dabgpu_resample_input_needed,
dabgpu_resample_bank_* before any device call; dab-radio_amd/csrc/dabgpu_host_logic.cpp): every refusal and every acceptance at its edge,
the step word's round trips, the input span against brute force, and the planner fuzzed on its own under ASan + UBSan
(tests/cpp/resample_plan_fuzz.cpp)."""
import ctypes as C
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import resample_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
INVALID_ARG = 2
ONE = RM.ONE


@pytest.fixture(scope="module")
def dabgpu():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu


def plan(dabgpu, plist, design):
    return dabgpu.resample_plan([RM.to_struct(P, dabgpu.ResampleStream) for P in plist], design)


def test_acceptances_at_their_edges(dabgpu):
    assert C.sizeof(dabgpu.ResampleStream) == 32 and C.sizeof(dabgpu.ResampleFilter) == 48 + 257 * 48 * 4
    assert (dabgpu.RESAMPLE_PHASES, dabgpu.RESAMPLE_TAPS, dabgpu.RESAMPLE_BLOCK) == (RM.L, RM.TAPS, RM.BLOCK)
    two, one = dabgpu.resample_design(2.0), dabgpu.resample_design(1.0)
    assert two.error <= 1e-4 and one.error <= 1e-4 and one.passband_cycles == 0.375
    # identity streams stage no rows; the window is ceil(1024 step) + taps + 2
    assert plan(dabgpu, [RM.params_dict()], one) == {"block_samples": 1024, "window_samples": 1024 + 50, "table_rows": 0, "lds_bytes": 1074 * 8}
    assert plan(dabgpu, [RM.params_dict(ONE, 0, 1)], one) == {"block_samples": 1024, "window_samples": 1074, "table_rows": 5, "lds_bytes": 1074 * 8 + 5 * 49 * 4}
    assert plan(dabgpu, [RM.params_dict(ONE << 1, 1 << 62, ONE - 1, gain=-3e38), RM.params_dict(ONE >> 1, -(1 << 62), 0)], two) == \
        {"block_samples": 1024, "window_samples": 2048 + 50, "table_rows": 257, "lds_bytes": 2098 * 8 + 257 * 49 * 4}
    assert plan(dabgpu, [RM.params_dict(ONE >> 1)], one)["window_samples"] == 512 + 50
    assert plan(dabgpu, [RM.params_dict(ONE + 1)], two)["window_samples"] == 1025 + 50            # ceil
    # 20 ppm: a block moves 1023 * 2e-5 * 256 = 5.2 rows -> 5 + 5; the window is odd, LDS holds the next even count
    g = plan(dabgpu, [RM.params_dict(RM.step_q62(1.0, 1.0, 20.0))], two)
    assert g == {"block_samples": 1024, "window_samples": 1075, "table_rows": 10, "lds_bytes": 1076 * 8 + 10 * 49 * 4}
    assert plan(dabgpu, [RM.params_dict(RM.step_q62(1.0, 1.0, -20.0))], two)["table_rows"] == 10
    assert plan(dabgpu, [RM.params_dict(RM.step_q62(2.4e6, 2.048e6))], two)["table_rows"] == 257
    # a design serves steps up to its max_step, rounded up to Q2.62
    d12 = dabgpu.resample_design(2.4 / 2.048)
    assert plan(dabgpu, [RM.params_dict(RM.step_q62(2.4e6, 2.048e6))], d12)["window_samples"] == 1200 + 50


def test_every_refusal(dabgpu):
    L = dabgpu.lib()
    nan, inf = float("nan"), float("inf")
    two, one = dabgpu.resample_design(2.0), dabgpu.resample_design(1.0)
    bad = [
        ([], two, "0 streams"),
        ([RM.params_dict(), RM.params_dict((ONE << 1) + 1)], two, "stream 1: step"),
        ([RM.params_dict((ONE >> 1) - 1)], two, "stream 0: step"),
        ([RM.params_dict(ONE + 1)], one, "above the design's max_step"),
        ([RM.params_dict(gain=nan)], two, "gain is not finite"),
        ([RM.params_dict(gain=-inf)], two, "gain is not finite"),
        ([RM.params_dict(ONE, (1 << 62) + 1)], two, "offset_samples outside"),
        ([RM.params_dict(ONE, -(1 << 62) - 1)], two, "offset_samples outside"),
        ([RM.params_dict(ONE, 0, ONE)], two, "offset_frac_q62"),
    ]
    for plist, design, text in bad:
        with pytest.raises(dabgpu.DabGpuError) as err:
            plan(dabgpu, plist, design)
        assert text in str(err.value), (text, str(err.value))
    with pytest.raises(dabgpu.DabGpuError) as err:
        plan(dabgpu, [RM.params_dict()], None)
    assert "null design" in str(err.value)
    one_stream = (dabgpu.ResampleStream * 1)(RM.to_struct(RM.params_dict(), dabgpu.ResampleStream))
    assert L.dabgpu_resample_plan(None, 1, C.byref(two), None) == INVALID_ARG and b"null parameters" in L.dabgpu_last_error()
    assert L.dabgpu_resample_plan(one_stream, (1 << 20) + 1, C.byref(two), None) == INVALID_ARG and b"1048577 streams" in L.dabgpu_last_error()
    assert L.dabgpu_resample_plan(one_stream, 1, C.byref(two), None) == 0
    for ms, pb in ((0.4999, 0.0), (2.0001, 0.0), (nan, 0.0), (1.0, 0.4501), (1.0, -0.1), (1.0, nan)):
        with pytest.raises(dabgpu.DabGpuError):
            dabgpu.resample_design(ms, pb)
    broken = dabgpu.resample_design(1.0)
    broken.max_step = 3.0
    with pytest.raises(dabgpu.DabGpuError) as err:
        plan(dabgpu, [RM.params_dict()], broken)
    assert "max_step" in str(err.value)


def test_bank_entry_points_check_before_any_device_call(dabgpu):
    """no device here: a call that reached one would fail differently (or crash on the fake handles)"""
    L = dabgpu.lib()
    h = C.c_void_p()
    two = dabgpu.resample_design(2.0)
    one = (dabgpu.ResampleStream * 1)(RM.to_struct(RM.params_dict(), dabgpu.ResampleStream))
    fake = C.c_void_p(0x1000)
    assert L.dabgpu_resample_bank_create(None, 1, one, C.byref(two), C.byref(h)) == INVALID_ARG
    assert L.dabgpu_resample_bank_create(fake, 1, one, C.byref(two), None) == INVALID_ARG
    assert L.dabgpu_resample_bank_create(fake, 1, one, None, C.byref(h)) == INVALID_ARG and b"null design" in L.dabgpu_last_error()
    assert L.dabgpu_resample_bank_create(fake, 0, one, C.byref(two), C.byref(h)) == INVALID_ARG
    assert L.dabgpu_resample_bank_create(fake, 1, None, C.byref(two), C.byref(h)) == INVALID_ARG
    bad = (dabgpu.ResampleStream * 1)(RM.to_struct(RM.params_dict(gain=float("nan")), dabgpu.ResampleStream))
    assert L.dabgpu_resample_bank_create(fake, 1, bad, C.byref(two), C.byref(h)) == INVALID_ARG and b"gain" in L.dabgpu_last_error()
    assert L.dabgpu_resample_bank_set_params(None, one, None) == INVALID_ARG
    assert L.dabgpu_resample_bank_seek(None, 0, None) == INVALID_ARG
    assert L.dabgpu_resample_bank_seek(fake, (1 << 62) + 1, None) == INVALID_ARG and b"2^62" in L.dabgpu_last_error()
    assert L.dabgpu_resample_bank_apply(None, fake, 0, 1, 0, 1, fake, 10, 0, 1.0, None) == INVALID_ARG and b"null bank" in L.dabgpu_last_error()
    assert L.dabgpu_resample_bank_apply_host_sync(None, fake, 0, 1, 0, 1, fake, 10, 0, 1.0) == INVALID_ARG
    L.dabgpu_resample_bank_destroy(None)


def test_step_word_round_trips(dabgpu):
    L = dabgpu.lib()
    q, back = L.dabgpu_resample_step_q62, L.dabgpu_resample_step
    assert q(2.048e6, 2.048e6, 0.0) == ONE and q(1.0, 2.0, 0.0) == ONE >> 1 and q(4.096e6, 2.048e6, 0.0) == ONE << 1
    assert back(ONE) == 1.0 and back(ONE >> 1) == 0.5 and back(ONE << 1) == 2.0 and back(ONE + (1 << 10)) == 1.0 + 2.0 ** -52
    for bad in ((float("nan"), 1.0, 0.0), (1.0, float("nan"), 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 1.0, 0.0), (1.0, 1.0, float("inf")),
                (4.0, 1.0, 0.0), (1.0, 1.0, -1e6)):
        assert q(*bad) == 0
    # rates whose ratio no binary fraction holds, ppm of both signs: within 2^-52 relative of the exact rational (the product is taken in
    # double: two roundings), and back to a double within one more
    rng = np.random.default_rng(9500)
    cases = [(2.4e6, 2.048e6, 0.0), (2.048e6, 2.4e6, 0.0), (2.56e6, 2.048e6, 0.0), (3.072e6, 2.048e6, 0.0), (2.048e6, 2.048e6, 20.0),
             (2.048e6, 2.048e6, -20.0), (2.4e6, 2.048e6, 100.0), (2.4e6, 2.048e6, -100.0), (1.0, 3.0, 0.0), (2.0, 3.0, 1.0)]
    cases += [(float(a), float(b), float(p)) for a, b, p in zip(rng.integers(1000000, 4000000, 500), rng.integers(2000000, 2100000, 500), rng.uniform(-300, 300, 500))]
    for a, b, ppm in cases:
        exact = Fraction(a) / Fraction(b) * (1 + Fraction(ppm) / 1000000)
        if not Fraction(1, 2) <= exact <= 2:
            continue
        w = q(a, b, ppm)
        assert abs(Fraction(w, ONE) - exact) <= exact * Fraction(3, 1 << 53) + Fraction(1, ONE), (a, b, ppm)
        assert abs(back(w) - float(exact)) <= 4 * 2.0 ** -53 * float(exact)
        assert w == RM.step_q62(a, b, ppm)
    assert q(2.048e6, 2.048e6, 20.0) > ONE > q(2.048e6, 2.048e6, -20.0)
    assert q(2.048e6, 2.048e6, 20.0) - ONE == pytest.approx(20e-6 * ONE, rel=1e-9)


def test_input_needed_against_brute_force(dabgpu):
    rng = np.random.default_rng(9600)
    cases = [(RM.params_dict(), 0, 1), (RM.params_dict(), 5, 1000), (RM.params_dict(ONE, 0, 1), 0, 1), (RM.params_dict(ONE << 1, -77, ONE - 1), 1 << 40, 2049),
             (RM.params_dict(ONE >> 1, 1 << 62, 0), (1 << 62), 4), (RM.params_dict(ONE, -(1 << 62), 0), 0, 3), (RM.params_dict(ONE + 5, 9, 9), 123, 0)]
    for _ in range(300):
        P = RM.params_dict(int(rng.integers(ONE >> 1, (ONE << 1) + 1, dtype=np.uint64)), int(rng.integers(-(1 << 40), 1 << 40)), int(rng.integers(0, ONE)))
        cases.append((P, int(rng.integers(0, 1 << 45)), int(rng.integers(1, 3000))))
    for P, pos, n_out in cases:
        first, count = dabgpu.resample_input_needed(RM.to_struct(P, dabgpu.ResampleStream), pos, n_out)
        if n_out == 0:
            assert count == 0
            continue
        before, after = (0, 0) if RM.is_identity(P) else (RM.TAPS // 2 - 1, RM.TAPS // 2)
        idx = [RM.time_of(P, pos + i)[0] for i in range(n_out)]                         # every output's index: brute force
        assert first == min(idx) - before and first + count - 1 == max(idx) + after, (P, pos, n_out)
    S = RM.to_struct(RM.params_dict(ONE << 1, 1 << 62, 0), dabgpu.ResampleStream)
    with pytest.raises(dabgpu.DabGpuError) as err:                                       # the span's end does not fit the signed result
        dabgpu.resample_input_needed(S, 1 << 62, 10)
    assert "2^63" in str(err.value)
    with pytest.raises(dabgpu.DabGpuError):
        dabgpu.resample_input_needed(S, (1 << 62) + 1, 10)
    L = dabgpu.lib()
    assert L.dabgpu_resample_input_needed(None, 0, 1, C.byref(C.c_int64()), C.byref(C.c_uint64())) == INVALID_ARG
    assert L.dabgpu_resample_input_needed(C.byref(S), 0, 1, None, C.byref(C.c_uint64())) == INVALID_ARG


def test_planner_fuzzed_under_asan_and_ubsan(tmp_path):
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(p) or not os.path.exists(p):
        pytest.skip("libasan.so is not installed with this gcc")
    exe = tmp_path / "resample_plan_fuzz"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "resample_plan_fuzz.cpp"),
                          os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    for seed in (1, 2):
        res = subprocess.run([str(exe), "40000", str(seed)], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
        assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
        out = json.loads(res.stdout.strip().splitlines()[-1])
        assert out["failed_checks"] == 0
        # both sides of every decision were reached: acceptance and refusal, and of each refusal its low and its high edge
        keys = ["accepted", "whole_table", "narrow", "fits_no", "fits_yes", "spans", "times"]
        keys += [k + e for k in ("n_streams", "step", "above_design", "gain", "offset", "frac", "null_params", "null_design") for e in ("_low", "_high")]
        assert min(out[k] for k in keys) > 100, {k: out[k] for k in keys if out[k] <= 100}
        assert out["round_trips"] == out["iterations"]
