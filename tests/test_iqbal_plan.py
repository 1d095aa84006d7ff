"""CPU: the IQ balance planner, host helpers and argument checks (dabgpu_iqbal_plan, dabgpu_iqbal_impairment, dabgpu_iqbal_forget,
dabgpu_iqbal_solve_host, dabgpu_iqbal_bank_* before any device call; dab-radio_amd/csrc/dabgpu_host_logic.cpp): every refusal and every
acceptance at its edge, NULL handles, and planner and solve fuzzed on their own, plain and under ASan + UBSan, as a stand-alone program
(tests/cpp/iqbal_plan_fuzz.cpp)."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import iqbal_model as IM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
INVALID_ARG = 2


@pytest.fixture(scope="module")
def dabgpu():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu


def plan(dabgpu, plist, max_call=196608):
    return dabgpu.iqbal_plan([IM.to_struct(P, dabgpu.IqBalanceStream) for P in plist], max_call)


def test_defaults_layouts_and_acceptances_at_their_edges(dabgpu):
    assert C.sizeof(dabgpu.IqBalanceStream) == 40 and C.sizeof(IM.Stream) == 40 and C.sizeof(dabgpu.IqBalanceGeometry) == 16
    assert np.dtype(dabgpu.IQBAL_RECORD_DTYPE).itemsize == 104 and np.dtype(dabgpu.IQBAL_RECORD_DTYPE) == IM.RECORD_DTYPE
    P = dabgpu.iqbal_stream()
    assert (P.mode, P.a_re, P.a_im, P.b_re, P.b_im, P.c_re, P.c_im, P.min_weight) == (IM.TRACK, 1, 0, 0, 0, 0, 0, 65536)
    assert np.float32(P.forget) == np.float32(IM.DEFAULTS["forget"]) == np.float32(math.exp(-1024 / (16 * 196608)))
    assert dabgpu.iqbal_plan([P], 196608) == {"tile_samples": 1024, "tiles_per_call": 192, "scratch_bytes": 192 * 32}
    assert plan(dabgpu, [IM.params()] * 7, 1024) == {"tile_samples": 1024, "tiles_per_call": 1, "scratch_bytes": 7 * 32}
    assert plan(dabgpu, [IM.params(mode=IM.OFF), IM.params(mode=IM.FIXED, a=-3 + 2j, b=1e30j, c=-1e-30)], 1 << 31)["tiles_per_call"] == 1 << 21
    assert plan(dabgpu, [IM.params(forget=1.0, min_weight=1024.0), IM.params(forget=1e-45, min_weight=3e38)])["tiles_per_call"] == 192
    Q = dabgpu.iqbal_stream(mode=IM.FIXED, a=1 + 2j, b=3 - 4j, c=-5j, forget=0.5, min_weight=2048)
    assert (Q.mode, Q.a_re, Q.a_im, Q.b_re, Q.b_im, Q.c_re, Q.c_im, Q.forget, Q.min_weight) == (IM.FIXED, 1, 2, 3, -4, 0, -5, 0.5, 2048)


def test_every_refusal_of_the_planner(dabgpu):
    L = dabgpu.lib()
    nan, inf = float("nan"), float("inf")
    bad = [
        ([], 1024, "0 streams"),
        ([IM.params(), IM.params(mode=3)], 1024, "stream 1: mode 3"),
        ([IM.params(mode=-1)], 1024, "stream 0: mode -1"),
        ([IM.params(a=complex(nan, 0))], 1024, "a_re is not finite"),
        ([IM.params(a=complex(0, inf))], 1024, "a_im is not finite"),
        ([IM.params(b=complex(-inf, 0))], 1024, "b_re is not finite"),
        ([IM.params(b=complex(0, nan))], 1024, "b_im is not finite"),
        ([IM.params(mode=IM.OFF, c=complex(nan, 0))], 1024, "c_re is not finite"),      # an OFF stream is checked all the same
        ([IM.params(c=complex(0, inf))], 1024, "c_im is not finite"),
        ([IM.params(forget=0.0)], 1024, "forget 0 "),
        ([IM.params(forget=-0.5)], 1024, "forget -0.5"),
        ([IM.params(forget=1.0000001)], 1024, "forget 1"),
        ([IM.params(forget=nan)], 1024, "forget nan"),
        ([IM.params(min_weight=1023.0)], 1024, "min_weight 1023"),
        ([IM.params(min_weight=inf)], 1024, "min_weight inf"),
        ([IM.params(min_weight=nan)], 1024, "min_weight nan"),
        ([IM.params()], 0, "max_samples_per_call = 0"),
        ([IM.params()], 1023, "max_samples_per_call = 1023"),
        ([IM.params()], 1025, "max_samples_per_call = 1025"),
        ([IM.params()], (1 << 31) + 1024, "max_samples_per_call"),
    ]
    for plist, max_call, text in bad:
        with pytest.raises(dabgpu.DabGpuError) as err:
            plan(dabgpu, plist, max_call)
        assert text in str(err.value), (text, str(err.value))
    one = (dabgpu.IqBalanceStream * 1)(dabgpu.iqbal_stream())
    assert L.dabgpu_iqbal_plan(None, 1, 1024, None) == INVALID_ARG and b"null parameters" in L.dabgpu_last_error()
    assert L.dabgpu_iqbal_plan(one, (1 << 20) + 1, 1024, None) == INVALID_ARG and b"1048577 streams" in L.dabgpu_last_error()
    many = (dabgpu.IqBalanceStream * 2048)(*([dabgpu.iqbal_stream()] * 2048))
    assert L.dabgpu_iqbal_plan(many, 2048, 1 << 31, None) == INVALID_ARG and b"too large for one call" in L.dabgpu_last_error()
    assert L.dabgpu_iqbal_plan(one, 1, 1024, None) == 0


def test_impairment_forget_and_solve_host(dabgpu):
    L = dabgpu.lib()
    S = dabgpu.iqbal_impairment(0.0, 0.0)
    assert (S.mode, S.a_re, S.a_im, S.b_re, S.b_im, S.c_re, S.c_im) == (IM.FIXED, 1, 0, 0, 0, 0, 0)          # a perfect front end
    S = dabgpu.iqbal_impairment(0.42, 3.0, 0.3 + 0.2j)
    K1, K2 = IM.front_end(0.42, 3.0)
    assert abs(IM.irr_db(K1, K2) - 28.96) < 0.01                                # the issue's raw rejection
    assert np.float32(S.a_re) == np.float32(K1.real) and np.float32(S.b_im) == np.float32(K2.imag) and np.float32(S.c_re) == np.float32(0.3)
    for g, p in ((20.0, 45.0), (-20.0, -45.0)):
        assert dabgpu.iqbal_impairment(g, p).mode == IM.FIXED
    for args, text in (((20.001, 0), "gain_db"), ((-21, 0), "gain_db"), ((float("nan"), 0), "gain_db"), ((0, 45.5), "phase_deg"),
                       ((0, float("inf")), "phase_deg"), ((0, 0, complex(float("nan"), 0)), "DC"), ((0, 0, complex(0, 1e39)), "DC")):
        with pytest.raises(dabgpu.DabGpuError) as err:
            dabgpu.iqbal_impairment(*args)
        assert text in str(err.value)
    assert L.dabgpu_iqbal_impairment(0.0, 0.0, 0.0, 0.0, None) == INVALID_ARG
    f = dabgpu.iqbal_forget
    assert f(1024) == float(np.float32(math.exp(-1))) and f(1023.9) == 0.0 and f(0) == 0.0 and f(-5) == 0.0 and f(float("nan")) == 0.0
    assert f(float("inf")) == 1.0 and f(196608) == float(np.float32(math.exp(-1024 / 196608)))
    assert f(1e30) == 1.0                                                      # rounds to 1: an infinite memory
    # solve_host: the fold's state in, everything else out, the counters kept
    rec = dabgpu.iqbal_solve_host(dabgpu.iqbal_stream(min_weight=1024), 4096.0, [0, 0, 4096, 409.6, 0])
    assert rec["valid"] == 1 and abs(rec["C_re"] - 0.1) < 1e-6 and abs(rec["w_re"] - 0.1 / (1 + math.sqrt(0.99))) < 1e-6 and rec["b_re"] == -rec["w_re"]
    assert dabgpu.iqbal_solve_host(dabgpu.iqbal_stream(), 4096.0, [0, 0, 4096, 409.6, 0])["valid"] == 0      # below the default min_weight
    one = dabgpu.iqbal_stream()
    r = np.zeros(1, np.dtype(dabgpu.IQBAL_RECORD_DTYPE))
    assert L.dabgpu_iqbal_solve_host(None, r.ctypes.data) == INVALID_ARG and L.dabgpu_iqbal_solve_host(C.byref(one), None) == INVALID_ARG
    one.forget = 2.0
    assert L.dabgpu_iqbal_solve_host(C.byref(one), r.ctypes.data) == INVALID_ARG and b"iqbal_solve_host: stream 0: forget" in L.dabgpu_last_error()


def test_bank_entry_points_check_before_any_device_call(dabgpu):
    """no device here: a call that reached one would fail differently (or crash on the fake handles)"""
    L = dabgpu.lib()
    h = C.c_void_p()
    one = (dabgpu.IqBalanceStream * 1)(dabgpu.iqbal_stream())
    fake = C.c_void_p(0x1000)
    assert L.dabgpu_iqbal_bank_create(None, 1, one, 1024, C.byref(h)) == INVALID_ARG
    assert L.dabgpu_iqbal_bank_create(fake, 1, one, 1024, None) == INVALID_ARG
    assert L.dabgpu_iqbal_bank_create(fake, 0, one, 1024, C.byref(h)) == INVALID_ARG
    assert L.dabgpu_iqbal_bank_create(fake, 1, None, 1024, C.byref(h)) == INVALID_ARG
    assert L.dabgpu_iqbal_bank_create(fake, 1, one, 1000, C.byref(h)) == INVALID_ARG and b"iqbal_bank_create: max_samples_per_call = 1000" in L.dabgpu_last_error()
    bad = (dabgpu.IqBalanceStream * 1)(dabgpu.iqbal_stream(mode=9))
    assert L.dabgpu_iqbal_bank_create(fake, 1, bad, 1024, C.byref(h)) == INVALID_ARG and b"iqbal_bank_create: stream 0: mode 9" in L.dabgpu_last_error()
    assert L.dabgpu_iqbal_bank_set_params(None, one, None) == INVALID_ARG
    assert L.dabgpu_iqbal_bank_seek(None, 0, None) == INVALID_ARG
    assert L.dabgpu_iqbal_bank_seek(fake, (1 << 62) + 1, None) == INVALID_ARG and b"2^62" in L.dabgpu_last_error()
    assert L.dabgpu_iqbal_bank_reset(None, None) == INVALID_ARG
    assert L.dabgpu_iqbal_bank_apply(None, fake, 0, 1024, fake, 10, 0, 1.0, 3, None) == INVALID_ARG and b"null bank" in L.dabgpu_last_error()
    assert L.dabgpu_iqbal_bank_apply_host_sync(None, fake, 0, 1024, fake, 10, 0, 1.0, 3) == INVALID_ARG
    assert L.dabgpu_iqbal_bank_read_state_host_sync(None, fake) == INVALID_ARG
    assert L.dabgpu_iqbal_bank_read_moments_host_sync(None, 1, fake) == INVALID_ARG
    L.dabgpu_iqbal_bank_destroy(None)


def build_fuzzer(tmp_path, sanitize):
    exe = tmp_path / ("iqbal_plan_fuzz_san" if sanitize else "iqbal_plan_fuzz")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    res = subprocess.run(["g++", "-std=c++17"] + flags + ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                                                          os.path.join(ROOT, "tests", "cpp", "iqbal_plan_fuzz.cpp"),
                                                          os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


def check_fuzz_output(res):
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["failed_checks"] == 0
    # both sides of every decision were reached: acceptance and refusal, and of each refusal its low and its high edge
    keys = ["accepted_low", "accepted_high", "null_list_low", "solved_identity", "solved_valid", "impairment_refused", "impairment_ok", "apply_ok_a", "apply_ok_b"]
    keys += [k + e for k in ("n_streams", "mode", "coef", "forget", "min_weight", "max_call") for e in ("_low", "_high")]
    keys += ["apply_" + k + e for k in ("flags", "n", "null", "in_stride", "out_stride", "align", "in_place", "measure_n", "measure_max") for e in ("_a", "_b")]
    assert min(out[k] for k in keys) > 100, {k: out[k] for k in keys if out[k] <= 100}


def test_planner_and_solve_fuzzed_plain(tmp_path):
    exe = build_fuzzer(tmp_path, False)
    check_fuzz_output(subprocess.run([str(exe), "60000", "1"], capture_output=True, text=True, timeout=600))


def test_planner_and_solve_fuzzed_under_asan_and_ubsan(tmp_path):
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(p) or not os.path.exists(p):
        pytest.skip("libasan.so is not installed with this gcc")
    exe = build_fuzzer(tmp_path, True)
    for seed in (1, 2):
        check_fuzz_output(subprocess.run([str(exe), "60000", str(seed)], capture_output=True, text=True, timeout=600,
                                         env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")))
