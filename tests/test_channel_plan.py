"""CPU: the channel model's planner and argument checks (dabgpu_channel_plan, dabgpu_channel_freq_q64 / _cycles, dabgpu_channel_bank_*
before any device call; dab-radio_amd/csrc/dabgpu_host_logic.cpp): every refusal and every acceptance at its edge, the frequency word's
round trips, and the planner fuzzed on its own under ASan + UBSan (tests/cpp/channel_plan_fuzz.cpp)."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import channel_model as CM

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


def plan(dabgpu, plist):
    return dabgpu.channel_plan([CM.to_struct(P, dabgpu.ChannelStream) for P in plist])


def test_acceptances_at_their_edges(dabgpu):
    assert dabgpu.CHANNEL_MAX_DELAY >= 504                                  # the mode I guard interval
    assert C.sizeof(dabgpu.ChannelStream) == 144
    assert plan(dabgpu, [CM.params_dict()]) == {"halo": 0, "block_samples": 1024, "lds_bytes": 0, "staged": 0}
    assert plan(dabgpu, [CM.params_dict(taps=[(1, 1.0, 0.0)])]) == {"halo": 2, "block_samples": 1024, "lds_bytes": (1024 + 2 + 2) * 8, "staged": 1}
    assert plan(dabgpu, [CM.params_dict(taps=[(0, 1.0, 0.0)] * 2)])["staged"] == 1                     # two taps at delay 0 still sum in LDS
    eight = [(2047, 3.0e38, -3.0e38)] + [(k, 0.0, 0.0) for k in range(7)]
    assert plan(dabgpu, [CM.params_dict(), CM.params_dict(taps=eight, noise_sigma=0.0, gain=-3.0e38)]) == \
        {"halo": 2048, "block_samples": 1024, "lds_bytes": (1024 + 2048 + 2) * 8, "staged": 1}
    assert plan(dabgpu, [CM.params_dict(noise_sigma=3.0e38, start=-(1 << 62), seed=(1 << 64) - 1, freq_q64=(1 << 64) - 1)])["halo"] == 0
    assert plan(dabgpu, [CM.params_dict(taps=[(504, 1.0, 0.0)])])["halo"] == 504
    assert plan(dabgpu, [CM.params_dict(taps=[(505, 1.0, 0.0)])])["halo"] == 506


def test_every_refusal(dabgpu):
    L = dabgpu.lib()
    nan, inf = float("nan"), float("inf")
    bad = [
        ([], "0 streams"),
        ([CM.params_dict(taps=[])], "0 taps"),
        ([CM.params_dict(), CM.params_dict(taps=[(2048, 1.0, 0.0)])], "stream 1: tap 0: delay 2048"),
        ([CM.params_dict(taps=[(0, 1.0, 0.0), (-1, 1.0, 0.0)])], "stream 0: tap 1: delay -1"),
        ([CM.params_dict(gain=nan)], "gain is not finite"),
        ([CM.params_dict(gain=-inf)], "gain is not finite"),
        ([CM.params_dict(noise_sigma=inf)], "noise_sigma is not finite"),
        ([CM.params_dict(noise_sigma=nan)], "noise_sigma is not finite"),
        ([CM.params_dict(noise_sigma=-1e-30)], "noise_sigma is negative"),
        ([CM.params_dict(taps=[(0, nan, 0.0)])], "tap 0 is not finite"),
        ([CM.params_dict(start=(1 << 62) + 1)], "start outside"),
        ([CM.params_dict(start=-(1 << 62) - 1)], "start outside"),
        ([CM.params_dict(taps=[(0, 1.0, 0.0), (3, 0.0, inf)])], "tap 1 is not finite"),
    ]
    for plist, text in bad:
        with pytest.raises(dabgpu.DabGpuError) as err:
            plan(dabgpu, plist)
        assert text in str(err.value), (text, str(err.value))
    nine = CM.to_struct(CM.params_dict(), dabgpu.ChannelStream)
    nine.n_taps = 9
    with pytest.raises(dabgpu.DabGpuError) as err:
        dabgpu.channel_plan([nine])
    assert "9 taps" in str(err.value)
    one = (dabgpu.ChannelStream * 1)(CM.to_struct(CM.params_dict(), dabgpu.ChannelStream))
    assert L.dabgpu_channel_plan(None, 1, None) == INVALID_ARG
    assert L.dabgpu_channel_plan(one, (1 << 20) + 1, None) == INVALID_ARG and b"1048577 streams" in L.dabgpu_last_error()
    assert L.dabgpu_channel_plan(one, 1, None) == 0


def test_bank_entry_points_check_before_any_device_call(dabgpu):
    """no device here: a call that reached one would fail differently (or crash on the fake handles)"""
    L = dabgpu.lib()
    h = C.c_void_p()
    one = (dabgpu.ChannelStream * 1)(CM.to_struct(CM.params_dict(), dabgpu.ChannelStream))
    fake = C.c_void_p(0x1000)
    assert L.dabgpu_channel_bank_create(None, 1, one, C.byref(h)) == INVALID_ARG
    assert L.dabgpu_channel_bank_create(fake, 1, one, None) == INVALID_ARG
    assert L.dabgpu_channel_bank_create(fake, 0, one, C.byref(h)) == INVALID_ARG
    assert L.dabgpu_channel_bank_create(fake, 1, None, C.byref(h)) == INVALID_ARG
    bad = (dabgpu.ChannelStream * 1)(CM.to_struct(CM.params_dict(noise_sigma=-1.0), dabgpu.ChannelStream))
    assert L.dabgpu_channel_bank_create(fake, 1, bad, C.byref(h)) == INVALID_ARG and b"negative" in L.dabgpu_last_error()
    assert L.dabgpu_channel_bank_set_params(None, one, None) == INVALID_ARG
    assert L.dabgpu_channel_bank_seek(None, 0, None) == INVALID_ARG
    assert L.dabgpu_channel_bank_seek(fake, (1 << 62) + 1, None) == INVALID_ARG and b"2^62" in L.dabgpu_last_error()
    assert L.dabgpu_channel_bank_apply(None, fake, 0, 1, 0, 1, fake, 10, 0, 1.0, None) == INVALID_ARG and b"null bank" in L.dabgpu_last_error()
    assert L.dabgpu_channel_bank_apply_host_sync(None, fake, 0, 1, 0, 1, fake, 10, 0, 1.0) == INVALID_ARG
    L.dabgpu_channel_bank_destroy(None)


def test_frequency_word_round_trips(dabgpu):
    L = dabgpu.lib()
    q, cyc = L.dabgpu_channel_freq_q64, L.dabgpu_channel_freq_cycles
    assert q(0.0) == 0 and q(-0.0) == 0
    assert q(0.25) == 1 << 62 and q(-0.25) == 3 << 62
    assert q(0.5) == 1 << 63 and q(-0.5) == 1 << 63                         # half a cycle per sample either way
    assert cyc(1 << 63) == -0.5 and cyc((1 << 63) - (1 << 11)) == 0.5 - 2.0 ** -53
    assert q(2.0 ** -64) == 1 and q(-2.0 ** -64) == (1 << 64) - 1
    assert q(float("nan")) == 0 and q(0.5000001) == 0 and q(-0.6) == 0 and q(float("inf")) == 0
    rng = np.random.default_rng(9)
    for c in list(rng.uniform(-0.5, 0.5, 2000)) + [0.4999, -0.4999, 0.5 - 2.0 ** -53, -0.5 + 2.0 ** -53, 1e-12, -1e-12]:
        w = q(float(c))
        assert w == round(c * 2 ** 64) % (1 << 64)                          # Python integers: exact
        back = cyc(w)
        assert -0.5 <= back < 0.5
        assert abs(back - c) <= 2.0 ** -54 or (c == 0.5 and back == -0.5)
    # Hz at DAB's sample rate: a quarter of mode I's carrier spacing (250 Hz), both signs, to a word and back within a double's ulp
    for hz in (250.0, -250.0, 1.0e6, -1.0e6, 1023999.0):
        w = q(hz / 2.048e6)
        assert abs(cyc(w) * 2.048e6 - hz) <= 1e-9 * abs(hz) + 1e-9
        assert (q(hz / 2.048e6) + q(-hz / 2.048e6)) % (1 << 64) == 0


def test_planner_fuzzed_under_asan_and_ubsan(tmp_path):
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(p) or not os.path.exists(p):
        pytest.skip("libasan.so is not installed with this gcc")
    exe = tmp_path / "channel_plan_fuzz"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "channel_plan_fuzz.cpp"),
                          os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    for seed in (1, 2):
        res = subprocess.run([str(exe), "60000", str(seed)], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
        assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
        out = json.loads(res.stdout.strip().splitlines()[-1])
        assert out["failed_checks"] == 0
        # both sides of every decision were reached: acceptance and refusal, and of each refusal its low and its high edge where it has two
        two_sided = ("n_streams", "taps", "delay", "start", "apply_format", "apply_n_in", "apply_null", "apply_in_stride", "apply_out_stride", "apply_align")
        keys = ["accepted", "direct", "staged", "fits_no", "fits_yes_smaller", "fits_yes_equal", "apply_ok_a", "apply_ok_b"]
        keys += [k + e for k in two_sided for e in (("_low", "_high") if not k.startswith("apply") else ("_a", "_b"))]
        keys += [k + "_low" for k in ("gain", "sigma_not_finite", "sigma_negative", "tap_value", "null_params")]
        keys += [k + "_high" for k in ("gain", "sigma_not_finite", "sigma_negative", "tap_value", "null_params")]
        keys += ["apply_n_out_a", "apply_scale_a", "apply_grid_a"]
        assert min(out[k] for k in keys) > 100, {k: out[k] for k in keys if out[k] <= 100}
        assert out["round_trips"] == out["iterations"]
