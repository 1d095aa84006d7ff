"""CPU: the channeliser's planner and argument checks (dabgpu_channeliser_design / _plan / _freq_q64 / _input_needed / _decim_for,
dabgpu_channeliser_bank_* before any device call; dab-radio_amd/csrc/dabgpu_host_logic.cpp): every refusal and every acceptance at its
edge, the frequency word's round trips, the input span against brute force, and the planner and the design fuzzed on their own under
ASan + UBSan as a stand-alone program (tests/cpp/channelise_plan_fuzz.cpp)."""
import ctypes as C
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import channelise_model as CM

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


def plan(dabgpu, chs, n_streams, design, start=0):
    return dabgpu.channeliser_plan([CM.to_struct(c, dabgpu.ChanneliserChannel) for c in chs], n_streams, design, start)


def test_acceptances_at_their_edges(dabgpu):
    assert C.sizeof(dabgpu.ChanneliserChannel) == 24 and C.sizeof(dabgpu.ChanneliserFilter) == 8 + 7 * 8 + 576 * 4
    assert C.sizeof(CM.Filter) == C.sizeof(dabgpu.ChanneliserFilter) and C.sizeof(CM.Channel) == 24
    assert (dabgpu.CHANNELISER_TAPS_PER_PHASE, dabgpu.CHANNELISER_MAX_DECIM, dabgpu.CHANNELISER_MAX_CHANNELS) == (CM.TPP, CM.MAX_D, CM.MAX_CH)
    assert (dabgpu.CHANNELISER_SPLIT_TILE, dabgpu.CHANNELISER_COMBINE_ROWS) == (CM.SPLIT_TILE, CM.COMBINE_ROWS)
    four, one, eight = dabgpu.channeliser_design(4), dabgpu.channeliser_design(1), dabgpu.channeliser_design(8)
    assert (four.passband_cycles, four.stopband_cycles, four.cutoff_cycles, four.beta) == (0.375, 0.4609375, 0.41796875, 9.25)
    assert four.error <= 1e-4 and eight.error <= 1e-4 and one.error == 0.0 and (one.taps, four.taps, eight.taps) == (1, 288, 576)
    assert plan(dabgpu, [CM.channel()], 1, four) == {"decim": 4, "taps": 288, "split_tile": 512, "split_window": 584 * 4, "split_lds_bytes": 2 * 16 * 147 * 8,
                                                     "combine_tile": 512, "combine_window": 199, "combine_lds_bytes": 1600}
    assert plan(dabgpu, [CM.channel()], 1, one) == {"decim": 1, "taps": 1, "split_tile": 512, "split_window": 0, "split_lds_bytes": 0,
                                                    "combine_tile": 128, "combine_window": 128, "combine_lds_bytes": 1024}
    g = plan(dabgpu, [CM.channel(stream=s, gain=-3e38) for s in (0,) * 8 + (2,) * 8], 3, eight, CM.MAX_START)       # 8 per stream, one stream empty
    assert g["split_lds_bytes"] == 2 * 32 * 147 * 8 <= 160 * 1024 and g["combine_tile"] == 1024
    assert plan(dabgpu, [CM.channel(M := (1 << 64) - 1, M)], 1, four, -CM.MAX_START)["taps"] == 288
    # edges of the design: the stopband may reach the wideband Nyquist frequency, the passband anything below the stopband
    assert dabgpu.channeliser_design(4, 0.375, 2.0).stopband_cycles == 2.0 and dabgpu.channeliser_design(2, 1e-9, 1e-8).taps == 144
    assert dabgpu.channeliser_design(4, 0.375, 0.625).cutoff_cycles == 0.5                    # the alias-only edges of the resampler


def test_every_refusal(dabgpu):
    L = dabgpu.lib()
    nan, inf = float("nan"), float("inf")
    four = dabgpu.channeliser_design(4)
    bad = [
        ([], 1, 0, "0 channels"),
        ([CM.channel()] * 9, 1, 0, "9 channels on 1 streams"),
        ([CM.channel(stream=1)] * 9 + [CM.channel(stream=2)], 3, 0, "more than 8 channels on stream 1"),
        ([CM.channel(stream=1), CM.channel(stream=0)], 2, 0, "sorted by stream"),
        ([CM.channel(stream=0), CM.channel(stream=2)], 2, 0, "channel 1: stream 2 of 2"),
        ([CM.channel(gain=nan)], 1, 0, "gain is not finite"),
        ([CM.channel(), CM.channel(gain=-inf)], 1, 0, "channel 1: gain is not finite"),
        ([CM.channel()], 1, CM.MAX_START + 1, "start outside"),
        ([CM.channel()], 1, -CM.MAX_START - 1, "start outside"),
        ([CM.channel()], 0, 0, "0 streams"),
        ([CM.channel()], (1 << 20) + 1, 0, "1048577 streams"),
    ]
    for chs, n_streams, start, text in bad:
        with pytest.raises(dabgpu.DabGpuError) as err:
            plan(dabgpu, chs, n_streams, four, start)
        assert text in str(err.value), (text, str(err.value))
    with pytest.raises(dabgpu.DabGpuError) as err:
        plan(dabgpu, [CM.channel()], 1, None)
    assert "null design" in str(err.value)
    assert L.dabgpu_channeliser_plan(None, 1, 1, 0, C.byref(four), None) == INVALID_ARG and b"null channel list" in L.dabgpu_last_error()
    for D in (0, 9, -1):
        with pytest.raises(dabgpu.DabGpuError) as err:
            dabgpu.channeliser_design(D)
        assert "decimation" in str(err.value)
        broken = dabgpu.channeliser_design(4)
        broken.decim = D
        with pytest.raises(dabgpu.DabGpuError):
            plan(dabgpu, [CM.channel()], 1, broken)
    for pb, sb, text in ((nan, 0.46, "positive"), (0.375, nan, "positive"), (-0.1, 0.46, "positive"), (0.375, -1.0, "positive"), (0.46, 0.375, "no transition"),
                         (0.4, 0.4, "no transition"), (0.375, 2.0001, "beyond"), (0.375, inf, "beyond"), (inf, inf, "no transition")):
        with pytest.raises(dabgpu.DabGpuError) as err:
            dabgpu.channeliser_design(4, pb, sb)
        assert text in str(err.value), (pb, sb, str(err.value))
    with pytest.raises(dabgpu.DabGpuError):
        dabgpu.channeliser_design(1, 0.375, 0.51)                                      # D = 1 holds nothing beyond 0.5
    assert L.dabgpu_channeliser_design(4, 0.0, 0.0, None) == INVALID_ARG


def test_bank_entry_points_check_before_any_device_call(dabgpu):
    """no device here: a call that reached one would fail differently (or crash on the fake handles)"""
    L = dabgpu.lib()
    h = C.c_void_p()
    four = dabgpu.channeliser_design(4)
    one = (dabgpu.ChanneliserChannel * 1)(CM.to_struct(CM.channel(), dabgpu.ChanneliserChannel))
    fake = C.c_void_p(0x1000)
    assert L.dabgpu_channeliser_bank_create(None, one, 1, 1, 0, C.byref(four), C.byref(h)) == INVALID_ARG
    assert L.dabgpu_channeliser_bank_create(fake, one, 1, 1, 0, C.byref(four), None) == INVALID_ARG
    assert L.dabgpu_channeliser_bank_create(fake, one, 1, 1, 0, None, C.byref(h)) == INVALID_ARG and b"null design" in L.dabgpu_last_error()
    assert L.dabgpu_channeliser_bank_create(fake, one, 0, 1, 0, C.byref(four), C.byref(h)) == INVALID_ARG
    assert L.dabgpu_channeliser_bank_create(fake, None, 1, 1, 0, C.byref(four), C.byref(h)) == INVALID_ARG
    assert L.dabgpu_channeliser_bank_create(fake, one, 1, 1, 1 << 62, C.byref(four), C.byref(h)) == INVALID_ARG and b"start" in L.dabgpu_last_error()
    bad = (dabgpu.ChanneliserChannel * 1)(CM.to_struct(CM.channel(gain=float("nan")), dabgpu.ChanneliserChannel))
    assert L.dabgpu_channeliser_bank_create(fake, bad, 1, 1, 0, C.byref(four), C.byref(h)) == INVALID_ARG and b"gain" in L.dabgpu_last_error()
    assert L.dabgpu_channeliser_bank_set_params(None, one, 1, 0, None) == INVALID_ARG
    assert L.dabgpu_channeliser_bank_seek(None, 0, None) == INVALID_ARG
    assert L.dabgpu_channeliser_bank_seek(fake, (1 << 58) + 1, None) == INVALID_ARG and b"2^58" in L.dabgpu_last_error()
    assert L.dabgpu_channeliser_bank_split(None, fake, 0, 1, 0, 1, fake, 0, None) == INVALID_ARG and b"null bank" in L.dabgpu_last_error()
    assert L.dabgpu_channeliser_bank_split_host_sync(None, fake, 0, 1, 0, 1, fake, 0) == INVALID_ARG
    assert L.dabgpu_channeliser_bank_combine(None, fake, 0, 1, 0, 1, fake, 10, 0, 1.0, None) == INVALID_ARG and b"null bank" in L.dabgpu_last_error()
    assert L.dabgpu_channeliser_bank_combine_host_sync(None, fake, 0, 1, 0, 1, fake, 10, 0, 1.0) == INVALID_ARG
    L.dabgpu_channeliser_bank_destroy(None)


def test_frequency_word_round_trips_and_decimations(dabgpu):
    q = dabgpu.channeliser_freq
    nan = float("nan")
    assert q(0.0, 8192000.0) == 0 and q(2048000.0, 8192000.0) == 1 << 62 and q(-2048000.0, 8192000.0) == 3 << 62
    assert q(4096000.0, 8192000.0) == 1 << 63 == q(-4096000.0, 8192000.0)               # +- half the rate: one word
    for bad in ((4096000.1, 8192000.0), (-4096001.0, 8192000.0), (nan, 8192000.0), (1.0, nan), (1.0, 0.0), (1.0, -8192000.0), (1.0, float("inf"))):
        assert q(*bad) == 0
    rng = np.random.default_rng(9700)
    cases = [(300000.0, 8192000.0), (-1712000.0, 8192000.0), (1712000.0 + 300000.0, 8192000.0), (3424000.0, 10240000.0), (-6848000.0, 16384000.0)]
    cases += [(float(o), float(r)) for o, r in zip(rng.integers(-4000000, 4000000, 500), rng.integers(8000000, 17000000, 500))]
    for off, rate in cases:
        exact = Fraction(off) / Fraction(rate)
        w = q(off, rate)
        signed = w - (1 << 64) if w >> 63 else w
        assert abs(Fraction(signed, 1 << 64) - exact) <= Fraction(1, 1 << 53), (off, rate)       # the quotient is one double
        assert w == CM.freq_q64(off, rate)
        assert (q(-off, rate) + w) & ((1 << 64) - 1) == 0                               # two's complement
        assert abs(dabgpu.lib().dabgpu_channel_freq_cycles(w) - float(exact)) <= 2.0 ** -53
    d = dabgpu.channeliser_decim_for
    assert [d(r) for r in (8192000.0, 10240000.0, 10000000.0, 16384000.0, 2048000.0, 4095999.9, 4096000.0, 2.4e6, 1e9)] == [4, 5, 4, 8, 1, 1, 2, 1, 8]
    assert [d(r) for r in (2047999.9, 0.0, -1.0, nan)] == [0, 0, 0, 0] and d(float("inf")) == 8


def test_input_needed_against_brute_force(dabgpu):
    rng = np.random.default_rng(9800)
    cases = [(1, 0, 0, 1), (1, 5, -3, 1000), (4, 0, 0, 1), (4, 0, 0, 0), (8, CM.MAX_POSITION, CM.MAX_START, 1 << 31), (8, CM.MAX_POSITION, -CM.MAX_START, 7),
             (5, 123, -1000, 513)]
    for _ in range(300):
        cases.append((int(rng.integers(1, 9)), int(rng.integers(0, 1 << 45)), int(rng.integers(-(1 << 40), 1 << 40)), int(rng.integers(1, 3000))))
    for D, pos, start, n_out in cases:
        first, count = dabgpu.channeliser_input_needed(D, pos, start, n_out)
        if n_out == 0:
            assert count == 0
            continue
        lo = pos * D + start - CM.peak(D)                                    # tap 0 of the first output
        hi = (pos + n_out - 1) * D + start - CM.peak(D) + CM.taps(D) - 1     # the last tap of the last
        assert (first, first + count - 1) == (lo, hi), (D, pos, start, n_out)
    for bad in ((0, 0, 0, 1), (9, 0, 0, 1), (4, CM.MAX_POSITION + 1, 0, 1), (4, 0, CM.MAX_START + 1, 1), (4, 0, -CM.MAX_START - 1, 1), (4, 0, 0, (1 << 31) + 1)):
        with pytest.raises(dabgpu.DabGpuError):
            dabgpu.channeliser_input_needed(*bad)
    L = dabgpu.lib()
    assert L.dabgpu_channeliser_input_needed(4, 0, 0, 1, None, C.byref(C.c_uint64())) == INVALID_ARG
    assert L.dabgpu_channeliser_input_needed(4, 0, 0, 1, C.byref(C.c_int64()), None) == INVALID_ARG


def test_planner_and_design_fuzzed_under_asan_and_ubsan(tmp_path):
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(p) or not os.path.exists(p):
        pytest.skip("libasan.so is not installed with this gcc")
    exe = tmp_path / "channelise_plan_fuzz"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "channelise_plan_fuzz.cpp"),
                          os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    for seed in (1, 2):
        res = subprocess.run([str(exe), "20000", str(seed)], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
        assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
        out = json.loads(res.stdout.strip().splitlines()[-1])
        assert out["failed_checks"] == 0
        # both sides of every decision were reached: acceptance and refusal, and of each refusal its low and its high edge
        keys = ["accepted", "spans", "freqs", "firsts"]
        keys += [k + e for k in ("n_streams", "n_channels", "stream_range", "unsorted", "nine", "gain", "start", "decim", "null_list", "null_design")
                 for e in ("_low", "_high")]
        assert min(out[k] for k in keys) > 100, {k: out[k] for k in keys if out[k] <= 100}
        assert out["spans"] == out["iterations"] and out["designs"] > 30 and out["design_refusals"] > 100
