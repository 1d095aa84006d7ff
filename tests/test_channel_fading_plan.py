"""CPU: the fading planner (dabgpu_channel_fading_plan, dabgpu_channel_profile, dabgpu_channel_fading_gain_host and the fading bank's
entry points before any device call; dab-radio_amd/csrc/dabgpu_host_logic.cpp): every refusal with its message, every range at both
ends, the Philox counter layout as known answers of tests/channel_model.py's Philox, the frequency words against float64, the
amplitudes' unit power, the presets, and the planner fuzzed on its own under ASan + UBSan (tests/cpp/channel_fading_fuzz.cpp)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import channel_fading_model as FM
import channel_model as CM

ROOT = CM.ROOT
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
INVALID_ARG = 2


@pytest.fixture(scope="module")
def dabgpu():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu


def plan(dabgpu, plist, specs):
    return dabgpu.channel_fading_plan([CM.to_struct(P, dabgpu.ChannelStream) for P in plist], [dabgpu.channel_fading_spec(**s) for s in specs])


TAPS3 = [(0, 1.0, 0.0), (5, 0.5, 0.5), (2047, 0.0, -0.25)]


def test_layouts_and_constants(dabgpu):
    assert C.sizeof(dabgpu.ChannelFadingTap) == 17 * 16 + 8 == C.sizeof(FM.FadingTap)
    assert C.sizeof(dabgpu.ChannelFadingStream) == 32 + 8 * 280 == C.sizeof(FM.FadingStream)
    assert C.sizeof(dabgpu.ChannelFadingSpec) == 16 + 3 * 32 == C.sizeof(FM.FadingSpec)
    assert (dabgpu.FADING_OSC, dabgpu.FADING_GRID, dabgpu.FADING_MAX_DOPPLER_CYCLES) == (17, 64, 2.0 ** -11)
    assert C.sizeof(dabgpu.ChannelStream) == 144                              # the plain stream is the struct of before


def test_every_refusal(dabgpu):
    nan, inf = float("nan"), float("inf")
    P = CM.params_dict(taps=TAPS3)
    ok = dict(doppler_cycles=1e-5, seed=1, kinds=[1, 0, 1])
    bad = [
        (dict(ok, doppler_cycles=-1e-300), "doppler_cycles"),
        (dict(ok, doppler_cycles=np.nextafter(2.0 ** -11, 1.0)), "doppler_cycles"),
        (dict(ok, doppler_cycles=nan), "doppler_cycles"),
        (dict(ok, doppler_cycles=inf), "doppler_cycles"),
        (dict(ok, kinds=[1, 2, 1]), "stream 1: tap 1: kind 2"),
        (dict(ok, kinds=[-1, 0, 0]), "stream 1: tap 0: kind -1"),
        (dict(ok, rice_k=[0.0, 0.0, -1e-30]), "stream 1: tap 2: rice_k"),
        (dict(ok, rice_k=[nan, 0.0, 0.0]), "stream 1: tap 0: rice_k"),
        (dict(ok, rice_k=[inf, 0.0, 0.0]), "stream 1: tap 0: rice_k"),
        (dict(ok, los_cos=[float(np.nextafter(np.float32(1), np.float32(2))), 0.0, 0.0]), "stream 1: tap 0: los_cos"),
        (dict(ok, los_cos=[0.0, 0.0, float(np.nextafter(np.float32(-1), np.float32(-2)))]), "stream 1: tap 2: los_cos"),
        (dict(ok, los_cos=[nan, 0.0, 0.0]), "stream 1: tap 0: los_cos"),
    ]
    for spec, text in bad:
        with pytest.raises(dabgpu.DabGpuError) as err:
            plan(dabgpu, [P, P], [ok, spec])
        assert text in str(err.value), (text, str(err.value))
    # rice_k and los_cos of a static tap, and everything past n_taps, are not read
    plan(dabgpu, [P], [dict(ok, kinds=[1, 0, 1, 9, 9], rice_k=[0.0, -1.0, 0.0, nan], los_cos=[0.0, 5.0, 0.0, nan])])
    # whatever dabgpu_channel_plan refuses, with its message
    for Q, text in ((CM.params_dict(taps=[(2048, 1.0, 0.0)]), "delay 2048"), (CM.params_dict(noise_sigma=-1.0), "noise_sigma is negative"),
                    (CM.params_dict(taps=[]), "0 taps"), (CM.params_dict(gain=nan), "gain is not finite")):
        with pytest.raises(dabgpu.DabGpuError) as err:
            plan(dabgpu, [Q], [dict(doppler_cycles=0.0)])
        assert text in str(err.value)
    L = dabgpu.lib()
    one = (dabgpu.ChannelStream * 1)(CM.to_struct(P, dabgpu.ChannelStream))
    sp = (dabgpu.ChannelFadingSpec * 1)(dabgpu.channel_fading_spec(**ok))
    out = (dabgpu.ChannelFadingStream * 1)()
    for args in ((None, sp, 1, out), (one, None, 1, out), (one, sp, 1, None)):
        assert L.dabgpu_channel_fading_plan(*args) == INVALID_ARG and b"null" in L.dabgpu_last_error()
    assert L.dabgpu_channel_fading_plan(one, sp, 0, out) == INVALID_ARG and b"0 streams" in L.dabgpu_last_error()
    assert L.dabgpu_channel_fading_plan(one, sp, 1, out) == 0


def test_bank_and_gain_entry_points_check_before_any_device_call(dabgpu):
    L = dabgpu.lib()
    h = C.c_void_p()
    P = CM.params_dict(taps=TAPS3)
    one = (dabgpu.ChannelStream * 1)(CM.to_struct(P, dabgpu.ChannelStream))
    tab = plan(dabgpu, [P], [dict(doppler_cycles=1e-5, kinds=[1, 1, 1])])
    fake = C.c_void_p(0x1000)
    assert L.dabgpu_channel_bank_create_fading(None, 1, one, tab, C.byref(h)) == INVALID_ARG and b"channel_bank_create_fading" in L.dabgpu_last_error()
    assert L.dabgpu_channel_bank_create_fading(fake, 1, one, tab, None) == INVALID_ARG
    assert L.dabgpu_channel_bank_create_fading(fake, 1, one, None, C.byref(h)) == INVALID_ARG and b"null" in L.dabgpu_last_error()
    assert L.dabgpu_channel_bank_create_fading(fake, 0, one, tab, C.byref(h)) == INVALID_ARG
    tab[0].kind[1] = 3
    assert L.dabgpu_channel_bank_create_fading(fake, 1, one, tab, C.byref(h)) == INVALID_ARG and b"tap 1: kind 3" in L.dabgpu_last_error()
    tab[0].kind[1] = 1
    tab[0].tap[2].amp_diffuse = float("inf")
    assert L.dabgpu_channel_bank_create_fading(fake, 1, one, tab, C.byref(h)) == INVALID_ARG and b"tap 2: fading amplitudes" in L.dabgpu_last_error()
    assert L.dabgpu_channel_bank_set_fading(None, tab, None) == INVALID_ARG and b"null bank" in L.dabgpu_last_error()
    out = np.zeros(8, np.float32)
    assert L.dabgpu_channel_fading_gain_host(None, 0, 0, 4, out.ctypes.data) == INVALID_ARG
    assert L.dabgpu_channel_fading_gain_host(tab, 8, 0, 4, out.ctypes.data) == INVALID_ARG and b"tap 8" in L.dabgpu_last_error()
    assert L.dabgpu_channel_fading_gain_host(tab, -1, 0, 4, out.ctypes.data) == INVALID_ARG
    assert L.dabgpu_channel_fading_gain_host(tab, 0, 0, 4, None) == INVALID_ARG
    assert L.dabgpu_channel_fading_gain_host(tab, 0, 0, 0, None) == 0


@pytest.mark.parametrize("doppler", [0.0, 2.0 ** -11, 100.0 / 2.048e6])
def test_tables_equal_the_model_planner(dabgpu, doppler):
    """both ends of every range accepted; the Philox counter layout (n, k, s, 1) under key = seed as known answers of
    channel_model.philox4x32_10; every freq_q64 within 2^12 counts (2^-52 cycles per sample: the host's cosine) of the float64 value;
    amp_diffuse^2 16 + amp_los^2 = 1 to float rounding"""
    seed = 0xfedcba9876543210
    P = CM.params_dict(taps=TAPS3 + [(7, 0.1, 0.1)])
    kinds, rice, los = [1, 1, 0, 1], [0.0, 4.0, 0.0, 1e6], [1.0, -1.0, 0.0, 0.25]
    tabs = plan(dabgpu, [P, P, P], [dict(doppler_cycles=0.0)] + [dict(doppler_cycles=doppler, seed=seed, kinds=kinds, rice_k=rice, los_cos=los)] * 2)
    assert list(tabs[0].kind) == [0] * 8
    for s in (1, 2):
        want = FM.plan_stream(P, doppler, seed, s, kinds, rice, los)
        got = FM.from_struct(tabs[s], 8)
        assert got[2] is None and got[4:] == [None] * 4
        assert bytes(tabs[s].tap[2]) == bytes(280) and bytes(tabs[s].tap[7]) == bytes(280)
        for k in (0, 1, 3):
            assert got[k]["phase"] == want[k]["phase"], (s, k)
            for n in range(17):
                d = (got[k]["freq"][n] - want[k]["freq"][n]) % (1 << 64)
                assert min(d, (1 << 64) - d) <= 1 << 12, (s, k, n)
                signed = got[k]["freq"][n] - (1 << 64) if got[k]["freq"][n] >> 63 else got[k]["freq"][n]
                assert abs(signed) <= round(doppler * 2 ** 64) + 1
            assert got[k]["amp_diffuse"] == want[k]["amp_diffuse"] and got[k]["amp_los"] == want[k]["amp_los"]
            assert abs(16 * got[k]["amp_diffuse"] ** 2 + got[k]["amp_los"] ** 2 - 1) <= 4 * CM.U
        assert got[0]["amp_los"] == 0.0 and got[0]["amp_diffuse"] == 0.25          # Rayleigh
        assert got[0]["freq"][16] == FM.freq_q64(doppler) and got[1]["freq"][16] == FM.freq_q64(-doppler)      # los_cos = +-1: exact
    assert FM.from_struct(tabs[1], 4)[0]["phase"] != FM.from_struct(tabs[2], 4)[0]["phase"]                  # the stream is in the counter
    # the first words as plain numbers: key (seed lo, seed hi), counter (n, k, s, 1)
    w = [int(v) for v in CM.philox4x32_10((seed & CM.M32, seed >> 32), (5, 3, 2, 1))]
    assert tabs[2].tap[3].phase_q64[5] == (w[2] << 32) | w[3]
    w0 = [int(v) for v in CM.philox4x32_10((seed & CM.M32, seed >> 32), (5, 3, 2, 0))]                        # the noise's counter word
    assert tabs[2].tap[3].phase_q64[5] != (w0[2] << 32) | w0[3]


def test_stratified_angles(dabgpu):
    """oscillator n's frequency lies in its sixteenth of the circle: cos(2 pi (n + 1) / 16) .. cos(2 pi n / 16) of the Doppler"""
    P = CM.params_dict()
    d = 2.0 ** -11
    for seed in range(20):
        T = FM.from_struct(plan(dabgpu, [P], [dict(doppler_cycles=d, seed=seed, kinds=[1])])[0], 1)[0]
        for n in range(16):
            f = T["freq"][n]
            c = (f - (1 << 64) if f >> 63 else f) / 2.0 ** 64 / d
            lo, hi = sorted((np.cos(2 * np.pi * n / 16), np.cos(2 * np.pi * (n + 1) / 16)))
            assert lo - 1e-12 <= c <= hi + 1e-12, (seed, n, c)


def test_profiles(dabgpu):
    want = {"tu6": ([0, 0, 1, 3, 5, 10], [-3, 0, -2, -6, -8, -10]), "ra6": ([0, 0, 0, 1, 1, 1], [0, -4, -8, -12, -16, -20]), "sfn2": ([0, 200], [0, -6])}
    for name, (delays, db) in want.items():
        p = dabgpu.channel_profile(name)
        assert [t[0] for t in p["taps"]] == delays and all(t[2] == 0.0 for t in p["taps"])
        pw = 10.0 ** (np.array(db) / 10.0)
        assert np.allclose([t[1] for t in p["taps"]], np.sqrt(pw / pw.sum()), rtol=1e-6, atol=0)
        assert abs(sum(t[1] ** 2 for t in p["taps"]) - 1) < 1e-6
        assert p["kinds"] == [1] * len(delays)
        rice = [k > 0 for k in p["rice_k"]]
        assert rice == ([True] + [False] * 5 if name == "ra6" else [False] * len(delays))
        # a preset plans as it stands
        plan(dabgpu, [CM.params_dict(taps=p["taps"])], [dict(doppler_cycles=10 / 2.048e6, seed=1, kinds=p["kinds"], rice_k=p["rice_k"], los_cos=p["los_cos"])])
    with pytest.raises(dabgpu.DabGpuError) as err:
        dabgpu.channel_profile("tu12")
    assert "unknown profile" in str(err.value)
    # the fields a preset does not own stay
    L = dabgpu.lib()
    S, F = CM.to_struct(CM.params_dict(gain=3.0, noise_sigma=0.5, seed=77, start=5), dabgpu.ChannelStream), dabgpu.ChannelFadingSpec()
    F.doppler_cycles, F.seed = 1e-4, 9
    assert L.dabgpu_channel_profile(b"sfn2", C.byref(S), C.byref(F)) == 0
    assert (S.gain, S.noise_sigma, S.seed, S.start, S.n_taps, F.doppler_cycles, F.seed) == (3.0, 0.5, 77, 5, 2, 1e-4, 9)
    assert L.dabgpu_channel_profile(None, C.byref(S), C.byref(F)) == INVALID_ARG


def test_planner_fuzzed_under_asan_and_ubsan(tmp_path):
    """a stand-alone program with its own main; nothing loaded into Python runs under a sanitizer.  Where this gcc has no libasan.so the
    program is built and run without the sanitizers -- its checks of the stated rules still run -- instead of the test skipping itself"""
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if os.path.isabs(p) and os.path.exists(p) else []
    print("sanitizers:", san or "none (libasan.so is not installed with this gcc)")
    exe = tmp_path / "channel_fading_fuzz"
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + san + [
                          "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          os.path.join(ROOT, "tests", "cpp", "channel_fading_fuzz.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    for seed in (1, 2):
        res = subprocess.run([str(exe), "6000", str(seed)], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
        assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
        out = json.loads(res.stdout.strip().splitlines()[-1])
        assert out["failed_checks"] == 0
        keys = ["accepted", "edge_dopplers", "gains", "tables_pass", "tables_fail"] + [k + e for k in ("doppler", "kind", "rice", "los", "params")
                                                                                          for e in ("_low", "_high")]
        assert min(out[k] for k in keys) > 100, {k: out[k] for k in keys if out[k] <= 100}
        assert out["null_low"] + out["null_high"] > 100
        assert out["tables_pass"] == out["tables_fail"] == out["accepted"]
