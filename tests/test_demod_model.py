"""The oracle's demodulator (oracle.demod_frame_mode, oracle.demod_frame, oracle.update_fine_freq_mode) held to the float64 model of
tests/demod_model.py, stage by stage, in modes I-IV: spectra, soft bits as intervals, cyclic-prefix correlation and angle, summed
phase, fine-frequency update with its fmod wrap.  The same hold_* functions hold the device in tests/test_gpu_demod_float64.py; here
they also show that the conditions on the INPUT (few ambiguous soft bits, no energy-free carrier) hold for the model's own frames.
Each test prints the worst ratio to every bound."""
import numpy as np
import pytest

import demod_model as DM

# offset handed to the PLL (the frame is rotated by its negative), noise, scale, extras: none, a few 1e-3 of either sign, a third of
# a mode I carrier grid (333 carriers), just under half a cycle per sample; tiny and huge frames; a notch; a purely real symbol
CASES = [
    dict(f=0.0, noise=0.03, real_symbol=3),
    dict(f=7e-4, noise=0.05, notch=(5, 6, 7, 100, 101, -3)),
    dict(f=-1e-3, noise=0.03, scale=1e-12),
    dict(f=1.7e-3, noise=0.2, scale=1e12),
    dict(f=-2.3e-3, noise=1.0),                      # about -3 dB
    dict(f=333 / 2048, noise=0.03),
    dict(f=-0.4999, noise=0.03),
]


def frame_of(mode, k, case):
    g = DM.Geometry(mode)
    kw = {key: v for key, v in case.items() if key != "f"}
    if "notch" in kw:
        kw["notch"] = tuple(s % g.NC for s in kw["notch"])
    return DM.make_frame(mode, np.random.default_rng(9000 + 10 * mode + k), f=case["f"], **kw)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_oracle_demodulator_equals_the_float64_model_stage_by_stage(oracle, mode):
    g = DM.Geometry(mode)
    og = oracle.geometry(mode)
    assert (og.nb_frame_symbols, og.nb_fft, og.nb_cp, og.nb_null_period, og.nb_carriers) == DM.Geometry.TABLE[mode]
    for k, case in enumerate(CASES):
        f = np.float32(case["f"])
        frame, sent = frame_of(mode, k, case)
        ref = DM.demodulate(frame, f, mode)
        runs = [("demod_frame_mode", oracle.demod_frame_mode(mode, frame, f, want_fft=True))]
        if mode == 1:
            runs.append(("demod_frame", oracle.demod_frame(frame, f, want_fft=True)))
        for name, r in runs:
            what = (mode, float(f), name)
            r_fft = DM.hold_fft(r["fft"], ref, mode, f, what)
            iv = DM.soft_bit_intervals(r["fft"].reshape(g.L + 1, g.N), mode)
            differ, ambiguous = DM.hold_soft_bits(r["bits"], iv, what)
            if not {"notch", "real_symbol"} & set(case) and case["noise"] < 0.1:
                assert np.array_equal(iv["w"] >= 0, sent.astype(bool)), "the model demodulates its own frame"
            r_corr = DM.hold_cp(r["cp_corr"], ref, mode, f, what)
            r_angle = DM.hold_angles(r["cp_phase"], ref, DM.angle_bounds_from_input(ref, mode, f), what)
            fine0 = np.float32(1e-5 * (k - 3))
            fine1 = oracle.update_fine_freq_mode(mode, fine0, r["total_phase"], 0.9)
            r_total, r_fine, near = DM.hold_phase_tail(r["cp_corr"], r["total_phase"], fine0, fine1, 0.9, mode, what)
            assert not near
            print(f"mode {mode} f {float(f):+.4e} {name}: spectrum {r_fft:.3f}, correlation {r_corr:.3f}, angle {r_angle:.3f}, total {r_total:.3f}, "
                  f"fine {r_fine:.3f} of their bounds; soft bits: delta {iv['delta'].min():.2e} .. {iv['delta'].max():.2e} counts, "
                  f"{differ:.5%} differ from plain truncation, {ambiguous:.5%} ambiguous")


def test_a_noise_free_frame_is_refused():
    """|re| = |im| on every carrier: the soft bits sit on the 126 / 127 boundary and decide nothing; hold_soft_bits must say so"""
    frame, _ = DM.make_frame(2, np.random.default_rng(1), noise=0.0)
    X = DM.demodulate(frame, 0.0, 2)["X"].astype(np.complex64)
    iv = DM.soft_bit_intervals(X, 2)
    with pytest.raises(AssertionError, match="no noise"):
        DM.hold_soft_bits(np.trunc(iv["w"]), iv)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_fine_frequency_update_and_its_wrap(oracle, mode):
    """update_fine_freq_mode against the float64 update over a table that crosses the wrap point 0.5 x 1.01 / N in both directions,
    once and not at all; the one designed case that sits ON the wrap point (fine = wrap, total = 0) is the only one that may be excused"""
    g = DM.Geometry(mode)
    wrap = 0.5 * 1.01 / g.N
    span = g.L * np.pi                                                  # |total| <= L pi
    table = [(0.0, 0.3 * span, 0.9), (1e-5, -0.7 * span, 0.9), (0.9 * wrap, -0.9 * span, 0.9), (-0.99 * wrap, 0.5 * span, 0.9),
             (0.7 * wrap, -span, 1.0), (-0.7 * wrap, span, 1.0), (0.5 * wrap, 0.01, 0.1), (-wrap * 0.999, 1e-3, 0.9), (0.3 * wrap, 0.0, 0.9),
             (wrap, 0.0, 0.9)]
    worst, excused, wrapped = 0.0, 0, 0
    for fine, total, beta in table:
        fine, total = np.float32(fine), np.float32(total)
        got = oracle.update_fine_freq_mode(mode, fine, total, beta)
        exp, bound, near = DM.fine_freq_update(mode, fine, float(total), 0.0, beta)
        wrapped += abs(float(fine) - float(np.float32(beta)) * float(total) / (g.N * g.L * 2 * np.pi)) > wrap
        if near:
            excused += 1
            continue
        assert abs(float(got) - exp) <= bound, (mode, float(fine), float(total), beta, float(got), exp, bound)
        worst = max(worst, abs(float(got) - exp) / bound)
    print(f"mode {mode}: fine-frequency update at most {worst:.3f} of its bound; {wrapped} cases wrap, {excused} excused")
    assert excused <= 1 and wrapped >= 4
    if mode == 1:                                                       # the mode I entry point is the same function
        assert oracle.update_fine_freq(np.float32(1e-5), np.float32(-0.7 * span)) == oracle.update_fine_freq_mode(1, 1e-5, np.float32(-0.7 * span), 0.9)


@pytest.mark.parametrize("fmt", ["raw_u8", "raw_s8", "raw_s16l"])
def test_capture_decoding_equals_the_oracles_reader(oracle, fmt):
    """the model's own statement of the three fused capture formats against the reader the oracle is pinned to, every code"""
    dtype = DM.CAPTURE[fmt][0]
    codes = np.arange(np.iinfo(dtype).min, np.iinfo(dtype).max + 1).astype(dtype)
    raw = codes.view(np.uint8)
    got = DM.decode_capture(raw, fmt).view(np.float32)
    assert np.array_equal(got.view(np.uint32), oracle.iq_convert(raw, oracle.IQ_MODES.index(fmt)).view(np.uint32))
