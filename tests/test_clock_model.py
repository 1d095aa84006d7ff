"""CPU: the sampling-clock tracker's arithmetic (csrc/clock_core.h compiled for the host) against the independent float64 model of
tests/clock_model.py, inside the bounds derived in that module's docstring.

Recorded here (host model, products() of clock_model.py, 200 ppm, one frame from a zero state): estimate over truth against carrier SNR
    20 dB 1.00   15 dB 0.86   12 dB 0.58   9 dB 0.19   6 dB 0.04
(the two-path channel of products() has carriers 7 dB below the mean; test_under_read_is_monotone_and_the_loop_converges prints the
figures it sees).  Only the order of the curve is asserted, and that the
loop closes what one frame leaves."""
import math

import numpy as np
import pytest

import clock_model as CM

F32 = np.float32
LOOP_FRAMES = 16


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return CM.build_host_model(tmp_path_factory.mktemp("clock_model"))


def test_constants_ppm_round_trip_and_sign(lib):
    assert lib.clkm_lag() == CM.LAG == 32 and lib.clkm_pairs() == CM.N_PAIRS == 110400
    assert lib.clkm_max_slope() == CM.MAX_SLOPE == 22986372498099012
    # ppm -> slope -> ppm: a double holds 53 bits, the slope of 1000 ppm has 55
    for ppm in (0.0, 1.0, -1.0, 0.37, 150.0, -200.0, 999.9, 1000.0, -1000.0, 1e-6):
        s = lib.dabgpu_clock_slope_q64(ppm)
        assert abs(s - CM.slope_q64(ppm)) <= 4 and abs(lib.dabgpu_clock_ppm(s) - ppm) <= 1e-12 * max(1.0, abs(ppm)), ppm
        assert (s > 0) == (ppm > 0) and (s < 0) == (ppm < 0)
    assert lib.dabgpu_clock_slope_q64(float("nan")) == 0
    assert lib.dabgpu_clock_slope_q64(1e30) == 2 ** 63 - 1 and lib.dabgpu_clock_slope_q64(-1e30) == -2 ** 63
    assert abs(lib.dabgpu_clock_slope_q64(1000.0) - CM.MAX_SLOPE) <= 4
    # 100 ppm is 34 degrees at the band edge, the lag sees 1/24 of it
    assert abs(CM.ppm_of(CM.slope_q64(100.0)) - 100.0) < 1e-9 and abs(100.0 * CM.CYCLES_PER_PPM * 768 * 360 - 34.45) < 0.01


def test_angle_polynomial_stays_inside_its_bound(lib):
    # every float32 t on a grid of 2^22 + 1 points of [-1, 1], the ends, one ulp beyond (the quotient can reach it) and the small values
    t = np.concatenate([np.linspace(-1.0, 1.0, (1 << 22) + 1), [np.nextafter(F32(1), F32(2)), -np.nextafter(F32(1), F32(2))],
                        2.0 ** -np.arange(1, 60), -2.0 ** -np.arange(1, 60), [0.0]]).astype(F32)
    got = CM.host_atan_cycles(lib, t).astype(np.float64)
    want = np.arctan(t.astype(np.float64)) / (2.0 * math.pi)
    err = np.abs(got - want)
    # the approximation alone: the float32 coefficients evaluated in float64
    z = t.astype(np.float64) ** 2
    p = np.zeros_like(z)
    for c in CM.ATAN_COEFFS[::-1]:
        p = p * z + float(F32(c))
    approx = np.abs(p * t.astype(np.float64) - want).max()
    # Horner in float32: six fused steps and two products, each within u of a value below sum |c_i| = 0.272
    rounding = 8 * CM.U * sum(abs(c) for c in CM.ATAN_COEFFS)
    print(f"atan polynomial: worst {err.max():.3e} cycles = {err.max() * 2 * math.pi:.3e} rad; approximation {approx:.3e}, rounding bound {rounding:.3e}")
    assert approx + rounding <= CM.ATAN_BOUND_CYCLES
    assert err.max() <= approx + rounding
    assert err.max() * 2.0 * math.pi < CM.ATAN_LIMIT_RAD
    assert np.array_equal(got[t == 0], np.zeros(int((t == 0).sum()))) and np.array_equal(CM.host_atan_cycles(lib, -t), -CM.host_atan_cycles(lib, t))


def test_fold_is_exact(lib):
    rng = np.random.default_rng(5)
    p = rng.standard_normal((4000, 2)).astype(F32)
    p[:8] = [[1, 1], [1, -1], [-1, 1], [-1, -1], [0, 0], [0, 2], [0, -2], [-3, 0]]                     # ties and axes
    want = CM.fold(p[:, 0].astype(np.float64) + 1j * p[:, 1].astype(np.float64))
    for i in range(len(p)):
        out = np.zeros(2, F32)
        lib.clkm_fold(p[i].ctypes.data, out.ctypes.data)
        assert out[0] == want[i].real and out[1] == want[i].imag and out[0] >= abs(out[1]), (p[i], out)
        assert {abs(out[0]), abs(out[1])} == {abs(p[i, 0]), abs(p[i, 1])}                          # signs and swaps only


@pytest.mark.parametrize("ppm, prior_ppm", [(0.0, 0.0), (3.0, 0.0), (-50.0, 0.0), (150.0, 0.0), (200.0, 0.0), (-200.0, 0.0), (900.0, 0.0),
                                            (200.0, 180.0), (-400.0, -350.0), (150.0, 400.0), (0.0, 999.0)])
def test_noiseless_ramp_is_estimated_within_the_float32_bound(lib, ppm, prior_ppm):
    rng = np.random.default_rng(int(abs(ppm) * 10 + abs(prior_ppm)) + 1)
    dq = CM.products(rng, ppm, amplitude=37.0)
    s_in = CM.slope_q64(prior_ppm)
    est = CM.estimate(dq, s_in)
    assert est["valid"] and est["dropped"] == 0 and est["min_margin_rad"] > math.radians(5.0)         # both sides fold alike
    got = CM.host_estimate(lib, dq, s_in)
    bound = CM.residual_bound_cycles(est, prior_ppm != 0.0)
    err = abs(got["residual"] / 2.0 ** 59 - est["residual_cycles"])
    truth = (ppm - prior_ppm) * CM.CYCLES_PER_PPM * CM.LAG
    print(f"{ppm} ppm after {prior_ppm}: residual {got['residual'] / 2.0 ** 59:.9f} cycles, float64 {est['residual_cycles']:.9f}, truth {truth:.9f}; "
          f"error {err:.2e}, bound {bound:.2e} cycles = {bound * 2 * math.pi / CM.RAD_PER_PPM:.3f} ppm")
    assert got["valid"] == 1 and err <= bound
    # ... and the float64 model against the truth: the products are float32 (an angle within sqrt(2) u each, twice in a lag product)
    assert abs(est["residual_cycles"] - truth) <= 2.0 * math.sqrt(2.0) * CM.U / (2.0 * math.pi) + (2.0 ** -24 if prior_ppm else 0.0)
    # the update at gain 1 is the clamped sum, exactly; the sum A is within its bound as well
    assert got["slope"] == CM.clamp(CM.clamp(s_in) + got["residual"])
    assert abs(complex(got["corr"][0], got["corr"][1]) - est["A"]) <= est["sum_abs"] * (CM.LAG_BOUND + CM.ROTATION_BOUND + 2 * CM.SUM_ROUNDINGS * CM.U)
    assert (got["residual"] > 0) == (truth > 0) or abs(truth) < bound                                  # the sign is the ramp's
    # the library's host form is the same statements
    s, corr = CM.C.c_int64(0), np.zeros(2, F32)
    assert lib.dabgpu_clock_estimate_host(CM._frame(dq).ctypes.data, s_in, 1.0, CM.C.byref(s), corr.ctypes.data) == 1
    assert s.value == got["slope"] and corr.tobytes() == got["corr"].tobytes()


def test_gain_and_clamp(lib):
    rng = np.random.default_rng(11)
    dq = CM.products(rng, 200.0)
    full = CM.host_estimate(lib, dq, 0, 1.0)
    for gain in (0.5, 0.25, 0.3, 1e-3):
        e = CM.host_estimate(lib, dq, 0, gain)
        assert e["residual"] == full["residual"] and e["valid"] == 1                                  # the residual is reported without the gain
        assert abs(e["slope"] - gain * full["residual"]) <= 2.0 * CM.U * abs(full["residual"]) + 1, gain
    assert CM.host_estimate(lib, dq, 0, 0.5)["slope"] * 2 == full["residual"]                         # a power of two is exact
    # the clamp: at the maximum a positive residual leaves the maximum, a state beyond it is taken as the maximum
    top = CM.host_estimate(lib, CM.products(rng, 1100.0), CM.MAX_SLOPE)
    assert top["valid"] == 1 and top["residual"] > 0 and top["slope"] == CM.MAX_SLOPE
    wild = CM.host_estimate(lib, CM.products(rng, 1000.0), 2 ** 62)
    assert wild["valid"] == 1 and abs(wild["residual"]) < CM.slope_q64(0.5) and abs(wild["slope"] - CM.MAX_SLOPE) <= abs(wild["residual"])
    low = CM.host_estimate(lib, CM.products(rng, -1100.0), -CM.MAX_SLOPE)
    assert low["slope"] == -CM.MAX_SLOPE and low["residual"] < 0
    for gain in (0.0, -1.0, 1.5, float("nan"), float("inf")):
        assert lib.dabgpu_clock_estimate_host(CM._frame(dq).ctypes.data, 0, gain, None, None) == -1
    assert lib.dabgpu_clock_estimate_host(None, 0, 1.0, None, None) == -1 and lib.dabgpu_clock_derotate_host(None, None, 0) == -1


def test_bad_pairs_are_dropped_and_counted(lib):
    rng = np.random.default_rng(12)
    dq = CM.products(rng, 120.0).reshape(CM.N_SYMBOLS, CM.N_CARRIERS).copy()
    dq[3, 100] = complex(np.nan, 1.0)          # carrier 100: the low end of (100, 132) and the high end of (68, 100)
    dq[9, 10] = complex(1.0, np.inf)           # carrier 10: the low end of (10, 42) only
    dq[70, 760] = complex(-np.inf, 0.0)        # carrier 760: the high end of (728, 760) only
    dq[20, 1535] = np.nan                      # the high end of (1503, 1535)
    dq[21, 752:768] = np.nan                   # 16 carriers that are high ends only
    est = CM.estimate(dq, 0)
    assert est["dropped"] == 2 + 1 + 1 + 1 + 16
    corr, n = CM.host_sum(lib, dq, 0)
    assert n == est["dropped"] and np.isfinite(corr).all()
    got = CM.host_estimate(lib, dq, 0)
    assert got["valid"] == 1 and abs(got["residual"] / 2.0 ** 59 - est["residual_cycles"]) <= CM.residual_bound_cycles(est, False)
    # a NaN row with a prior: the rotation does not hide it
    assert CM.host_sum(lib, dq, CM.slope_q64(100.0))[1] == est["dropped"]
    # half of the pairs gone: the frame is skipped and keeps its state (38 rows are 55936 of 110400 pairs, 37 rows are 54464)
    for rows, valid in ((37, 1), (38, 0)):
        bad = dq.copy()
        bad[:rows] = np.nan
        e = CM.host_estimate(lib, bad, 12345)
        assert e["valid"] == valid
        if not valid:
            assert e["slope"] == 12345 and e["residual"] == 0 and e["corr"].tobytes() == np.zeros(2, F32).tobytes()


def test_skipped_frames_keep_their_state(lib):
    zeros = np.zeros((CM.N_SYMBOLS, CM.N_CARRIERS), np.complex64)
    for s_in in (0, 777, -CM.MAX_SLOPE, 2 ** 62):                                                      # as it came, not clamped
        e = CM.host_estimate(lib, zeros, s_in)
        assert e["valid"] == 0 and e["slope"] == s_in and e["residual"] == 0 and e["corr"].tobytes() == bytes(8)
        e = CM.host_estimate(lib, None, s_in, sync_ok=False)                                           # not read at all
        assert e["valid"] == 0 and e["slope"] == s_in and e["residual"] == 0 and e["corr"].tobytes() == bytes(8)
    # a sum that points backwards (every lag product at 180 degrees cannot happen after the fold; a tiny frame can underflow instead)
    tiny = np.full((CM.N_SYMBOLS, CM.N_CARRIERS), 1e-30 + 0j, np.complex64)
    assert CM.host_estimate(lib, tiny, 5)["valid"] == 0


@pytest.mark.parametrize("ppm", [0.7, -200.0, 1000.0])
def test_derotation_stays_within_its_bound(lib, ppm):
    rng = np.random.default_rng(21)
    dq = CM.products(rng, ppm, snr_db=15.0, amplitude=3.0)
    slope = CM.slope_q64(ppm)
    got = CM.host_derotate(lib, dq, slope).astype(np.complex128)
    want = CM.derotate(dq, slope)
    bound = np.abs(dq.astype(np.complex128)) * CM.ROTATION_BOUND * (1.0 + 2.0 * CM.U)
    ratio = (np.abs(got - want) / bound).max()
    print(f"de-rotation at {ppm} ppm: worst error {ratio:.3f} of the bound")
    assert ratio <= 1.0
    assert CM.host_derotate(lib, dq, slope, in_place=True).tobytes() == CM.host_derotate(lib, dq, slope).tobytes()
    # de-rotating a ramp by its own slope leaves the decisions' diagonal: the estimate of what is left is zero within the noise floor
    left = CM.host_estimate(lib, got.astype(np.complex64), 0)
    assert abs(CM.ppm_of(left["residual"])) < 5.0 * CM.noise_floor_ppm(15.0) + 0.5
    # the library's host form is the same statements
    out = np.zeros(CM.N_SYMBOLS * CM.N_CARRIERS, np.complex64)
    assert lib.dabgpu_clock_derotate_host(CM._frame(dq).ctypes.data, out.ctypes.data, slope) == 0
    assert out.tobytes() == CM.host_derotate(lib, dq, slope).tobytes()


def test_slope_zero_is_the_identity_bit_for_bit(lib):
    rng = np.random.default_rng(22)
    dq = CM.products(rng, 50.0, snr_db=10.0).reshape(-1).copy()
    raw = dq.view(np.uint32)
    raw[:6] = [0x7FC01234, 0xFFC00001, 0x80000000, 0x7F800000, 0x00000001, 0x807FFFFF]                 # NaN payloads, -0, infinity, subnormals
    assert CM.host_derotate(lib, dq, 0).tobytes() == dq.tobytes()
    assert CM.host_derotate(lib, dq, 0, in_place=True).tobytes() == dq.tobytes()
    assert CM.host_derotate(lib, dq, 1).tobytes() != dq.tobytes()                                      # the smallest slope is a rotation (NaN * 1)


def test_under_read_is_monotone_and_the_loop_converges(lib):
    truth = 200.0
    ratios = []
    for snr in (20.0, 15.0, 12.0, 9.0, 6.0):
        rng = np.random.default_rng(100 + int(snr))
        e = CM.host_estimate(lib, CM.products(rng, truth, snr_db=snr), 0)
        assert e["valid"] == 1
        ratios.append(CM.ppm_of(e["slope"]) / truth)
    print("estimate over truth at 20, 15, 12, 9, 6 dB:", " ".join(f"{r:.3f}" for r in ratios))
    assert all(a > b for a, b in zip(ratios, ratios[1:])) and ratios[0] <= 1.0 + 5.0 * CM.noise_floor_ppm(20.0) / truth and ratios[-1] > 0.0
    # the loop: fresh noise every frame, the state carried, one pass per frame, gain 1.  What is left of the ramp, |truth - state|,
    # shrinks from frame to frame while it is told from noise (five deviations of one frame's estimate), and stays below that afterwards;
    # the residual the estimator reports is that remainder under-read, and ends below where it began
    for snr in (12.0, 9.0):
        rng = np.random.default_rng(200 + int(snr))
        model = CM.HostModel(lib)
        res, left = [], [truth]
        for _ in range(LOOP_FRAMES):
            _, e = model.track(CM.products(rng, truth, snr_db=snr))
            assert e["valid"] == 1
            res.append(abs(CM.ppm_of(e["residual"])))
            left.append(abs(truth - CM.ppm_of(model.slope)))
        told = 5.0 * CM.noise_floor_ppm(snr)
        print(f"{snr} dB: |residual| {' '.join(f'{r:.1f}' for r in res)} ppm; left {' '.join(f'{r:.1f}' for r in left)}; told from noise above {told:.1f}")
        assert all(b < a if a > told else b < told for a, b in zip(left, left[1:])) and left[-1] < told
        assert res[-1] < told < res[0]
