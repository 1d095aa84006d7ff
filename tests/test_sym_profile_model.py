"""CPU: the symbol noise profile (include/dabgpu.h, "Symbol noise profile") -- the numpy float32 model of tests/sym_profile_model.py
against the compiled csrc/sym_profile_core.h bit for bit (random products, bursts, NaN and infinity rows, zeros, denormals), the two
constants as the nearest floats, the float32 steps against the float64 model inside the bound derived in that file's head (the
cancellation of step 2 is the term that counts), and a float64 Monte Carlo of one row: unbiased where decisions are right, monotone in
SNR and in burst power, the deviation the first-order figure."""
import math
from fractions import Fraction

import numpy as np
import pytest

import sym_profile_model as M

F32 = np.float32
SEEDS = range(9300, 9364)                                # 64 seeds, 8 rows each
SNRS_DB = (-10.0, 0.0, 6.0, 12.0, 20.0, 30.0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("sym_profile_host_model"))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def assert_frames_equal(got, want, what):
    for name in ("symbol_weight", "symbol_noise"):
        assert same_bits(got[name], want[name]), (what, name)
    assert same_bits(got["ref_noise"], want["ref_noise"]) and int(got["valid"]) == int(want["valid"]), what


def test_constants_are_the_nearest_floats(host):
    got = F32(host.sypm_k1536())
    assert got.view(np.uint32) == M.K1536.view(np.uint32)
    for other in (np.nextafter(got, F32(0)), np.nextafter(got, F32(1))):
        assert abs(Fraction(float(other)) - Fraction(1, 1536)) >= abs(Fraction(float(got)) - Fraction(1, 1536))
    got = F32(host.sypm_rsqrt2())
    assert got.view(np.uint32) == M.RSQRT2.view(np.uint32)
    for other in (np.nextafter(got, F32(0)), np.nextafter(got, F32(1))):                # 1 / sqrt 2: compare squares with 1 / 2, exactly
        mid = (Fraction(float(other)) + Fraction(float(got))) / 2
        assert (mid * mid > Fraction(1, 2)) == (other > got)


def test_owner_order_covers_every_carrier_once():
    assert sorted(M.owner_order().reshape(-1).tolist()) == list(range(1536))


def test_host_model_equals_numpy_model_on_random_products(host):
    rng = np.random.Generator(np.random.PCG64(9201))
    for snr, burst in ((30.0, None), (12.0, (20, 3, 6.0)), (9.0, (0, 1, 12.0)), (-5.0, (60, 16, 0.0)), (12.0, (10, 50, 6.0))):
        d = M.frame_products(rng, snr, burst=burst)
        S = M.sums(d)
        hS = M.host_sums(host, d)
        assert all(same_bits(x, y) for x, y in zip(hS, S)), (snr, burst)
        qa, R = M.figures(*S)
        hqa, hR = M.host_figures(host, *S)
        assert same_bits(hqa, qa) and same_bits(hR, R) and (qa > 0).all()
        for x in (qa, R):
            assert same_bits(M.host_median(host, x), M.median(x))
        want = M.frame(d)
        assert want["valid"] == 1
        assert_frames_equal(M.host_frame(host, d), want, (snr, burst))
        assert_frames_equal(M.host_frame(host, d, entry="dabgpu_sym_profile_rows_host"), want, (snr, burst, "ABI"))
    # plain Gaussian products over twelve decades of scale per row
    d = ((rng.standard_normal((75, 1536)) + 1j * rng.standard_normal((75, 1536))) * 10.0 ** rng.uniform(-6, 6, 75)[:, None]).astype(np.complex64)
    assert_frames_equal(M.host_frame(host, d), M.frame(d), "decades")
    assert M.frame(d)["valid"] == 1


def test_median_ties_break_by_row(host):
    x = np.zeros(75, F32)
    x[40:] = 1.0                                                                         # rank 37 is row 37 of the zeros
    assert M.median(x) == 0 and M.host_median(host, x) == 0
    x[30:] = 1.0                                                                         # 30 zeros: rank 37 is among the ones
    assert M.median(x) == 1 and M.host_median(host, x) == 1
    rng = np.random.Generator(np.random.PCG64(9206))
    for _ in range(20):
        x = rng.integers(0, 5, 75).astype(F32)
        assert M.host_median(host, x) == M.median(x) == np.sort(x)[37]


def test_at_least_38_rows_have_weight_one_always(host):
    rng = np.random.Generator(np.random.PCG64(9202))
    for snr, burst in ((30.0, None), (12.0, (5, 30, 9.0)), (0.0, (40, 36, 3.0)), (12.0, (0, 76, 6.0)), (20.0, (37, 1, 20.0))):
        f = M.host_frame(host, M.frame_products(rng, snr, burst=burst))
        assert f["valid"] == 1 and int((f["symbol_weight"] == 1).sum()) >= 38, (snr, burst)
        assert (f["symbol_weight"] > 0).all() and (f["symbol_weight"] <= 1).all()
        assert f["ref_noise"] == M.median(f["symbol_noise"])


def test_burst_rows_are_weighed_down_and_monotone_in_burst_power(host):
    """a 3-symbol burst from OFDM symbol 20: products 19 .. 22 hear it (19 and 22 with one symbol each); the weight of the rows inside falls
    as the burst grows, and the rows well outside stay at 1 or next to it"""
    inside, last = np.arange(20, 22), None
    for is_db in (0.0, 3.0, 6.0, 9.0, 12.0):
        rng = np.random.Generator(np.random.PCG64(9203))                                # the same signal and noise at every power
        f = M.host_frame(host, M.frame_products(rng, 12.0, burst=(20, 3, is_db)))
        v = f["symbol_weight"]
        assert f["valid"] == 1 and (v[inside] < 0.5).all(), (is_db, v[18:24])
        assert (np.delete(v, np.arange(19, 23)) > M.clean_row_floor(12.0)).all()
        assert v[19] < 1 and v[22] < 1                                                   # the edge rows: one of their two symbols is hit
        if last is not None:
            assert (v[inside] < last).all(), is_db
        last = v[inside]


def test_nan_and_infinity_rows(host):
    rng = np.random.Generator(np.random.PCG64(9204))
    d = M.frame_products(rng)
    d[10, 100] = complex(np.nan, 1.0)
    d[20, 200] = complex(np.inf, 0.0)
    d[30, 300] = complex(2.0e38, 2.0e38)                      # S2 overflows
    d[40, 400] = complex(-np.inf, np.nan)
    want = M.frame(d)
    assert_frames_equal(M.host_frame(host, d), want, "bad rows")
    bad = [10, 20, 30, 40]
    assert want["valid"] == 1 and not want["symbol_weight"][bad].any() and np.isinf(want["symbol_noise"][bad]).all()
    good = np.delete(np.arange(75), bad)
    assert np.isfinite(want["symbol_noise"][good]).all() and (want["symbol_weight"][good] > M.clean_row_floor(15.0)).all()
    assert int((want["symbol_weight"] == 1).sum()) >= 38
    # 37 bad rows: the medians are still finite rows (they rank last); 38: the reference is infinite and the frame is skipped
    d = M.frame_products(rng)
    d[:37, 7] = np.nan
    want = M.frame(d)
    assert_frames_equal(M.host_frame(host, d), want, "37 bad rows")
    assert want["valid"] == 1 and not want["symbol_weight"][:37].any() and (want["symbol_weight"][37:] > 0).all()
    d[37, 7] = np.inf
    want = M.frame(d)
    assert_frames_equal(M.host_frame(host, d), want, "38 bad rows")
    assert want["valid"] == 0 and not want["symbol_weight"].any() and not want["symbol_noise"].any() and want["ref_noise"] == 0


def test_skipped_frames(host):
    z = np.zeros((75, 1536), np.complex64)
    assert_frames_equal(M.host_frame(host, z), M.frame(z), "all zero")
    f = M.host_frame(host, z)
    assert f["valid"] == 0 and not f["symbol_weight"].any() and not f["symbol_noise"].any() and f["ref_noise"] == 0
    assert M.host_frame(host, z, entry="dabgpu_sym_profile_rows_host")["valid"] == 0
    skipped = M.host_frame(host, None, sync_ok=False)                                   # the products are not even looked at
    assert_frames_equal(skipped, M.frame(None, sync_ok=False), "refused")
    assert skipped["valid"] == 0 and not skipped["symbol_weight"].any()
    assert host.dabgpu_sym_profile_rows_host(None, None, None, None) == -1
    # denormal products: the reference is below the normal range
    d = np.full((75, 1536), complex(1.0e-41, -1.0e-42), np.complex64)
    assert_frames_equal(M.host_frame(host, d), M.frame(d), "denormal")
    # squares below the normal range, sums above it
    d = np.full((75, 1536), complex(1.0e-20, 3.0e-20), np.complex64)
    d[::2] *= 2
    assert_frames_equal(M.host_frame(host, d), M.frame(d), "small")


def test_noise_free_frame(host):
    """unit-modulus steps at one amplitude per carrier: |re| = |im| up to rounding, SD is rounding alone and qa a few ulp of P; the
    weights stay finite through the floor q_ref 2^-20"""
    rng = np.random.Generator(np.random.PCG64(9207))
    amp = M.ripple() * 2.0e5
    d = (amp[None, :] * np.exp(1j * math.pi * (rng.integers(0, 4, (75, 1536)) * 0.5 + 0.25))).astype(np.complex64)
    want = M.frame(d)
    assert_frames_equal(M.host_frame(host, d), want, "noise free")
    if want["valid"]:
        assert np.isfinite(want["symbol_weight"]).all() and (want["symbol_weight"] >= F32(2.0 ** -21)).all()


def test_float32_keeps_the_derived_bound(host):
    rng = np.random.Generator(np.random.PCG64(9205))
    worst = dict(qa=0.0, R=0.0, q=0.0, v=0.0)
    for snr, a, burst in ((30.0, 2.0e5, None), (30.0, 2.0e5, (20, 3, 6.0)), (12.0, 3.0e5, (20, 3, 6.0)), (0.0, 1.0e3, (50, 8, 9.0)), (-10.0, 7.0, None)):
        d = M.frame_products(rng, snr, a, burst)
        f64 = M.frame64(d)
        b_qa, b_R, b_q = M.bounds64(f64)
        qa, R = M.host_figures(host, *M.host_sums(host, d))
        f = M.host_frame(host, d)
        e_qa, e_R = np.abs(qa.astype(np.float64) - f64["qa"]), np.abs(R.astype(np.float64) - f64["R"])
        e_q = np.abs(f["symbol_noise"].astype(np.float64) - f64["q"])
        assert (e_qa <= b_qa).all() and (e_R <= b_R).all() and (e_q <= b_q).all() and abs(float(f["ref_noise"]) - f64["q_ref"]) <= b_q
        b_v = f64["v"] * (b_q / f64["q_ref"] + b_q / f64["q"] + 4 * M.U)
        e_v = np.abs(f["symbol_weight"].astype(np.float64) - f64["v"])
        assert (e_v <= b_v).all()
        for name, e, b in (("qa", e_qa, b_qa), ("R", e_R, b_R), ("q", e_q, b_q), ("v", e_v, b_v)):
            worst[name] = max(worst[name], float((e / b).max()))
    print("largest float32 - float64 difference over its bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.fixture(scope="module")
def sweep():
    return {snr: M.monte_carlo(snr, SEEDS) for snr in SNRS_DB}


def test_monte_carlo_of_one_row(sweep):
    """E[qa] / q and the deviation of one row's figure at mean carrier SNR -10 .. 30 dB over the ripple (the table of DESIGN 4.31)"""
    for snr in SNRS_DB:
        ratio, dev, n = sweep[snr]
        print(f"carrier SNR {snr:5.1f} dB: E[qa] / q = {ratio:.4f}, relative deviation of a row {dev:.4f} ({n} rows)")
    # unbiased where decisions are right: inside five standard errors of the mean
    for snr in (20.0, 30.0):
        ratio, dev, n = sweep[snr]
        assert abs(ratio - 1.0) < 5.0 * dev * ratio / math.sqrt(n), (snr, ratio)
    # monotone: at one channel power more noise reads as more noise, and a larger share of it is seen as the SNR rises
    q_hat = [sweep[snr][0] / 10.0 ** (snr / 10.0) for snr in SNRS_DB]
    assert all(x > y for x, y in zip(q_hat, q_hat[1:]))
    ratios = [sweep[snr][0] for snr in SNRS_DB]
    assert all(x < y + 5.0 * sweep[s][1] / math.sqrt(sweep[s][2]) for x, y, s in zip(ratios, ratios[1:], SNRS_DB[1:]))
    assert all(0.0 < r <= 1.0 + 5.0 * sweep[s][1] / math.sqrt(sweep[s][2]) for r, s in zip(ratios, SNRS_DB))
    # the first-order deviation of the head: sqrt(2 / 1536) times the ripple's sqrt(E[a^2]) / E[a]; the estimate of a deviation from n
    # draws has relative standard error 1 / sqrt(2 n): five of them
    a = M.ripple()
    first_order = M.FIRST_ORDER_DEVIATION * math.sqrt((a * a).mean()) / a.mean()
    n = sweep[30.0][2]
    assert abs(sweep[30.0][1] / first_order - 1.0) < 5.0 / math.sqrt(2.0 * n) + 2.0 / 1000.0         # (+ the q / a terms left out: 1e-3 at 30 dB)
