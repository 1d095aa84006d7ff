"""CPU: the decision-directed noise profile (include/dabgpu.h, "Decision-directed noise profile") -- the numpy float32 model of
tests/dd_profile_model.py against the compiled csrc/dd_profile_core.h bit for bit (random products, NaN, infinity, zeros, denormals, a
noise-free frame), the two constants as the nearest floats, the float32 steps against the float64 model inside the bound derived in that
file's head, and a float64 Monte Carlo of one band against what the derivation there gives: the finite-sample mean at high SNR,
monotony, and a deviation below the NULL profile's."""
import math
from fractions import Fraction

import numpy as np
import pytest

import dd_profile_model as M
import noise_profile_model as PM

F32 = np.float32
SEEDS = range(9100, 9164)                                # 64 seeds, 16 bands each
SNRS_DB = (-10.0, 0.0, 6.0, 12.0, 20.0, 30.0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("dd_profile_host_model"))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def frame_products(rng, snr_db=15.0, a=3.0e5):
    """one frame's products in float32: the band model at every carrier, channel power a"""
    d, _ = M.band_products(rng, snr_db, M.N_BANDS, a)
    return d.astype(np.complex64)


def assert_frames_equal(got, want, what):
    for name in ("profile", "band_weight", "carrier_noise", "carrier_amplitude"):
        assert same_bits(got[name], want[name]), (what, name)
    assert same_bits(got["mean_noise"], want["mean_noise"]) and int(got["valid"]) == int(want["valid"]), what


def test_constants_are_the_nearest_floats(host):
    for got, model, exact in ((F32(host.ddm_k75()), M.K75, Fraction(1, 75)), (F32(host.ddm_k1()), M.K1, None)):
        assert got.view(np.uint32) == model.view(np.uint32)
        for other in (np.nextafter(got, F32(0)), np.nextafter(got, F32(1))):
            if exact is not None:
                assert abs(Fraction(float(other)) - exact) >= abs(Fraction(float(got)) - exact)
            else:                                           # 1 / (75 sqrt 2): compare squares, 1 / 11250, exactly
                mid = (Fraction(float(other)) + Fraction(float(got))) / 2
                assert (mid * mid > Fraction(1, 11250)) == (other > got)


def test_host_model_equals_numpy_model_on_random_products(host):
    rng = np.random.Generator(np.random.PCG64(9001))
    for snr in (30.0, 9.0, -5.0):
        d = frame_products(rng, snr)
        Q, A = M.carriers(d)
        hQ, hA = M.host_carriers(host, d)
        assert same_bits(hQ, Q) and same_bits(hA, A) and (Q > 0).any()
        aQ, aA = M.host_carriers(host, d, "dabgpu_dd_profile_carriers_host")
        assert same_bits(aQ, Q) and same_bits(aA, A)
    # plain Gaussian products over twelve decades of scale
    d = (rng.standard_normal((75, 1536)) + 1j * rng.standard_normal((75, 1536))) * 10.0 ** rng.uniform(-6, 6, 1536)[None, :]
    Q, A = M.carriers(d.astype(np.complex64))
    hQ, hA = M.host_carriers(host, d.astype(np.complex64))
    assert same_bits(hQ, Q) and same_bits(hA, A)


def test_whole_frames_and_every_path_behind_the_carriers(host):
    rng = np.random.Generator(np.random.PCG64(9002))
    d = frame_products(rng)
    mask = PM.exclude_words(np.r_[rng.choice(1536, 150, replace=False), 12 * 7:12 * 8])          # band 7 wholly excluded
    prev = (rng.uniform(0.5, 2.0, 128) * 1.0e4).astype(F32)
    prev[[3, 90]] = [0.0, np.nan]
    for kw in (dict(), dict(exclude=mask), dict(profile_in=prev, alpha=0.25), dict(exclude=mask, profile_in=prev, alpha=1.0),
               dict(sync_ok=False), dict(sync_ok=False, profile_in=prev, alpha=0.25)):
        assert_frames_equal(M.host_frame(host, d, **kw), M.frame(d, **kw), kw)
    skipped = M.host_frame(host, None, sync_ok=False, profile_in=prev, alpha=0.25)               # the products are not even looked at
    assert same_bits(skipped["profile"], prev) and not skipped["band_weight"].any() and skipped["valid"] == 0
    # the two host forms of the ABI are the same definition
    Q, _ = M.host_carriers(host, d, "dabgpu_dd_profile_carriers_host")
    want = M.frame(d, exclude=mask, profile_in=prev, alpha=0.25)
    got = PM.host_bands(host, Q, mask, prev, 0.25, "dabgpu_noise_profile_bands_host")
    assert same_bits(got[0], want["profile"]) and same_bits(got[1], want["band_weight"]) and same_bits(got[2], want["mean_noise"]) and got[3] == 1


def test_special_values(host):
    rng = np.random.Generator(np.random.PCG64(9003))
    d = frame_products(rng)
    d[10, 100] = complex(np.nan, 1.0)                      # a NaN: Q 0, A NaN, the frame lives on through the other eleven of the band
    d[20, 200] = complex(np.inf, 0.0)                      # an infinity in both sums: inf - inf
    d[30, 300] = complex(2.0e38, 0.0)                      # S2 overflows, S1 does not: Q infinite, the frame is skipped below
    d[:, 400] = 0.0
    d[:, 500] = complex(1.0e-41, -1.0e-42)                 # denormal products
    d[:, 501] = complex(1.0e-20, 1.0e-20)                  # squares below the normal range
    Q, A = M.carriers(d)
    hQ, hA = M.host_carriers(host, d)
    assert same_bits(hQ, Q) and same_bits(hA, A)
    assert Q[100] == 0 and np.isnan(A[100]) and Q[200] == 0 and np.isinf(A[200]) and np.isinf(Q[300]) and Q[400] == 0 and A[400] == 0
    assert_frames_equal(M.host_frame(host, d), M.frame(d), "infinite band")
    assert M.frame(d)["valid"] == 0
    d[30, 300] = 1.0
    f = M.frame(d)
    assert_frames_equal(M.host_frame(host, d), f, "NaN and infinity that give Q = 0")
    assert f["valid"] == 1 and np.isfinite(f["band_weight"]).all()
    z = np.zeros((75, 1536), np.complex64)
    assert_frames_equal(M.host_frame(host, z), M.frame(z), "all zero")
    assert M.frame(z)["valid"] == 0 and not M.host_frame(host, z)["band_weight"].any()


def test_noise_free_frame(host):
    """unit-modulus steps at one amplitude per carrier: rms and projected amplitude are the same number, so Q is 0 or a few ulp of it, and
    the weights stay finite through the floor M 2^-20"""
    rng = np.random.Generator(np.random.PCG64(9004))
    amp = rng.uniform(0.5, 2.0, 1536) * 2.0e5
    d = (amp[None, :] * np.exp(1j * math.pi * (rng.integers(0, 4, (75, 1536)) * 0.5 + 0.25))).astype(np.complex64)
    Q, A = M.carriers(d)
    hQ, hA = M.host_carriers(host, d)
    assert same_bits(hQ, Q) and same_bits(hA, A)
    assert (Q <= 120 * M.U * A).all() and np.allclose(A, amp, rtol=1e-5)
    f = M.frame(d)
    assert_frames_equal(M.host_frame(host, d), f, "noise free")
    if f["valid"]:
        assert np.isfinite(f["band_weight"]).all() and (f["band_weight"] > 0).all()
        assert f["band_weight"].max() <= 1.0001 * 2.0 ** 20 / float(f["mean_noise"])
    e = (amp[None, :] * np.exp(0.25j * math.pi) * np.ones((75, 1))).astype(np.complex64)       # one phase: |re| = |im| up to rounding
    assert_frames_equal(M.host_frame(host, e), M.frame(e), "noise free, one phase")


def test_float32_keeps_the_derived_bound():
    rng = np.random.Generator(np.random.PCG64(9005))
    worst = 0.0
    for snr, a in ((30.0, 2.0e5), (12.0, 3.0e5), (0.0, 1.0e3), (-10.0, 7.0)):
        d = frame_products(rng, snr, a)
        Q, A = M.carriers(d)
        Q64, A64, R64 = M.carriers64(d)
        bound_q = M.BOUND_R * R64 + M.BOUND_A * A64 + M.U * np.abs(R64 - A64)
        assert (np.abs(A.astype(np.float64) - A64) <= M.BOUND_A * A64).all()
        assert (np.abs(Q.astype(np.float64) - Q64) <= bound_q).all()
        worst = max(worst, float((np.abs(Q.astype(np.float64) - Q64) / bound_q).max()))
    print(f"largest |Q32 - Q64| over its bound: {worst:.3f}")


@pytest.fixture(scope="module")
def sweep():
    return {snr: M.monte_carlo(snr, SEEDS) for snr in SNRS_DB}


def test_monte_carlo_of_one_band(sweep):
    """E[q^] / q and the deviation of a band's estimate at carrier SNR -10 .. 30 dB (the table of DESIGN 4.30)"""
    for snr in SNRS_DB:
        ratio, dev, n = sweep[snr]
        print(f"carrier SNR {snr:5.1f} dB: E[q^] / q = {ratio:.4f}, relative deviation of a band {dev:.4f} ({n} bands)")
    # unbiased within the finite-sample term where decisions are right: 1 - 1 / 75, inside five standard errors of the mean
    for snr in (20.0, 30.0):
        ratio, dev, n = sweep[snr]
        assert abs(ratio - M.HIGH_SNR_RATIO) < 5.0 * dev * ratio / math.sqrt(n), (snr, ratio)
    # monotone: at one channel power more noise reads as more noise, and a larger share of it is seen as the SNR rises
    q_hat = [sweep[snr][0] / 10.0 ** (snr / 10.0) for snr in SNRS_DB]
    assert all(x > y for x, y in zip(q_hat, q_hat[1:]))
    ratios = [sweep[snr][0] for snr in SNRS_DB]
    assert all(x < y + 5.0 * sweep[s][1] / math.sqrt(sweep[s][2]) for x, y, s in zip(ratios, ratios[1:], SNRS_DB[1:]))
    assert all(0.0 < r <= 1.0 for r in ratios)
    # steadier than one NULL symbol's band mean at every SNR, and at the first-order figure where decisions are right
    for snr in SNRS_DB:
        assert sweep[snr][1] < M.NULL_DEVIATION, snr
    # (a product shares its symbols with its two neighbours only, and a correlation is at most 1: the variance of the sum is at most
    # three times the independent one)
    first_order = math.sqrt(2.0 / 149.0 / 12.0)
    assert first_order < sweep[30.0][1] < math.sqrt(3.0) * first_order
