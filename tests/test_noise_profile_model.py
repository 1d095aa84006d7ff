"""CPU: the noise profile and the banded combiner (include/dabgpu.h, "Noise profile", "Banded receive diversity") -- the numpy float32
model of tests/noise_profile_model.py against the compiled csrc/noise_profile_core.h bit for bit, R[n] as the nearest floats, the float32
steps against a float64 model inside the bound derived in that file's head, and the statistics under white noise against their derived
values: band means, one frame's deviation, the smoothed deviation, the mean against the estimator's noise power, and TII carriers that
are excluded."""
import math
from fractions import Fraction

import numpy as np
import pytest

import diversity_model as DM
import noise_model as NM
import noise_profile_model as M
import tii_model as TM

F32 = np.float32
N_FRAMES = 256
S2 = 2.5
TXS = [(11, 5, 1.0), (40, 17, 1.0), (0, 0, 1.0), (69, 23, 1.0)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("noise_profile_host_model"))


@pytest.fixture(scope="module")
def noise_frames():
    """N_FRAMES seeded NULL periods of white noise, power S2 per complex sample (one set, shared, read only)"""
    rng = np.random.Generator(np.random.PCG64(8300))
    x = math.sqrt(S2 / 2.0) * (rng.standard_normal((N_FRAMES, M.NB_NULL)) + 1j * rng.standard_normal((N_FRAMES, M.NB_NULL)))
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def noise_powers(noise_frames):
    """their carrier powers, float64 -> float32 [N_FRAMES][1536], without and with four TII transmitters on the air"""
    tii = TM.null_period(np.ones(2048, np.complex128), TXS)
    plain = np.array([M.carrier_powers64(f, 0) for f in noise_frames]).astype(F32)
    lit = np.array([M.carrier_powers64(f + tii, 0) for f in noise_frames]).astype(F32)
    plain.setflags(write=False)
    lit.setflags(write=False)
    return plain, lit


def tii_mask():
    return M.exclude_words(M.carrier_index(np.concatenate([TM.carriers(p, c) for p, c, _ in TXS])))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def test_count_reciprocals_are_the_nearest_floats(host):
    for n in range(1, 13):
        r = F32(host.npm_count_reciprocal(n))
        assert r.view(np.uint32) == M.R[n].view(np.uint32)
        exact = Fraction(1, n)
        d = abs(Fraction(float(r)) - exact)
        for other in (np.nextafter(r, F32(0)), np.nextafter(r, F32(2))):
            assert abs(Fraction(float(other)) - exact) >= d, n
    assert [host.npm_carrier_bin(c) for c in (0, 767, 768, 1535)] == [1280, 2047, 1, 768]
    assert np.array_equal([host.npm_carrier_bin(c) for c in range(1536)], M.carrier_bins())
    assert M.carrier_index(-768) == 0 and M.carrier_index(-1) == 767 and M.carrier_index(1) == 768 and M.carrier_index(768) == 1535


def test_exclusion_words(host):
    import dabgpu
    want = tii_mask()
    got = dabgpu.noise_profile_exclude([(p, c) for p, c, _ in TXS])
    assert np.array_equal(got, want) and sum(bin(int(w)).count("1") for w in got) == 32 * len(TXS)
    assert not dabgpu.noise_profile_exclude([]).any()
    for bad in ([(70, 0)], [(0, 24)]):
        with pytest.raises(dabgpu.DabGpuError):
            dabgpu.noise_profile_exclude(bad)
    # a band's twelve bits out of the words, every band, a random table
    rng = np.random.default_rng(8301)
    words = rng.integers(0, 1 << 32, 48, dtype=np.uint64).astype(np.uint32)
    ex = M.excluded(words).reshape(128, 12)
    for b in range(128):
        assert host.npm_band_mask(words.ctypes.data, b) == sum(int(ex[b, i]) << i for i in range(12)), b
    assert host.npm_band_mask(None, 5) == 0


def cases(rng):
    """(carrier powers, exclude, profile_in, alpha) that take every path of steps 2 to 5"""
    Cp = (rng.exponential(1.0, 1536) * 5000.0).astype(F32)
    mask = M.exclude_words(rng.choice(1536, 200, replace=False))
    band7 = M.exclude_words(np.arange(84, 96))                                        # band 7 fully excluded: its mask is ignored
    prev = (rng.exponential(1.0, 128) * 2.5).astype(F32)
    mixed = prev.copy()
    mixed[::4], mixed[1::8], mixed[2::16], mixed[3::32] = 0.0, np.nan, np.inf, -1.0
    out = [(Cp, None, None, 1.0), (Cp, mask, None, 1.0), (Cp, band7, None, 1.0), (Cp, np.full(48, 0xFFFFFFFF, np.uint32), None, 1.0),
           (Cp, None, prev, 0.25), (Cp, mask, prev, 1.0), (Cp, mask, mixed, 0.25), (Cp, None, np.zeros(128, F32), 0.25),
           (Cp, None, np.full(128, np.nan, F32), 0.25)]
    quiet = Cp.copy()
    quiet[240:360] = 0.0                                                              # bands without noise: the cap
    out.append((quiet, None, None, 1.0))
    for bad in (np.nan, np.inf):
        c = Cp.copy()
        c[700] = bad
        out.append((c, None, prev, 0.25))
    out.append((np.zeros(1536, F32), None, prev, 0.25))                              # an all-zero NULL: the state decays, M stays normal
    out.append((np.zeros(1536, F32), None, None, 1.0))                               # ... and without a state M = 0: skipped
    out.append((np.full(1536, 1e-42, F32), None, None, 1.0))                         # a mean below the normal range
    out.append((np.full(1536, 3e38, F32), None, None, 1.0))                          # a sum that overflows
    return out


def test_model_equals_compiled_header(host):
    import dabgpu
    rng = np.random.default_rng(8302)
    n_valid = 0
    for i, (Cp, ex, pin, alpha) in enumerate(cases(rng)):
        want = M.bands(Cp, ex, pin, alpha)
        for entry in ("npm_frame_bands", "dabgpu_noise_profile_bands_host"):
            got = M.host_bands(host, Cp, ex, pin, alpha, entry)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2], want[2]) and got[3] == want[3], (i, entry)
        py = dabgpu.noise_profile_bands_host(Cp, ex, pin, alpha)
        assert same_bits(py[0], want[0]) and same_bits(py[1], want[1]) and py[3] == want[3]
        n_valid += want[3]
        if not want[3]:                                                               # skipped: zeros, the state kept
            assert not want[1].any() and want[2] == 0
            assert same_bits(want[0], np.zeros(128, F32) if pin is None else pin)
    assert n_valid == 11 and i == 15
    # all excluded = nothing excluded; a fully excluded band = that band not excluded
    Cp = cases(rng)[0][0]
    assert same_bits(M.bands(Cp, np.full(48, 0xFFFFFFFF, np.uint32))[0], M.bands(Cp)[0])
    assert same_bits(M.bands(Cp, M.exclude_words(np.arange(84, 96)))[0], M.bands(Cp)[0])
    # the cap: a band without noise weighs 2^20 / M
    quiet = M.bands(cases(rng)[9][0])
    assert quiet[3] == 1 and (quiet[0][20:30] == 0).all() and np.allclose(quiet[1][20:30] * quiet[2], 2.0 ** 20, rtol=2 ** -22)
    for alpha in (0.0, -0.5, 1.0000001, np.nan, np.inf):
        assert host.dabgpu_noise_profile_bands_host(Cp.ctypes.data, None, None, F32(alpha), None, None, None) == -1
    assert host.dabgpu_noise_profile_bands_host(None, None, None, F32(1.0), None, None, None) == -1
    # in place
    state = cases(rng)[4][2].copy()
    want = M.bands(Cp, None, state, 0.25)[0]
    assert host.dabgpu_noise_profile_bands_host(Cp.ctypes.data, None, state.ctypes.data, F32(0.25), state.ctypes.data, None, None) == 1
    assert same_bits(state, want)


def test_tree_mean_and_branch_weight(host):
    import dabgpu
    rng = np.random.default_rng(8303)
    for _ in range(20):
        v = (rng.exponential(1.0, 128) * 10.0 ** rng.uniform(-30, 30)).astype(F32)
        assert F32(host.npm_mean128(v.ctypes.data)).view(np.uint32) == M.tree_mean(v).view(np.uint32)
    bw = rng.exponential(1.0, 128).astype(F32)
    bw[[3, 40, 77, 100, 127]] = [0.0, np.nan, np.inf, -2.0, -0.0]
    want = M.branch_weight(bw)
    clean = np.where(np.isfinite(bw) & (bw > 0), bw, 0).astype(F32)
    assert want.view(np.uint32) == M.tree_mean(clean).view(np.uint32)
    for got in (host.npm_branch_weight(bw.ctypes.data), host.dabgpu_diversity_band_mean_host(bw.ctypes.data), dabgpu.diversity_band_mean(bw)):
        assert F32(got).view(np.uint32) == want.view(np.uint32)
    # one normal value in every band: the mean is that value exactly (below 2^121, where the sum of 128 still fits)
    for w in (1.0, 0.4, 1.17549435e-38, 3.3e-7, 12345.678, 2.0 ** 120 * 1.9999999):
        assert M.branch_weight(np.full(128, w, F32)).view(np.uint32) == F32(w).view(np.uint32), w
    assert not np.isfinite(M.branch_weight(np.full(128, 2.0 ** 122, F32)))


def test_float32_inside_the_float64_bound(host):
    rng = np.random.default_rng(8304)
    for i, (Cp, ex, pin, alpha) in enumerate(cases(rng)[:8]):
        n32, w32, M32, ok = M.bands(Cp, ex, pin, alpha)
        assert ok
        m64, n64, M64, w64 = M.bands64(Cp, ex, pin, alpha)
        m32 = M.bands(Cp, ex)[0]
        assert (np.abs(m32 - m64) <= M.BOUND_M * m64).all(), i
        p = np.zeros(128) if pin is None else np.where(np.isfinite(pin) & (pin > 0), pin, 0.0).astype(np.float64)
        err_n = np.abs(n32.astype(np.float64) - n64) / np.maximum(m64, p)
        assert (err_n <= M.BOUND_N).all(), (i, err_n.max() / M.U)
        err_M = abs(float(M32) - float(n32.astype(np.float64).mean())) / float(M32)
        assert err_M <= M.BOUND_MEAN, (i, err_M / M.U)
        den = np.maximum(n32.astype(np.float64), float(F32(M32 * F32(M.WEIGHT_CAP))))
        assert (np.abs(w32 * den - 1.0) <= 2 * M.U * 1.0000001).all(), i
        print(f"case {i}: m {np.abs(m32 / m64 - 1).max() / M.U:.2f} u of {M.BOUND_M / M.U:.0f}, n {err_n.max() / M.U:.2f} u of {M.BOUND_N / M.U:.0f}, "
              f"M {err_M / M.U:.2f} u of 8, w {np.abs(w32 * den - 1).max() / M.U:.2f} u of 2")


def test_band_means_under_white_noise(host, noise_powers):
    """every band's mean over the frames at s2 within four standard errors of the derived deviation; one frame's deviation at 1 / sqrt(12)"""
    plain, _ = noise_powers
    n = np.array([M.host_bands(host, c)[0] for c in plain], np.float64) / S2                  # [frames][128]
    assert same_bits(M.bands(plain[0])[0], M.host_bands(host, plain[0])[0])
    se = M.relative_deviation() / math.sqrt(N_FRAMES)
    worst = np.abs(n.mean(axis=0) - 1.0).max()
    print(f"band means: worst {worst:.4f} of s2, four standard errors {4 * se:.4f}; overall mean {n.mean():.5f}")
    assert worst < 4.0 * se
    assert abs(n.mean() - 1.0) < 4.0 * se / math.sqrt(128)
    # the deviation of one frame's value.  A band is a Gamma(12) draw over 12: kurtosis 3 + 6 / 12, so the sample deviation of N values
    # has the relative standard error sqrt((3.5 - 1) / (4 N))
    N = n.size
    tol = 4.0 * math.sqrt(2.5 / (4.0 * N))
    print(f"one frame: deviation {n.std():.5f}, derived {M.relative_deviation():.5f}, tolerance {tol * 100:.2f} %")
    assert abs(n.std() / M.relative_deviation() - 1.0) < tol


def test_smoothed_deviation(host, noise_powers):
    """alpha = 0.25 over the frames in sequence, each band a series: deviation sqrt(alpha / (2 - alpha)) / sqrt(12), mean still s2"""
    plain, _ = noise_powers
    alpha, burn = 0.25, 32                                                             # 0.75^32 = 1e-4 of the first frame is left
    state = np.zeros(128, F32)
    series = []
    for c in plain:
        state = M.host_bands(host, c, None, state, alpha)[0]
        series.append(state.astype(np.float64) / S2)
    first = M.host_bands(host, plain[0])[0]
    assert same_bits(np.array(series[0] * S2, F32), first)                                # a zeroed state starts at the first measurement
    s = np.array(series[burn:])
    want = M.relative_deviation(alpha)
    # neighbours correlate with rho^k, rho = 0.75: for the sample variance the series counts as N (1 - rho^2) / (1 + rho^2) independent
    # values; the smoothed value is close to normal (kurtosis 3): relative standard error of the deviation sqrt(2 / (4 N_eff))
    rho2 = (1.0 - alpha) ** 2
    n_eff = s.size * (1.0 - rho2) / (1.0 + rho2)
    tol = 4.0 * math.sqrt(2.0 / (4.0 * n_eff))
    print(f"alpha {alpha}: deviation {s.std():.5f}, derived {want:.5f}, tolerance {tol * 100:.2f} %, mean {s.mean():.5f}")
    assert abs(s.std() / want - 1.0) < tol
    # the mean of the smoothed series is, but for its two ends, the mean of the measurements it smoothed
    assert abs(s.mean() - 1.0) < 1.1 * 4.0 * M.relative_deviation() / math.sqrt(s.size)


def test_mean_noise_against_the_estimator(host, noise_frames, noise_powers, tmp_path_factory):
    """M of the profile and the estimator's calibrated floor on the same NULLs: both estimate s2, M with the relative deviation
    1 / sqrt(1536), N with the estimator's derived one; they share bins, so their difference deviates by less than the root of the
    squares' sum"""
    plain, _ = noise_powers
    Mv = np.array([M.host_bands(host, c)[2] for c in plain], np.float64)
    Nv = np.array([NM.floor_of(NM.group_energy(f, 0, 0.0)) * NM.unbias() for f in noise_frames])
    dev_M, dev_N = 1.0 / math.sqrt(1536.0), NM.relative_deviation()
    both = math.sqrt(dev_M ** 2 + dev_N ** 2)
    print(f"M / s2: mean {Mv.mean() / S2:.5f} deviation {Mv.std() / S2:.5f} (derived {dev_M:.5f}); N / s2: mean {Nv.mean() / S2:.5f} deviation "
          f"{Nv.std() / S2:.5f} (derived {dev_N:.5f}); largest |M - N| / s2 {np.abs(Mv - Nv).max() / S2:.4f}, four deviations {4 * both:.4f}")
    assert abs(Mv.mean() / S2 - 1.0) < 4.0 * dev_M / math.sqrt(N_FRAMES)
    assert (np.abs(Mv / S2 - 1.0) < 4.0 * dev_M * 1.1).all()
    assert (np.abs(Mv - Nv) / S2 < 4.0 * both).all()
    assert abs((Mv - Nv).mean()) / S2 < 4.0 * both / math.sqrt(N_FRAMES)


def test_excluded_tii_carriers_leave_the_profile_alone(host, noise_powers):
    """four transmitters of the modulator's TII symbol on the air, their carriers excluded: the profile is the one of the same frames
    without TII under the same mask, and its band means sit at s2 with the deviation of the carriers that are left"""
    plain, lit = noise_powers
    mask = tii_mask()
    count = (~M.excluded(mask)).reshape(128, 12).sum(axis=1)
    assert count.min() >= 8 and count.max() == 12 and (count < 12).sum() >= 32
    a = np.array([M.host_bands(host, c, mask)[0] for c in plain], np.float64)
    b = np.array([M.host_bands(host, c, mask)[0] for c in lit], np.float64)
    # (float64 transforms: what a lit carrier of power 2048^2 leaves on the others is rounding, 1e-16 of 4e6 against 5e3)
    assert np.abs(b / a - 1.0).max() < 1e-6
    se = 1.0 / np.sqrt(count * N_FRAMES)
    dev = np.abs(b.mean(axis=0) / S2 - 1.0) / se
    print(f"masked: worst band {dev.max():.2f} standard errors; bands with excluded carriers {(count < 12).sum()}")
    assert (dev < 4.0).all()
    # without the mask the bands under a transmitter are far off
    c = np.array([M.host_bands(host, x)[0] for x in lit[:8]], np.float64)
    assert (c.mean(axis=0)[count < 12] / S2 > 20.0).all()


def test_banded_combiner_model_equals_compiled_header(host):
    rng = np.random.default_rng(8305)
    mapper = DM.host_mapper(host)
    shape = (75, 1536)
    dq = [(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64) for _ in range(3)]
    k = np.array([0.011, 0.02, 0.007], F32)
    t0 = rng.exponential(1.0, 128).astype(F32)
    t1 = rng.exponential(3.0, 128).astype(F32)
    t1[[0, 5, 64, 127]] = [0.0, np.nan, np.inf, -1.0]
    sets = [dict(band=[t0, None, None]), dict(band=[t0, t1, None], w=[9.0, 9.0, 0.5]), dict(band=[None, t1, t0], valid=[1, 1, 0]),
            dict(band=[np.zeros(128, F32), t1, None]), dict(band=[np.full(128, np.nan, F32)] * 3), dict(band=[None, None, None], w=[1.0, 2.0, 0.5])]
    for i, kw in enumerate(sets):
        for layout in (DM.BITS_NATURAL, DM.BITS_MSC_CLASSED):
            want = M.combine_frame(dq, k, mapper, kw.get("w"), kw.get("valid"), kw["band"], layout)
            got = M.host_combine_frame(host, dq, k, kw.get("w"), kw.get("valid"), kw["band"], layout)
            assert np.array_equal(got[0], want[0]) and F32(got[1]).view(np.uint32) == F32(want[1]).view(np.uint32) and got[2] == want[2], (i, layout)
    assert M.combine_frame(dq, k, mapper, None, None, sets[3]["band"])[2] == 0b110            # a table of zeros: a dead branch
    dead = M.combine_frame(dq, k, mapper, None, None, sets[4]["band"])
    assert dead[1] == 0 and dead[2] == 0 and not dead[0].any()
    # one normal value in all bands = the scalar weight, bit for bit; ones on one branch = the demodulator's weighted soft bits
    for w in (0.37, 1.0, 5.5e3):
        a = M.combine_frame(dq[:2], k[:2], mapper, None, None, [np.full(128, w, F32), None])
        b = DM.combine_frame(dq[:2], k[:2], mapper, [w, 1.0])
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]
    one = M.combine_frame(dq[:1], k[:1], mapper, None, None, [np.ones(128, F32)])
    import softbit_model as SM
    assert np.array_equal(one[0], SM.frame_bits(dq[0], mapper, k[0])) and one[1] == k[0]
