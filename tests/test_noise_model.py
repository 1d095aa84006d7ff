"""CPU: the noise estimate (include/dabgpu.h, "Noise estimate") -- the calibration constant derived and pinned, the estimator's mean under
white noise and under TII against the derived expectation and variance, and the float32 host model (csrc/noise_core.h by g++ around the
oracle's PLL and transform) against the float64 model of tests/noise_model.py inside a bound derived here."""
import math

import numpy as np
import pytest

import noise_model as M
import tii_model as TM

U = 2.0 ** -24
N_FRAMES = 256            # 4 standard errors = 4 * 0.0319 / 16 = 0.8 % (asserted below from the model's own deviation)


@pytest.fixture(scope="module")
def dabgpu():
    import dabgpu as D
    return D


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("noise_host_model"))


def test_constant_is_derived(dabgpu, host):
    mu, err = M.derive_mu()
    assert err < 1e-9
    assert abs(M.low_four_moments(1 << 16, 120.0)[0] / 4.0 - mu) < 1e-9            # the upper limit of the quadrature does not matter
    mc, se = M.mu_monte_carlo()
    assert abs(mc - mu) < 4.0 * se and se < 2e-3
    lit = np.float32(host.noise_host_unbias())
    print(f"mu = {mu!r}, 8 / (mu 8 2048) = {M.unbias()!r}, literal {float(lit)!r}")
    assert lit.view(np.uint32) == np.float32(M.unbias()).view(np.uint32)
    # nearest: both float neighbours are farther from the derived value
    for other in (np.nextafter(lit, np.float32(0)), np.nextafter(lit, np.float32(1))):
        assert abs(float(other) - M.unbias()) > abs(float(lit) - M.unbias())
    assert np.float32(dabgpu.noise_unbias()).view(np.uint32) == lit.view(np.uint32)
    assert 0.0318 < M.relative_deviation() < 0.0320


@pytest.fixture(scope="module")
def noise_frames():
    """N_FRAMES seeded NULL periods of white noise, power s2 = 2.5 per complex sample (one set, shared, read only)"""
    rng = np.random.Generator(np.random.PCG64(8200))
    s2 = 2.5
    x = math.sqrt(s2 / 2.0) * (rng.standard_normal((N_FRAMES, M.NB_NULL)) + 1j * rng.standard_normal((N_FRAMES, M.NB_NULL)))
    x.setflags(write=False)
    return x, s2


@pytest.mark.parametrize("T", [0, 1, 4])
def test_mean_of_the_estimate(noise_frames, oracle, host, dabgpu, T):
    """the mean of N / s2 over the frames within four standard errors (of the model's derived variance, not the sample's) of 1, and of
    the derived factor with T strong transmitters on distinct combs -- in the float64 model, and in the library's own arithmetic on the
    same frames: the host model's fold and floor (csrc/noise_core.h) and dabgpu_noise_unbias()"""
    x, s2 = noise_frames
    txs = [(11, 5, 1.0), (40, 17, 1.0), (0, 0, 1.0), (69, 23, 1.0)][:T]
    tii = TM.null_period(np.ones(2048, np.complex128), txs) if T else 0.0          # a lit bin: 2048^2 against 2048 s2 of noise
    got = np.array([M.floor_of(M.group_energy(x[i] + tii, 0, 0.0)) * M.unbias() / s2 for i in range(N_FRAMES)])
    se = M.relative_deviation(T) / math.sqrt(N_FRAMES)
    assert 4.0 * se < 0.01
    want = M.tii_factor(T)
    print(f"T = {T}: mean N / s2 = {got.mean():.5f}, derived {want:.5f}, standard error {se:.5f}, sample deviation {got.std():.4f} "
          f"(derived {M.relative_deviation(T):.4f})")
    assert abs(got.mean() - want) < 4.0 * se
    m32 = M.HostModel(host, oracle)
    unbias = np.float32(dabgpu.noise_unbias())
    lib = np.array([np.float32(host.noise_host_floor(m32.energy((x[i] + tii).astype(np.complex64), 0, 0.0).ctypes.data)) * unbias / s2
                    for i in range(N_FRAMES)])
    print(f"T = {T}: the library's arithmetic: mean N / s2 = {lib.mean():.5f}, largest distance from the float64 model {np.abs(lib - got).max():.2e}")
    assert abs(lib.mean() - want) < 4.0 * se
    rec = dabgpu.noise_floor_host(m32.energy((x[0] + tii).astype(np.complex64), 0, 0.0), 1.0e9)
    assert rec["valid"] == 1 and np.float32(rec["noise_power"]) == np.float32(lib[0] * s2)
    if T == 0:
        assert want == 1.0
    if T == 4:
        assert abs(10.0 * math.log10(want) - 0.24) < 0.005


def test_reciprocal_within_one_ulp(host):
    """all 2^23 mantissas: at most one unit in the last place from the correctly rounded quotient; the exponent is mirrored exactly"""
    off = np.zeros(1, np.uint32)
    worst = host.noise_host_reciprocal_worst(off.ctypes.data)
    print(f"reciprocal: {int(off[0])} of 8388608 mantissas differ from the correctly rounded quotient, worst {worst} ulp")
    assert worst <= 1.0
    for e in (-126, -40, -1, 0, 1, 57, 126):
        for m in (1.0, 1.3330078125, 1.99999988079071044921875):
            x = np.float32(math.ldexp(m, e))
            r = np.float32(host.noise_host_reciprocal(x))
            assert abs(float(r) * float(x) - 1.0) <= 2.0 ** -22, (e, m)
    # x > 2^126: the result is below the normal range and rounds once more there
    x = np.float32(math.ldexp(1.5, 127))
    assert abs(float(np.float32(host.noise_host_reciprocal(x))) - 1.0 / float(x)) <= 2.0 ** -149


def bound_frame(x, freq, E64, F64, P64):
    """the float32 host model's distance from the float64 model on the samples x of one NULL window, derived (u = 2^-24):
    rotation   the angle dt = i4 f + k f (+ 1/4) is three float operations on values up to 2048 |f| + 1/4: 4 u of that, times 2 pi; sine and
               cosine eps_cs = 8.73e-8 + 17.6 u (DESIGN 4.16 derives 8.73e-8 + 8.8 u for the fused form of this polynomial; the PLL's is unfused, two
               roundings for each fused one), the complex product 2 sqrt 2 u:  eps_rot per sample, relative
    transform  Higham, Accuracy and Stability, theorem 24.2: ||dX|| / ||X|| <= log2(2048) eta, eta = mu + gamma_4 (sqrt 2 + mu), mu = sqrt 2 u
               for a table of rounded exact values (the radix 4 / 8 passes do no more operations per level than radix 2)
    so every bin is off by at most D = (eps_rot + eta_fft (1 + eps_rot)) sqrt(2048) ||x||_2.
    power      |d p| <= 2 |X| D + D^2, its two roundings 2 u
    group      8 powers, three levels of sums: 3 u; sum_8 |X| <= sqrt(8 E)
    floor      an order statistic moves by at most the largest change of its comb; the share's sum two levels (its 1/4 exact), the 24
               shares 23 sequential sums, the constant 1/24 and its product 2 u: 27 u; the literal and its product 2 u
    power P    16 fused steps per lane, 6 levels in the wave, 2 across: gamma_24 on a sum of squares
    weight     the relative error of max(N, P 2^-40), u for the correctly rounded quotient and 2 u for the one ulp the Newton form may add
    Returns (bound on every E, on N, on P, relative on weight, on snr)."""
    eps_cs = 8.73e-8 + 17.6 * U
    eps_rot = 2.0 * math.pi * 4.0 * U * (2048.0 * abs(freq) + 0.25) + math.sqrt(2.0) * eps_cs + 2.0 * math.sqrt(2.0) * U
    mu = math.sqrt(2.0) * U
    eta = 11.0 * (mu + 4.0 * U / (1.0 - 4.0 * U) * (math.sqrt(2.0) + mu))
    norm = math.sqrt(float(np.sum(np.abs(x.astype(np.complex128)) ** 2)))
    D = (eps_rot + eta * (1.0 + eps_rot)) * math.sqrt(2048.0) * norm
    dE = (1.0 + 6.0 * U) * (2.0 * D * np.sqrt(8.0 * E64) + 8.0 * D * D) + 6.0 * U * E64
    dF = float(np.mean(dE.max(axis=1))) * (1.0 + 29.0 * U) + 27.0 * U * F64
    dN = M.unbias() * (dF + 2.0 * U * (F64 + dF))
    dP = 24.0 * U / (1.0 - 24.0 * U) * P64
    N64 = F64 * M.unbias()
    cap = P64 * M.RATIO_CAP
    if N64 + dN < cap * (1.0 - dP / P64):                # both models take the cap
        rel_den = dP / P64 + U
    elif N64 - dN > cap * (1.0 + dP / P64):              # both take N
        rel_den = dN / N64
    else:
        rel_den = max(dN / max(N64, cap), dP / P64 + U)
    assert rel_den < 0.5, "the bound says nothing about this case"
    rel_w = (rel_den + 3.0 * U) / (1.0 - rel_den)
    w64 = 1.0 / max(N64, cap)
    gap = abs(P64 - N64)
    d_snr = w64 * ((dP + dN + U * gap) * (1.0 + rel_w) + gap * rel_w) + U * max(P64 - N64, 0.0) * w64 * (1.0 + rel_w)
    return dE, dN, dP, rel_w, d_snr


CASES = [  # (noise sigma per component, transmitters, carrier offset in spacings, PRS amplitude)
    (1.5, [], 0.0, 1.0),
    (1.5, [(11, 5, 1.0), (40, 17, 0.5), (33, 17, 0.7)], 3.05, 1.0),
    (0.02, [], -0.4, 30.0),                                  # the 120 dB cap decides the weight
    (40.0, [(69, 23, 2.0), (3, 1, 1.0), (20, 9, 1.0), (50, 14, 1.0)], 0.5, 0.1),
]


def test_host_model_against_float64_model(oracle, host):
    prs = oracle.prs_fft()
    m32 = M.HostModel(host, oracle)
    rng = np.random.default_rng(8300)
    worst = {"E": 0.0, "N": 0.0, "P": 0.0, "w": 0.0, "snr": 0.0}
    for sigma, txs, spacings, amp in CASES:
        cfo = spacings / 2048.0
        s = np.zeros(6000, np.complex128)
        a = 137
        if txs:
            s[a:a + M.NB_NULL] += TM.null_period(prs, txs)
        sym = np.fft.ifft(prs.astype(np.complex128)) * 2048 * amp
        s[a + M.NB_NULL:a + M.NB_NULL + 2552] += np.concatenate([sym[-504:], sym])
        s *= np.exp(2j * np.pi * cfo * np.arange(s.size))
        s += sigma * (rng.standard_normal(s.size) + 1j * rng.standard_normal(s.size))
        s = s.astype(np.complex64)
        f = np.float32(-cfo)
        E64 = M.group_energy(s, a, float(f))
        F64, P64 = M.floor_of(E64), M.signal_power(s, a)
        want = M.finish(F64, P64)
        rec, E32 = m32.estimate(s, a, f)
        dE, dN, dP, rel_w, d_snr = bound_frame(s[a + M.NB_PREFIX:a + M.NB_PREFIX + M.NB_FFT], float(f), E64, F64, P64)
        assert rec["valid"] == 1 == want[4]
        errs = {"E": float((np.abs(E32.reshape(24, 8) - E64) / dE).max()), "N": abs(float(rec["noise_power"]) - want[0]) / dN,
                "P": abs(float(rec["signal_power"]) - want[1]) / dP, "w": abs(float(rec["weight"]) - want[2]) / (want[2] * rel_w),
                "snr": abs(float(rec["snr"]) - want[3]) / d_snr}
        print(f"sigma {sigma}, {len(txs)} transmitters, offset {spacings}: measured / bound", {k: round(v, 4) for k, v in errs.items()},
              f"N = {want[0]:.4g} (2 sigma^2 = {2 * sigma * sigma:.4g}), snr = {want[3]:.4g}")
        for k, v in errs.items():
            assert v <= 1.0, (k, v)
            worst[k] = max(worst[k], v)
        # the library's host form is the same arithmetic
        import dabgpu
        lib_rec = dabgpu.noise_floor_host(E32, rec["signal_power"])
        assert lib_rec.tobytes() == rec.tobytes()
    print("worst measured / bound:", {k: round(v, 4) for k, v in worst.items()})


def test_scale_of_signal_power_is_the_demodulators(dabgpu, host):
    """sb_scale(level, signal_power) equals dabgpu_soft_scale_host on the same samples, bit for bit"""
    import ctypes as C
    L = dabgpu.lib()
    L.dabgpu_soft_scale_host.restype = C.c_float
    L.dabgpu_soft_scale_host.argtypes = [C.c_void_p, C.c_float]
    rng = np.random.default_rng(8400)
    for amp in (1e-12, 0.03, 1.0, 700.0, 1e15):
        x = (amp * (rng.standard_normal(2048) + 1j * rng.standard_normal(2048))).astype(np.complex64)
        P = np.float32(host.noise_host_frame_power(x.ctypes.data))
        for level in (1.0, 64.0, 127.0):
            got = np.float32(host.noise_host_scale(np.float32(level), P))
            want = np.float32(L.dabgpu_soft_scale_host(x.ctypes.data, np.float32(level)))
            assert got.view(np.uint32) == want.view(np.uint32), (amp, level)
            assert amp > 1e14 or got > 0


def test_skipped_frames_and_the_cap(dabgpu, host):
    E = np.full(192, 3.0, np.float32)
    ok = dabgpu.noise_floor_host(E, 100.0)
    assert ok["valid"] == 1 and ok["noise_power"] == np.float32(3.0) * np.float32(dabgpu.noise_unbias())
    for P in (0.0, -1.0, float("nan"), float("inf")):
        assert not any(dabgpu.noise_floor_host(E, P).tolist())
    for bad in (float("nan"), float("inf")):
        Eb = E.copy(); Eb[:8] = bad
        assert not any(dabgpu.noise_floor_host(Eb, 100.0).tolist())
    # no noise at all: the cap, exactly 2^40 / P, and snr = P * weight
    z = dabgpu.noise_floor_host(np.zeros(192, np.float32), 4096.0)
    assert z["valid"] == 1 and z["noise_power"] == 0 and z["weight"] == np.float32(2.0 ** 28) and z["snr"] == np.float32(2.0 ** 40)
    # a power whose capped denominator leaves the normal range has no finite weight: skipped
    assert not any(dabgpu.noise_floor_host(np.zeros(192, np.float32), 1e-30).tolist())
    # noise above the signal: snr 0, the weight still that of the noise
    n = dabgpu.noise_floor_host(np.full(192, 1e6, np.float32), 10.0)
    assert n["valid"] == 1 and n["snr"] == 0 and n["weight"] > 0
