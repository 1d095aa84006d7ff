"""CPU: the interferer's definition (include/dabgpu.h, "Interferer").  The host model -- dab-radio_amd/csrc/interferer_core.h under g++, the
functions the kernel is made of -- against the independent numpy model (tests/interferer_model.py): integer parts exact, float output inside
the bound derived there; the design record against the closed form and an FFT of its own table; the gate, the tone's frequency, split
invariance, and the power of the noise sources inside the intervals derived in the model's docstring."""
import ctypes as C
import os

import numpy as np
import pytest

import interferer_model as IM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [0.6, 0.3, 96000.0 / 2048000.0, 2.0 ** -6, 2.0 ** -7, 2.0 ** -8]          # L = 1, 2, 16, 32, 64, 64


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return IM.build_host_model(tmp_path_factory.mktemp("interferer_host_model"))


@pytest.fixture(scope="module")
def dabgpu():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu


@pytest.fixture(scope="module")
def shapes(dabgpu):
    """InterfererShape records of WIDTHS as the model's structures"""
    out = []
    for w in WIDTHS:
        H = dabgpu.interferer_design(w)
        out.append(IM.Shape.from_buffer_copy(bytes(H)))
    return out


def test_philox_known_answers_for_the_counter_layout(host):
    """the published vector through the host model's Philox, and the interferer's layout: (low word of n >> 1, high word, s, 16 + k)"""
    c = (C.c_uint32 * 4)(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)
    out = (C.c_uint32 * 4)()
    host.itm_philox(0xa4093822, 0x299f31d0, c, out)
    assert tuple(out) == (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    # seed = the vector's key, pair = its first two words, s = its third, 16 + k = its fourth: k would be 0x03707344 - 16
    host.itm_noise_words(0x299f31d0a4093822, 0x13198a2e, 0x03707344 - 16, 0x85a308d3243f6a88, out)
    assert tuple(out) == (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    rng = np.random.default_rng(5)
    for _ in range(300):
        seed, pair = (int(rng.integers(0, 1 << 64, dtype=np.uint64)) for _ in range(2))
        s, k = int(rng.integers(0, 1 << 20)), int(rng.integers(0, 4))
        host.itm_noise_words(seed, s, k, pair, out)
        want = IM.CM.philox4x32_10((seed & IM.CM.M32, seed >> 32), (pair & IM.CM.M32, pair >> 32, s, 16 + k))
        assert tuple(out) == tuple(int(v) for v in want)
    # g[n] takes words 2 (n & 1), 2 (n & 1) + 1 of the call of n >> 1, and n wraps below 0
    g = np.zeros(8, np.float32)
    host.itm_gauss(77, 2, 3, IM.M64 - 1, 4, g.ctypes.data)                   # n = 2^64 - 2, 2^64 - 1, 0, 1
    g0, g1 = IM.gauss(77, 2, 3, np.array([IM.M64 - 1, IM.M64, 0, 1], np.uint64))
    assert np.abs(g[0::2] - g0).max() < 1e-5 and np.abs(g[1::2] - g1).max() < 1e-5
    other, _ = IM.gauss(77, 2, 2, np.array([0, 1], np.uint64))               # another source: other numbers
    assert np.abs(other - g0[2:]).min() > 1e-3


@pytest.mark.parametrize("width", WIDTHS + [1.0, 0.5, 0.375, 0.3750001])
def test_design_equals_the_closed_form_and_its_own_figures(dabgpu, width):
    H = dabgpu.interferer_design(width)
    L, closed = IM.design_closed_form(width)
    assert H.interp == L and H.width_cycles == width and H.beta == IM.BETA
    got = np.array(H.taps[:], np.float32)
    want = closed.astype(np.float32)
    ulp = np.spacing(np.abs(want))
    assert np.all(np.abs(got[:16 * L].astype(np.float64) - want.astype(np.float64)) <= ulp), "table beyond 1 ulp of the closed form"
    assert np.all(got[16 * L:] == 0)
    per_phase = (got[:16 * L].astype(np.float64).reshape(16, L) ** 2).sum(0)
    assert abs(per_phase.mean() - 0.5) < 1e-6                                # E |v|^2 = amp^2
    w3, share, stop, ripple = IM.design_figures(got, L, width)
    print(f"width {width:.6f}: L {L}, -3 dB width {H.width_3db_cycles:.6f}, in-band share {H.inband_share:.4f}, stopband {H.stopband_level:.2e}, "
          f"phase ripple {H.phase_ripple:.6f}")
    assert abs(H.width_3db_cycles - w3) <= 1e-9 and abs(H.inband_share - share) <= 1e-9
    assert abs(H.stopband_level - stop) <= 1e-9 + 1e-6 * stop and abs(H.phase_ripple - ripple) <= 1e-9
    if L > 1:                                                                # the images lie in the stopband: stationary across the phases
        assert H.stopband_level < 2e-3 and H.phase_ripple < 1.001
        assert width - IM.TRANSITION / L < H.width_3db_cycles < width       # the -6 dB point is the nominal edge


def test_design_refusals(dabgpu):
    for w, text in ((float("nan"), "not finite"), (float("inf"), "not finite"), (1.0000001, "width_cycles"), (2.0 ** -8 * 0.999, "width_cycles"),
                    (0.0, "width_cycles"), (-0.1, "width_cycles")):
        with pytest.raises(dabgpu.DabGpuError) as err:
            dabgpu.interferer_design(w)
        assert text in str(err.value)
    assert dabgpu.lib().dabgpu_interferer_design(0.1, None) == 2
    assert [dabgpu.interferer_design(w).interp for w in (1.0, 0.3750001, 0.375, 0.75 / 64, 0.7500001 / 64, 2.0 ** -8)] == [1, 1, 2, 64, 32, 64]


def test_gate_counts_exact(host):
    """the remainder against Python's, the kernel's stepped form against it, and the on-counts of the host model's output over several periods"""
    rng = np.random.default_rng(6)
    def pick(values):                                                        # (Python integers: numpy would make floats of the large ones)
        return values[int(rng.integers(0, len(values)))]

    for _ in range(4000):
        period = pick([1, 2, 3, 1000, 4095, 4096, 4097, 196608, (1 << 40) + 7, (1 << 62), (1 << 64) - 1])
        m = pick([0, 1, 5, 1 << 33, (1 << 62) - 1, (1 << 62) + (1 << 31)]) + int(rng.integers(0, 3000))
        off = pick([0, 1, -1, 77, -77, (1 << 62) - 1, -(1 << 62) + 1, m, m + 1, m - 1])
        if abs(off) >= 1 << 62:
            off = 0
        r = host.itm_gate_rem(m, off, period)
        assert r == (m - off) % period
        k = int(rng.integers(0, 2048))
        assert host.itm_gate_step(r, k, period) == (m + k - off) % period
    for period, on, off in ((7, 3, 0), (7, 7, 2), (5, 0, 0), (1, 1, 0), (1, 0, 0), (100, 33, -41), (64, 1, -(1 << 40)), (9, 4, 1 << 35)):
        P = IM.stream([IM.source(IM.TONE, amp=1.0, gate_period=period, gate_on=on, gate_offset=off)])
        n = 5 * period + 3
        for pos in (0, 11):
            y = IM.host_apply(host, [P], [], None, pos, n)[0]
            want = np.array([((pos + i - off) % period) < on for i in range(n)])
            assert np.array_equal(y != 0, want), (period, on, off)
            assert np.all(np.abs(np.abs(y[want]) - 1.0) < 1e-6)


def test_tone_frequency_exact(host):
    """the phase increments of the host model's output are the frequency word's top bits: the angle of y[m] conj(y[0]) is m f within the float
    error of two phasors, for every m, without drift, at a position beyond 2^40"""
    for cycles in (250.0 / 2048000.0, -0.3771, 0.4999):
        f = int(round(cycles * 2 ** 64)) & IM.M64
        P = IM.stream([IM.source(IM.TONE, amp=2.0, freq_q64=f, phase0_q64=12345 << 40)])
        for pos in (0, (1 << 40) + 3):
            y = IM.host_apply(host, [P], [], None, pos, 4096)[0].astype(np.complex128)
            want = 2.0 * np.exp(2j * np.pi * IM.CM.osc_cycles(12345 << 40, f, [pos + i for i in range(4096)]))
            assert np.abs(y - want).max() < 2.0 * 4e-7
            turn = np.angle(y[1:] * np.conj(y[:-1])) / (2 * np.pi)
            assert np.abs(turn - cycles).max() < 2.0 ** -24 + 3e-7         # the 24-bit angle steps in units of 2^-24


def mixed_stream():
    return IM.stream([IM.source(IM.TONE, amp=0.7, freq_q64=int(0.0123 * 2 ** 64), phase0_q64=1 << 62),
                      IM.source(IM.BAND, amp=1.3, shape=2, freq_q64=int(0.146484375 * 2 ** 64), gate_period=700, gate_on=450, gate_offset=-13),
                      IM.source(IM.BAND, amp=0.5, shape=-1, freq_q64=(1 << 64) - int(0.2 * 2 ** 64)),
                      IM.source(IM.BAND, amp=2.0, shape=4)], seed=0x1234567890abcdef)


@pytest.mark.parametrize("case", ["mixed", "each_shape", "white_unrotated"])
def test_host_model_within_derived_bound_of_numpy_model(host, shapes, case):
    pairs = [IM.shape_pair(H) for H in shapes]
    if case == "mixed":
        plist = [mixed_stream()]
    elif case == "each_shape":
        plist = [IM.stream([IM.source(IM.BAND, amp=1.0, shape=i, freq_q64=int(0.01 * (i + 1) * 2 ** 64))], seed=40 + i) for i in range(len(shapes))]
    else:
        plist = [IM.stream([IM.source(IM.BAND, amp=3.0, shape=-1, gate_period=1, gate_on=1)], seed=9)]
    rng = np.random.default_rng(21)
    n = 1500
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    for P in plist:
        for pos in (0, (1 << 40) + 3):
            got = IM.host_apply(host, [P, P], shapes, x, pos, n)[1].astype(np.complex128)
            ref = IM.apply(P, pairs, 1, x, pos, n)
            err = max(np.abs(got.real - ref.real).max(), np.abs(got.imag - ref.imag).max())
            B = IM.bound(P, pairs, float(max(np.abs(x.real).max(), np.abs(x.imag).max())))
            print(f"{case} seed {P['seed']} pos {pos}: max component error {err:.3e}, derived bound {B:.3e}")
            assert err <= B
    # no input: the interferer alone, bit for bit what it adds to zeros; a stream with no live source returns its input bit for bit
    alone = IM.host_apply(host, plist[:1], shapes, None, 5, 300)
    on_zero = IM.host_apply(host, plist[:1], shapes, np.zeros(300, np.complex64), 5, 300)
    assert np.array_equal(alone.view(np.uint32), on_zero.view(np.uint32))
    dead = IM.stream([IM.source(IM.OFF, amp=1.0), IM.source(IM.TONE, amp=0.0), IM.source(IM.BAND, amp=1.0, shape=-1, gate_period=5, gate_on=0)])
    assert np.array_equal(IM.host_apply(host, [dead], shapes, x, 0, n)[0].view(np.uint32), x.view(np.uint32))


def test_split_invariance_at_every_split(host, shapes):
    """a call of a + b samples equals a call of a and then one of b on the following input, at every a"""
    P = mixed_stream()
    rng = np.random.default_rng(22)
    n = 150
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    for pos in (0, 1021):
        whole = IM.host_apply(host, [P], shapes, x, pos, n)[0]
        for a in range(n + 1):
            first = IM.host_apply(host, [P], shapes, x, pos, a)[0] if a else np.zeros(0, np.complex64)
            second = IM.host_apply(host, [P], shapes, x[a:], pos + a, n - a)[0] if a < n else np.zeros(0, np.complex64)
            assert np.array_equal(np.concatenate([first, second]).view(np.uint32), whole.view(np.uint32)), a


@pytest.mark.parametrize("which", [0, 2, 4, -1])
def test_mean_power_inside_the_derived_interval(host, shapes, which):
    """K seeds x N samples of one BAND source (shape `which`, -1 = white): the mean of |v|^2 within 5 sqrt(Gamma_max / (K N)) of amp^2 -- the
    interval of interferer_model's docstring, from the independent low-rate values; each seed within 5 sqrt(Gamma_max / N)"""
    amp, K, N = 1.5, 24, 1 << 14
    if which < 0:
        gamma, L = 1.0, 1
    else:
        L, taps = IM.shape_pair(shapes[which])
        gamma = IM.gamma_max(taps, L)
    assert N % L == 0
    plist = [IM.stream([IM.source(IM.BAND, amp=amp, shape=which, freq_q64=int(0.1 * 2 ** 64))], seed=1000 + k) for k in range(K)]
    y = IM.host_apply(host, plist, shapes, None, 64 * 977, N).astype(np.complex128)
    p = (np.abs(y) ** 2).mean(1) / amp ** 2
    one, mean = 5 * np.sqrt(gamma / N), 5 * np.sqrt(gamma / (K * N))
    print(f"shape {which}: L {L}, Gamma_max {gamma:.2f} (N / Gamma = {N / gamma:.0f} independent values of {N} samples, {N // L} low-rate values), "
          f"mean power / amp^2 = {p.mean():.4f} +- {mean:.4f}, worst seed {np.abs(p - 1).max():.4f} of {one:.4f}")
    assert gamma >= L * 0.999 or which < 0                                  # never more independent values than low-rate values
    assert abs(p.mean() - 1) <= mean and np.abs(p - 1).max() <= one


@pytest.mark.parametrize("which", [2, 4])
def test_in_band_share_of_a_long_run(host, shapes, which):
    """the share of a long run's power inside +-width / 2, from a Hann-windowed periodogram, is not below the record's figure less its own
    statistical margin.  The out-of-band power is a quadratic form of mean (1 - share) and variance <= lambda_max x mean with
    lambda_max <= Gamma_max / N_eff, N_eff = N mean(w^2) / max(w^2) = 3 N / 8 for the Hann window; the total likewise around 1.  With 5
    standard deviations each: share_hat >= 1 - ((1 - share) + 5 sqrt(Gamma (1 - share) / N_eff)) / (1 - 5 sqrt(Gamma / N_eff))"""
    H = shapes[which]
    L, taps = IM.shape_pair(H)
    N = 1 << 17
    y = IM.host_apply(host, [IM.stream([IM.source(IM.BAND, amp=1.0, shape=which)], seed=31)], shapes, None, 0, N)[0].astype(np.complex128)
    spec = np.abs(np.fft.fft(y * np.hanning(N + 1)[:N])) ** 2
    f = np.fft.fftfreq(N)
    share = spec[np.abs(f) <= 0.5 * H.width_cycles].sum() / spec.sum()
    gamma, n_eff = IM.gamma_max(taps, L), 3 * N / 8
    out = 1 - H.inband_share
    floor = 1 - (out + 5 * np.sqrt(gamma * out / n_eff)) / (1 - 5 * np.sqrt(gamma / n_eff))
    print(f"shape {which}: in-band share {share:.4f}, record {H.inband_share:.4f}, floor {floor:.4f}")
    assert share >= floor
