"""CPU: the fading taps' definition.  The host model (dab-radio_amd/csrc/channel_core.h under g++, tests/cpp/channel_fading_host_model.cpp)
and the library's dabgpu_channel_fading_gain_host against the independent float64 model of tests/channel_fading_model.py: gains and
outputs inside the derived bounds of DESIGN.md 4.18 (asserted; the measured maxima printed), the interpolation against the plain sum of
phasors, the statistics of Rayleigh and Rice gains over 64 seeds, and the all-static table against the static model."""
import os

import numpy as np
import pytest

import channel_fading_model as FM
import channel_model as CM
from test_channel_model import CASES

POSITIONS = (0, (1 << 33) - 1701)
# the four cases of DESIGN.md 4.16's table with kinds: all Rayleigh; Rice; mixed with a static echo; eight taps, static ones between
FADING = [
    dict(kinds=[1], doppler=2.0 ** -11),
    dict(kinds=[1], rice_k=[4.0], los_cos=[0.7], doppler=100 / 2.048e6),
    dict(kinds=[1, 0], doppler=2.0 ** -11),
    dict(kinds=[1, 1, 0, 1, 1, 0, 1, 1], rice_k=[0.0, 2.0, 0.0, 0.0, 0.5, 0.0, 0.0, 10.0], los_cos=[0.0, -1.0, 0.0, 0.0, 0.3, 0.0, 0.0, 1.0], doppler=300 / 2.048e6),
]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return FM.build_host_model(tmp_path_factory.mktemp("channel_fading_host_model"))


@pytest.fixture(scope="module")
def static_host(tmp_path_factory):
    return CM.build_host_model(tmp_path_factory.mktemp("channel_host_model"))


@pytest.fixture(scope="module")
def dabgpu():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(CM.ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu


def table_of(case, s, seed=0x5eed):
    P = CM.params_dict(**CASES[case])
    f = FADING[case]
    return P, FM.plan_stream(P, f["doppler"], seed, s, f["kinds"], f.get("rice_k"), f.get("los_cos"))


def library_gain(dabgpu, T, m0, count):
    F = FM.to_struct([T], dabgpu.ChannelFadingStream)
    return dabgpu.channel_fading_gain(F, 0, m0, count).astype(np.complex128)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_gains_within_derived_bound_of_numpy_model(host, dabgpu, case):
    """dabgpu_channel_fading_gain_host and the host model's grid gains against the float64 gains, every fading tap of the case"""
    P, table = table_of(case, 1)
    n = 3400
    for pos in POSITIONS:
        m = np.arange(pos, pos + n, dtype=np.uint64)
        for k, T in enumerate(table):
            F = FM.to_struct(table)
            if T is None:
                assert np.array_equal(dabgpu.channel_fading_gain(FM.to_struct(table, dabgpu.ChannelFadingStream), k, pos, 5), np.ones(5, np.complex64))
                continue
            got = dabgpu.channel_fading_gain(FM.to_struct(table, dabgpu.ChannelFadingStream), k, pos, n).astype(np.complex128)
            ref = FM.gain(T, m)
            err = max(np.abs(got.real - ref.real).max(), np.abs(got.imag - ref.imag).max())
            B = FM.gain_bound(T)
            print(f"case {case} tap {k} pos {pos}: max gain component error {err:.3e}, derived bound {B:.3e}")
            assert err <= B
            assert np.abs(ref).max() <= FM.amp_max(T)
            # the library's gains at the grid are the host model's grid gains, and between two of them the line of the definition in float
            j0 = pos >> 6
            G = np.zeros(3, np.complex64)
            host.chfm_grid_gain(np.ctypeslib.as_ctypes(np.frombuffer(bytes(F), np.uint8).copy()), k, j0 + 1, 3, G.ctypes.data)
            at = 64 * (j0 + 1) - pos
            assert np.array_equal(got[at:at + 129:64].astype(np.complex64), G)


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_host_model_within_derived_bound_of_numpy_model(host, case, wrap):
    """3077-sample input, 3400 output samples, positions 0 and 2^33 - 1701: grid points fall off tile boundaries"""
    P, table = table_of(case, 1)
    rng = np.random.default_rng(120 + case)
    n_in, n_out = 3077, 3400
    x = (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)).astype(np.complex64)
    for pos in POSITIONS:
        got = FM.host_apply(host, [P, P], [table_of(case, 0)[1], table], x, pos, n_out, wrap)[1].astype(np.complex128)
        ref = FM.apply(P, table, 1, x, pos, n_out, wrap)
        err = max(np.abs(got.real - ref.real).max(), np.abs(got.imag - ref.imag).max())
        B = FM.bound(P, table, float(np.abs(x).max()))
        print(f"case {case} wrap {wrap} pos {pos}: max component error {err:.3e}, derived bound {B:.3e}")
        assert err <= B
        assert np.abs(ref).max() > 0.1 or (not wrap and pos > 0)                  # (without wrap the far position lies outside the input)


@pytest.mark.parametrize("doppler", [2.0 ** -11, 2.0 ** -15])
def test_interpolation_against_the_plain_sum(doppler):
    """the interpolated float64 gain against the un-interpolated sum of phasors: within (16 amp_diffuse + amp_los) phi^2 / 8"""
    phi = 2 * np.pi * 64 * doppler
    m = np.concatenate([np.arange(0, 20000, dtype=np.uint64), np.arange((1 << 33) - 1701, (1 << 33) + 9000, dtype=np.uint64)])
    for seed, (K, los) in enumerate([(0.0, 0.0), (4.0, 1.0), (0.5, -0.3), (100.0, -1.0)]):
        T = FM.plan_tap(doppler, seed, 0, 0, K, los)
        d = FM.gain(T, m) - FM.phasor_sum(T, m)
        err = max(np.abs(d.real).max(), np.abs(d.imag).max())
        B = FM.amp_max(T) * phi ** 2 / 8
        print(f"doppler {doppler:.3e} K {K}: max |interpolated - plain| {err:.3e}, bound {B:.3e}")
        assert err <= B
        on_grid = (m & np.uint64(63)) == 0
        assert np.array_equal(FM.gain(T, m[on_grid]), FM.phasor_sum(T, m[on_grid]))


N_SEEDS, N_TIME = 64, 1 << 17


def within_five_standard_errors(values, expected, name):
    v = np.asarray(values, np.float64)
    mean, se = v.mean(), v.std(ddof=1) / np.sqrt(v.size)
    print(f"{name}: mean {mean:.5f}, expected {expected:.5f}, standard error {se:.5f}")
    assert abs(mean - expected) <= 5 * se, name


def test_rayleigh_statistics_over_64_seeds(dabgpu):
    """the library's gains, 2^17 samples of each of 64 seeds at the largest Doppler (64 Doppler periods): per seed the time averages, over
    the seeds their mean within five standard errors (estimated from the 64 values) of: power 1, equal I and Q variances, no I/Q
    correlation, autocorrelation J0(2 pi f_D tau) at 8 lags up to J0's first zero"""
    doppler = 2.0 ** -11
    lags = np.rint(2.404825557695773 / (2 * np.pi * doppler) * np.arange(1, 9) / 8).astype(int)
    power, diff, cross, acf = [], [], [], []
    for seed in range(N_SEEDS):
        T = FM.plan_tap(doppler, seed, 0, 0)
        g = library_gain(dabgpu, T, 1000 * seed, N_TIME + int(lags[-1]))
        a = g[:N_TIME]
        power.append((np.abs(a) ** 2).mean())
        diff.append((a.real ** 2).mean() - (a.imag ** 2).mean())
        cross.append((a.real * a.imag).mean())
        acf.append([(g[t:t + N_TIME] * np.conj(a)).real.mean() for t in lags])
    within_five_standard_errors(power, 1.0, "mean power")
    within_five_standard_errors(diff, 0.0, "I variance - Q variance")
    within_five_standard_errors(cross, 0.0, "I/Q correlation")
    acf = np.array(acf)
    want = FM.bessel_j0(2 * np.pi * doppler * lags)
    assert abs(want[-1]) < 1e-3 and abs(FM.bessel_j0(0.0) - 1) < 1e-12 and abs(FM.bessel_j0(1.0) - 0.7651976865579666) < 1e-12
    for i, t in enumerate(lags):
        within_five_standard_errors(acf[:, i], want[i], f"autocorrelation at lag {t}")


def test_rice_line_of_sight_over_64_seeds(dabgpu):
    """K = 4: the time average of g conj(line-of-sight phasor) is amp_los"""
    doppler, K = 2.0 ** -11, 4.0
    vals = []
    for seed in range(N_SEEDS):
        T = FM.plan_tap(doppler, seed, 0, 0, K, 0.7)
        g = library_gain(dabgpu, T, 0, N_TIME)
        los = np.exp(2j * np.pi * FM.osc_angles(T, np.arange(N_TIME, dtype=np.uint64))[16])
        vals.append(g * np.conj(los))
    vals = np.array(vals).mean(1)
    assert abs(T["amp_los"] - np.sqrt(0.8)) < 1e-7
    within_five_standard_errors(vals.real, T["amp_los"], "Re g conj(LOS)")
    within_five_standard_errors(vals.imag, 0.0, "Im g conj(LOS)")


def test_oscillator_angles_equal_python_integers():
    """the vectorised uint64 phases of the model against channel_model.osc_cycles (Python integers)"""
    T = FM.plan_tap(2.0 ** -11, 3, 1, 2, 1.0, -0.5)
    m = [0, 1, 63, 64, (1 << 33) - 1, 1 << 33, (1 << 62) - 64, (1 << 62)]
    a = FM.osc_angles(T, np.array(m, np.uint64))
    for n in range(17):
        assert np.array_equal(a[n], CM.osc_cycles(T["phase"][n], T["freq"][n], m))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_all_static_equals_the_static_model_exactly(host, static_host, case):
    P = CM.params_dict(**CASES[case])
    table = [None] * len(P["taps"])
    rng = np.random.default_rng(160 + case)
    x = (rng.standard_normal(3077) + 1j * rng.standard_normal(3077)).astype(np.complex64)
    for pos in POSITIONS:
        assert np.array_equal(FM.apply(P, table, 1, x, pos, 3400, True), CM.apply(P, 1, x, pos, 3400, True))
        for fmt in (CM.F32, CM.U8):
            a = FM.host_apply(host, [P, P], [table, table], x, pos, 3400, True, fmt, scale=20.0)
            b = CM.host_apply(static_host, [P, P], x, pos, 3400, True, fmt, scale=20.0)
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
