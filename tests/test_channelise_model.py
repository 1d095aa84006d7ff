"""CPU: the channeliser's definition three ways (include/dabgpu.h, "Channeliser").  The table of dabgpu_channeliser_design against a numpy
table and the record's own error figures against numpy's; the host model (channelise_core.h under g++, the lines the kernels compile)
against the independent float64 model inside a DERIVED bound; tones against their closed form inside the record's
figures; split of combine of three blocks.  The measured margins are printed (pytest -s) and recorded in DESIGN.md 4.20."""
import ctypes as C

import numpy as np
import pytest

import channelise_model as CM

RATE = 8192000.0                    # D = 4: Band III blocks 1.712 MHz apart in an 8.192 MS/s capture
SPACING = 1712000.0


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return CM.build_host_model(tmp_path_factory.mktemp("channelise_host_model"))


def ulp_distance(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib).max()


@pytest.mark.parametrize("D", range(1, 9))
def test_table_equals_numpy_and_its_error_record_is_inside_the_target(host, D):
    F = CM.host_design(host, D)
    assert (F.decim, F.taps) == (D, CM.taps(D)) and F.beta == CM.BETA and F.cutoff_cycles == 0.5 * (CM.PASSBAND + CM.STOPBAND)
    got, exp = CM.table_of(F), CM.design_table(D)
    # 1 ulp of float between the two roundings of values that agree to a few ulp of double; taps below 2^-24 of the peak (the window's
    # edge, where np.i0 and the series differ in the last digits of a tiny number) are held to 1e-9 of the peak instead
    big = np.abs(exp) > exp.max() * 2.0 ** -24
    assert ulp_distance(got[big], exp[big]) <= 1 and np.abs(got.astype(np.float64) - exp)[~big].max(initial=0.0) <= 1e-9 * exp.max()
    assert np.all(np.ctypeslib.as_array(F.table)[F.taps:] == 0)
    assert abs(float(got.astype(np.float64).sum()) - 1.0) <= F.taps * CM.U and int(np.argmax(got)) == CM.peak(D)
    dev, stop = CM.design_error(got, D)
    print(f"D = {D}: K = {F.taps}, passband error {F.passband_error:.3e} (numpy {dev:.3e}), stopband level {F.stopband_level:.3e} (numpy {stop:.3e})")
    assert abs(dev - F.passband_error) <= 1e-9 and abs(stop - F.stopband_level) <= 1e-9 and F.error == F.passband_error + F.stopband_level
    if D == 1:
        assert got.tolist() == [1.0] and F.error == 0.0
    else:
        assert dev + stop <= 1e-4 and F.error <= 1e-4


def test_alias_only_edges_pass_the_neighbours_edge(host):
    """the library's table for the resampler's kind of edges (0.375 / 0.625, cutoff 0.5): its record is as good as the default's, and the
    neighbour's edge at 944 kHz passes almost whole -- the record alone does not say a filter suits adjacent blocks, the edges do"""
    F = CM.host_design(host, 4, 0.375, 0.625)
    assert F.cutoff_cycles == 0.5 and F.error <= 1e-4
    assert abs(CM.response(CM.table_of(F), 4, np.array([CM.STOPBAND / 4]))[0]) > 0.5
    assert abs(CM.response(CM.table_of(CM.host_design(host, 4)), 4, np.array([CM.STOPBAND / 4]))[0]) <= CM.host_design(host, 4).stopband_level


def signal(rng, n, scale=1.0):
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


SPLIT_CASES = [   # D, channel, start, pos, wrap
    (4, CM.channel(CM.freq_q64(300000.0, RATE), 0x123456789ABCDEF0, 1.0), 0, 0, False),
    (4, CM.channel(CM.freq_q64(-1412000.0, RATE), 0, -0.7), -37, 5, True),
    (4, CM.channel(0, 0, 1.5), 11, 3, False),                                        # the skipped rotation
    (2, CM.channel(CM.freq_q64(500000.0, 4096000.0), 1 << 63, 1.0), 1, 40, True),
    (3, CM.channel(CM.freq_q64(-1.0, 3.0), 7, 0.25), -5, (1 << 40) + 1, True),
    (5, CM.channel(CM.freq_q64(2012000.0, 10240000.0), 99, 1.0), 100, 0, False),
    (8, CM.channel(CM.freq_q64(-5136000.0, 16384000.0), 5, 2.0), -(1 << 61), (1 << 58) - 40, True),
    (1, CM.channel(CM.freq_q64(100.0, 2048000.0), 0, 1.0), 3, 17, False),
    (1, CM.channel(0, 0, 1.0), -2, 0, True),
]


@pytest.mark.parametrize("case", range(len(SPLIT_CASES)))
def test_split_host_model_inside_the_derived_bound(host, case):
    D, ch, start, pos, wrap = SPLIT_CASES[case]
    rng = np.random.default_rng(4200 + case)
    n_in, n_out = 601, 40
    x = signal(rng, n_in)
    x_max = float(np.abs(x).max())
    F = CM.host_design(host, D)
    table = CM.table_of(F)
    got = CM.host_split(host, [ch], F, x, pos, start, n_out, wrap)[0]
    exp = CM.split(ch, D, table, x, pos, start, n_out, wrap)
    mixes = (ch["freq_q64"] | ch["phase0_q64"]) != 0
    bound = CM.split_bound(table, x_max, ch["gain"], mixes)
    err = max(np.abs(got.real - exp.real).max(), np.abs(got.imag - exp.imag).max())
    print(f"split D = {D}, case {case}: measured {err:.2e}, derived bound {bound:.2e}")
    assert err <= bound
    for i in (0, 1, n_out - 1):                                              # the definition's own loop, bit for bit
        one = CM.host_split_sample(host, ch, F, x, pos + i, start, wrap)
        assert np.array_equal(np.array([one]).view(np.uint32), got[i:i + 1].view(np.uint32))
    if not wrap:
        assert np.abs(exp).max() > 0                                         # the window meets the input
    if D == 1 and not mixes and ch["gain"] == 1.0:
        assert np.array_equal(got.view(np.uint32), np.array([x[(pos + i + start) % n_in] for i in range(n_out)], np.complex64).view(np.uint32))


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 8])
def test_combine_host_model_inside_the_derived_bound(host, D):
    rng = np.random.default_rng(4300 + D)
    rate = 2048000.0 * D
    chs = [CM.channel(CM.freq_q64(-0.21 * rate, rate), 12345 << 40, 1.0, 0), CM.channel(0, 0, -0.5, 0),
           CM.channel(CM.freq_q64(0.2089 * rate, rate), 1 << 62, 3.0, 0), CM.channel(CM.freq_q64(0.1 * rate, rate), 0, 1.0, 1)]
    n_in, n_out = 211, 90
    x = np.stack([signal(rng, n_in) for _ in chs])
    x_max = float(np.abs(x).max())
    F = CM.host_design(host, D)
    table = CM.table_of(F)
    for start, pos, wrap in ((0, 0, False), (-13, 7, True), (29, (1 << 58) - 100, True)):
        got = CM.host_combine(host, chs, 2, F, x, pos, start, n_out, wrap)
        for s, members in ((0, [0, 1, 2]), (1, [3])):
            exp = CM.combine([chs[c] for c in members], D, table, [x[c] for c in members], pos, start, n_out, wrap)
            bound = CM.combine_bound(table, D, x_max, [chs[c]["gain"] for c in members])
            err = max(np.abs(got[s].real - exp.real).max(), np.abs(got[s].imag - exp.imag).max())
            print(f"combine D = {D}, stream {s}, start {start}: measured {err:.2e}, derived bound {bound:.2e}")
            assert err <= bound
        # the u8 form quantises the same sums: a byte differs from the float64 model's only where the model lies within the bound of a step
        q = CM.host_combine(host, chs, 2, F, x, pos, start, n_out, wrap, CM.U8, 20.0)
        exp = CM.combine(chs[:3], D, table, x[:3], pos, start, n_out, wrap)
        pre = CM.u8_pre(exp, 20.0)
        differs = q[0] != CM.u8_of(pre)
        near = np.abs(pre - np.round(pre)) <= 20.0 * CM.combine_bound(table, D, x_max, [c["gain"] for c in chs[:3]]) + 256 * CM.U
        assert np.all(~differs | near)


def tone(f_cycles, n, amp=1.0, phase=0.0):
    return (amp * np.exp(2j * np.pi * (f_cycles * np.arange(n) + phase))).astype(np.complex64)


@pytest.mark.parametrize("D", [2, 4, 5, 8])
def test_passband_tones_come_back_as_the_closed_form(host, D):
    """x = sum of tones at f_c + d, d inside the passband: y[m] = gain sum A e^(2 pi i (d (m D + start) - phase0)) within the record's
    passband error, the 24-bit angle of the oscillator (2 pi 2^-24 per unit of amplitude), the input's float rounding and the derived bound"""
    F = CM.host_design(host, D)
    table = CM.table_of(F)
    fc_word = CM.freq_q64(300000.0, 2048000.0 * D)
    fc = fc_word / 2.0 ** 64
    ds = np.array([0.0, 0.1, -0.25, 0.374, -0.375]) / D                       # cycles per wideband sample, relative to the channel
    amps = np.array([0.5, 1.0, 0.7, 0.4, 0.9])
    n_in, start, n_out = 1000 * D, 17, 700
    x = sum(tone(fc + d, n_in, a).astype(np.complex128) for d, a in zip(ds, amps)).astype(np.complex64)
    ch = CM.channel(fc_word, 0, -1.25)
    got = CM.host_split(host, [ch], F, x, 100, start, n_out, False)[0]
    at = (100 + np.arange(n_out)) * D + start
    exp = -1.25 * sum(a * np.exp(2j * np.pi * d * at) for d, a in zip(ds, amps))
    A = 1.25 * amps.sum()
    allowed = A * (F.passband_error + 2 * np.pi * 2.0 ** -24 + CM.tap_sum(table) * 2 * CM.U) + CM.split_bound(table, amps.sum(), 1.25)
    err = np.abs(got - exp).max()
    print(f"tones D = {D}: |y - closed form| {err:.2e}, allowed {allowed:.2e} (record {F.passband_error:.2e})")
    assert err <= allowed


@pytest.mark.parametrize("D", [2, 4, 5, 8])
def test_a_tone_at_the_neighbours_edge_comes_back_under_the_stopband_level(host, D):
    """944 kHz from the channel's centre (0.4609375 cycles per block sample), at the band's far end and where the first alias folds"""
    F = CM.host_design(host, D)
    table = CM.table_of(F)
    fc_word = CM.freq_q64(-300000.0, 2048000.0 * D)
    for d in (CM.STOPBAND / D, -CM.STOPBAND / D, 0.5, (1.0 - 0.375) / D):
        x = tone(fc_word / 2.0 ** 64 + d, 1000 * D)
        got = CM.host_split(host, [CM.channel(fc_word, 0, 1.0)], F, x, 100, 0, 600, False)[0]
        level = np.abs(got).max()
        allowed = F.stopband_level + CM.split_bound(table, 1.0) + CM.tap_sum(table) * (2 * CM.U + 2 * np.pi * 2.0 ** -24)
        print(f"stopband D = {D}, {d * D:+.4f} cycles per block sample: {level:.2e}, allowed {allowed:.2e} (record {F.stopband_level:.2e})")
        assert level <= allowed


def test_split_of_combine_of_three_blocks_returns_each_block(host):
    """Three blocks 1.712 MHz apart on an 8.192 MS/s stream, each a sum of tones inside its passband, at different levels.  A block comes
    back through H twice (2 passband errors); each neighbour reaches it through the split filter's stopband and, folded by the
    interpolation, as D - 1 images that the combine filter holds at its stopband level: D stopband levels per unit of neighbour
    amplitude; its own images pass two stopbands.  Both oscillators take 24-bit angles: 2 pi 2^-24 each."""
    D = 4
    F = CM.host_design(host, D)
    table = CM.table_of(F)
    rng = np.random.default_rng(4400)
    n_blk = 1200
    fs = [rng.uniform(-0.375, 0.375, 6) for _ in range(3)]
    am = [rng.uniform(0.2, 1.0, 6) * lvl for lvl in (1.0, 10.0, 0.1)]                  # the middle block 20 dB up, the last 20 dB down
    blocks = np.stack([sum(tone(f, n_blk, a, p).astype(np.complex128) for f, a, p in zip(fs[c], am[c], rng.uniform(0, 1, 6))).astype(np.complex64)
                       for c in range(3)])
    chs = [CM.channel(CM.freq_q64(off, RATE), ph, 1.0, 0) for off, ph in ((-SPACING, 1 << 60), (0.0, 3 << 50), (SPACING, 7 << 61))]
    wide = CM.host_combine(host, chs, 1, F, blocks, 0, 0, n_blk * D, False)[0]
    back = CM.host_split(host, chs, F, wide, 0, 0, n_blk, False)
    A = [float(a.sum()) for a in am]
    edge = 2 * CM.TPP                                                       # both filters' transients at the ends of the input
    S = CM.tap_sum(table)
    for c in range(3):
        others = sum(A) - A[c]
        allowed = A[c] * (2 * F.passband_error + F.passband_error ** 2 + (D - 1) * F.stopband_level ** 2) + others * D * F.stopband_level \
            + sum(A) * 4 * np.pi * 2.0 ** -24 + S * (CM.combine_bound(table, D, max(A), [1.0] * 3) + CM.split_bound(table, S * sum(A))) + S * S * sum(A) * 2 * CM.U
        err = np.abs(back[c] - blocks[c])[edge:-edge].max()
        print(f"block {c} (amplitude {A[c]:.2f}, neighbours {others:.2f}): |split(combine) - block| {err:.2e}, allowed {allowed:.2e}")
        assert err <= allowed
