"""CPU: the impulse blanker's definition (include/dabgpu.h, "Impulse blanker").  The host model -- dab-radio_amd/csrc/blanker_core.h under
g++, the functions the kernel is made of -- equals the independent float32 numpy model (tests/blanker_model.py) bit for bit: block powers,
flags, output samples and mask words; the float64 model decides the same where the margin is wide; the false-alarm figures of DESIGN.md
4.29 are recomputed; 2^22 blocks of Gaussian samples flag nothing; a call equals any two-way split."""
import numpy as np
import pytest

import blanker_model as BM

N = 8192                                       # samples of the small cases: 256 blocks, 8 tiles


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return BM.build_host_model(tmp_path_factory.mktemp("blanker_host_model"))


def noise(rng, n, sigma=1.0):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (sigma / np.sqrt(2.0))).astype(np.complex64)


def burst(x, rng, at, length, amp):
    x = x.copy()
    x[at:at + length] += noise(rng, length, amp)
    return x


def both(host, P, x, pos, n_out):
    """host model and float32 numpy model of one stream agree bit for bit; -> (y, words)"""
    y, m = BM.host_apply(host, [P], x, pos, n_out)
    yn, mn, count = BM.apply(P, x, len(x), pos, n_out)
    assert np.array_equal(y[0].view(np.uint32), yn.view(np.uint32))
    assert np.array_equal(m[0], mn)
    assert BM.popcount(mn) == count
    return y[0], m[0]


def test_block_powers_bit_for_bit(host):
    """the fused |x|^2, the tree and the mean: numpy's float32 model equals g++'s, on values of every magnitude, at negative blocks and past the end"""
    rng = np.random.default_rng(1)
    x = noise(rng, N) * np.exp(rng.uniform(-40, 40, N)).astype(np.float32)
    for start in (0, 7, -45):
        a = BM.host_powers(host, x, start, -3, N // 32 + 6)
        b = BM.block_powers(x, N, start, -3, N // 32 + 6)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.all(BM.host_powers(host, x, 0, -3, 3) == 0) and np.all(BM.host_powers(host, x, 0, N // 32, 3) == 0)
    # the tree is not a running sum: the two differ on this input
    z = noise(rng, 32)
    run = np.float32(0)
    for v in BM._energy32(z):
        run = np.float32(run + v)
    assert np.float32(run * np.float32(1 / 32)) != BM.block_powers(z, 32, 0, 0, 1)[0]


def test_random_streams_and_planted_bursts(host):
    rng = np.random.default_rng(2)
    x = noise(rng, N)
    y, m = both(host, BM.params(), x, 0, N)
    assert BM.popcount(m) == 0 and np.array_equal(y, x)                   # nothing flagged: a copy
    xb = burst(x, rng, 3000, 100, 8.0)                                     # samples 3000..3099 = blocks 93..96
    for pos, n_out in ((0, N), (31, 6000), (1000, 6000), (2977, 200)):
        y, m = both(host, BM.params(), xb, pos, n_out)
        lo, hi = 92 * 32, 98 * 32                                          # blocks 93..96 and the guard of 1 either side
        idx = np.arange(pos, pos + n_out)
        inside = (idx >= lo) & (idx < hi)
        assert np.all(y[inside].view(np.uint32) == 0)                      # +0 + j(+0)
        assert np.array_equal(y[~inside], xb[idx[~inside]])
    # the float64 model decides the same on this input
    _, f64, b64 = BM.decide(BM.params(), xb, N, 0, N // 32, np.float64)
    f32, b32 = BM.host_decide(host, BM.params(), xb, 0, N // 32)
    assert np.array_equal(f64, f32) and np.array_equal(b64, b32) and list(np.nonzero(f32)[0]) == [93, 94, 95, 96]


def test_start_shifts_the_input(host):
    rng = np.random.default_rng(3)
    xb = burst(noise(rng, N), rng, 3000, 100, 8.0)
    for start in (-100, 37, 1024):
        P = BM.params(start=start)
        y, m = both(host, P, xb, 0, N)
        fl, _ = BM.host_decide(host, P, xb, 0, N // 32 + 40)
        assert fl.any() and np.nonzero(fl)[0][0] == (3000 + start) >> 5


def test_nan_and_infinity_blank_their_block_only(host):
    """a block with a sample that is not finite is flagged; its neighbours are decided from q (that block counted as 0)"""
    rng = np.random.default_rng(4)
    for bad in (np.nan, np.inf, -np.inf, 3e38):                            # (3e38 squared overflows: p is infinite)
        x = noise(rng, N)
        x[100 * 32 + 5] = bad
        y, m = both(host, BM.params(), x, 0, N)
        fl, bl = BM.host_decide(host, BM.params(), x, 0, N // 32)
        assert list(np.nonzero(fl)[0]) == [100] and list(np.nonzero(bl)[0]) == [99, 100, 101]
        assert np.all(np.isfinite(y.view(np.float32)))


def test_all_zero_input_flags_nothing(host):
    x = np.zeros(N, np.complex64)
    y, m = both(host, BM.params(), x, 0, N)
    assert BM.popcount(m) == 0 and np.all(y.view(np.uint32) == 0)
    # a lone block of signal in zeros: ref = 0, so it is not flagged either
    x[4096:4128] = 1
    y, m = both(host, BM.params(), x, 0, N)
    assert BM.popcount(m) == 0 and np.array_equal(y, x)


def test_bursts_at_the_very_start_and_end(host):
    """the side that lies outside the input is 0, the greater of the two still holds the level"""
    rng = np.random.default_rng(5)
    x = noise(rng, N)
    x = burst(burst(x, rng, 0, 40, 8.0), rng, N - 40, 40, 8.0)
    y, m = both(host, BM.params(), x, 0, N)
    fl, bl = BM.host_decide(host, BM.params(), x, 0, N // 32)
    assert list(np.nonzero(fl)[0]) == [0, 1, N // 32 - 2, N // 32 - 1]
    assert np.all(y[:96] == 0) and np.all(y[-96:] == 0) and np.array_equal(y[96:-96], x[96:-96])


def test_null_to_prs_edge_is_not_blanked(host):
    """noise only, then the signal 15 dB above it from one sample on (a NULL symbol's end): the greater side is the signal's own level"""
    rng = np.random.default_rng(6)
    for edge in (4096, 4096 + 17):
        x = noise(rng, N, 0.178)
        x[edge:] += noise(rng, N - edge, 1.0)
        y, m = both(host, BM.params(), x, 0, N)
        assert BM.popcount(m) == 0 and np.array_equal(y, x)
        # the smaller of the two sides would have blanked it
        p = BM.block_powers(x, N, 0, 0, N // 32)
        b = edge // 32 + 1
        assert 16 * p[b] > 3.0 * p[b - 24:b - 8].sum()


@pytest.mark.parametrize("gap", [0, 32])
@pytest.mark.parametrize("window", [1, 32])
@pytest.mark.parametrize("guard", [0, 4])
def test_every_corner_of_gap_window_guard(host, gap, window, guard):
    rng = np.random.default_rng(7)
    x = burst(noise(rng, N), rng, 2976, 128, 8.0)                          # blocks 93..96, whole
    x[5000] = np.nan
    P = BM.params(gap=gap, window=window, guard=guard, threshold=3.0 if window > 1 else 6.0)
    for pos, n_out in ((0, N), (2900, 777)):
        both(host, P, x, pos, n_out)
    fl, bl = BM.host_decide(host, P, x, 0, N // 32)
    assert fl[156] and bl[156 - guard:156 + guard + 1].all() and (guard == 4 or not bl[156 + guard + 1])
    if window == 32:                                                       # (a window of one block is a noisy reference: no count is asserted)
        assert list(np.nonzero(fl)[0]) == [93, 94, 95, 96, 156]


def test_disabled_stream_copies(host):
    rng = np.random.default_rng(8)
    x = burst(noise(rng, N), rng, 3000, 100, 8.0)
    x[77] = np.nan
    y, m = BM.host_apply(host, [BM.params(enabled=0, start=5)], x, 3, 4000)
    assert BM.popcount(m) == 0
    assert np.array_equal(y[0][2:].view(np.uint32), x[:3998].view(np.uint32)) and np.all(y[0][:2].view(np.uint32) == 0)
    yn, mn, _ = BM.apply(BM.params(enabled=0, start=5), x, N, 3, 4000)
    assert np.array_equal(y[0].view(np.uint32), yn.view(np.uint32)) and np.array_equal(m[0], mn)


def test_split_invariance(host):
    """one call equals any two-way split, inside a block too; the mask words of the parts OR together to the whole's"""
    rng = np.random.default_rng(9)
    x = burst(burst(noise(rng, N), rng, 1000, 60, 8.0), rng, 3050, 100, 8.0)
    x[2047] = np.inf
    P = BM.params(start=-3)
    pos, n = 31, 6000
    y, m = BM.host_apply(host, [P], x, pos, n)
    assert BM.popcount(m) > 8
    for a in (0, 1, 32, 33, 993, 1025, 2016, 3037, 5999, 6000):
        ya, ma = BM.host_apply(host, [P], x, pos, a)
        yb, mb = BM.host_apply(host, [P], x, pos + a, n - a)
        assert np.array_equal(np.concatenate([ya[0], yb[0]]).view(np.uint32), y[0].view(np.uint32))
        whole = np.zeros(len(m[0]) + 2, np.uint32)
        whole[:len(ma[0])] |= ma[0]
        off = ((pos + a) >> 10) - (pos >> 10)
        whole[off:off + len(mb[0])] |= mb[0]
        assert np.array_equal(whole[:len(m[0])], m[0]) and not whole[len(m[0]):].any()


def test_false_alarm_figures():
    """DESIGN.md 4.29's figures, from the Beta form and from the integral of the Gamma(32) tail over the Gamma(512) reference"""
    for T, want in ((3.0, 3.9e-13), (2.5, 2.9e-9), (2.0, 9.7e-6)):
        p = BM.false_alarm(T)
        print(f"threshold {T}: per-block false-alarm probability {p:.3e}")
        assert abs(p / want - 1) < 0.05
        assert abs(BM.false_alarm_quad(T) / p - 1) < 1e-3
    assert BM.false_alarm(BM.DEFAULTS["threshold"], BM.DEFAULTS["window"]) <= 1e-11


def test_gaussian_samples_flag_nothing(host):
    """2^22 blocks of complex Gaussian samples at the default parameters: expected false alarms 2^22 x 3.9e-13 = 1.6e-6"""
    rng = np.random.default_rng(10)
    chunk = 1 << 16                                                          # blocks per piece; the pieces overlap by the reach
    n = chunk * 32
    flagged = 0
    tail = noise(rng, 50 * 32)
    for _ in range((1 << 22) // chunk):
        z = rng.standard_normal((n, 2), dtype=np.float32).view(np.complex64)[:, 0]
        x = np.concatenate([tail, z])
        fl, _ = BM.host_decide(host, BM.params(), x, 25, chunk)              # the blocks with both sides inside the piece; the next goes on behind
        flagged += int(fl.sum())
        tail = x[-50 * 32:]
    assert flagged == 0
