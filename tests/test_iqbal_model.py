"""The IQ balance arithmetic (dab-radio_amd/csrc/iqbal_core.h under g++, tests/cpp/iqbal_host_model.cpp) against the independent numpy
models of tests/iqbal_model.py: map and moments within the float32 bounds derived there, the tree, the fold and the solve bit for bit
against the numpy float32 restatement, the fixed point against the closed form, the fallbacks, and what the estimator reaches on the
two-block signal in float32 beside float64 (the figures of DESIGN.md 4.32)."""
import numpy as np
import pytest

import iqbal_model as IM

U = IM.U
F32 = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return IM.build_host_model(tmp_path_factory.mktemp("iqbal_host_model"))


def noise(rng, n, sigma=1.0):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (sigma / np.sqrt(2.0))).astype(np.complex64)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def c32(z):
    return complex(F32(z.real), F32(z.imag))


def test_map_within_the_float32_bound(host):
    rng = np.random.default_rng(1)
    y = noise(rng, 5000, 3.0)
    for a, b, c in ((1 + 0j, 0j, 0j), (1.02 - 0.03j, -0.02 - 0.03j, 0.3 + 0.2j), (-0.7 + 2.5j, 1.5 - 0.25j, -40 + 0.001j)):
        a, b, c = c32(a), c32(b), c32(c)
        got = IM.host_map(host, a, b, c, y).astype(np.complex128)
        want = IM.map64(a, b, c, y)
        big = np.maximum(abs(y.real), abs(y.imag)).astype(np.float64)
        k = abs(a.real) + abs(a.imag) + abs(b.real) + abs(b.imag)
        for comp, c0 in ((np.real, abs(c.real)), (np.imag, abs(c.imag))):
            bound = 4 * U * (c0 + k * big) * (1 + 4 * U)
            assert np.all(abs(comp(got) - comp(want)) <= bound)
    assert same_bits(IM.host_map(host, 1 + 0j, 0j, 0j, y), y)                   # identity coefficients pass finite non-zero samples through


def test_moments_within_the_float32_bound_and_tree_order_bit_for_bit(host):
    rng = np.random.default_rng(2)
    y = (noise(rng, 7 * IM.TILE, 2.0) + np.complex64(0.5 - 0.25j)).astype(np.complex64)
    y[3 * IM.TILE:4 * IM.TILE] *= np.float32(1e-3)
    got = IM.host_moments(host, y)
    want = IM.moments64(y)
    t = y.astype(np.complex128).reshape(-1, IM.TILE)
    size = np.stack([abs(t.real).sum(1), abs(t.imag).sum(1)] + [(abs(t) ** 2).sum(1)] * 3, axis=1)
    assert np.all(abs(got - want) <= IM.gamma(12) * size)
    assert same_bits(got, IM.moments32(y)), "the tree order of iqbal_core.h is not the restated one"
    # the order matters: neighbours-first gives other bits somewhere in 35 sums
    plain = IM.terms32(y).reshape(5, -1, IM.TILE)
    while plain.shape[2] > 1:
        plain = plain[:, :, 0::2] + plain[:, :, 1::2]
    assert not same_bits(plain[:, :, 0].T, got)


def test_fold_and_solve_bit_for_bit(host):
    rng = np.random.default_rng(3)
    for case, (forget, min_weight, dc) in enumerate(((1.0, 1024.0, 0j), (IM.DEFAULTS["forget"], 4096.0, 0.3 + 0.2j), (0.75, 2048.0, -5 + 1j))):
        x = noise(rng, 12 * IM.TILE)
        y = IM.impair(x, 0.42 + case, 3.0 - 4 * case, dc).astype(np.complex64)
        m = IM.host_moments(host, y)
        P = IM.params(forget=forget, min_weight=min_weight)
        rec = IM.host_records(host, 1)
        N, S = F32(0), np.zeros(5, F32)
        for lo, hi in ((0, 1), (1, 5), (5, 12)):                               # the solve after every call, the state carried on
            IM.host_fold_and_solve(host, P, rec, m[lo:hi])
            N, S, used, skipped = IM.fold32(m[lo:hi], forget, N, S)
            assert same_bits(rec["N"], N) and same_bits(rec["S"][0], S)
            want = IM.solve32(N, S, min_weight)
            for name in IM.SOLVED:
                assert same_bits(rec[name][0], want[name]), (case, hi, name, rec[name][0], want[name])
            assert int(rec["valid"][0]) == want["valid"] == (1 if N >= min_weight else 0)
        assert int(rec["tiles_used"][0]) == 12 and int(rec["tiles_skipped"][0]) == 0
        # and near the float64 solve of the float64 sums
        N64, S64 = IM.fold64(IM.moments64(y), forget)
        w64 = IM.solve64(N64, S64)["w"]
        A = float((abs(y.astype(np.complex128)) ** 2).sum())
        assert abs(complex(rec["w_re"][0], rec["w_im"][0]) - w64) <= IM.margin_w(12, A, N64, IM.solve64(N64, S64)["P"]) + abs(w64) ** 5


def test_fixed_point_against_the_closed_form(host):
    """three steps from w0 = C / 2: the map x -> (C / 2)(1 + |x|^2) contracts with L <= |C| |w| near the root w, and |w0 - w| = (|C| / 2) |w|^2,
    so the truncation is at most (|C| / 2) |w|^2 L^3; the float32 steps add a few u (8 u allowed)"""
    P = IM.params(min_weight=1024.0)
    for mag in (1e-4, 0.01, 0.05, 0.1, 0.2):
        for ang in (0.0, 1.0, 2.5, -2.0):
            Cq = mag * np.exp(1j * ang)
            rec = IM.host_records(host, 1)
            rec["N"], rec["S"] = 1024.0, np.array([0, 0, 1024.0, 1024.0 * Cq.real, 1024.0 * Cq.imag], F32)
            IM.host_fold_and_solve(host, P, rec, np.zeros((0, 5), F32))
            assert rec["valid"][0] == 1
            C32 = complex(rec["C_re"][0], rec["C_im"][0])
            w = C32 / (1 + np.sqrt(1 - abs(C32) ** 2))
            trunc = abs(C32) / 2 * abs(w) ** 2 * (abs(C32) * abs(w) * 1.01) ** 3
            assert abs(complex(rec["w_re"][0], rec["w_im"][0]) - w) <= trunc + 8 * U * abs(w)


@pytest.mark.parametrize("gain_db, phase_deg, dc", [(0.42, 3.0, 0.3 + 0.2j), (-1.0, -5.0, 0j), (0.0, 0.0, -0.1j), (1.5, 8.0, 2 - 1j)])
def test_impairment_then_solve_of_exact_moments_returns_the_image_coefficient(host, gain_db, phase_deg, dc):
    import dabgpu
    S = dabgpu.iqbal_impairment(gain_db, phase_deg, dc)
    K1, K2 = IM.front_end(gain_db, phase_deg)
    assert S.mode == IM.FIXED
    for got, want in ((S.a_re, K1.real), (S.a_im, K1.imag), (S.b_re, K2.real), (S.b_im, K2.imag), (S.c_re, dc.real), (S.c_im, dc.imag)):
        assert F32(got) == F32(want)                                          # double, rounded once
    N = 2.0 ** 20
    power, second = abs(K1) ** 2 + abs(K2) ** 2, 2 * K1 * K2
    state = [dc.real * N, dc.imag * N, (power + abs(dc) ** 2) * N, (second + dc * dc).real * N, (second + dc * dc).imag * N]
    rec = dabgpu.iqbal_solve_host(dabgpu.iqbal_stream(), N, state)
    w = K2 / np.conj(K1)
    Cq = second / power
    trunc = abs(Cq) / 2 * abs(w) ** 2 * (abs(Cq) * abs(w) * 1.01) ** 3
    assert rec["valid"] == 1
    assert abs(complex(rec["w_re"], rec["w_im"]) - w) <= IM.margin_w(0, state[2], N, power) + trunc
    assert abs(complex(rec["b_re"], rec["b_im"]) + w) <= IM.margin_w(0, state[2], N, power) + trunc
    assert abs(complex(rec["d_re"], rec["d_im"]) - dc) <= 4 * U * abs(dc)
    # the corrector undoes the front end up to the gain K1 (1 - |w|^2)
    K1r, K2r = IM.residual(K1, K2, complex(rec["w_re"], rec["w_im"]))
    assert IM.irr_db(K1r, K2r) > -20 * np.log10(IM.margin_w(0, state[2], N, power) + trunc) - 0.1
    assert abs(complex(rec["c_re"], rec["c_im"]) + (dc - w * np.conj(dc))) <= (IM.margin_w(0, state[2], N, power) + trunc + 8 * U) * (abs(dc) + 1e-30)


def test_identity_fallbacks(host):
    ident = dict(a_re=1, a_im=0, b_re=0, b_im=0, c_re=0, c_im=0, valid=0)

    def solved(N, S, min_weight=1024.0):
        rec = IM.host_records(host, 1)
        rec["N"], rec["S"] = N, np.array(S, F32)
        return IM.host_fold_and_solve(host, IM.params(min_weight=min_weight), rec, np.zeros((0, 5), F32))[0]

    fresh = IM.host_records(host, 1)[0]
    assert all(fresh[k] == v for k, v in ident.items()) and fresh["N"] == 0
    for rec in (solved(2048.0, [0, 0, 2048, 100, 50], min_weight=4096.0),      # N too small
                solved(4096.0, [0, 0, 0, 0, 0]),                               # all-zero input: P = 0
                solved(4096.0, [4096, 0, 4096, 4096, 0]),                      # DC only: P = 0
                solved(4096.0, [0, 0, 4096, 4096, 0]),                         # |C| = 1 (a real signal)
                solved(4096.0, [0, 0, 4096, 0, 5000]),                         # |C| > 1
                solved(4096.0, [0, 0, np.inf, 0, 0]),
                solved(4096.0, [0, 0, np.nan, 0, 0])):
        assert all(rec[k] == v for k, v in ident.items()), rec
    x = np.zeros(4 * IM.TILE, np.complex64)
    rec = IM.host_records(host, 1)
    y, _, adv = IM.host_apply(host, [IM.params(min_weight=1024.0, forget=1.0)], rec, x, 0, x.size, IM.MEASURE | IM.APPLY)
    assert adv == x.size and rec["N"][0] == 4096 and rec["valid"][0] == 0 and rec["tiles_used"][0] == 4 and not y.view(np.uint32).any()


def test_a_nan_tile_is_skipped_and_counted_and_any_split_gives_the_same_state(host):
    rng = np.random.default_rng(5)
    x = IM.impair(noise(rng, 10 * IM.TILE), 0.42, 3.0, 0.3 + 0.2j).astype(np.complex64)
    x[3 * IM.TILE + 17] = np.nan
    x[7 * IM.TILE] = np.complex64(complex(np.inf, 0))
    plist = [IM.params(min_weight=1024.0, forget=0.9)]
    one = IM.host_records(host, 1)
    _, m, _ = IM.host_apply(host, plist, one, x, 0, x.size, IM.MEASURE)
    assert int(one["tiles_used"][0]) == 8 and int(one["tiles_skipped"][0]) == 2 and one["valid"][0] == 1
    clean = np.delete(x.reshape(10, IM.TILE), (3, 7), axis=0).reshape(-1)
    ref = IM.host_records(host, 1)
    IM.host_apply(host, plist, ref, clean, 0, clean.size, IM.MEASURE)
    for name in ("N", "S") + IM.SOLVED:
        assert same_bits(one[name], ref[name]), name                           # as if the two tiles had not been there
    for at in range(1, 10):
        two = IM.host_records(host, 1)
        IM.host_apply(host, plist, two, x, 0, at * IM.TILE, IM.MEASURE)
        IM.host_apply(host, plist, two, x[at * IM.TILE:], at * IM.TILE, x.size - at * IM.TILE, IM.MEASURE)
        assert same_bits(two, one), f"split at tile {at}"
    # off a tile edge the model refuses as the device does
    rec = IM.host_records(host, 1)
    assert IM.host_apply(host, plist, rec, x, 31, IM.TILE, IM.MEASURE)[2] == 0 and rec["calls_refused"][0] == 1 and rec["N"][0] == 0


GAIN_DB, PHASE_DEG, DC = 0.42, 3.0, 0.3 + 0.2j
SEEDS = range(8)
OCCUPANCY = {0: 2 * 1536.0 / 8192.0, 30: 1536.0 / 8192.0}                       # the share of the band that carries the power


@pytest.mark.parametrize("neighbour_db", [0, 30])
def test_residual_image_and_dc_after_one_and_four_frames(host, neighbour_db, capsys):
    """float64 and float32 side by side on the two-block signal, 8 seeds.  Asserted: (1) the float32 w and d stay within margin_w and the
    fold's bound of the float64 ones (tests/iqbal_model.py derives both); (2) the float64 residual image is no worse than the 1 / sqrt(N)
    law allows: for a proper Gaussian input E|delta w|^2 = 1 / (2 N_eff), N_eff = N x the occupied share of the band, and ten times that mean
    (probability e^-10 per draw of a complex Gaussian error) is the cap; (3) the DC error likewise against P / N_eff.  The figures
    themselves are printed (and stand in DESIGN.md 4.32)."""
    K1, K2 = IM.front_end(GAIN_DB, PHASE_DEG)
    rows = []
    for seed in SEEDS:
        x = IM.two_blocks(4, neighbour_db, seed)
        x /= np.sqrt(np.mean(abs(x) ** 2))
        y = IM.impair(x, GAIN_DB, PHASE_DEG, DC).astype(np.complex64)
        m32, m64 = IM.host_moments(host, y), IM.moments64(y)
        for frames in (1, 4):
            T = frames * IM.FRAME // IM.TILE
            N64, S64 = IM.fold64(m64[:T])
            want = IM.solve64(N64, S64)
            rec = IM.host_records(host, 1)
            IM.host_fold_and_solve(host, IM.params(forget=1.0), rec, m32[:T])
            w32, d32 = complex(rec["w_re"][0], rec["w_im"][0]), complex(rec["d_re"][0], rec["d_im"][0])
            A = float((abs(y[:T * IM.TILE].astype(np.complex128)) ** 2).sum())
            assert rec["valid"][0] == 1 and rec["N"][0] == N64
            assert abs(w32 - want["w"]) <= IM.margin_w(T, A, N64, want["P"]) + abs(want["w"]) ** 5     # (+ the three-step truncation)
            assert abs(d32 - want["d"]) <= IM.gamma(T + 14) * np.sqrt(A / N64) + 4 * U
            n_eff = N64 * OCCUPANCY[neighbour_db]
            irr64 = IM.irr_db(*IM.residual(K1, K2, want["w"]))
            irr32 = IM.irr_db(*IM.residual(K1, K2, w32))
            assert irr64 >= 10 * np.log10(2 * n_eff) - 10.0
            assert abs(want["d"] - DC) ** 2 <= 10.0 * want["P"] / n_eff
            rows.append((seed, frames, irr64, irr32, abs(want["d"] - DC), abs(d32 - DC), abs(w32 - want["w"])))
    with capsys.disabled():
        print(f"\nneighbour {neighbour_db:+d} dB, raw rejection {IM.irr_db(K1, K2):.1f} dB")
        for frames in (1, 4):
            r = np.array([row[2:] for row in rows if row[1] == frames])
            print(f"  {frames} frame(s): IRR f64 min/median {r[:, 0].min():.1f}/{np.median(r[:, 0]):.1f} dB, f32 {r[:, 1].min():.1f}/{np.median(r[:, 1]):.1f} dB, "
                  f"DC error f64 max {r[:, 2].max():.2e}, f32 max {r[:, 3].max():.2e}, |w32 - w64| max {r[:, 4].max():.2e}")
