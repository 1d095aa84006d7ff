"""CPU: the arithmetic contract of the channel-state weighted soft bits.  The numpy float32 model (tests/softbit_model.py) against the
compiled header (dab-radio_amd/csrc/softbit_csi_core.h under g++ -ffp-contract=off, tests/cpp/softbit_host_model.cpp) bit for bit; the
scale against a float64 evaluation inside a derived bound; the erasure, clamp and NaN rules; the level's edges; and the model's
normalised policy against the oracle's dab_dqpsk_demap."""
import ctypes as C

import numpy as np
import pytest

import softbit_model as SM

F32 = np.float32
U = 2.0 ** -24


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return SM.build_host_model(tmp_path_factory.mktemp("softbit_host_model"))


def bits_of(x):
    return np.asarray(x, dtype=F32).view(np.uint32)


def prs_cases():
    rng = np.random.default_rng(9300)
    out = []
    for scale in (1.0, 1e-3, 300.0, 2.0 ** -70, 2.0 ** -64, 2.0 ** 60, 2.0 ** 63, 2.0 ** -20, 1e4):
        x = (rng.standard_normal(2048) + 1j * rng.standard_normal(2048)) * scale
        out.append(x.astype(np.complex64))
    q = (rng.integers(0, 256, (2048, 2)).astype(np.float32) - F32(127.5)) * (F32(1) / F32(127.5))        # what the u8 loader delivers
    out.append(q.view(np.complex64).reshape(-1))
    out.append(np.zeros(2048, np.complex64))
    one = np.zeros(2048, np.complex64); one[777] = 3.0 - 4.0j
    out.append(one)
    for bad in (np.nan, np.inf, -np.inf):
        x = out[0].copy(); x[1234] = complex(bad, 1.0)
        out.append(x)
    return out


def test_frame_power_and_scale_equal_the_compiled_header_bit_for_bit(host):
    n_zero = 0
    for x in prs_cases():
        P, Ph = SM.frame_power(x), SM.host_frame_power(host, x)
        assert bits_of(P) == bits_of(Ph) or (np.isnan(P) and np.isnan(Ph))
        for level in (1.0, 64.0, 127.0, 33.3):
            k, kh = SM.scale(level, P), SM.host_scale(host, level, Ph)
            assert bits_of(k) == bits_of(kh), (level, P, k, kh)
            assert bits_of(k) == bits_of(host.dabgpu_soft_scale_host(np.ascontiguousarray(x).ctypes.data, F32(level)))
            assert np.isfinite(k) and k >= 0
            n_zero += int(k == 0)
    assert n_zero >= 4 * 6                         # zero power, the overflowing and vanishing scales, NaN and the infinities: erased


def test_scale_over_the_whole_range_of_the_power(host):
    """every exponent of P, random mantissas: the model equals the header, and where k is a number it is the float64 quotient to a
    relative 4 u (the level's product, the quotient within one ulp = 2 u, and the comparison's own rounding)"""
    rng = np.random.default_rng(9301)
    for e in range(-149, 128):
        for _ in range(3):
            P = F32(np.ldexp(1.0 + rng.random(), e))
            level = F32(1.0 + 126.0 * rng.random())
            k, kh = SM.scale(level, P), SM.host_scale(host, level, P)
            assert bits_of(k) == bits_of(kh), (e, P, level)
            exact = float(level) * 1536.0 / (2048.0 * float(P)) if P > 0 else np.inf
            den = 2048.0 * float(P)
            if den > float(SM.FLT_MAX) or den < float(SM.FLT_MIN) or exact > float(SM.FLT_MAX):
                assert k == 0 or exact <= float(SM.FLT_MAX) * (1 + 4 * U)
            else:
                assert abs(float(k) - exact) <= 4 * U * exact, (e, P, level, k, exact)
    for P in (0.0, -0.0, np.nan, np.inf, -1.0):
        assert SM.scale(64.0, P) == 0 and SM.host_scale(host, 64.0, P) == 0


def test_scale_is_held_by_a_float64_evaluation(host):
    """k against level * 1536 / (2048 sum |x|^2) in float64.  The power is a sum of 4096 non-negative squares: a lane's chain rounds 16
    times (one product, 15 fused steps), the fold over lanes 6 times, the join twice -- no term passes through more than 24 roundings,
    and as no term is negative the relative error of P is at most 24 u to first order.  The level's product rounds once (u), the
    quotient lies within one ulp (2 u), the powers of two are exact: 27 u, taken as 27 u / (1 - 27 u) for the higher orders.  Where
    squares fall below the normal range (the frame scaled by 2^-64) a rounding is absolute, at most 2^-150: 4096 in the chains and 255
    additions, 4351 x 2^-150 over P."""
    rel = 27 * U / (1 - 27 * U)
    worst = 0.0
    for x in prs_cases():
        P64 = float(np.sum(x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2))
        for level in (1.0, 64.0, 127.0, 33.3):
            k = float(host.dabgpu_soft_scale_host(np.ascontiguousarray(x).ctypes.data, F32(level)))        # the compiled header itself
            assert F32(k).view(np.uint32) == SM.soft_scale(x, level).view(np.uint32)
            if not np.isfinite(P64) or P64 == 0 or k == 0:
                continue
            exact = float(F32(level)) * 1536.0 / (2048.0 * P64)
            bound = rel + (4351 * 2.0 ** -150 / P64) * (1 + rel)
            if bound == rel:
                worst = max(worst, abs(k - exact) / exact)
            assert abs(k - exact) <= bound * exact, (level, P64, k, exact)
    print(f"scale against float64: worst relative error {worst / U:.2f} u where no square underflows, bound {rel / U:.2f} u")
    assert worst > 0


def test_soft_bits_equal_the_compiled_header_and_keep_their_rules(host):
    rng = np.random.default_rng(9302)
    d = ((rng.standard_normal(6000) + 1j * rng.standard_normal(6000)) * np.exp(rng.uniform(-12, 12, 6000))).astype(np.complex64)
    edge = np.array([0, -0.0, 1, -1, 127, -127, 127.5, -127.5, 128, -128, 1e30, -1e30, np.inf, -np.inf, np.nan, 126.999, -126.999, 0.999, -0.999,
                     2.0 ** -140, 3.4e38], np.float32)
    grid = np.empty((edge.size, edge.size), np.complex64)
    grid.real, grid.imag = edge[:, None], edge[None, :]
    d = np.concatenate([d, grid.reshape(-1)])
    for k in (F32(1.0), F32(0.0), F32(64.0 / 3.0), F32(1e-30), F32(3e38), F32(2.0 ** -120), F32(0.37)):
        a, b = SM.csi_bits(d, k)
        ha, hb = SM.host_soft_bits(host, d, k)
        assert np.array_equal(a, ha) and np.array_equal(b, hb)
        assert a.min() >= -127 and b.min() >= -127 and a.max() <= 127 and b.max() <= 127            # -128 never leaves
        if k == 0:
            # an erased frame: every soft bit 0 -- also where the product is infinite or NaN (inf * 0 = NaN -> 0)
            assert not a.any() and not b.any()
    a, b = SM.csi_bits(d, F32(1.0))
    assert (a[np.isnan(d.real)] == 0).all() and (b[np.isnan(d.imag)] == 0).all()                     # a NaN component gives 0
    assert (a[d.real >= 127] == -127).all() and (a[d.real <= -127] == 127).all()                     # the clamp, with the sign of to_vbit
    assert (b[d.imag >= 127] == 127).all() and (b[d.imag <= -127] == -127).all()
    x = np.array([126.999 + 0.999j, -5.5 - 5.5j], np.complex64)
    assert SM.csi_bits(x, 1.0)[0].tolist() == [-126, 5] and SM.csi_bits(x, 1.0)[1].tolist() == [0, -5]   # towards zero


def test_level_edges_and_refusals(host):
    for ok in (1.0, 127.0, 64.0, 1.0000001):
        assert host.sbm_level_ok(F32(ok)) == 1
    for bad in (0.0, 0.99999, 127.00001, -64.0, np.nan, np.inf, -np.inf, 128.0):
        assert host.sbm_level_ok(F32(bad)) == 0
        assert host.dabgpu_soft_scale_host(np.ones(4096, np.float32).ctypes.data, F32(bad)) == 0
    x = prs_cases()[0]
    k1, k127 = SM.soft_scale(x, 1.0), SM.soft_scale(x, 127.0)
    assert k1 > 0 and abs(float(k127) / float(k1) - 127.0) <= 127.0 * 8 * U
    cfg = (C.c_int * 2)()
    host.dabgpu_soft_cfg_default(cfg)
    assert cfg[0] == SM.SOFT_NORMALISED and np.array([cfg[1]], np.int32).view(F32)[0] == 64.0


def test_policy_normalised_is_the_oracles_demapper(oracle):
    rng = np.random.default_rng(9303)
    m = oracle.mapper()
    for scale in (1.0, 2.0 ** -40, 2.0 ** 50):
        x0 = ((rng.standard_normal(2048) + 1j * rng.standard_normal(2048)) * scale).astype(np.complex64)
        x1 = ((rng.standard_normal(2048) + 1j * rng.standard_normal(2048)) * scale).astype(np.complex64)
        x1[5] = 0
        exp = oracle.dqpsk_demap(x0, x1, m)
        c = np.arange(1536)
        bins = np.where(c < 768, c - 768, c - 768 + 1) % 2048                                       # carrier order -> transform bins
        got = SM.symbol_bits(SM.dqpsk(x0[bins], x1[bins]), m)
        assert np.array_equal(got, exp)
