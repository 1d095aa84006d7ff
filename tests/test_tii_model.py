"""CPU: the TII definition (include/dabgpu.h, "TII") in three forms that share no code -- the float64 model of tests/tii_model.py, the
library's host logic (dabgpu_tii_pattern / _carriers / _main_id) and the float32 host model (csrc/tii_core.h by g++ around the oracle's
PLL and transform) -- and the derivation of the default threshold."""
import itertools

import numpy as np
import pytest

import tii_model as M


@pytest.fixture(scope="module")
def dabgpu():
    import os
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(M.ROOT, "dab-radio_amd", "libdabgpu.so")):
        g.build()
    import dabgpu
    return dabgpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("tii_host_model"))


def test_pattern_table(dabgpu, host):
    T = M.TABLE
    assert len(T) == 70 and T[:3] == [0x0F, 0x17, 0x1B] and T[69] == 0xF0
    assert all(bin(v).count("1") == 4 for v in T) and T == sorted(set(T))
    assert [dabgpu.tii_pattern(p) for p in range(70)] == T == [host.tii_host_pattern(p) for p in range(70)]
    assert dabgpu.tii_pattern(-1) == dabgpu.tii_pattern(70) == -1
    L = dabgpu.lib()
    for mask in range(256):
        want = T.index(mask) if mask in T else -1
        assert L.dabgpu_tii_main_id(mask) == want == host.tii_host_main_id(mask)
    assert L.dabgpu_tii_main_id(0x10F) == -1 and L.dabgpu_tii_main_id(0xF0000000) == -1
    assert M.a(0, 4) == 1 and M.a(0, 3) == 0 and M.a(69, 0) == 1           # a_b = bit 7 - b


def test_carriers_of_every_pair(dabgpu):
    sets = {}
    for p in range(70):
        for c in range(24):
            ks = M.carriers(p, c)
            assert list(dabgpu.tii_carriers(p, c)) == ks
            assert len(ks) == 32 == len(set(ks)) and 0 not in ks and min(ks) >= -768 and max(ks) <= 768
            assert all(k1 == k0 + 1 for k0, k1 in zip(ks[0::2], ks[1::2]))
            sets[(p, c)] = frozenset(ks)
    assert len(set(sets.values())) == 1680
    combs = [frozenset().union(*(sets[(p, c)] for p in range(70))) for c in range(24)]
    assert all(len(s) == 64 for s in combs)
    assert all(combs[i].isdisjoint(combs[j]) for i in range(24) for j in range(i))
    assert frozenset().union(*combs) == frozenset(k for k in range(-768, 769) if k != 0)


def test_default_threshold_derivation(dabgpu):
    thr, root = M.derive_threshold(frames=2, target=1e-6, step=0.01)
    assert thr == pytest.approx(dabgpu.TII_DEFAULT_THRESHOLD, abs=1e-9) and dabgpu.TII_DEFAULT_THRESHOLD == 2.16
    assert thr - 0.01 < root <= thr
    assert M.false_alarm_probability(thr, 2) < 1e-6 <= M.false_alarm_probability(thr - 0.01, 2)
    # the Monte Carlo resolves it: another seed moves the root by far less than the step, and more frames only lower the probability
    assert abs(root - M.derive_threshold(2, seed=7)[1]) < 0.002
    assert M.false_alarm_probability(thr, 2, seed=7) < 1e-6 <= M.false_alarm_probability(thr - 0.01, 2, seed=7)
    assert M.false_alarm_probability(thr, 4) < M.false_alarm_probability(thr, 2)
    cfg = np.zeros(2, np.float32)
    dabgpu.lib().dabgpu_tii_cfg_default(cfg.ctypes.data)
    assert cfg[0] == np.float32(2.16)
    # the formula against a direct simulation where one can afford it (threshold 1.6: about 1 decision in 40)
    rng = np.random.Generator(np.random.PCG64(99))
    g = rng.gamma(16, 1.0, (40000, 24, 8))
    s = np.sort(g, axis=2)
    floor = s[:, :, :4].mean(axis=(1, 2))
    hit = float(np.mean((s[:, :, 4] >= 1.6 * floor[:, None]).any(axis=1)))
    p = M.false_alarm_probability(1.6, 2)
    assert abs(hit - (p - p * p / 2)) < 5 * np.sqrt(hit / 40000)


def test_sort_network(host):
    for bits in itertools.product([0.0, 1.0], repeat=8):                    # the 0-1 principle
        v, s = np.array(bits, np.float32), np.zeros(8, np.float32)
        host.tii_host_sort8(v.ctypes.data, s.ctypes.data)
        assert list(s) == sorted(bits)


def test_host_model_against_float64_model(oracle, host):
    """three transmitters (two on one comb), echo, offset, noise: the float32 model's energies inside float32's reach of the float64
    model's, its records identical (strength to 1e-4)"""
    prs = oracle.prs_fft()
    rng = np.random.default_rng(3300)
    x = M.null_period(prs, [(11, 5, 1.0), (40, 17, 0.5), (33, 17, 0.7)])
    cfo = 3.05 / 2048
    m32 = M.HostModel(host, oracle, 2.16)
    acc64 = np.zeros((24, 8))
    for f in range(3):
        s = np.zeros(4000, np.complex128)
        s[137:137 + 2656] += x
        s[337:337 + 2656] += 0.5 * x
        s *= np.exp(2j * np.pi * cfo * np.arange(4000))
        s += 1.5 * (rng.standard_normal(4000) + 1j * rng.standard_normal(4000))
        s = s.astype(np.complex64)
        m32.process(s, 137, np.float32(-cfo))
        acc64 += M.window_energy(s, 137, float(np.float32(-cfo)))
        assert np.allclose(m32.acc.reshape(24, 8), acc64, rtol=2e-4, atol=0)
        r32, r64 = m32.decide(), M.decide(acc64, 2.16)
        assert M.records_as_tuples(r32) == [t[:3] for t in r64] == [(5, 11, M.TABLE[11]), (17, -1, M.TABLE[40] | M.TABLE[33])]
        assert np.allclose(r32["strength"], [t[3] for t in r64], rtol=1e-4)
    # no energy at all: no record; one comb lit on a flat floor: its record alone
    assert len(M.HostModel(host, oracle, 2.16).decide()) == 0 and M.decide(np.zeros(192), 2.16) == []
    flat = np.ones((24, 8), np.float32)
    flat[9, [0, 2, 5, 7]] = 50.0
    m32.acc = flat.reshape(-1).copy()
    assert M.records_as_tuples(m32.decide()) == [(9, M.TABLE.index(0xA5), 0xA5)] == [t[:3] for t in M.decide(flat, 2.16)]


def test_noise_alone_gives_no_record(oracle, host):
    rng = np.random.default_rng(3400)
    m = M.HostModel(host, oracle, 2.16)
    for seed in range(64):
        m.reset()
        for f in range(2):
            s = (rng.standard_normal(2656) + 1j * rng.standard_normal(2656)).astype(np.complex64)
            m.process(s, 0, np.float32(1e-3))
        assert len(m.decide()) == 0, seed
