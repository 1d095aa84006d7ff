"""CPU: the arithmetic contract of receive diversity.  The numpy float32 model (tests/diversity_model.py) against the compiled header
(dab-radio_amd/csrc/diversity_core.h under g++ -ffp-contract=off, tests/cpp/diversity_host_model.cpp) bit for bit -- live rule, scale,
weighted sum, soft bits, both layouts; the scale and the quantiser's arguments against a float64 evaluation inside a derived bound; the
single-branch identity against the demodulator's weighted soft bits (tests/softbit_model.py)."""
import itertools

import numpy as np
import pytest

import diversity_model as DM
import softbit_model as SM

F32 = np.float32
U = 2.0 ** -24
SHAPE = (DM.NB_DATA_SYMBOLS, DM.NB_CARRIERS)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return DM.build_host_model(tmp_path_factory.mktemp("diversity_host_model"))


@pytest.fixture(scope="module")
def mapper(host):
    return DM.host_mapper(host)


def bits_of(x):
    return np.asarray(x, dtype=F32).view(np.uint32)


def products(rng, n, gain=1.0):
    return [((rng.standard_normal(SHAPE) + 1j * rng.standard_normal(SHAPE)) * gain * (1 + 0.3 * b)).astype(np.complex64) for b in range(n)]


def gamma(n):
    return n * U / (1 - n * U)


def test_reciprocal_over_the_whole_range(host):
    """every exponent, random mantissas: the model equals the header, and the result is the float64 reciprocal within one ulp of a
    normal result (2 u relative); below the normal range of the RESULT one more absolute rounding of 2^-150.  An argument below the
    normal range, zero or NaN gives +infinity."""
    rng = np.random.default_rng(9500)
    for e in range(-126, 128):
        for _ in range(4):
            x = F32(np.ldexp(1.0 + rng.random(), e))
            r, rh = DM.reciprocal(x), F32(host.dvm_reciprocal(x))
            assert bits_of(r) == bits_of(rh), (e, x)
            exact = 1.0 / float(x)
            assert abs(float(r) - exact) <= 2 * U * exact + 2.0 ** -150, (e, x, r)
    for x in (1.0, 2.0, 0.5, 3.0, 2.0 ** 127, 2.0 ** -126, float(SM.FLT_MAX)):
        assert bits_of(DM.reciprocal(x)) == bits_of(host.dvm_reciprocal(F32(x)))
    assert DM.reciprocal(1.0) == 1 and DM.reciprocal(4.0) == 0.25
    for x in (0.0, 2.0 ** -127, 2.0 ** -149, np.nan, -1.0):
        assert np.isposinf(DM.reciprocal(x)) and np.isposinf(F32(host.dvm_reciprocal(F32(x))))


def test_live_rule(host):
    for k, w, ok in ((1.0, 1.0, True), (0.0, 1.0, False), (-1.0, 1.0, False), (np.nan, 1.0, False), (np.inf, 1.0, False), (1.0, 0.0, False),
                     (1.0, -2.0, False), (1.0, np.nan, False), (1.0, np.inf, False), (2.0 ** -149, 1.0, True), (float(SM.FLT_MAX), 2.0 ** -149, True)):
        for sync in (0, 1):
            assert DM.live(sync, k, w) == (ok and sync == 1) == bool(host.dvm_branch_live(sync, F32(k), F32(w))), (k, w, sync)


def test_scale_equals_the_compiled_header_bit_for_bit(host):
    """K = 1, 2, 3, 8; every live / dead pattern for K = 3 by sync flag, by scale and by weight; weights; scales at the ends of the
    float range; both host entries (the header's function and the library's dabgpu_diversity_scale_host)"""
    rng = np.random.default_rng(9501)
    n_checked = n_zero = 0
    specials = [0.0, -1.0, np.nan, np.inf, 2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 2.0 ** 127, float(SM.FLT_MAX), 1.0, 64.0 / 3]

    def check(k, w, valid):
        nonlocal n_checked, n_zero
        a, ma = DM.scale(k, w, valid)
        for entry in ("dvm_scale", "dabgpu_diversity_scale_host"):
            b, mb = DM.host_scale(host, k, w, valid, entry)
            assert bits_of(a) == bits_of(b) and ma == mb, (k, w, valid, a, b, ma, mb)
        assert np.isfinite(a) and a >= 0
        n_checked += 1
        n_zero += int(a == 0)
        return a, ma

    for n in (1, 2, 3, 8):
        for _ in range(60):
            k = np.exp(rng.uniform(-20, 20, n)).astype(F32)
            check(k, None, None)
            check(k, np.exp(rng.uniform(-8, 8, n)).astype(F32), None)
            check(k, np.ones(n, F32), rng.integers(0, 2, n))
    for kill in itertools.product((None, "sync", "scale", "weight"), repeat=3):
        k, w, v = np.array([0.7, 1.9, 0.31], F32), np.array([1.0, 0.5, 3.0], F32), np.ones(3, np.int32)
        for b, how in enumerate(kill):
            if how == "sync": v[b] = 0
            if how == "scale": k[b] = 0
            if how == "weight": w[b] = 0
        a, m = check(k, w, v)
        assert m == sum(1 << b for b, how in enumerate(kill) if how is None)
        assert (a == 0) == (m == 0)
    for ks in itertools.product(specials, repeat=2):
        check(np.array(ks, F32), None, None)
        check(np.array(ks, F32), np.array([2.0, 2.0 ** -100], F32), None)
        check(np.array(ks + (1.0,), F32), np.array([2.0 ** 100, 1.0, 2.0 ** -149], F32), [1, 1, 1])
    # the stated exception: one live branch of weight exactly 1 keeps its scale, whatever it is; weight 2 goes through the formula
    for k1 in (0.37, 2.0 ** -149, float(SM.FLT_MAX), 2.0 ** -127):
        assert bits_of(check([0.0, k1, np.nan], None, None)[0]) == bits_of(F32(k1))
        assert bits_of(check([5.0, k1], None, [0, 1])[0]) == bits_of(F32(k1))
    assert check([0.5], [2.0], None)[0] == F32(0.25)
    assert check([2.0 ** -149], [2.0], None)[0] == 0                   # a scale whose reciprocal no float holds: erased
    assert check([0.0, np.nan], None, None) == (0, 0)
    assert n_checked > 1000 and n_zero > 20
    for n in (0, 9, -1):
        assert host.dabgpu_diversity_scale_host(np.ones(16, F32).ctypes.data, None, None, n, None) == 0


def test_scale_is_held_by_a_float64_evaluation(host):
    """k against 1 / sum w_b / k_b in float64.  Each reciprocal lies within one ulp of the exact one (2 u); the sum of n positive
    terms is a chain of n fused steps, a term passes through at most n roundings ((1 + u)^n - 1 <= gamma_n = n u / (1 - n u)); so the sum
    s is off by at most a = (1 + 2 u)(1 + gamma_n) - 1 relative, and k = (1 / s)(1 + 2 u) by at most (a + 2 u) / (1 - a)."""
    rng = np.random.default_rng(9502)
    worst = 0.0
    for n in (2, 3, 8):
        a = (1 + 2 * U) * (1 + gamma(n)) - 1
        bound = (a + 2 * U) / (1 - a)
        for _ in range(300):
            k = np.exp(rng.uniform(-15, 15, n)).astype(F32)
            w = np.exp(rng.uniform(-6, 6, n)).astype(F32)
            got, _ = DM.host_scale(host, k, w)
            exact = 1.0 / float(np.sum(w.astype(np.float64) / k.astype(np.float64)))
            err = abs(float(got) - exact) / exact
            worst = max(worst, err / bound)
            assert err <= bound, (n, k, w, got, exact)
    print(f"scale against float64: worst error {worst:.2f} of the bound")
    assert worst > 0
    # k = L 1536 / (2048 sum w_b P_b): the combined scale of branches demodulated at one level is the scale of their summed power
    P = np.array([0.8, 2.5, 0.03], np.float64)
    kb = np.array([SM.scale(64.0, F32(p)) for p in P], F32)
    got, _ = DM.host_scale(host, kb)
    assert abs(float(got) - 64.0 * 1536 / (2048 * P.astype(F32).astype(np.float64).sum())) <= 16 * U * float(got)


def frame_case(rng, n, weights, dead=()):
    dq = products(rng, n)
    k = (30 * n * np.exp(rng.uniform(-1, 1, n))).astype(F32)           # the combined scale lands near 30: soft bits over the whole range
    w = np.exp(rng.uniform(-2, 2, n)).astype(F32) if weights else None
    valid = np.ones(n, np.int32)
    for b in dead:
        valid[b] = 0
        dq[b] = None                                                  # never read: the host model is handed a null address
    return dq, k, w, valid


@pytest.mark.parametrize("n,weights,dead", [(1, False, ()), (1, True, ()), (2, False, ()), (2, True, ()), (3, True, (1,)), (3, False, (0, 2)),
                                            (8, True, ()), (8, False, (0, 3, 7)), (2, False, (0, 1))])
def test_frames_equal_the_compiled_header_bit_for_bit(host, mapper, n, weights, dead):
    rng = np.random.default_rng(9503 + n)
    dq, k, w, valid = frame_case(rng, n, weights, dead)
    for layout in (DM.BITS_NATURAL, DM.BITS_MSC_CLASSED):
        bits, kk, mask = DM.combine_frame(dq, k, mapper, w, valid, layout)
        hb, hk, hm = DM.host_combine_frame(host, dq, k, w, valid, layout)
        assert bits_of(kk) == bits_of(hk) and mask == hm == sum(1 << b for b in range(n) if b not in dead)
        assert np.array_equal(bits, hb)
        assert bits.min() >= -127
        if mask == 0:
            assert not bits.any() and kk == 0
        else:
            assert np.abs(bits.astype(np.int32)).mean() > 5            # the frame carries something
    # the class order is a permutation of the MSC rows and leaves the FIC alone
    nat = DM.combine_frame(dq, k, mapper, w, valid)[0]
    cls = DM.combine_frame(dq, k, mapper, w, valid, DM.BITS_MSC_CLASSED)[0]
    assert np.array_equal(nat[:DM.FIC_BITS], cls[:DM.FIC_BITS])
    i = np.arange(DM.CIF_BITS)
    for q in range(4):
        a = DM.FIC_BITS + q * DM.CIF_BITS
        assert np.array_equal(cls[a + (i % 16) * 3456 + i // 16], nat[a + i])


def test_non_finite_products_and_extreme_scales(host, mapper):
    """NaN and infinite products in a live branch propagate through the sum and end as 0 / +-127; a dead branch's NaNs are never seen;
    scales at the ends of the float range erase or saturate, model and header alike"""
    rng = np.random.default_rng(9510)
    dq = products(rng, 3)
    dq[0][3, 100] = complex(np.nan, 1.0); dq[0][3, 101] = complex(np.inf, -np.inf); dq[1][3, 101] = complex(-np.inf, 2.0)
    dq[1][10, 5] = complex(3e38, -3e38); dq[0][10, 5] = complex(3e38, -3e38)
    poisoned = np.full(SHAPE, np.nan + 1j * np.nan, np.complex64)
    for k, w, valid, d in (([1.0, 2.0, 0.5], None, None, dq),
                           ([1.0, 2.0, 0.5], [1.0, 1.0, 1.0], [1, 1, 0], dq[:2] + [poisoned]),
                           ([1.0, 0.0, 0.5], [1.0, 1.0, 0.0], None, [dq[0], poisoned, poisoned]),
                           ([2.0 ** -149, 1.0, 1.0], None, None, dq),                 # 1 / k_0 is not a float: the frame is erased
                           ([float(SM.FLT_MAX), float(SM.FLT_MAX), 1e30], None, None, dq),
                           ([2.0 ** -126, 2.0 ** -126, 2.0 ** -120], [1.0, 2.0 ** -20, 1.0], None, dq),
                           ([2.0 ** 127, 2.0 ** 127, 2.0 ** 127], [2.0 ** -149, 2.0 ** -149, 2.0 ** -149], None, dq)):
        for layout in (DM.BITS_NATURAL, DM.BITS_MSC_CLASSED):
            bits, kk, mask = DM.combine_frame(d, k, mapper, w, valid, layout)
            hb, hk, hm = DM.host_combine_frame(host, d, k, w, valid, layout)
            assert bits_of(kk) == bits_of(hk) and mask == hm and np.array_equal(bits, hb), (k, w, valid)
            if kk == 0:
                assert not bits.any()
    bits, kk, mask = DM.combine_frame(dq, [1.0, 2.0, 0.5], mapper)
    inv = np.argsort(mapper)
    assert kk > 0 and mask == 7
    assert bits[3 * 3072 + inv[100]] == 0                               # NaN -> 0
    assert bits[3 * 3072 + inv[101]] == 0                               # inf - inf = NaN -> 0
    assert bits[10 * 3072 + inv[5]] == -127 and bits[10 * 3072 + 1536 + inv[5]] == -127        # overflow of the sum saturates
    erased = DM.combine_frame(dq, [2.0 ** -149, 1.0, 1.0], mapper)
    assert erased[1] == 0 and erased[2] == 7 and not erased[0].any()


def test_soft_bit_arguments_are_held_by_a_float64_evaluation(host, mapper):
    """v = -(S k), S = sum w_b c_b, against float64.  With A = sum |w_b c_b|: the computed sum is off by at most gamma_n A (a term of
    the chain passes through at most n roundings: its product or fused step, then the later steps); k by at most E = (a + 2 u) / (1 - a),
    a = (1 + 2 u)(1 + gamma_n) - 1 (the scale's test); the product rounds once.  So
    |v - v64| <= k64 (|S| (E + u + E u) + gamma_n A (1 + E)(1 + u)).  Products of order one, scales of some tens: nothing leaves the
    normal range, so no absolute rounding term enters.  The single branch of weight 1 has k exact and lies inside the same bound."""
    rng = np.random.default_rng(9520)
    worst = 0.0
    for n, weights in ((1, False), (2, False), (3, True), (8, True)):
        dq, k, w, valid = frame_case(rng, n, weights)
        first, second, kk, mask = DM.combine_frame(dq, k, mapper, w, valid, values=True)
        hb, hk, hm, sums = DM.host_combine_frame(host, dq, k, w, valid, sums=True)
        assert bits_of(kk) == bits_of(hk)
        ww = np.ones(n) if w is None else w.astype(np.float64)
        k64 = 1.0 / float(np.sum(ww / k.astype(np.float64)))
        terms = np.stack([ww[b] * dq[b].astype(np.complex128) for b in range(n)])
        S = terms.sum(axis=0)
        A_re, A_im = np.abs(terms.real).sum(axis=0), np.abs(terms.imag).sum(axis=0)
        a = (1 + 2 * U) * (1 + gamma(n)) - 1
        E = (a + 2 * U) / (1 - a)
        for got, s64, A in ((first, -S.real[:, mapper], A_re[:, mapper]), (second, S.imag[:, mapper], A_im[:, mapper])):
            bound = k64 * (np.abs(s64) * (E + U + E * U) + gamma(n) * A * (1 + E) * (1 + U))
            err = np.abs(got.astype(np.float64) - s64 * k64)
            assert (err <= bound).all(), (n, float((err / bound).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        # the compiled header's sums are the model's
        re, im = DM.weighted_sum(dq, w, mask)
        assert np.array_equal(re.view(np.uint32), sums.real.view(np.uint32)) and np.array_equal(im.view(np.uint32), sums.imag.view(np.uint32))
    print(f"quantiser arguments against float64: worst error {worst:.2f} of the bound")
    assert 0 < worst <= 1


def test_one_branch_of_weight_one_is_the_weighted_demodulator(host, mapper):
    """K = 1, w = 1 (no weights, or a weight of exactly 1): the frame equals softbit_model.frame_bits with the branch's own scale"""
    rng = np.random.default_rng(9530)
    dq = products(rng, 1)
    for k in (F32(0.37), SM.scale(64.0, F32(1.7)), F32(2.0 ** -149), F32(0.0)):
        exp = SM.frame_bits(dq[0], mapper, k)
        for w in (None, [1.0]):
            for fn in (lambda: DM.combine_frame(dq, [k], mapper, w), lambda: DM.host_combine_frame(host, dq, [k], w)):
                bits, kk, mask = fn()
                assert np.array_equal(bits, exp) and bits_of(kk) == bits_of(k) and mask == int(k > 0)
    # a dead second branch changes nothing; a weight of 2 on the single branch does not take the exception but lands on the same bits
    # for a power-of-two weight (the sum doubles, the scale halves, both exactly)
    k = F32(0.37)
    exp = SM.frame_bits(dq[0], mapper, k)
    assert np.array_equal(DM.combine_frame([None, dq[0]], [0.0, k], mapper)[0], exp)
    two = DM.combine_frame(dq, [k], mapper, [2.0])
    assert abs(float(two[1]) - float(k) / 2) <= 4 * U * float(k) and (np.abs(two[0].astype(int) - exp.astype(int)) <= 1).all()
