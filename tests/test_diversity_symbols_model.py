"""CPU: the symbol-weighted combiner (include/dabgpu.h, "Symbol-weighted receive diversity") -- the numpy rule of
tests/diversity_symbols_model.py against the compiled host model bit for bit (1, 2 and 3 branches, band tables and symbol tables mixed
with branches that have none, weights that are not positive and finite, a dead branch, both layouts), a table of ones against the banded
rule, no table at all against the banded rule, and that the symbol weights leave scale and live mask alone."""
import numpy as np
import pytest

import diversity_model as DM
import diversity_symbols_model as M
import noise_profile_model as PM

F32 = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return M.build_host_model(tmp_path_factory.mktemp("diversity_symbols_host_model"))


@pytest.fixture(scope="module")
def banded_host(tmp_path_factory):
    return PM.build_host_model(tmp_path_factory.mktemp("diversity_symbols_banded_host_model"))


@pytest.fixture(scope="module")
def mapper(host):
    return M.host_mapper(host)


def products(rng, n):
    return [((rng.standard_normal((75, 1536)) + 1j * rng.standard_normal((75, 1536))) * 10.0 ** rng.uniform(3, 5)).astype(np.complex64) for _ in range(n)]


def tables(rng, n, which):
    """which[b] in "-", "b", "s", "bs": no table, a band table, a symbol table, both"""
    band = [(rng.uniform(0.2, 3.0, 128) * 1.0e-4).astype(F32) if "b" in w else None for w in which]
    sym = [rng.uniform(0.01, 1.0, 75).astype(F32) if "s" in w else None for w in which]
    return band, sym


def same(got, want):
    return np.array_equal(got[0], want[0]) and F32(got[1]).view(np.uint32) == F32(want[1]).view(np.uint32) and got[2] == want[2]


@pytest.mark.parametrize("which", [("s",), ("bs",), ("s", "-"), ("-", "bs"), ("b", "s", "bs")])
@pytest.mark.parametrize("layout", [DM.BITS_NATURAL, DM.BITS_MSC_CLASSED])
def test_host_model_equals_numpy_rule(host, mapper, which, layout):
    rng = np.random.Generator(np.random.PCG64(9400 + len(which) + 10 * layout))
    n = len(which)
    dq = products(rng, n)
    k = (rng.uniform(0.5, 2.0, n) * 1.0e-3).astype(F32)
    w = rng.uniform(0.5, 2.0, n).astype(F32)
    band, sym = tables(rng, n, which)
    wa = [None if band[b] is not None else w[b] for b in range(n)]
    ws = None if all(x is None for x in wa) else np.array([1.0 if x is None else x for x in wa], F32)
    want = M.combine_frame(dq, k, mapper, ws, None, band, sym, layout)
    got = M.host_combine_frame(host, dq, k, ws, None, band, sym, layout)
    assert same(got, want) and want[2] == (1 << n) - 1 and np.abs(want[0]).max() > 20


def test_weights_that_are_not_positive_and_finite_erase_their_rows(host, mapper):
    rng = np.random.Generator(np.random.PCG64(9410))
    dq = products(rng, 2)
    k = np.array([1.0e-3, 2.0e-3], F32)
    sym = [rng.uniform(0.1, 1.0, 75).astype(F32), rng.uniform(0.1, 1.0, 75).astype(F32)]
    sym[0][[3, 10, 20, 30]] = [np.nan, -1.0, np.inf, 0.0]
    sym[1][[3, 11]] = [0.0, np.nan]
    want = M.combine_frame(dq, k, mapper, None, None, None, sym)
    got = M.host_combine_frame(host, dq, k, None, None, None, sym)
    assert same(got, want)
    assert not want[0][3 * 3072:4 * 3072].any()                                          # row 3: erased in both branches
    assert want[0][10 * 3072:11 * 3072].any()                                            # row 10: the other branch carries it
    one = M.combine_frame(dq[1:], k[1:], mapper, None, None, None, [np.where(np.arange(75) == 10, sym[1], F32(0)).astype(F32)])
    assert np.array_equal(want[0][10 * 3072:11 * 3072], M.combine_frame(dq, k, mapper, None, None, None,
                                                                         [np.zeros(75, F32), sym[1]])[0][10 * 3072:11 * 3072])
    assert one[2] == 1


def test_symbol_weights_leave_scale_and_live_mask_alone(host, mapper):
    rng = np.random.Generator(np.random.PCG64(9411))
    dq = products(rng, 3)
    k = np.array([1.0e-3, 0.0, 3.0e-3], F32)                                             # branch 1 is dead
    dq[1] = None
    band, sym = tables(rng, 3, ("b", "s", "s"))
    plain = PM.combine_frame(dq, k, mapper, None, None, band)
    for s in (sym, [np.zeros(75, F32)] * 3):
        want = M.combine_frame(dq, k, mapper, None, None, band, s)
        got = M.host_combine_frame(host, dq, k, None, None, band, s)
        assert same(got, want)
        assert F32(want[1]).view(np.uint32) == F32(plain[1]).view(np.uint32) and want[2] == plain[2] == 0b101
    assert not M.combine_frame(dq, k, mapper, None, None, band, [np.zeros(75, F32)] * 3)[0].any()


@pytest.mark.parametrize("layout", [DM.BITS_NATURAL, DM.BITS_MSC_CLASSED])
def test_ones_and_no_tables_are_the_banded_rule(host, banded_host, mapper, layout):
    rng = np.random.Generator(np.random.PCG64(9412 + layout))
    dq = products(rng, 2)
    k = (rng.uniform(0.5, 2.0, 2) * 1.0e-3).astype(F32)
    w = np.array([1.0, 0.7], F32)
    band, _ = tables(rng, 2, ("b", "-"))
    banded = PM.host_combine_frame(banded_host, dq, k, w, None, band, layout)
    assert same(PM.combine_frame(dq, k, mapper, w, None, band, layout), banded)
    ones = np.ones(75, F32)
    for sym in ([ones, ones], [ones, None], [None, ones], [None, None], None):
        assert same(M.host_combine_frame(host, dq, k, w, None, band, sym, layout), banded), sym is None
        assert same(M.combine_frame(dq, k, mapper, w, None, band, sym, layout), banded)
    # no band table either: the scalar rule, and one branch of weight 1 keeps the demodulator's own scale
    scalar = DM.combine_frame(dq[:1], k[:1], mapper, None, None, layout)
    assert same(M.host_combine_frame(host, dq[:1], k[:1], None, None, None, [ones], layout), scalar)
    assert same(M.host_combine_frame(host, dq[:1], k[:1], None, None, None, None, layout), scalar)
    assert F32(scalar[1]).view(np.uint32) == k[:1].view(np.uint32)[0]
