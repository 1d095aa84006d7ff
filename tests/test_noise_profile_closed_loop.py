"""CPU: what the band weights buy, end to end (tests/noise_profile_loop.py): the transmission of tests/channel_loop.py through its
two-path channel at 9 dB with a band-limited interferer 96 carriers wide 300.3 spacings above the centre, received frame by frame,
decoded once from the demodulator's weighted soft bits and once from the banded combiner over the one branch with the band weights the
float32 models take from each frame's NULL.  The operating point I / S = 0 dB, and 3 dB either side, was re-established with these
models by the sweep DESIGN 4.27 records (none, -12 .. +6 dB): the band weights deliver every FIB and byte at both alphas where the plain
soft bits lose nearly all; without an interferer both deliver.  A second branch with an interferer of its own elsewhere in the block: each
branch alone and their unit-weight sum fail, the banded pair delivers."""
import numpy as np
import pytest

import channel_loop as CL
import noise_model as NM
import noise_profile_loop as PL
import noise_profile_model as PM


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    return PL.Loop(oracle, tmp_path_factory.mktemp("noise_profile_loop"))


@pytest.mark.parametrize("is_db", [PL.POINT_DB - 3.0, PL.POINT_DB, PL.POINT_DB + 3.0])
def test_band_weights_deliver_where_plain_soft_bits_do_not(loop, is_db):
    plain = loop.plain(is_db)
    banded = {a: loop.banded(is_db, alpha=a) for a in PL.ALPHAS}
    print(f"I / S {is_db} dB: plain {plain}, banded {banded}")
    assert loop.branch(is_db, "A")["valid"].all()                      # no frame refused: the difference is the weights'
    for a in PL.ALPHAS:
        assert banded[a] == PL.DELIVERED
    assert plain[0] < 12 * CL.N_FRAMES and plain[1] > 0


def test_without_an_interferer_the_weighting_costs_nothing(loop):
    assert loop.branch(None, "A")["valid"].all()
    assert loop.plain(None) == PL.DELIVERED
    for a in PL.ALPHAS:
        assert loop.banded(None, alpha=a) == PL.DELIVERED


def test_profile_follows_the_interferer(loop):
    """the weights behind the counts at the operating point: the interferer covers carriers +252.3 .. +348.3, places 1019.3 .. 1115.3 of
    the 1536, so bands 85 .. 91 lie wholly under it; the bands well clear of it keep the noise floor of the 9 dB channel within five
    deviations of a band, and the bands under it sit at the interferer's density, 2048 / 96 of its power, over the floor"""
    b = loop.branch(PL.POINT_DB, "A")
    sigma2 = 2.0 * CL.sigma_for(loop.iq, PL.SNR_DB) ** 2
    w = b["w"][1.0]
    lo, hi = int(768 + 252.3 - 1) // 12, int(768 + 348.3 - 1) // 12
    inside = np.arange(lo + 1, hi)                                      # whole bands under it
    clear = np.r_[0:lo - 2, hi + 3:128]
    # a band's value over its mean is a Gamma(12) draw over 12, whose tails are not a normal's: the interval it leaves with probability
    # 1e-9 on either side, from the distribution function itself (some 600 values are looked at)
    t = np.arange(0.01, 8.0, 0.01)
    cdf = NM.gamma_cdf(12, 12.0 * t)
    low, high = t[cdf < 1e-9].max(), t[1.0 - cdf < 1e-9].min()
    ratio = 1.0 / w[:, clear] / sigma2
    assert (ratio > low).all() and (ratio < high).all(), (ratio.min(), ratio.max(), low, high)
    assert abs(ratio.mean() - 1.0) < 4.0 * PM.relative_deviation() / np.sqrt(ratio.size)
    # under the interferer neighbouring carriers of a window are correlated (a band of noise cut out of a long stream), so a band counts
    # for fewer than 12 independent draws: held to the interval of 6
    density = loop.S * 10.0 ** (PL.POINT_DB / 10.0) * 2048.0 / PL.WIDTH + sigma2
    cdf = NM.gamma_cdf(6, 6.0 * t)
    low, high = t[cdf < 1e-9].max(), t[1.0 - cdf < 1e-9].min()
    ratio_in = 1.0 / w[:, inside] / density
    assert (ratio_in > low).all() and (ratio_in < high).all(), (ratio_in.min(), ratio_in.max(), low, high)
    print(f"floor {sigma2:.3e}, under the interferer {density:.3e}: clear bands {ratio.min():.2f} .. {ratio.max():.2f} of the floor (mean {ratio.mean():.4f}), "
          f"bands under it {ratio_in.min():.2f} .. {ratio_in.max():.2f} of the density")


def test_two_branches_jammed_in_different_bands(loop):
    is_db = PL.POINT_DB
    alone = [loop.plain(is_db, n) for n in ("A", "B")]
    unit, banded = loop.plain_pair(is_db), loop.banded(is_db, ("A", "B"))
    print(f"I / S {is_db} dB: A {alone[0]}, B {alone[1]}, unit-weight pair {unit}, banded pair {banded}")
    for n in ("A", "B"):
        assert loop.branch(is_db, n)["valid"].all()
    for c in alone + [unit]:
        assert c[0] < 12 * CL.N_FRAMES and c[1] > 0
    assert banded == PL.DELIVERED
    assert loop.banded(is_db, ("A", "B"), 0.25) == PL.DELIVERED
