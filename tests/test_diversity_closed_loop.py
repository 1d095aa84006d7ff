"""CPU: what receive diversity buys in a fading channel.  The loop of tests/diversity_loop.py -- oracle transmitter -> one realisation of
the fading host model per branch (`tu6`, six Rayleigh taps at 10 Hz, timing 37, no carrier offset; branch = fading seed, each with a
noise seed of its own) -> the oracle's synchroniser, transform and fine-frequency loop per branch -> weighted soft bits of a single
branch (tests/softbit_model.py), or the branches' DQPSK products combined by the numpy model of csrc/diversity_core.h with its own
scale rule k = 1 / sum 1 / k_b (level 64, weights 1: the branches have equal noise) -> the oracle's FIC and MSC decoders.  Counted per
cell: FIB CRCs of 60 / wrong bytes of the five delivered logical frames of the EEP 3-A sub-channel.

    SNR dB  seed 1    seed 7    seed 3    seed 6    1+7     3+6    1+3     7+6    all four
       3    35/891    0/866     36/584    44/611    44/192  60/0   60/23   48/37  60/0
       4    36/823    10/781    36/316    48/363    48/41   60/0   60/0    48/6   60/0
       5    36/667    14/591    40/111    48/167    54/2    60/0   60/0    48/0   60/0
       6    36/454    19/279    49/21     48/54     59/0    60/0   60/0    51/0   60/0
       7    37/266    23/125    56/5      48/16     60/0    60/0   60/0    57/0   60/0
       8    46/110    34/21     59/2      48/9      60/0    60/0   60/0    60/0   60/0

The synchroniser refused no frame of the table.  Two branches that each lose most of their frames deliver every byte together, 4 to
6 dB below where a single weighted branch delivers (10 to 12 dB, tests/test_softbit_closed_loop.py): more than the 3 dB of array gain,
the rest is the diversity.  The two asserted points, 6 dB with the branches (3, 6) and with (1, 3), are points at which neither branch
delivers alone (fewer than 60 FIB CRCs or a wrong byte) and the pair delivers everything -- also 1 dB below and 1 dB above."""
import pytest

import diversity_loop as DL


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    return DL.Loop(oracle, tmp_path_factory.mktemp("diversity_loop_host_model"))


@pytest.mark.parametrize("snr_db,seeds", DL.POINTS)
def test_two_branches_deliver_where_neither_does_alone(loop, snr_db, seeds):
    assert len({DL.NOISE_SEED[s] for s in seeds}) == len(seeds)                  # no two branches share their noise
    singles = [loop.single(snr_db, s) for s in seeds]
    pair = {d: loop.combined(snr_db + d, seeds) for d in (-1.0, 0.0, 1.0)}
    print(f"{snr_db} dB, branches {seeds}: alone {singles}, together {pair[0.0]}; 1 dB below {pair[-1.0]}, 1 dB above {pair[1.0]} "
          f"(FIB CRCs of 60, wrong bytes); frames refused {loop.refused(snr_db, seeds)}")
    for s in singles:
        assert s != DL.DELIVERED
    assert pair[0.0] == DL.DELIVERED
    # the point is not an edge: the pair delivers a decibel either side of it
    assert pair[-1.0] == DL.DELIVERED and pair[1.0] == DL.DELIVERED


def test_four_branches_and_the_order_of_the_gain(loop):
    """all four branches at 5 dB deliver everything; and the pair is no accident of its scale: at 6 dB each of its branches alone loses
    frames that the other one carries"""
    assert loop.combined(5.0, (1, 7, 3, 6)) == DL.DELIVERED
    a, b = loop.single(6.0, 3), loop.single(6.0, 6)
    assert a[1] > 0 and b[1] > 0 and a[0] < 60 and b[0] < 60
