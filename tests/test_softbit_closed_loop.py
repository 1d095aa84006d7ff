"""CPU: what the channel-state weighted soft bits buy in a fading channel.  The loop of tests/softbit_loop.py -- oracle transmitter ->
fading host model (`tu6`, six Rayleigh taps at 10 Hz, timing 37, no carrier offset) -> the frame cut at the known position -> the
oracle's transform -> soft bits of either policy from the numpy float32 model (level 64, the scale from the time-domain power of the
phase reference symbol) -> the oracle's FIC and MSC decoders.  Counted per point: FIB CRCs of 60 / wrong bytes of the five delivered
logical frames of the EEP 3-A sub-channel, normalised -> weighted, for the fading seeds 0..7:

    SNR dB  seed 0        1              2            3            4            5            6            7              totals
       6    34/64->58/2   36/675->36/478 36/205->36/35 37/225->53/41 53/218->60/7 47/127->60/0 48/183->48/77 9/677->20/326  300/2374 -> 371/966
       7    44/28->59/0   36/458->37/266 36/89->38/3  42/85->56/10 59/106->60/0 56/44->60/0  48/79->48/26 19/475->27/98   340/1364 -> 385/403
       8    51/6->60/0    36/278->47/107 36/32->51/0  49/32->58/3  60/37->60/0  58/15->60/0  48/24->48/7  21/295->39/26   359/719  -> 423/143
       9    57/0->60/0    39/141->54/31  40/15->56/0  55/15->60/3  60/18->60/0  58/5->60/0   48/4->48/4   30/125->43/12   387/323  -> 441/50
      10    60/0->60/0    45/26->59/8    45/9->60/0   57/0->60/3   60/3->60/0   60/1->60/0   48/2->49/0   39/63->54/0     414/104  -> 462/11
      11    60/0->60/0    54/8->60/0     57/0->60/0   59/0->60/0   60/1->60/0   60/0->60/0   48/0->51/0   42/19->58/0     440/28   -> 469/0
      12    60/0->60/0    60/0->60/0     59/0->60/0   60/0->60/0   60/1->60/0   60/0->60/0   48/0->59/0   54/5->59/0      461/6    -> 478/0

About 2 dB at equal delivery.  The two asserted points, (10 dB, seed 2) and (8 dB, seed 0), are points at which the reference's soft
bits do not deliver (fewer than 60 FIB CRCs or a wrong byte) and the weighted ones deliver everything."""
import pytest

import channel_fading_model as FM
import channel_loop as CL
import softbit_loop as SL
import softbit_model as SM


@pytest.fixture(scope="module")
def loop(oracle, tmp_path_factory):
    host = FM.build_host_model(tmp_path_factory.mktemp("softbit_loop_host_model"))
    fib, pay, nb = CL.inputs(oracle)
    return host, CL.oracle_iq(oracle, fib, pay), fib, pay, nb


def delivers(result):
    return result == (12 * CL.N_FRAMES, 0)


@pytest.mark.parametrize("snr_db,seed", SL.POINTS)
def test_weighted_soft_bits_deliver_where_the_reference_policy_does_not(oracle, loop, snr_db, seed):
    host, iq, fib, pay, nb = loop
    r = SL.cpu_point(oracle, host, iq, fib, pay, nb, snr_db, seed)
    print(f"{snr_db} dB, fading seed {seed}: normalised {r[SM.SOFT_NORMALISED]}, weighted {r[SM.SOFT_CSI]} (FIB CRCs of 60, wrong bytes)")
    assert not delivers(r[SM.SOFT_NORMALISED])
    assert delivers(r[SM.SOFT_CSI])


def test_more_fib_crcs_over_the_seeds_at_10_db(oracle, loop):
    host, iq, fib, pay, nb = loop
    total = {SM.SOFT_NORMALISED: [0, 0], SM.SOFT_CSI: [0, 0]}
    for seed in range(8):
        r = SL.cpu_point(oracle, host, iq, fib, pay, nb, 10.0, seed)
        for p in total:
            total[p][0] += r[p][0]; total[p][1] += r[p][1]
    print(f"10 dB, seeds 0..7: normalised {total[SM.SOFT_NORMALISED]}, weighted {total[SM.SOFT_CSI]} (FIB CRCs of 480, wrong bytes)")
    assert total[SM.SOFT_CSI][0] > total[SM.SOFT_NORMALISED][0]
    assert total[SM.SOFT_CSI][1] < total[SM.SOFT_NORMALISED][1]
