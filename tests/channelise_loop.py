"""The closed loop transmitter -> channel -> combiner -> channeliser -> receiver, shared by its CPU form
(tests/test_channelise_closed_loop.py: oracle transmitter -> host models of the channel and of the channeliser -> oracle receive chain)
and its device form (tests/test_gpu_channelise_loop.py).  The wanted ensemble is tests/channel_loop.py's -- five frames, both
sub-channels, two paths, carrier offset, 37 samples late, noise -- and sits in an 8.192 MS/s capture (D = 4) whose centre lies 300 kHz
under the block's: the combiner puts it at +300 kHz with a neighbour at -1.712 MHz and one at +1.712 MHz from it, each ADJACENT_DB above
the wanted block's signal power; the neighbours carry the same transmission, noise-free and rolled by 50001 and 120007 samples, so their
content differs from the wanted block's at every instant.  The channeliser splits the wanted block back out; combiner and channeliser
keep block sample m on wideband sample 4 m, so the receiver finds every frame 37 samples late as without them.
ADJACENT_DB is 10 dB under the top rung of the ladder 0, 10, 20, 30, 40 dB that delivers every byte at SNR_DB and 3 dB below (sweep(),
run on the CPU with the oracle chain; every rung delivers, so the top is 40 dB; the ladder is recorded in DESIGN.md 4.20).  With the alias-only edges of the resampler's kind
(0.375 / 0.625) that level does not survive: the neighbour's lowest 336 kHz pass the transition band."""
import numpy as np

import channel_loop as CL
import channel_model as CHM
import channelise_model as CM
import tx_encode_cases as T

D = 4
RATE = 2048000.0 * D
CAPTURE_OFFSET_HZ = 300000.0
SPACING_HZ = 1712000.0
ROLLS = (50001, 120007)
LADDER_DB = (0.0, 10.0, 20.0, 30.0, 40.0)
ADJACENT_DB = 30.0
ALIAS_ONLY_EDGES = (0.375, 0.625)
EXTRA = 256                                 # block samples beyond the channel loop's: the last outputs' later taps
N_WIDE = CL.N_OUT * D + CM.TPP * D


def channels(adjacent_db, sides=2):
    """the wanted block, then its neighbours (sides = 1: the upper one alone); the neighbours' gains against a unit-power transmission"""
    level = float(np.sqrt(1.0 + CL.TAP2 ** 2) * 10.0 ** (adjacent_db / 20.0))
    chs = [CM.channel(CM.freq_q64(CAPTURE_OFFSET_HZ, RATE), 0, 1.0)]
    if sides == 2:
        chs.append(CM.channel(CM.freq_q64(CAPTURE_OFFSET_HZ - SPACING_HZ, RATE), 0x3243F6A8885A308D, level))
    chs.append(CM.channel(CM.freq_q64(CAPTURE_OFFSET_HZ + SPACING_HZ, RATE), 0xB7E151628AED2A6A, level))
    return chs


def wanted_channel():
    return [CM.channel(CM.freq_q64(CAPTURE_OFFSET_HZ, RATE), 0, 1.0)]


def block_rows(oracle, ch_host, snr_db, sides=2):
    """(fib, pay, nb, rows): row 0 the wanted transmission through the channel's host model, the others the clean transmission rolled"""
    fib, pay, nb = CL.inputs(oracle)
    iq = CL.oracle_iq(oracle, fib, pay)
    n = CL.N_OUT + EXTRA
    rows = np.zeros((1 + sides, n), np.complex64)
    rows[0] = CHM.host_apply(ch_host, [CL.params(iq, snr_db)], iq, 0, n, False)[0]
    for k, roll in enumerate(ROLLS[2 - sides:]):
        rows[1 + k, :iq.size] = np.roll(iq, roll)
    return fib, pay, nb, rows


def delivered(exp, offsets, fib, pay, nb):
    """what check_delivery of the channel loop asks, with the fine time offset of EVERY frame pinned to 37; a list of what failed"""
    bad = []
    if exp["sync_failed"] != 0:
        bad.append("sync failed")
    if any(o != CL.TIMING for o in offsets):
        bad.append(f"fine time offsets {offsets}")
    if exp["fib_crc_ok"] != 12 * CL.N_FRAMES:
        bad.append(f"{exp['fib_crc_ok']} of {12 * CL.N_FRAMES} FIB CRCs")
    if not all(np.array_equal(exp["fib"][g, 32 * i:32 * i + 30], fib[0, CL.N_FRAMES - 1, g, i]) for g in range(4) for i in range(3)):
        bad.append("FIB bodies")
    cifs = pay.reshape(4 * CL.N_FRAMES, nb)
    if not all(np.array_equal(exp["msc"][c], cifs[4 * (CL.N_FRAMES - 1) + c - 15]) for c in range(4)):
        bad.append("sub-channel bytes")
    return bad


def receive(oracle, rx):
    """the oracle receive chain over the first 1 .. N_FRAMES slices: (the last call's result, the fine time offset after every frame)"""
    slices = CL.slices_of(rx)
    subs = [T.o_sub(oracle, d) for d in CL.SUBS]
    offsets, exp = [], None
    for k in range(1, CL.N_FRAMES + 1):
        exp = oracle.receive_frames(slices[:k], CL.STRIDE, CL.P, k, subs)
        offsets.append(int(exp["state"].fine_time_offset))
    return exp, offsets


def run(oracle, ch_host, cs_host, adjacent_db, snr_db, edges=(0.0, 0.0), sides=2):
    """(what failed, offsets, the receive result, the wideband capture, the split block)"""
    fib, pay, nb, rows = block_rows(oracle, ch_host, snr_db, sides)
    F = CM.host_design(cs_host, D, *edges)
    wide = CM.host_combine(cs_host, channels(adjacent_db, sides), 1, F, rows, 0, 0, N_WIDE, False)[0]
    back = CM.host_split(cs_host, wanted_channel(), F, wide, 0, 0, CL.N_OUT, False)[0]
    exp, offsets = receive(oracle, back)
    return delivered(exp, offsets, fib, pay, nb), offsets, exp, wide, back


def sweep(oracle, ch_host, cs_host, edges=(0.0, 0.0)):
    """the ladder: {(adjacent dB, snr): what failed}"""
    return {(a, snr): run(oracle, ch_host, cs_host, a, snr, edges)[0] for a in LADDER_DB for snr in (CL.SNR_DB, CL.SNR_DB - 3.0)}
