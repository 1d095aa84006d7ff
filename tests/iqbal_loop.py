"""The closed loop transmitter -> channel -> combiner -> front end -> IQ balance -> channeliser -> receiver, shared by its CPU form
(tests/test_iqbal_closed_loop.py: host models and the oracle receive chain) and its device form (tests/test_gpu_iqbal_loop.py).  The wanted
ensemble is tests/channel_loop.py's and sits at +856 kHz in an 8.192 MS/s capture (D = 4); ONE neighbour sits at -856 kHz, ADJACENT_DB
above the wanted block's signal power (the clean transmission rolled by 120007 samples, as tests/channelise_loop.py's): the mirror
frequency of the wanted block.  The chain is host combine -> host impairment (a FIXED stream of dabgpu_iqbal_impairment's coefficients)
-> [prime + correct: MEASURE over the capture's whole tiles, back to sample 0, APPLY; a TRACK stream with the library's defaults] -> host
split -> oracle receive chain.  GAIN_DB, PHASE_DEG: a front end that rejects the mirror frequency by 29.0 dB, so that the neighbour's image
is as strong as the wanted block at ADJACENT_DB = 30 (sweep(), run on the CPU; the ladder is recorded in DESIGN.md 4.32)."""
import numpy as np

import channel_loop as CL
import channel_model as CHM
import channelise_loop as XL
import channelise_model as CM
import iqbal_model as IM

D = XL.D
RATE = XL.RATE
CAPTURE_OFFSET_HZ = 856000.0
NEIGHBOUR_HZ = -856000.0
ROLL = 120007
LADDER_DB = (0.0, 10.0, 20.0, 30.0)
ADJACENT_DB = 30.0
GAIN_DB, PHASE_DEG, DC = 0.42, 3.0, 0.3 + 0.2j
UNCORRECTED_CAP = 15                        # of 60 FIBs: the contrast must not vanish unnoticed
N_WIDE = XL.N_WIDE


def channels(adjacent_db):
    """the wanted block, then its one neighbour at the mirror frequency; the neighbour's gain against a unit-power transmission"""
    level = float(np.sqrt(1.0 + CL.TAP2 ** 2) * 10.0 ** (adjacent_db / 20.0))
    return [CM.channel(CM.freq_q64(CAPTURE_OFFSET_HZ, RATE), 0, 1.0), CM.channel(CM.freq_q64(NEIGHBOUR_HZ, RATE), 0xB7E151628AED2A6A, level)]


def wanted_channel():
    return [CM.channel(CM.freq_q64(CAPTURE_OFFSET_HZ, RATE), 0, 1.0)]


def block_rows(oracle, ch_host, snr_db):
    """(fib, pay, nb, rows): row 0 the wanted transmission through the channel's host model, row 1 the clean transmission rolled"""
    fib, pay, nb = CL.inputs(oracle)
    iq = CL.oracle_iq(oracle, fib, pay)
    n = CL.N_OUT + XL.EXTRA
    rows = np.zeros((2, n), np.complex64)
    rows[0] = CHM.host_apply(ch_host, [CL.params(iq, snr_db)], iq, 0, n, False)[0]
    rows[1, :iq.size] = np.roll(iq, ROLL)
    return fib, pay, nb, rows


def impairment(gain_db=GAIN_DB, phase_deg=PHASE_DEG, dc=DC):
    K1, K2 = IM.front_end(gain_db, phase_deg)
    return IM.params(mode=IM.FIXED, a=K1, b=K2, c=dc)


def front_end(iq_host, wide, impaired):
    """the capture as the tuner delivers it (the host model's FIXED map), or as it is"""
    if not impaired:
        return wide
    return IM.host_apply(iq_host, [impairment()], IM.host_records(iq_host, 1), wide, 0, wide.size, IM.APPLY)[0][0]


def correct(iq_host, wide):
    """prime + correct on the host model: (the corrected capture, the record)"""
    rec = IM.host_records(iq_host, 1)
    P = [IM.params()]
    tiles = wide.size // IM.TILE * IM.TILE
    IM.host_apply(iq_host, P, rec, wide, 0, tiles, IM.MEASURE)
    return IM.host_apply(iq_host, P, rec, wide, 0, wide.size, IM.APPLY)[0][0], rec


def run(oracle, hosts, adjacent_db, snr_db, impaired=True, corrected=True):
    """hosts = (channel, channeliser, IQ balance) host models -> (what failed, the receive result, the record or None)"""
    ch_host, cs_host, iq_host = hosts
    fib, pay, nb, rows = block_rows(oracle, ch_host, snr_db)
    F = CM.host_design(cs_host, D)
    wide = CM.host_combine(cs_host, channels(adjacent_db), 1, F, rows, 0, 0, N_WIDE, False)[0]
    wide = front_end(iq_host, wide, impaired)
    rec = None
    if corrected:
        wide, rec = correct(iq_host, wide)
    back = CM.host_split(cs_host, wanted_channel(), F, wide, 0, 0, CL.N_OUT, False)[0]
    exp, offsets = XL.receive(oracle, back)
    return XL.delivered(exp, offsets, fib, pay, nb), exp, rec


def sweep(oracle, hosts):
    """the ladder: {(adjacent dB, snr, corrected): FIB CRCs of 60, what failed}"""
    return {(a, snr, c): (lambda r: (r[1]["fib_crc_ok"], r[0]))(run(oracle, hosts, a, snr, True, c))
            for a in LADDER_DB for snr in (CL.SNR_DB, CL.SNR_DB - 3.0) for c in (False, True)}
