"""The closed loop transmitter -> channel -> resampler -> receiver, shared by its CPU form (tests/test_resample_closed_loop.py: oracle
transmitter -> host models of the channel and of the resampler -> oracle receive chain) and its device form
(tests/test_gpu_resample_loop.py).  The loop is tests/channel_loop.py's -- five frames, both sub-channels, two paths, carrier offset, noise
-- and the resampler comes behind the channel, so that the noise is resampled too, as at a receiver's ADC:
  (a) a sampling-clock error of CLOCK_PPM: the ADC's sample period is ppm 1e-6 longer than nominal, step = 1 + ppm 1e-6 input samples per
      output sample, so the frame start drifts EARLIER by ppm 1e-6 x 196608 samples per frame;
  (b) up to 2.4 MS/s and back down to 2.048 MS/s, the second pass at a fractional offset of UPDOWN_FRAC samples (of the 2.4 MS/s stream).
CLOCK_PPM is half the largest error of the ladder 5, 10, 20, 50, 100 ppm that delivers every byte at SNR_DB and 3 dB below (sweep(), run
on the CPU with the oracle chain; the ladder is recorded in DESIGN.md 4.19)."""
import numpy as np

import channel_loop as CL
import channel_model as CM
import resample_model as RM
import tx_encode_cases as T

LADDER_PPM = (5.0, 10.0, 20.0, 50.0, 100.0)
CLOCK_PPM = 50.0
UPDOWN_FRAC = 0.37
RATE_LOW, RATE_HIGH = 2.048e6, 2.4e6
ONE = RM.ONE


def clock_params(ppm):
    return RM.params_dict(RM.step_q62(RATE_LOW, RATE_LOW, ppm))


def updown_params():
    """(up, down): 2.048 -> 2.4 MS/s, then 2.4 -> 2.048 MS/s from UPDOWN_FRAC of a 2.4 MS/s sample on"""
    return RM.params_dict(RM.step_q62(RATE_LOW, RATE_HIGH)), RM.params_dict(RM.step_q62(RATE_HIGH, RATE_LOW), 0, int(round(UPDOWN_FRAC * ONE)))


N_UP = int(np.ceil(CL.N_OUT * RATE_HIGH / RATE_LOW)) + 64         # samples of the 2.4 MS/s stream that the way down reads


def predicted_offsets(plist):
    """fine time offset of every frame from T(m) alone.  Frame j's PRS starts at sample c_j = 2656 + 196608 j + TIMING of the channel's
    output; behind resamplers with times T_1, T_2, ... (in the order applied) it starts at the output sample m with T_1(T_2(.. m)) = c_j;
    the receiver expects it at 2656 + 196608 j"""
    out = []
    for j in range(CL.N_FRAMES):
        at = float(2656 + 196608 * j + CL.TIMING)
        for P in plist:
            step = P["step_q62"] / ONE
            at = (at - P["offset_samples"] - P["offset_frac_q62"] / ONE) / step
        out.append(at - (2656 + 196608 * j))
    return out


def receive(oracle, rx):
    """the oracle receive chain over the first 1 .. N_FRAMES slices: (the last call's result, the fine time offset after every frame)"""
    slices = CL.slices_of(rx)
    subs = [T.o_sub(oracle, d) for d in CL.SUBS]
    offsets, exp = [], None
    for k in range(1, CL.N_FRAMES + 1):
        exp = oracle.receive_frames(slices[:k], CL.STRIDE, CL.P, k, subs)
        offsets.append(int(exp["state"].fine_time_offset))
    return exp, offsets


def delivered(exp, offsets, predicted, fib, pay, nb):
    """what check_delivery of the channel loop asks, with the per-frame offsets pinned to the prediction +-1 sample; a list of what failed"""
    bad = []
    if exp["sync_failed"] != 0:
        bad.append("sync failed")
    if any(abs(o - p) > 1.0 for o, p in zip(offsets, predicted)):
        bad.append(f"fine time offsets {offsets} against {[round(p, 2) for p in predicted]}")
    if exp["fib_crc_ok"] != 12 * CL.N_FRAMES:
        bad.append(f"{exp['fib_crc_ok']} of {12 * CL.N_FRAMES} FIB CRCs")
    if not all(np.array_equal(exp["fib"][g, 32 * i:32 * i + 30], fib[0, CL.N_FRAMES - 1, g, i]) for g in range(4) for i in range(3)):
        bad.append("FIB bodies")
    cifs = pay.reshape(4 * CL.N_FRAMES, nb)
    if not all(np.array_equal(exp["msc"][c], cifs[4 * (CL.N_FRAMES - 1) + c - 15]) for c in range(4)):
        bad.append("sub-channel bytes")
    return bad


def channel_output(oracle, ch_host, snr_db, extra=0):
    """the loop's transmission through the channel's host model; `extra` samples more than the channel loop takes (the resampler reads ahead)"""
    fib, pay, nb = CL.inputs(oracle)
    iq = CL.oracle_iq(oracle, fib, pay)
    rx = CM.host_apply(ch_host, [CL.params(iq, snr_db)], iq, 0, CL.N_OUT + extra, False)[0]
    return fib, pay, nb, rx


def run_clock(oracle, ch_host, rs_host, ppm, snr_db):
    fib, pay, nb, rx = channel_output(oracle, ch_host, snr_db, extra=256)
    P = clock_params(ppm)
    D = RM.host_design(rs_host, RM.design_max_step(P["step_q62"]))
    out = RM.host_apply(rs_host, [P], D, rx, 0, CL.N_OUT, False)[0]
    exp, offsets = receive(oracle, out)
    return delivered(exp, offsets, predicted_offsets([P]), fib, pay, nb), offsets, exp


def run_updown(oracle, ch_host, rs_host, snr_db):
    fib, pay, nb, rx = channel_output(oracle, ch_host, snr_db, extra=256)
    up, down = updown_params()
    D_up, D_down = RM.host_design(rs_host, 1.0), RM.host_design(rs_host, RM.design_max_step(down["step_q62"]))
    high = RM.host_apply(rs_host, [up], D_up, rx, 0, N_UP, False)[0]
    out = RM.host_apply(rs_host, [down], D_down, high, 0, CL.N_OUT, False)[0]
    exp, offsets = receive(oracle, out)
    return delivered(exp, offsets, predicted_offsets([up, down]), fib, pay, nb), offsets, exp


def sweep(oracle, ch_host, rs_host):
    """the ladder: {(ppm, snr): what failed}"""
    return {(ppm, snr): run_clock(oracle, ch_host, rs_host, ppm, snr)[0] for ppm in LADDER_PPM for snr in (CL.SNR_DB, CL.SNR_DB - 3.0)}
