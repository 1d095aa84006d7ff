"""The oracle's synchroniser against the float64 model of ofdm_demodulator.cpp:360-548 (tests/sync_cases.py) over the edge table of all
four transmission modes, and the table's own coverage: what the device is compared with bit for bit (tests/test_gpu_sync_edges.py) is
pinned here by something other than the restatement itself."""
import numpy as np
import pytest

import sync_cases as SC

MODEL_GROUPS = ("position", "coarse-edge", "tracking", "cfg")


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_table_yields_every_kind_of_answer(oracle, mode):
    """the table is informative, not only large: on the oracle's own answers, per mode, at least one case of each kind of sync_cases.KINDS,
    every group present, and the two records the header promises (coarse disabled -> freq_coarse 0.0, invalid -> fine_time_offset retained)"""
    cases, exp = SC.table(mode), SC.expected(mode)
    g = oracle.geometry(mode)
    assert {c.group for c in cases} == set(SC.GROUPS)
    assert all(s.shape == (g.nb_fft,) and s.dtype == np.complex64 for c in cases for s in c.symbols)
    kinds = SC.kinds_of(mode, cases, exp)
    assert all(kinds[k] for k in SC.KINDS), {k: len(v) for k, v in kinds.items()}
    by_name = {c.name: steps for c, steps in zip(cases, exp)}
    off = by_name["cfg/coarse-disabled/incoming-coarse-nonzero"][0]
    assert off.coarse_in != 0.0 and off.coarse == 0.0 and np.signbit(off.coarse) == np.False_ and off.freq_resp is None
    kept = by_name["cfg/invalid-keeps-incoming-offset-12345"][0]
    assert not kept.valid and kept.offset == 12345
    # the tracking sequence steps as the issue lists them: fast, slow, slow, slow (error 1.2 bins < 1.5), slow, fast (large error while found), slow
    seq = by_name["tracking/sequence/beta0"]
    assert [bool(s.coarse != s.coarse_in) for s in seq] == [True, False, False, False, False, True, False]
    # |error| == 1.5 / N exactly is NOT large: a slow step of beta 0.1
    s = by_name["tracking/error-exactly-1.5-bins"][0]
    t = np.float32(1.5) / np.float32(g.nb_fft)
    assert s.found_in == 1 and s.coarse == np.float32(s.coarse_in + np.float32(0.1) * -t) and s.coarse != by_name["tracking/sequence/beta0"][0].coarse
    # a weighted winner far from the frame's true position 0: the dB weighting below 0 dB prefers far positions
    far = [c.name for c, steps in zip(cases, exp) if c.group == "scale" and steps[0].valid and steps[0].offset > g.nb_cp
           and np.isfinite(steps[0].coarse)]
    assert far, "no scale case shows the dB-weighting quirk"
    # fmodf wrapped the fine offset on the first update of the cases built for it
    wrap = 0.5 * (1.0 / g.nb_fft) * 1.01
    for name in ("tracking/fine-near-plus-wrap", "tracking/fine-near-minus-wrap", "tracking/fine-near-plus-wrap/slow-step"):
        s = by_name[name][0]
        delta = float(s.coarse) - float(s.coarse_in)
        assert abs(float(s.fine_in)) > 0.99 * wrap and abs(float(s.fine_in) - delta) > wrap > abs(float(s.fine)), name


def all_finite(steps):
    return all(np.isfinite(s.impulse).all() and (s.freq_resp is None or np.isfinite(s.freq_resp).all())
               and np.isfinite(s.coarse) and np.isfinite(s.fine) for s in steps)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_oracle_decisions_equal_the_float64_model_over_the_edge_table(oracle, mode):
    """Every step of the position, coarse-edge, tracking and cfg groups, and of the scale cases whose float32 responses are all finite, with
    the quantities and the rules of test_sync_decisions_equal_a_float64_model: the coarse peak index and delta against beta (pred - coarse)
    within 3e-6, validity and offset; a decision is excused as a near tie when the float64 margin between the two best candidates is below
    0.02 dB, the error within 2e-6 of the 1.5 / N threshold, or the peak within 0.05 dB of the peak threshold.  At most one fifth of a mode's
    decisions may be excused and no group as a whole.

    Decisions compared / excused (coarse and fine counted separately), as run:
        mode I    211 decisions: 209 compared, 2 excused (1 position, 1 tracking)
        mode II   209 decisions: 207 compared, 2 excused (1 coarse-edge, 1 tracking)
        mode III  209 decisions: 208 compared, 1 excused (tracking)
        mode IV   211 decisions: 210 compared, 1 excused (tracking)
    (the tracking excuse of every mode is tracking/error-exactly-1.5-bins, built to sit ON the 1.5 / N threshold)

    Underflow (-inf or subnormal values in a response), overflow and non-finite input are outside what a float64 model can say: there the
    reference source (src/ofdm/ofdm_demodulator.cpp:360-548), as the oracle restates it line by line, is the authority, and
    test_table_yields_every_kind_of_answer pins which branch each of those cases takes."""
    g = oracle.geometry(mode)
    N, cp, period = g.nb_fft, g.nb_cp, g.nb_symbol_period
    prs_fft = oracle.prs_fft_mode(mode)
    compared = {grp: 0 for grp in SC.GROUPS}
    excused = {grp: 0 for grp in SC.GROUPS}
    n_scale = 0
    for c, steps in zip(SC.table(mode), SC.expected(mode)):
        if not (c.group in MODEL_GROUPS or (c.group == "scale" and all_finite(steps))):
            continue
        n_scale += c.group == "scale"
        cfg = SC.make_cfg(oracle, c.cfg)
        for it, (sym, s) in enumerate(zip(c.symbols, steps)):
            where = (mode, c.name, it)
            if cfg.is_coarse_freq_correction:
                coarse_in = float(s.coarse_in)
                max_index, fast, pred, margin, thr_margin = SC.f64_coarse(sym, prs_fft, coarse_in, bool(s.found_in), cfg, N)
                if margin < 0.02 or thr_margin < 2e-6:               # float32 vs float64 may legitimately order a near-tie differently
                    excused[c.group] += 1
                else:
                    M = N // 2
                    mo = SC.max_off_of(cfg.max_coarse_freq_correction_norm, N)
                    lo, hi = M - mo, min(M + mo, N - 1)
                    o_peak = int(np.argmax(s.freq_resp[lo:hi + 1])) + lo - M
                    assert o_peak == max_index, where
                    delta = float(s.coarse) - coarse_in
                    beta = 1.0 if fast else float(cfg.coarse_freq_slow_beta)
                    assert abs(delta - beta * (pred - coarse_in)) < 3e-6, where + (fast,)
                    compared[c.group] += 1
            else:
                assert s.coarse == 0.0, where
            f = float(np.float32(s.coarse) + np.float32(s.fine))
            ok64, off64, m2, thr2 = SC.f64_fine(sym, prs_fft, f, cfg, N, cp, period)
            if thr2 < 0.05 or (ok64 and m2 < 0.02):
                excused[c.group] += 1
                continue
            assert bool(s.valid) == bool(ok64), where
            if ok64:
                assert s.offset == off64, where
            compared[c.group] += 1
    print(f"mode {mode}: compared {sum(compared.values())} excused {sum(excused.values())} per group "
          f"{ {grp: (compared[grp], excused[grp]) for grp in SC.GROUPS if compared[grp] + excused[grp]} } scale cases {n_scale}")
    total = sum(compared.values()) + sum(excused.values())
    assert 5 * sum(excused.values()) <= total, (compared, excused)
    for grp in MODEL_GROUPS + ("scale",):
        assert compared[grp] > 0, (grp, compared, excused)
    assert n_scale >= 3
