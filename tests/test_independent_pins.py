"""Independent pins for the rows whose reference translation units cannot be compiled here (dab_viterbi_decoder.cpp needs the absent
vendor/viterbi_decoder, ofdm_demodulator.cpp needs <fftw3.h>).  Nothing below shares code with the oracle or the kernels:

* Viterbi: EXHAUSTIVE maximum-likelihood search over every message of short codewords (every puncturing family
  PI_1..PI_24 + the PI_X tail, every start state) must give the oracle's bytes and its path_error -- this pins the branch metric
  (sum of abs(+-127 - y), punctured symbols as 0), the start metrics (0 / 5080), the trellis orientation and the chain-back bit order.
  A textbook int64 dynamic programme (no u16 wrap, no renormalisation) then pins the renormalisation bookkeeping and the u16 arithmetic
  on FIC- and MSC-length codewords: same bytes, same total error, under either tie rule (strict compare = upstream scalar core,
  min + equality = upstream SIMD cores).  The exhaustive search excludes inputs whose ML path is not unique.
* PRS synchroniser (a5, a6): a float64 numpy model written from ofdm_demodulator.cpp:399-467 and :503-536 must make the same integer
  decisions (peak bin, fast / slow update, fine-time offset, reset) as the oracle over a CFO x timing x SNR grid.
* FFT rounding (a11-a13): a float64 demodulator (numpy FFT) must give the oracle's hard bits on the 20 dB-SNR config-1 frame.
* Transmitter (ofdm_modulator.cpp needs <fftw3.h> too): a float64 modulator written from ETSI EN 300 401 clause 14 (its own frequency
  interleaver, carrier-to-bin rule and unit phasors, numpy's complex128 inverse transform) holds the expectations of the -m gpu transmitter
  tests (oracle.modulate_frame_reference_payload, oracle.modulate_frame, tests/tx_model.py) in modes I-IV and both payload layouts: exact
  structure (NULL, cyclic prefix, every payload bit back through a complex128 demodulator), a derived float32 error bound per symbol,
  the u8 quantisation within one count at samples near an integer boundary only, and oracle.apply_pll against a float64 rotation.
"""
import numpy as np
import pytest

G = (109, 79, 83, 109)          # dab_viterbi_decoder.cpp:25 (decimal form of octal 133,171,145,133)


def parity(v):
    v = np.asarray(v, dtype=np.int64)
    v = v ^ (v >> 4); v = v ^ (v >> 2); v = v ^ (v >> 1)
    return (v & 1).astype(np.int64)


def encode(bits, start_state=0):
    """mother code of a bit sequence (tail included by the caller): register sr = (sr << 1) | bit, outputs parity(sr & G[r])"""
    sr = start_state
    out = []
    for b in bits:
        sr = ((sr << 1) | int(b)) & 0x7F
        out += [int(parity(sr & g)) for g in G]
    return np.array(out, dtype=np.int64)


def kept_mask(segments, n_tail_groups=6):
    """segments = [(kept-count vector of 8 entries, number of 4-symbol groups)]; returns 0/1 per mother symbol"""
    m = []
    for code, groups in segments:
        for g in range(groups):
            k = int(code[g % len(code)])
            m += [1] * k + [0] * (4 - k)
    return np.array(m, dtype=np.int64)


def depuncture(punctured, mask):
    y = np.zeros(mask.size, dtype=np.int64)
    y[mask == 1] = punctured
    return y


def all_messages_cost(y, n_info, start=0):
    """cost[start, message] = 5080*[start != 0] + sum over the n_info + 6 steps of sum_r abs(+-127 - y) along the path of `message`
    from `start` (6 zero tail bits); vectorised over all 64 start states x 2^n_info messages"""
    n_msg = 1 << n_info
    msgs = np.arange(n_msg, dtype=np.int32)[None, :]
    sr = np.repeat(np.arange(64, dtype=np.int32)[:, None], n_msg, axis=1)
    c = np.where(sr == start, 0, 5080).astype(np.int32)           # dab_viterbi_decoder.cpp:36-37, reset(starting_state) :109-112
    par = parity(np.arange(128)[:, None] & np.array(G)[None, :]).astype(np.int32)      # [register, r]
    for t in range(n_info + 6):
        bit = ((msgs >> (n_info - 1 - t)) & 1) if t < n_info else 0
        sr = ((sr << 1) | bit) & 0x7F
        step = np.abs(np.where(par == 1, 127, -127) - y[4 * t:4 * t + 4][None, :]).sum(axis=1).astype(np.int32)   # cost per register value
        c += step[sr]
    return c


@pytest.mark.parametrize("n_info", [8, 16])
def test_viterbi_equals_exhaustive_maximum_likelihood(oracle, n_info):
    rng = np.random.default_rng(100 + n_info)
    pis = range(1, 25) if n_info == 8 else (1, 5, 8, 12, 15, 16, 20, 24)
    checked = 0
    for pi in pis:
        code = oracle.puncture_code(pi)
        tail = oracle.puncture_code_tail()
        mask = kept_mask([(code, n_info), (tail, 6)])
        for trial in range(4 if n_info == 8 else 2):
            msg = rng.integers(0, 2, n_info)
            start = 0 if trial % 2 == 0 else int(rng.integers(1, 64))     # reset(starting_state) with a non-zero state as well
            tx = encode(np.concatenate([msg, np.zeros(6, dtype=np.int64)]), start_state=start)
            sigma = (25.0, 45.0, 70.0, 110.0)[(trial + pi) % 4]            # from clean to mostly wrong
            soft = np.clip(np.rint((2 * tx - 1) * 55.0 + rng.normal(0, sigma, tx.size)), -127, 127).astype(np.int64)
            punct = soft[mask == 1].astype(np.int8)
            y = depuncture(punct, mask)
            costs = all_messages_cost(y, n_info, start)
            best = int(costs.min())
            if int((costs == best).sum()) != 1:
                continue                                                   # ML tie: the winner depends on the tie rule
            si, mi = np.unravel_index(np.argmin(costs), costs.shape)
            n_main = int(mask[:4 * n_info].sum())
            for tie_rule in (0, 1):
                v = oracle.Viterbi(n_info + 6, tie_rule)
                v.reset(start)
                used = v.update(punct[:n_main], code, 4 * n_info)
                used += v.update(punct[n_main:], tail, 24)
                assert used == punct.size
                got, err = v.chainback(n_info // 8, 0)
                exp_bytes = np.packbits(np.array([(int(mi) >> (n_info - 1 - t)) & 1 for t in range(n_info)], dtype=np.uint8))   # MSB first
                # the decoder reports the cost of the best path into state 0 from ANY start state (others penalised by 5080)
                assert err == best, (pi, trial, tie_rule)
                assert np.array_equal(got, exp_bytes), (pi, trial, tie_rule)
                checked += 1
    assert checked >= (100 if n_info == 8 else 20)


def dp_decode(y, n_steps, n_out_bits, tie_rule=0):
    """textbook Viterbi over int64 metrics (no wrap, no renormalisation): returns (bits, total error of the survivor ending in state 0, tie seen)"""
    INF = np.int64(1) << 50
    states = np.arange(64, dtype=np.int64)
    metric = np.full(64, 5080, dtype=np.int64)
    metric[0] = 0
    # transition (old state s, input b) -> new state ((s << 1) | b) & 63 with register sr = ((s << 1) | b) & 127
    prev0 = (states >> 1)                      # predecessors of new state n: n >> 1 and (n >> 1) | 32, input bit = n & 1
    prev1 = (states >> 1) | 32
    sr0 = ((prev0 << 1) | (states & 1)) & 0x7F
    sr1 = ((prev1 << 1) | (states & 1)) & 0x7F
    exp0 = np.stack([np.where(parity(sr0 & g) == 1, 127, -127) for g in G])      # [4, 64]
    exp1 = np.stack([np.where(parity(sr1 & g) == 1, 127, -127) for g in G])
    choice = np.zeros((n_steps, 64), dtype=np.int8)
    tie = False
    for t in range(n_steps):
        sym = y[4 * t:4 * t + 4][:, None]
        c0 = metric[prev0] + np.abs(exp0 - sym).sum(axis=0)
        c1 = metric[prev1] + np.abs(exp1 - sym).sum(axis=0)
        tie |= bool(np.any(c0 == c1))
        choice[t] = (c1 <= c0) if tie_rule else (c1 < c0)        # the two upstream cores: strict compare / min + equality
        metric = np.minimum(c0, c1)
    s = 0
    bits = np.zeros(n_steps, dtype=np.uint8)
    for t in range(n_steps - 1, -1, -1):
        bits[t] = s & 1
        s = ((s >> 1) | 32) if choice[t, s] else (s >> 1)
    return bits[:n_out_bits], int(metric[0]), tie


@pytest.mark.parametrize("shape", ["fic", "msc_eep3a", "long_weak"])
def test_viterbi_equals_int64_dynamic_programme_on_long_codewords(oracle, shape):
    """FIC (774 steps) and 48 CU EEP 3-A (1542 steps) with heavy noise: the u16 metrics renormalise several times; bytes and the
    reported total error must equal the wrap-free int64 decoder"""
    rng = np.random.default_rng({"fic": 1, "msc_eep3a": 2, "long_weak": 3}[shape])
    segs = {"fic": [(16, 21 * 32), (15, 3 * 32)], "msc_eep3a": [(8, 45 * 32), (7, 3 * 32)], "long_weak": [(24, 40 * 32), (1, 24 * 32)]}[shape]
    n_info = sum(g for _, g in segs)
    tail = oracle.puncture_code_tail()
    mask = kept_mask([(oracle.puncture_code(pi), g) for pi, g in segs] + [(tail, 6)])
    done = 0
    for trial in range(6):
        msg = rng.integers(0, 2, n_info)
        tx = encode(np.concatenate([msg, np.zeros(6, dtype=np.int64)]))
        gain, sigma = ((60.0, 50.0), (100.0, 60.0), (30.0, 70.0))[trial % 3]
        soft = np.clip(np.rint((2 * tx - 1) * gain + rng.normal(0, sigma, tx.size)), -127, 127).astype(np.int64)
        punct = soft[mask == 1].astype(np.int8)
        y = depuncture(punct, mask)
        for tie_rule in (0, 1):
            bits, total, tie = dp_decode(y, n_info + 6, n_info, tie_rule)
            v = oracle.Viterbi(n_info + 6, tie_rule)
            v.reset(0)
            pos = 0
            for pi, g in segs:
                pos += v.update(punct[pos:], oracle.puncture_code(pi), 4 * g)
            pos += v.update(punct[pos:], tail, 24)
            assert pos == punct.size
            got, err = v.chainback(n_info // 8, 0)
            assert err == total, (shape, trial, tie_rule)              # the ML cost does not depend on how ties are broken
            assert np.array_equal(got, np.packbits(bits)), (shape, trial, tie_rule)
            done += 1
    assert done == 12


def dp_decode_core(y, n_steps, n_out_bits, core):
    """the two upstream cores as MODELS of their published add-compare-select, over Python integers: core 0 = ViterbiDecoder_Scalar (uint16_t sums
    that wrap, `m0 > m1`), core 1 = the SIMD cores (adds_epu16: the sums saturate at 65535; min_epu16; decision = cmpeq(survivor, upper candidate));
    both with the reference's renormalisation (dab_viterbi_decoder.cpp:31-41).  Returns (bits, path error, largest candidate sum seen before reduction)"""
    metric = [5080] * 64
    metric[0] = 0
    total, biggest = 0, 0
    choice = np.zeros((n_steps, 64), dtype=np.int8)
    par = [[int(parity(sr & g)) for g in G] for sr in range(128)]
    for t in range(n_steps):
        new = [0] * 64
        for n in range(64):
            cand = []
            for p in (n >> 1, (n >> 1) | 32):
                sr = ((p << 1) | (n & 1)) & 0x7F
                e = sum(abs((127 if par[sr][r] else -127) - int(y[4 * t + r])) for r in range(4))
                v = metric[p] + e
                biggest = max(biggest, v)
                cand.append(min(v, 65535) if core else (v & 0xFFFF))
            up = (cand[1] <= cand[0]) if core else (cand[1] < cand[0])
            choice[t, n] = up
            new[n] = cand[1] if up else cand[0]
        if new[0] >= 60455:
            mn = min(new)
            new = [v - mn for v in new]
            total += mn
        metric = new
    s = 0
    bits = np.zeros(n_steps, dtype=np.uint8)
    for t in range(n_steps - 1, -1, -1):
        bits[t] = s & 1
        s = ((s >> 1) | 32) if choice[t, s] else (s >> 1)
    return bits[:n_out_bits], total + metric[0], biggest


def test_u16_candidate_sums_cannot_reach_65535():
    """Where the two upstream cores could differ besides ties: the scalar core's uint16_t sums wrap, the SIMD cores' adds_epu16 saturates.  For THIS code
    (K = 7, polynomials 133 171 145 133) and symbols in [-127, 127] (include/dabgpu.h: -128 is read as -127) no input makes a sum reach 65535, so the two models differ in the tie rule only:
      * after the first six steps every state has a path from every state of six steps ago, hence  metric(s) - min metric <= 254 * d(s ^ s*), d = the
        weight of the lightest path from the all-zero state to that state difference (the code is linear) -- the fixed point computed below: 15 bits;
      * a candidate adds one branch (<= 4 x 254; the complementary cost 1016 - e of the butterfly stays in [0, 1016] too), and the reference renormalises as soon as metric[0] >= 60455 (dab_viterbi_decoder.cpp:31-41), so before
        any step min metric <= metric[0] <= 60454:  candidate <= 60454 + 254 * (15 + 4) = 65280 < 65535;
      * in the first six steps after reset() the level is at most 5080 + 6 * 1016.
    The bound is computed from the polynomials here (nothing shared with the oracle or the kernels) and then attacked: the hardest inputs a hill climb
    finds (erasures up to just below the renormalisation threshold, then 15-17 steps of extreme symbols) stay below it, and both core models -- and the
    oracle under both -- decode them identically."""
    d = [10 ** 9] * 64
    d[0] = 0
    for _ in range(64):
        nd = [min(d[p] + int(sum(parity((((p << 1) | (n & 1)) & 0x7F) & g) for g in G)) for p in (n >> 1, (n >> 1) | 32)) for n in range(64)]
        nd[0] = 0
        if nd == d:
            break
        d = nd
    spread_bits = max(d)
    assert spread_bits == 15
    bound = 60454 + 254 * (spread_bits + 4)
    assert bound == 65280 and bound < 65535
    import oracle as O
    O.build()
    rng = np.random.default_rng(5)
    worst = 0
    for n_a in (117, 118, 119):                                   # 508 per erased step: 59436, 59944, 60452 -- the last is 3 below the threshold
        n_steps = 134                                              # 128 message bits + the 6 tail steps the chain-back skips
        n_b = n_steps - n_a
        y = np.concatenate([np.zeros(4 * n_a, np.int64), rng.choice([-127, 127], size=4 * n_b)])
        _, _, best = dp_decode_core(y, n_steps, 8, 0)
        for _ in range(60):                                        # hill climb on the extreme symbols
            y2 = y.copy()
            y2[4 * n_a + rng.integers(0, 4 * n_b)] = rng.choice([-127, 127, 0])
            b2 = dp_decode_core(y2, n_steps, 8, 0)[2]
            if b2 >= best:
                y, best = y2, b2
        worst = max(worst, best)
        n_bits = n_steps - 6
        r0, r1 = dp_decode_core(y, n_steps, n_bits, 0), dp_decode_core(y, n_steps, n_bits, 1)
        assert r0[2] == r1[2] <= bound
        for core, r in ((0, r0), (1, r1)):
            v = O.Viterbi(n_steps, core)
            v.reset(0)
            assert v.update(y.astype(np.int8), np.array([4], np.uint8), 4 * n_steps) == 4 * n_steps
            got, err = v.chainback(n_bits // 8, 0)
            assert err == r[1] and np.array_equal(got, np.packbits(r[0])), (n_a, core)
    assert 60454 < worst <= bound, worst                          # the attack does get past the threshold level, and not past the bound


# ---------------------------------------------------------------------------------------------------------------------
# PRS synchroniser: float64 model of ofdm_demodulator.cpp:360-548
# ---------------------------------------------------------------------------------------------------------------------
from sync_cases import f64_coarse, f64_fine      # the model for any geometry (tests/sync_cases.py); the defaults are mode I's


def test_sync_decisions_equal_a_float64_model(oracle):
    rng = np.random.default_rng(77)
    prs_fft = oracle.prs_fft()
    conj_ref, time_ref = oracle.sync_refs()
    cfg = oracle.sync_cfg_default()
    bits = rng.integers(0, 2, oracle.NB_FRAME_BITS, dtype=np.uint8)
    tx0 = np.concatenate([oracle.modulate_frame(bits)] * 2)
    agreed = resets = 0
    for cfo_bins in (0.0, 0.3, 0.5, 1.0, 2.6, -3.7, 11.25, -40.49, 200.2, -333.0):
        tx_c = oracle.apply_pll(tx0, cfo_bins / 2048.0, 0.1)
        for toff in (0, 1, 37, -80, 200, -250):
            for noise in (0.0, 4.0, 20.0, 60.0):                         # PRS samples have |x| ~ 39: SNR from clean to -4 dB
                tx = tx_c
                if noise > 0:
                    tx = (tx_c + noise * (rng.standard_normal(tx_c.size) + 1j * rng.standard_normal(tx_c.size))).astype(np.complex64)
                start = oracle.NB_NULL_PERIOD - toff
                sym = tx[start:start + 2048].copy()
                st = oracle.SyncState(0.0, 0.0, 0, 0, 0, 0)
                coarse64, found64 = 0.0, False
                for it in range(2):                                      # first estimate (fast), then the tracking call
                    before = float(st.freq_coarse)
                    fr = oracle.coarse_freq_sync(sym, st, cfg, time_ref)
                    max_index, fast, pred, margin, thr_margin = f64_coarse(sym, prs_fft, coarse64, found64, cfg)
                    if margin < 0.02 or thr_margin < 2e-6:               # float32 vs float64 may legitimately order a near-tie differently
                        break
                    o_peak = int(np.argmax(fr[1024 - 1024:1024 + 1024 + 0])) - 1024     # oracle's dB response, fft-shifted
                    assert o_peak == max_index, (cfo_bins, toff, noise, it)
                    delta = float(st.freq_coarse) - before
                    beta = 1.0 if fast else cfg.coarse_freq_slow_beta
                    assert abs(delta - beta * (pred - coarse64)) < 3e-6, (cfo_bins, toff, noise, it, fast)
                    coarse64 += beta * (pred - coarse64)
                    found64 = True
                    f = float(np.float32(st.freq_coarse) + np.float32(st.freq_fine))
                    ok_o, off_o, ir = oracle.fine_time_sync(sym, f, cfg, conj_ref)
                    ok64, off64, m2, thr2 = f64_fine(sym, prs_fft, f, cfg)
                    if thr2 < 0.05 or (ok64 and m2 < 0.02):
                        break
                    assert ok_o == ok64, (cfo_bins, toff, noise, it)
                    if ok64:
                        assert off_o == off64, (cfo_bins, toff, noise, it)
                        agreed += 1
                    else:
                        resets += 1
    assert agreed > 250 and resets > 10


def test_float64_demodulator_gives_the_same_hard_bits_on_the_config1_frame(oracle):
    """CFO +3.7 bins, AWGN 20 dB SNR, seed 1, u8 quantised; the oracle's own FFT (float32, 4x8x8x8) against numpy's float64"""
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 2, oracle.NB_FRAME_BITS, dtype=np.uint8)
    cfo = 3.7 / 2048.0
    tx = oracle.apply_pll(oracle.modulate_frame(bits), cfo, 0.0)
    sig = np.sqrt(np.mean(np.abs(tx[oracle.NB_NULL_PERIOD:]) ** 2))
    tx = tx + (sig / 10.0 / np.sqrt(2.0)) * (rng.standard_normal(tx.size) + 1j * rng.standard_normal(tx.size))
    scale = 127.5 / (4.0 * sig)                                          # u8 capture with ~4 sigma head-room (app_iq_readers.h:23-30 inverse)
    q = np.clip(np.rint(np.stack([tx.real, tx.imag], -1) * scale + 127.5), 0, 255).astype(np.uint8)
    iq = ((q.astype(np.float32) - 127.5) / 127.5)
    x = (iq[:, 0] + 1j * iq[:, 1]).astype(np.complex64)
    frame = oracle.tx_to_frame_buffer(x)
    got = oracle.demod_frame(frame, -cfo)["bits"]
    # float64 model of steps 5-8 of SURVEY A.2
    n = np.arange(196608)
    y = frame.astype(np.complex128) * np.exp(2j * np.pi * (-cfo) * n)
    syms = y[:76 * 2552].reshape(76, 2552)[:, 504:]
    X = np.fft.fft(syms, axis=1)
    m = oracle.mapper().astype(np.int64)
    carriers = np.concatenate([np.arange(2048 - 768, 2048), np.arange(1, 769)])
    d = X[:-1, carriers] * np.conj(X[1:, carriers])                      # X_i conj(X_{i+1}), natural carrier order
    v = d[:, m]
    A = np.maximum(np.abs(v.real), np.abs(v.imag))
    soft = np.concatenate([-(v.real / A) * 127.0, (v.imag / A) * 127.0], axis=1).reshape(-1)
    hard64 = soft >= 0
    hard = got.astype(np.int32) >= 0
    # identical wherever the float64 value is not within rounding distance of the decision threshold
    safe = np.abs(soft) > 1.5
    assert np.array_equal(hard[safe], hard64[safe])
    assert safe.mean() > 0.98
    assert (hard != bits.astype(bool)).mean() < 5e-3                     # and both are the transmitted bits but for channel errors


# ---------------------------------------------------------------------------------------------------------------------
# Transmitter: float64 model from ETSI EN 300 401 clause 14 (read beside ofdm_modulator.cpp:49-156 and simulate_transmitter.cpp:138-178)
# ---------------------------------------------------------------------------------------------------------------------
import tx_model as TX

from pin_common import U32, fft_rounding_bound, pll_sample_bound, tx64_carriers, tx64_interleaver, tx64_slot   # shared with tests/demod_model.py


# quarter q <-> phase (2q + 1) pi / 4.  Reference layout: 2 bits v per carrier, ascending frequency, low bits first in a byte;
# PHASE_MAP[v] = (-A,-A), (A,-A), (A,A), (-A,A) (ofdm_modulator.cpp:102) = quarters 2, 3, 0, 1
TX64_Q_OF_V = np.array([2, 3, 0, 1])
TX64_V_OF_Q = np.array([2, 3, 0, 1])
# Frame-bits layout: z = ((1 - 2 b_n) + j (1 - 2 b_{n+NC})) / sqrt(2) (clause 14.5): (b_re, b_im) -> quarter
TX64_Q_OF_BITS = np.array([[0, 3], [1, 2]])


def tx64_quarters(payload, layout, N, NC, L):
    """[L-1][NC] quarter per data symbol and carrier slot (ascending frequency)"""
    pay = np.ascontiguousarray(payload, np.uint8).reshape(L - 1, NC // 4)
    if layout == TX.LAYOUT_REFERENCE:
        c = np.arange(NC)
        v = (pay[:, c // 4] >> (2 * (c % 4))) & 3
        return TX64_Q_OF_V[v]
    b = np.unpackbits(pay, axis=1, bitorder="little")                  # bit n of a symbol = bit (n & 7) of byte n >> 3
    q = np.empty((L - 1, NC), np.int64)
    q[:, tx64_slot(tx64_interleaver(N, NC), NC)] = TX64_Q_OF_BITS[b[:, :NC], b[:, NC:]]
    return q


def tx64_modulate(oracle, mode, payload, layout, prs=None):
    """complex128 frame, NULL first; every phasor has modulus one (integer eighths of a turn accumulated exactly)"""
    g = oracle.geometry(mode)
    N, NC, L, P, CP = g.nb_fft, g.nb_carriers, g.nb_frame_symbols, g.nb_symbol_period, g.nb_cp
    prs = (oracle.prs_fft_mode(mode) if prs is None else np.asarray(prs)).astype(np.complex128)
    bins = tx64_carriers(NC) % N                                        # carrier k sits in bin k mod N
    q = tx64_quarters(payload, layout, N, NC, L)
    eighths = np.concatenate([np.zeros((1, NC), np.int64), np.cumsum(2 * q + 1, axis=0)]) % 8
    spec = np.zeros((L, N), np.complex128)
    spec[:, bins] = prs[bins][None, :] * np.exp(0.25j * np.pi * eighths)
    spec[0] = prs                                                       # the PRS symbol is the whole spectrum as given
    t = np.fft.ifft(spec, axis=1) * N                                   # FFTW_BACKWARD is unnormalised
    out = np.zeros(g.nb_frame_samples, np.complex128)
    out[g.nb_null_period:] = np.concatenate([t[:, N - CP:], t], axis=1).reshape(-1)
    return out


def tx64_demodulate(oracle, mode, frame, layout):
    """complex128 differential demodulator of a NULL-first frame -> (payload bytes in `layout`, smallest |component| of
    X_s conj(X_{s-1}) / N^2 over all data carriers; the ideal value is |PRS bin|^2 / sqrt(2) = 1 / sqrt(2))"""
    g = oracle.geometry(mode)
    N, NC, L, P, CP = g.nb_fft, g.nb_carriers, g.nb_frame_symbols, g.nb_symbol_period, g.nb_cp
    syms = np.asarray(frame).astype(np.complex128)[g.nb_null_period:].reshape(L, P)[:, CP:]
    X = np.fft.fft(syms, axis=1)[:, tx64_carriers(NC) % N] / N
    d = X[1:] * np.conj(X[:-1])
    margin = float(min(np.abs(d.real).min(), np.abs(d.imag).min()))
    if layout == TX.LAYOUT_REFERENCE:
        q = np.where(d.imag > 0, np.where(d.real > 0, 0, 1), np.where(d.real > 0, 3, 2))
        v = TX64_V_OF_Q[q].astype(np.uint8).reshape(L - 1, NC // 4, 4)
        return (v[..., 0] | (v[..., 1] << 2) | (v[..., 2] << 4) | (v[..., 3] << 6)).astype(np.uint8).reshape(-1), margin
    dn = d[:, tx64_slot(tx64_interleaver(N, NC), NC)]                   # QPSK symbol n
    b = np.concatenate([dn.real < 0, dn.imag < 0], axis=1).astype(np.uint8)
    return np.packbits(b, axis=1, bitorder="little").reshape(-1), margin


def tx_symbol_bound(s, N, A):
    """relative L2 error of data symbol s (s = 0: the PRS) of the float32 transmitter against exact arithmetic, from first principles:
      * the chain: s complex products X <- X z.  |z| = sqrt(2 A A) against the model's 1: a modulus factor |2 A A - 1| / 2 (first order) per
        step; a float32 complex product by the 4-operation formula has relative error below sqrt(5) u < 3 u (Brent, Percival, Zimmermann,
        "Error bounds on complex floating-point multiplication", Math. Comp. 76 (2007), Theorem 3.1).  The transform is unitary up to its
        scale, so a relative L2 error of the spectrum is the same relative L2 error of the symbol.
      * the transform: Higham, "Accuracy and Stability of Numerical Algorithms" (2nd ed.), Theorem 24.2 (Cooley-Tukey radix 2):
        |y^ - y|_2 / |y|_2 <= log2(N) eta / (1 - log2(N) eta), eta = mu + gamma_4 (sqrt(2) + mu), gamma_4 = 4u / (1 - 4u), mu = the error
        of the stored twiddles, here u (each component is a double-precision value rounded once).  A radix-4 / radix-8 pass is two / three
        radix-2 butterfly levels with exact or once-rounded inner factors, so log2(N) levels in all: c = eta / u = 1 + 4 sqrt(2) ~ 6.66."""
    return s * (abs(2.0 * float(A) * float(A) - 1.0) / 2 + 3 * U32) + fft_rounding_bound(N)


def tx_expectations(oracle, mode, payload, layout):
    """what the -m gpu tests compare the device with: name -> float32 frame"""
    out = {"tx_model": TX.modulate(oracle, mode, payload, layout)}
    if mode == 1 and layout == TX.LAYOUT_REFERENCE:
        out["oracle.modulate_frame_reference_payload"] = oracle.modulate_frame_reference_payload(payload)
    if mode == 1 and layout == TX.LAYOUT_FRAME_BITS:
        out["oracle.modulate_frame"] = oracle.modulate_frame(np.unpackbits(np.ascontiguousarray(payload, np.uint8), bitorder="little"))
    return out


@pytest.mark.parametrize("layout", [TX.LAYOUT_REFERENCE, TX.LAYOUT_FRAME_BITS])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_transmitter_expectations_equal_a_float64_model(oracle, mode, layout):
    g = oracle.geometry(mode)
    N, NC, L, P, CP, NUL = g.nb_fft, g.nb_carriers, g.nb_frame_symbols, g.nb_symbol_period, g.nb_cp, g.nb_null_period
    rng = np.random.default_rng(7100 + 10 * mode + layout)
    payload = rng.integers(0, 256, TX.payload_bytes(oracle, mode), dtype=np.uint8)
    A = TX.A_REF if layout == TX.LAYOUT_REFERENCE else TX.A_BITS
    x64 = tx64_modulate(oracle, mode, payload, layout)
    # the model demodulates to its own payload (the two halves of the model agree before anything is held to them)
    back, margin = tx64_demodulate(oracle, mode, x64, layout)
    assert np.array_equal(back, payload) and margin > 0.70
    s64 = x64[NUL:].reshape(L, P)
    norm64 = np.sqrt((np.abs(s64[:, CP:]) ** 2).sum(axis=1))
    bound = np.array([tx_symbol_bound(s, N, A) for s in range(L)])
    scale32 = (np.float32(1.0) / np.float32(NC) * np.float32(4.0)) * np.float32(127.5)
    scale = float(scale32)
    for name, x32 in tx_expectations(oracle, mode, payload, layout).items():
        x32 = np.ascontiguousarray(x32, np.complex64)
        assert x32.size == g.nb_frame_samples
        # exact: NULL all zero bits, prefix = the symbol's last nb_cp samples as bit patterns, every payload bit back
        assert not x32[:NUL].view(np.uint32).any(), name
        s32 = x32[NUL:].reshape(L, P)
        assert np.array_equal(s32[:, :CP].copy().view(np.uint32), s32[:, N:].copy().view(np.uint32)), name
        back, margin = tx64_demodulate(oracle, mode, x32, layout)
        assert np.array_equal(back, payload), name
        assert margin > 0.5 / np.sqrt(2.0), (name, margin)
        # numeric: per symbol, relative L2 error of the useful part against the float64 model
        err = np.sqrt((np.abs(s32[:, CP:].astype(np.complex128) - s64[:, CP:]) ** 2).sum(axis=1)) / norm64
        worst = int(np.argmax(err / bound))
        print(f"mode {mode} layout {layout} {name}: max relative L2 error {err.max():.3e} (symbol {int(np.argmax(err))}); "
              f"closest to its bound at symbol {worst}: {err[worst]:.3e} of {bound[worst]:.3e}; decision margin {margin:.4f}")
        assert (err <= bound).all(), (name, worst, err[worst], bound[worst])
        # u8: at most one count, and only where the float64 value is within the bound of an integer boundary (1 .. 255; below 0 and
        # above 255 both sides clamp).  A sample's error is at most the symbol's L2 error; the float32 quantiser adds two roundings
        # of values below 256 (x * scale, + 127.5)
        q32 = TX.quantise_u8(oracle, x32, 0.0, NC).astype(np.int64)
        v64 = np.stack([x64.real, x64.imag], -1).reshape(-1) * scale + 127.5
        q64 = np.floor(np.clip(v64, 0.0, 255.0)).astype(np.int64)
        delta = np.concatenate([np.zeros(NUL), np.repeat(bound * norm64, P)]) * scale + 2 * 256 * U32
        delta = np.repeat(delta, 2)
        nearest = np.rint(v64)
        near = (np.abs(v64 - nearest) <= delta) & (nearest >= 1) & (nearest <= 255)
        diff = q32 != q64
        print(f"    u8: {int(diff.sum())} of {diff.size} samples differ by one count; {near.mean():.4%} lie within the bound of a boundary")
        assert np.abs(q32 - q64).max() <= 1, name
        assert not (diff & ~near).any(), (name, int((diff & ~near).sum()))
        assert near.mean() < 0.1, name                                  # (the bound is tight enough to mean something)


@pytest.mark.parametrize("mode", [1, 3])
def test_transmitter_shift_equals_a_float64_rotation(oracle, mode):
    """oracle.apply_pll (what the device's shifted output is held to) against frame * exp(2 pi j f n) in complex128 at every freq_norm the
    -m gpu transmitter tests use; the bound grows with n |f|: at |f| = 0.4999 the last samples of a mode I frame may be off by
    2 pi 2u x 98,285 = 0.074 rad (include/dabgpu.h states this for freq_norm)"""
    g = oracle.geometry(mode)
    rng = np.random.default_rng(7200 + mode)
    payload = rng.integers(0, 256, TX.payload_bytes(oracle, mode), dtype=np.uint8)
    frame = TX.modulate(oracle, mode, payload, TX.LAYOUT_REFERENCE)
    n = np.arange(frame.size)
    mag = np.abs(frame.astype(np.complex128))
    live = mag > 0
    for f in TX.shift_cases():
        got = oracle.apply_pll(frame, f).astype(np.complex128)
        exp = frame.astype(np.complex128) * np.exp(2j * np.pi * float(f) * n)
        assert not got[~live].any()                                     # the NULL period stays zero
        rel = np.abs(got - exp)[live] / mag[live]
        bound = pll_sample_bound(n, f)[live]
        worst = int(np.argmax(rel / bound))
        print(f"mode {mode} freq_norm {float(f):+.6e}: max relative error {rel.max():.3e}; closest to its bound: {rel[worst]:.3e} of "
              f"{bound[worst]:.3e} (bound at the frame's last sample {bound[-1]:.3e})")
        assert (rel <= bound).all(), (float(f), rel[worst], bound[worst])
