"""Shared by the synchroniser's edge tests (not a test module): ONE table of named cases per transmission mode, built from the oracle's
geometry, the oracle's answer to every case, the kinds of answer the table must produce, and the float64 model of
ofdm_demodulator.cpp:360-548 for any geometry (tests/test_independent_pins.py uses it for mode I).

A case is (name, group, symbols, cfg overrides, incoming state).  `symbols` holds one PRS-slot symbol of nb_fft complex64, or several: then
the state is carried from one symbol to the next (the tracking sequences).  Every position comes from oracle.geometry(mode):
cp = nb_cp, N = nb_fft, period = nb_symbol_period.

What the reference does in the branches these cases reach (the oracle restates it, the device must equal the oracle bit for bit):
  * the fine arg-max multiplies dB VALUES by the distance weight: below 0 dB the weight prefers FAR positions;
  * the fine scan starts from the UNWEIGHTED ir[0] and compares it with the weighted later values: a frame near offset N-1-cp is reported at -cp;
  * the validity test is !((max - avg) < threshold): a NaN response passes it, the record says sync_valid = 1, fine_time_offset = -cp."""
import collections
import functools

import numpy as np

GROUPS = ("position", "scale", "non-finite", "coarse-edge", "tracking", "cfg")
KINDS = ("weighted-above-cp", "weighted-below-cp", "unweighted-index-0", "invalid", "nan-state-valid", "coarse-minus-inf-next-to-finite",
         "impulse-all-below-0dB", "slow-step", "fast-large-step", "tied-maximum")
TRACK_BINS = (3.0, 3.2, 3.2, 4.4, 4.4, 6.0, 5.0)          # fast (first), slow, slow, slow (1.2 bins < 1.5), slow, fast (large error), slow
MODE1_RMS = 39.2                                            # the mode I modulator's PRS level (tests/test_gpu_modes.py divides by it); modes II-IV: 1
CFG_FIELDS = ("fine_freq_update_beta", "is_coarse_freq_correction", "max_coarse_freq_correction_norm", "coarse_freq_slow_beta",
              "impulse_peak_threshold_db", "impulse_peak_distance_probability")

Case = collections.namedtuple("Case", "name group symbols cfg state")       # cfg: sorted tuple of (field, value); state: (coarse, fine, found, offset)
Step = collections.namedtuple("Step", "coarse fine found valid offset freq_resp impulse coarse_in fine_in found_in offset_in")

# Scale factors of the `scale` group.  1e-3 .. 1e14 are the issue's; the smaller modes need other exponents for the same branches (their
# responses lie lower: fewer carriers, amplitude 1 instead of 39), found on the CPU with the oracle alone and recorded in the case names.
SCALES = {1: (1e-3, 1e-9, 1e-12, 1e-15, 1e-18, 1e10, 1e14),
          2: (1e-3, 1e-9, 1e-12, 1e-15, 1e-18, 1e10, 1e14),
          3: (1e-3, 1e-9, 1e-12, 1e-15, 1e-18, 1e10, 1e14),
          4: (1e-3, 1e-9, 1e-12, 1e-15, 1e-18, 1e10, 1e14)}


# Exact ties in the fine arg-max: with impulse_peak_distance_probability = 1 every weight is 1, and a sample whose squared magnitude overflows
# comes out of the dB function at one and the same value (it has no branch for +inf): at these scales several samples do, index 0 does not,
# and the reference's strict > keeps the LOWEST of them.  (Coarse stage off: at these scales it would make the offset NaN.)
TIE_SCALE = {1: 1e14, 2: 1e17, 3: 1e17, 4: 1e16}


def amplitude(mode):
    return MODE1_RMS if mode == 1 else 1.0


def make_cfg(module, overrides=()):
    """SyncCfg of `module` (oracle or dabgpu): the default with the case's overrides"""
    c = module.sync_cfg_default()
    for k, v in overrides:
        setattr(c, k, v)
    return c


def _prs_region(oracle, mode):
    """NULL + phase reference symbol of a clean frame in transmission order: every PRS slot of the table lies inside it"""
    g = oracle.geometry(mode)
    if mode == 1:
        tx = oracle.modulate_frame(np.zeros(oracle.NB_FRAME_BITS, np.uint8))
    else:
        import modes_model as MM
        tx = MM.make_tx_frame(oracle, mode, np.zeros(g.nb_frame_bits, np.uint8), np.random.default_rng(0))
    return tx[:g.nb_null_period + g.nb_symbol_period].copy()


def max_off_of(norm, N):
    return min(max(int(np.float32(norm) * np.float32(N)), 0), N // 2)


@functools.lru_cache(maxsize=None)
def _table(mode):
    import oracle
    oracle.build()
    g = oracle.geometry(mode)
    N, cp = g.nb_fft, g.nb_cp
    region = _prs_region(oracle, mode)
    amp = amplitude(mode)
    rng = np.random.default_rng(4100 + mode)

    def slot(toff, cfo_bins=0.0, noise=0.0):
        """the nb_fft samples at the expected PRS position when the NULL was found toff samples late"""
        x = oracle.apply_pll(region, cfo_bins / N, 0.1)
        if noise > 0:
            x = (x + noise * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))).astype(np.complex64)
        start = g.nb_null_period - toff
        assert 0 <= start and start + N <= x.size
        return x[start:start + N].copy()

    cases = []

    def add(name, group, symbols, cfg=(), state=(0.0, 0.0, 0, 0)):
        if isinstance(symbols, np.ndarray):
            symbols = (symbols,)
        symbols = tuple(np.ascontiguousarray(s, dtype=np.complex64) for s in symbols)
        assert all(s.shape == (N,) for s in symbols) and group in GROUPS
        cases.append(Case(name, group, symbols, tuple(sorted(cfg)), state))

    noise4 = 4.0 * amp / MODE1_RMS
    # ---- position ----
    for toff in (-cp, -cp + 1, -1, 0, 1, cp // 2, N // 4, N // 2, N - 1 - cp - 1, N - 1 - cp):
        add(f"position/toff{toff:+d}/clean", "position", slot(toff))
        add(f"position/toff{toff:+d}/noise4", "position", slot(toff, noise=noise4))
    clean0 = slot(0)
    noisy1 = slot(1, noise=noise4)
    # ---- scale ----
    for s in SCALES[mode]:
        add(f"scale/x{s:g}/clean", "scale", clean0 * np.float32(s))
    for s in SCALES[mode]:
        add(f"scale/x{s:g}/noise4", "scale", slot(0, noise=noise4) * np.float32(s))
    # ---- non-finite ----
    x = clean0.copy(); x[N // 3] = np.nan
    add("non-finite/one-nan", "non-finite", x)
    x = clean0.copy(); x[N // 3] = np.complex64(complex(np.inf, 0.0))
    add("non-finite/one-inf", "non-finite", x)
    add("non-finite/zeros", "non-finite", np.zeros(N, np.complex64))
    noise_only = (amp * (rng.standard_normal(N) + 1j * rng.standard_normal(N))).astype(np.complex64)
    add("non-finite/pure-noise", "non-finite", noise_only)
    # ---- coarse-edge ----
    M = N // 2
    for cfo in (M - 1, -(M - 1), M, -M, -M + 0.6, 300.5 * N / 2048):
        add(f"coarse-edge/default/cfo{cfo:+g}", "coarse-edge", slot(0, cfo, noise4))
    for norm in (0.05, 0.0, -0.1, 0.6):
        mo = max_off_of(norm, N)
        for what, cfo in (("at", mo), ("plus1", mo + 1), ("minus0.4", -(mo + 0.4)), ("far", mo + N // 4 + 0.3)):
            add(f"coarse-edge/norm{norm:g}/max_off{mo}/{what}/cfo{cfo:+g}", "coarse-edge", slot(0, cfo, noise4),
                cfg=(("max_coarse_freq_correction_norm", norm),))
    # ---- tracking ----
    track = tuple(slot(0, b, noise4) for b in TRACK_BINS)
    add("tracking/sequence/beta-default", "tracking", track)
    for beta in (0.0, 1.0):
        add(f"tracking/sequence/beta{beta:g}", "tracking", track, cfg=(("coarse_freq_slow_beta", beta),))
    add("tracking/found-40-bins-away", "tracking", slot(0, 3.0, noise4), state=(float(np.float32((-3.0 + 40.0) / N)), 0.0, 1, 0))
    wrap = 0.5 * (1.0 / N) * 1.01
    add("tracking/fine-near-plus-wrap", "tracking", slot(0, 3.0, noise4), state=(0.0, float(np.float32(0.995 * wrap)), 0, 0))
    add("tracking/fine-near-minus-wrap", "tracking", slot(0, -3.0, noise4), state=(0.0, float(np.float32(-0.995 * wrap)), 0, 0))
    add("tracking/fine-near-plus-wrap/slow-step", "tracking", slot(0, 3.2, noise4),
        state=(float(np.float32(-3.0 / N)), float(np.float32(0.999 * wrap)), 1, 0))
    # |error| EXACTLY 1.5 / N while found: `>` makes it a slow step.  p = the oracle's first estimate of the symbol, incoming freq_coarse =
    # p + 1.5 / N (exact in float32: p is near -3 / N, the sum is smaller in magnitude), so that p - freq_coarse = -1.5 / N without rounding
    st = oracle.SyncState(0.0, 0.0, 0, 0, 0, 0)
    oracle.coarse_freq_sync_mode(mode, track[0], st, oracle.sync_cfg_default())
    at = np.float32(st.freq_coarse) + np.float32(1.5) / np.float32(N)
    assert np.float32(st.freq_coarse) - at == -(np.float32(1.5) / np.float32(N))
    add("tracking/error-exactly-1.5-bins", "tracking", track[0], state=(float(at), 0.0, 1, 0))
    # ---- cfg ----
    for prob in (0.0, 0.15, 1.0):
        for thr in (0.0, 20.0, 60.0, 1e9, -1e9):
            for s in (1.0, 1e-3):
                add(f"cfg/prob{prob:g}/thr{thr:g}/x{s:g}", "cfg", noisy1 * np.float32(s),
                    cfg=(("impulse_peak_distance_probability", prob), ("impulse_peak_threshold_db", thr)))
    add("cfg/coarse-disabled/incoming-coarse-nonzero", "cfg", slot(cp // 2, 0.2, noise4), cfg=(("is_coarse_freq_correction", 0),),
        state=(float(np.float32(5.0 / N)), float(np.float32(0.1 / N)), 1, 0))
    add("cfg/invalid-keeps-incoming-offset-12345", "cfg", noise_only, state=(0.0, 0.0, 0, 12345))
    # (group non-finite: the squared magnitudes overflow inside the transform chain, which no float64 model follows)
    add(f"non-finite/overflow/x{TIE_SCALE[mode]:g}/coarse-disabled/prob1/tied-maximum", "non-finite", slot(cp // 2, 0.2, noise4) * np.float32(TIE_SCALE[mode]),
        cfg=(("is_coarse_freq_correction", 0), ("impulse_peak_distance_probability", 1.0)), state=(0.0, float(np.float32(0.1 / N)), 0, 0))
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def table(mode):
    """the cases of a transmission mode (built once per process)"""
    return _table(int(mode))


def configs(cases):
    """the distinct configurations of a table, in order of first appearance"""
    out = []
    for c in cases:
        if c.cfg not in out:
            out.append(c.cfg)
    return out


@functools.lru_cache(maxsize=None)
def _expected(mode):
    import oracle
    conj_ref, time_ref = oracle.sync_refs_mode(mode)
    N = oracle.geometry(mode).nb_fft
    out = []
    for c in table(mode):
        cfg = make_cfg(oracle, c.cfg)
        st = oracle.SyncState(c.state[0], c.state[1], c.state[2], c.state[3], 0, 0)
        offset = c.state[3]
        steps = []
        for sym in c.symbols:
            before = (np.float32(st.freq_coarse), np.float32(st.freq_fine), int(st.is_found_coarse), offset)
            if cfg.is_coarse_freq_correction:
                fr = oracle.coarse_freq_sync_mode(mode, sym, st, cfg, time_ref)
            else:
                fr = None                                   # the response is not written; freq_coarse comes back 0 (:363-367)
                oracle.coarse_freq_sync_mode(mode, sym, st, cfg, time_ref)
            f = np.float32(np.float32(st.freq_coarse) + np.float32(st.freq_fine))
            ok, off, ir = oracle.fine_time_sync_mode(mode, sym, f, cfg, conj_ref)
            if ok:
                offset = off                                # fine_time_offset is written "when sync_valid" (include/dabgpu.h)
            steps.append(Step(np.float32(st.freq_coarse), np.float32(st.freq_fine), int(st.is_found_coarse), int(ok), offset, fr, ir, *before))
        assert all(s.impulse.shape == (N,) for s in steps)
        out.append(tuple(steps))
    return tuple(out)


def expected(mode):
    """the oracle's answer to every case: a tuple of Steps per case, in table order (computed once per process, never modified)"""
    return _expected(int(mode))


def kinds_of(mode, cases, answers):
    """{kind: [case names]} for answers given as Steps (the oracle's, or the device's put into the same record)"""
    import oracle
    cp = oracle.geometry(mode).nb_cp
    found = {k: [] for k in KINDS}
    for c, steps in zip(cases, answers):
        for k, s in enumerate(steps):
            nan_state = bool(np.isnan(s.coarse) or np.isnan(s.fine))
            if nan_state and s.valid:
                found["nan-state-valid"].append(c.name)
            if not s.valid:
                found["invalid"].append(c.name)
            elif not nan_state:
                index = s.offset + cp
                kind = "unweighted-index-0" if index == 0 else ("weighted-above-cp" if index > cp else ("weighted-below-cp" if index < cp else None))
                if kind:
                    found[kind].append(c.name)
            if s.freq_resp is not None and np.isneginf(s.freq_resp).any() and np.isfinite(s.freq_resp).any():
                found["coarse-minus-inf-next-to-finite"].append(c.name)
            top = np.flatnonzero(s.impulse == np.max(s.impulse))
            if s.valid and dict(c.cfg).get("impulse_peak_distance_probability") == 1.0 and top.size > 1 and 0 < top[0] == s.offset + cp:
                found["tied-maximum"].append(c.name)
            if np.isfinite(s.impulse).all() and (s.impulse < 0).all():
                found["impulse-all-below-0dB"].append(c.name)
            # slow_beta = 0: a slow step leaves freq_coarse where it was, a fast one (first estimate, or large error) replaces it
            if k > 0 and dict(c.cfg).get("coarse_freq_slow_beta") == 0.0 and s.found_in and np.isfinite(s.coarse):
                found["slow-step" if s.coarse == s.coarse_in else "fast-large-step"].append(c.name)
    return found


# ---------------------------------------------------------------------------------------------------------------------
# float64 model of ofdm_demodulator.cpp:360-548 for a geometry (n = nb_fft, cp = nb_cp, period = nb_symbol_period)
# ---------------------------------------------------------------------------------------------------------------------
def f64_coarse(prs_sym, prs_fft, coarse, found, cfg, n=2048):
    X = np.fft.fft(prs_sym[:n].astype(np.complex128))
    rel = np.conj(X) * np.roll(X, -1)                                   # CalculateRelativePhase :901-909: arg(conj(z0) z1)
    rel[-1] = 0
    ref_rel = np.conj(prs_fft.astype(np.complex128)) * np.roll(prs_fft.astype(np.complex128), -1)
    ref_rel[-1] = 0
    tref = np.conj(np.fft.ifft(ref_rel))                                # constructor :127-135
    corr = np.fft.fft(np.fft.ifft(rel) * tref)
    mag = 20.0 * np.log10(np.abs(np.fft.fftshift(corr)) + 1e-300)       # CalculateMagnitude :911-920 (fft-shifted)
    M = n // 2
    mco = min(max(int(np.float32(cfg.max_coarse_freq_correction_norm) * np.float32(n)), 0), M)
    idx = [i for i in range(-mco, mco + 1) if i + M != n]
    vals = np.array([mag[i + M] for i in idx])
    k = int(np.argmax(vals))
    srt = np.sort(vals)
    margin = srt[-1] - srt[-2] if srt.size > 1 else np.inf
    max_index = idx[k]

    def peak(index):
        index = min(max(index, -mco), mco)
        fi = min(index + M, n - 1)
        return fi - M, 10.0 ** (mag[fi] / 20.0)
    pk = [peak(max_index - 1), peak(max_index), peak(max_index + 1)]
    s = sum(p[1] for p in pk)
    lerp = sum(p[0] * p[1] / s for p in pk)
    pred = -lerp / n
    err = pred - coarse
    large = abs(err) > 1.5 / n
    fast = large or not found
    return max_index, fast, pred, margin, abs(abs(err) - 1.5 / n)


def f64_fine(prs_sym, prs_fft, freq, cfg, n=2048, cp=504, period=2552):
    x = prs_sym[:n].astype(np.complex128) * np.exp(2j * np.pi * freq * np.arange(n))
    imp = n * np.fft.ifft(np.fft.fft(x) * np.conj(prs_fft.astype(np.complex128)))   # FFTW's backward transform is unnormalised, and the
    db = 20.0 * np.log10(np.abs(imp) + 1e-300)                                      # distance weighting below multiplies dB VALUES: scale matters
    w = 1.0 - (1.0 - np.float64(np.float32(cfg.impulse_peak_distance_probability))) * np.abs(cp - np.arange(n)) / period
    weighted = w * db
    best, bi = db[0], 0                                                  # :503 initialised with the UNWEIGHTED [0]
    for i in range(n):
        if weighted[i] > best:
            best, bi = weighted[i], i
    srt = np.sort(weighted)
    avg = db.mean()
    ok = (best - avg) >= cfg.impulse_peak_threshold_db
    return ok, bi - cp, srt[-1] - srt[-2], abs((best - avg) - cfg.impulse_peak_threshold_db)
