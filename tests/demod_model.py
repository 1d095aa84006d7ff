"""A float64 OFDM demodulator for transmission modes I-IV, and the error bounds a float32 implementation is held to, stage by stage.

Written from the reference's demodulator (ofdm_demodulator.cpp:57-72 soft bit, :606-618 and :779-840 fine-frequency loop, :650-766 the
pipeline, :768-777 cyclic-prefix phase, :842-889 DQPSK and demapper) and ETSI EN 300 401 clause 14 (frame geometry, carrier order,
frequency interleaver).  It shares nothing with oracle/ or csrc/: the carrier permutation comes from the clause 14.6 recurrence
(tests/pin_common.py), the capture formats are decoded here, the transform is numpy's complex128 one.

End to end (float32 samples in, soft bits out) a float64 model cannot pin a float32 demodulator tightly: with a carrier offset the
float32 phase of the PLL dominates (1e-4 of a symbol's spectrum), and one count of a soft bit is 1/127.  So every stage is pinned on its
own, with the stage's INPUT taken as exact:
  * the spectra against numpy's transform of the input rotated in float64          (fft_symbol_bound)
  * the DQPSK products and the soft bits against the float32 spectra themselves    (soft_bit_intervals)
  * the cyclic-prefix correlation against the float64 sum over the rotated input   (cp_corr_bound), its angle (atan2_bound)
  * the summed phase and the fine-frequency update against the correlations        (total_phase_bound, fine_freq_update)
Every bound is derived in its docstring from the unit roundoff u = 2^-24 and published constants; none is fitted to an implementation.
The hold_* functions assert one stage and return the worst ratio to its bound, which the tests print."""
import numpy as np

from pin_common import U32, fft_rounding_bound, pll_sample_bound, tx64_carriers, tx64_interleaver, tx64_slot


class Geometry:
    """EN 300 401 clause 14.2, in samples of 1 / 2.048 MHz: symbols per frame without the NULL symbol (L), useful part (N), guard
    interval (CP), NULL symbol (NUL), carriers (NC)"""
    TABLE = {1: (76, 2048, 504, 2656, 1536), 2: (76, 512, 126, 664, 384), 3: (153, 256, 63, 345, 192), 4: (76, 1024, 252, 1328, 768)}

    def __init__(self, mode):
        self.mode = mode
        self.L, self.N, self.CP, self.NUL, self.NC = self.TABLE[mode]
        self.P = self.N + self.CP
        self.frame_samples = self.L * self.P + self.NUL         # frame-buffer layout: L symbols (PRS first), then the NULL symbol
        self.frame_bits = (self.L - 1) * 2 * self.NC
        self.bins = tx64_carriers(self.NC) % self.N              # carrier slots in ascending frequency -> transform bins
        self.slot_of_symbol = tx64_slot(tx64_interleaver(self.N, self.NC), self.NC)      # QPSK symbol n sits on this carrier slot


# ---------------------------------------------------------------------------------------------------------------------
# capture formats (app_iq_readers.h:19-44, :79-84): component - bias, times the float32 constant 1 / full scale; the bias of an
# unsigned type is half its range (127.5), a signed one has none and its full scale is the type's maximum
# ---------------------------------------------------------------------------------------------------------------------
CAPTURE = {"raw_u8": (np.dtype("u1"), 127.5, 127.5), "raw_s8": (np.dtype("i1"), 0.0, 127.0), "raw_s16l": (np.dtype("<i2"), 0.0, 32767.0)}


def decode_capture(raw, fmt):
    """bytes of interleaved I, Q components -> complex64; the reader's own arithmetic is float32 (an exact difference, one rounded
    product), so its result IS the exact input of the demodulator"""
    dtype, bias, full = CAPTURE[fmt]
    v = np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=dtype).astype(np.float32)
    v = (v - np.float32(bias)) * (np.float32(1.0) / np.float32(full))
    return v.reshape(-1, 2).copy().view(np.complex64).reshape(-1)


def encode_capture(frame, fmt, peak):
    """test inputs: quantise a complex frame whose components stay below `peak` to the capture format (round to nearest, clamp)"""
    dtype, bias, full = CAPTURE[fmt]
    info = np.iinfo(dtype)
    v = np.stack([frame.real, frame.imag], -1).reshape(-1) / peak * full + bias
    return np.clip(np.floor(v + (0.5 if bias == 0.0 else 0.0)), info.min, info.max).astype(dtype).view(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# test inputs: a float64 DQPSK modulator (clause 14.4-14.7) with the impairments the pin needs
# ---------------------------------------------------------------------------------------------------------------------
def make_frame(mode, rng, f=0.0, noise=0.03, scale=1.0, notch=(), real_symbol=None):
    """-> (complex64 frame in frame-buffer layout, the frame's bits).  Unit r.m.s. symbols carrying random bits behind a random
    unit-modulus reference symbol; white noise of `noise` per component on every sample; the carrier slots in `notch` are not
    transmitted (their bins hold noise alone: the L-inf norm there is ~1e-3 of the other carriers' at the default noise); symbol
    `real_symbol` is made conjugate-symmetric in time after the noise, so that its spectrum is purely real; the whole frame is rotated
    by -f cycles per sample (a demodulator given +f undoes it) and scaled.

    Noise is not optional.  Noise-free DQPSK has |re| = |im| on every carrier: both soft bits then sit on the truncation boundary
    between 126 and 127, and nothing about truncation, scale or norm can be told from them (hold_soft_bits refuses such input)."""
    g = Geometry(mode)
    bits = rng.integers(0, 2, g.frame_bits, dtype=np.uint8)
    b = bits.reshape(g.L - 1, 2 * g.NC)
    z = np.empty((g.L - 1, g.NC), np.complex128)
    z[:, g.slot_of_symbol] = ((1.0 - 2.0 * b[:, :g.NC]) + 1j * (1.0 - 2.0 * b[:, g.NC:])) / np.sqrt(2.0)
    carriers = np.cumprod(np.concatenate([np.exp(0.5j * np.pi * rng.integers(0, 4, (1, g.NC))), z]), axis=0)
    carriers[:, list(notch)] = 0.0
    spec = np.zeros((g.L, g.N), np.complex128)
    spec[:, g.bins] = carriers
    t = np.fft.ifft(spec, axis=1) * (g.N / np.sqrt(g.NC))
    x = np.zeros(g.frame_samples, np.complex128)
    x[:g.L * g.P] = np.concatenate([t[:, g.N - g.CP:], t], axis=1).reshape(-1)
    x += noise * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    if real_symbol is not None:
        body = x[real_symbol * g.P + g.CP:(real_symbol + 1) * g.P]
        body[:] = 0.5 * (body + np.conj(body[(-np.arange(g.N)) % g.N]))
        x[real_symbol * g.P:real_symbol * g.P + g.CP] = body[g.N - g.CP:]
    x *= scale * np.exp(-2j * np.pi * float(np.float32(f)) * np.arange(x.size))
    return x.astype(np.complex64), bits


# ---------------------------------------------------------------------------------------------------------------------
# the demodulator
# ---------------------------------------------------------------------------------------------------------------------
def demodulate(frame, f, mode):
    """frame: float32 samples taken as exact; f: the float32 offset handed to the PLL.  -> dict of float64 results:
    X [L + 1][N] spectra (the NULL symbol's last), corr [L] = sum over the guard interval of y[N + n] conj(y[n]), mass [L] = the same sum
    over |y[N + n]| |y[n]|, angle [L] = arg corr, total = their sum."""
    g = Geometry(mode)
    x = np.asarray(frame).astype(np.complex128)
    assert x.size == g.frame_samples
    y = x * np.exp(2j * np.pi * float(np.float32(f)) * np.arange(x.size))         # phase 0 at the frame's first sample (:672-677)
    sym = y[:(g.L + 1) * g.P].reshape(g.L + 1, g.P)
    X = np.fft.fft(sym[:, g.CP:], axis=1)
    corr = (sym[:g.L, g.N:] * np.conj(sym[:g.L, :g.CP])).sum(axis=1)
    mass = (np.abs(sym[:g.L, g.N:]) * np.abs(sym[:g.L, :g.CP])).sum(axis=1)
    angle = np.arctan2(corr.imag, corr.real)
    return {"X": X, "corr": corr, "mass": mass, "angle": angle, "total": float(angle.sum())}


def fft_symbol_bound(mode, f):
    """[L + 1] relative L2 error of each symbol's spectrum: the transform (fft_rounding_bound; a relative L2 error of its input is the
    same relative L2 error of its output) plus, with a carrier offset, the PLL's error at the symbol's last sample, where it is largest
    (pll_sample_bound, first order).  The frame-buffer PLL restarts at every symbol with dt0 = float(i P) f, one more rounding of a
    phase of at most n |f| cycles than pll_sample_bound counts (it was derived for one run over the frame): a strict worst case of
    that term is 3/2 of it.  The bound is kept as stated; the phase error depends on (n, f) alone, not on the data."""
    g = Geometry(mode)
    last = np.arange(1, g.L + 2) * g.P - 1
    return fft_rounding_bound(g.N) + (pll_sample_bound(last, f) if float(f) != 0.0 else 0.0)


def cp_corr_bound(mode, f, mass):
    """[L] |corr^ - corr|: (2 e_pll + (3 + ceil(log2 CP) + 2) u) mass.
      * each factor of a term carries the PLL's relative error e_pll (pll_sample_bound at the symbol's last sample; 0 without offset):
        2 e_pll, first order;
      * the conjugate product in its two-FMA form, (fma(b, d, a c), fma(b, c, -(a d))): the components err by u (2|ac| + |bd|) and
        u (2|ad| + |bc|), in modulus at most u |x1| (2|a| + |b|) <= sqrt(5) u |x0| |x1| < 3u per term;
      * the sum is a balanced tree (pairs, then halving strides) of depth ceil(log2 CP), 9 in mode I: a term passes through that many
        additions, each within u of its own partial sum, and componentwise sums of |re|, |im| are at most the sum of moduli (Minkowski);
      * 2u for the second-order terms (e_pll^2 and cross terms), which covers them while e_pll < 3.4e-4, i.e. n |f| < 450 cycles.  At the
        half-cycle offsets of the CPU table the neglected e_pll^2 is 4 % of the bound."""
    g = Geometry(mode)
    e = pll_sample_bound(np.arange(1, g.L + 1) * g.P - 1, f) if float(f) != 0.0 else 0.0
    return (2 * e + (3 + np.ceil(np.log2(g.CP)) + 2) * U32) * mass


# Cephes atanf.c (the constants DESIGN.md 3 item 5 names): atan x ~ x + x z (((p0 z + p1) z + p2) z + p3), z = x x, for |x| <= tan(pi/8);
# above it atan x = pi/4 + atan((x - 1) / (x + 1))
ATAN_P = (8.05374449538e-2, -1.38776856032e-1, 1.99777106478e-1, -3.33329491539e-1)


def atan2_bound():
    """|angle^ - atan2(y, x)| in radians for float32 inputs taken as exact, from the published method, not from an implementation:
      * the polynomial's distance from atan on |x| <= tan(pi/8), computed below in float64;
      * a = min / max rounds once: u (atan is 1-Lipschitz, a <= 1).  Above tan(pi/8): a - 1, a + 1 and their quotient a' round once each,
        3u |a'| <= 3u tan(pi/8), and |da'/da| = 2 / (a + 1)^2 <= 1 there.  Together < 2.25 u;
      * the evaluation: the odd correction x z p(z) is at most tan(pi/8)^3 / 3 = 0.024 and collects under 9 roundings (z, three fused
        Horner steps, the product, z's error entering four times): 0.21 u; the closing fused step rounds a value <= pi/8: 0.40 u.  < u;
      * the octant: pi/4 + r, pi/2 - r, pi - r each round a value of at most pi/4, pi/2, pi once: 7 pi / 4 u, and the float32
        constants are off by |float32(c) - c| (computed below)."""
    t = np.tan(np.pi / 8)
    x = np.linspace(-t, t, 400001)
    z = x * x
    approx = float(np.abs(x + x * z * np.polyval(ATAN_P, z) - np.arctan(x)).max())
    consts = sum(abs(float(np.float32(c)) - c) for c in (np.pi / 4, np.pi / 2, np.pi))
    return approx + consts + (2.25 + 1.0 + 7 * np.pi / 4) * U32


def total_phase_bound(angle, angle_bound):
    """|total^ - total| of the float32 running sum total^ <- fl(total^ + angle^_k), k = 0 .. L - 1 (:685-690, one pipeline): with S_k the
    exact partial sums and e_k the error after step k,  e_k <= e_{k-1} + b_k + u (|S_k| + e_{k-1} + b_k),  b_k = the bound of angle k.
    No term is dropped."""
    e = 0.0
    for s, b in zip(np.cumsum(angle), np.broadcast_to(angle_bound, np.shape(angle))):
        e = e + b + U32 * (abs(s) + e + b)
    return e


def fine_freq_update(mode, fine, total, total_bound, beta):
    """:606-618, :779-840 in float64: fine' = fmod(fine + delta, wrap), delta = -beta (1/N) (total / L) / (2 pi), wrap = 0.5 (1/N) 1.01.
    fine, beta: float32 values taken as exact.  -> (fine', bound, near_wrap).
      * delta: total / L rounds once, 1/N is a power of two (exact, as is its product), the quotient by float32(pi) 2 rounds once and
        the constant is off by c = |float32(pi) - pi| / pi, the product with beta rounds once: (1 + u)^3 (1 + c) - 1 relative, on
        |delta| + the share of total's own bound;
      * the sum fine + delta rounds once: u |sum|;
      * fmod is exact, but wrap^ = fl(0.5 (1/N) float32(1.01)) is off by (|float32(1.01) - 1.01| / 1.01 + u) wrap, and k = trunc(sum / wrap)
        wraps are subtracted: |k| times that.
    near_wrap: |sum| lies within the bound of a multiple of wrap, where float32 may wrap once more or less -- the one excuse."""
    g = Geometry(mode)
    beta = float(np.float32(beta))
    gain = beta / (g.N * g.L * 2 * np.pi)
    delta = -gain * total
    rel = (1 + U32) ** 3 * (1 + abs(float(np.float32(np.pi)) - np.pi) / np.pi) - 1
    e_delta = gain * total_bound * (1 + rel) + abs(delta) * rel
    s = float(np.float32(fine)) + delta
    e_sum = e_delta + U32 * (abs(s) + e_delta)
    wrap = 0.5 * 1.01 / g.N
    e_wrap = wrap * (abs(float(np.float32(1.01)) - 1.01) / 1.01 + U32) * (1 + U32)
    k = np.trunc(s / wrap)
    nearest = np.rint(abs(s) / wrap)
    near = bool(nearest >= 1 and abs(abs(s) - nearest * wrap) <= e_sum + nearest * e_wrap)
    return s - k * wrap, e_sum + abs(k) * e_wrap, near


def soft_bit_intervals(X, mode):
    """X: [>= L][N] float32 spectra taken as exact.  For X_i = a + jb, X_{i+1} = c + jd (:861, in1 = symbol i):
        d = X_i conj(X_{i+1}) = (ac + bd) + j (bc - ad),  A = max(|re d|, |im d|)  (:882, the L-inf norm),
        soft bit n = trunc(-127 re d / A), soft bit n + NC = trunc(+127 im d / A), d on the carrier of QPSK symbol n  (:57-72, :874, :886-887)
    in float64 (the products of float32 values are exact there).  What float32 may do to it:
      * the two-FMA product, fma(b, d, fl(ac)): each rounding is within u / (1 + u) of its exact argument, so
        |re^ - re| <= u/(1+u) (|ac| + |ac| (1 + u/(1+u)) + |bd|) < 2u (|ac| + |bd|) = E_re strictly (reached only where bd vanishes and
        both roundings are at their worst: a purely real symbol comes within 1 % of it), likewise E_im = 2u (|bc| + |ad|);
      * A^ = max(|re^|, |im^|) is off by at most E_A = max(E_re, E_im) (max is 1-Lipschitz);
      * the quotient: |x^/A^ - x/A| <= (E_x + |x/A| E_A) / (A - E_A), then it rounds once, and its product with 127 rounds once:
        |x/A| ((1 + u)^2 - 1);
    in counts  delta = 127 ((E_x + |v| E_A) / (A - E_A) + |v| ((1 + u)^2 - 1)),  v = x/A, about 6e-5 -- and it grows as 1/A where the products
    cancel.  The soft bit lies in [trunc(w - delta), trunc(w + delta)], w = -+127 v.
      * the component that IS the norm gives x/A = +-1 exactly, hence -+127 exactly, whenever ||re| - |im|| > E_re + E_im (float32 then
        picks the same component).
    -> dict in frame-bit order: lo, hi (int), exact (the norm's component), w (float64 soft value), delta; and d, E_re, E_im [L-1][NC] in
    ascending carrier order (the DQPSK view)."""
    g = Geometry(mode)
    Xc = np.asarray(X)[:g.L][:, g.bins]
    a, b = Xc[:-1].real.astype(np.float64), Xc[:-1].imag.astype(np.float64)
    c, d = Xc[1:].real.astype(np.float64), Xc[1:].imag.astype(np.float64)
    re, im = a * c + b * d, b * c - a * d
    E_re, E_im = 2 * U32 * (np.abs(a * c) + np.abs(b * d)), 2 * U32 * (np.abs(b * c) + np.abs(a * d))
    A, E_A = np.maximum(np.abs(re), np.abs(im)), np.maximum(E_re, E_im)
    assert (A > 2 * E_A).all(), "a carrier without energy: its soft bits are not defined by the model"
    clear = np.abs(np.abs(re) - np.abs(im)) > E_re + E_im
    out = {"d": re + 1j * im, "E_re": E_re, "E_im": E_im}
    parts = {}
    for name, x, E_x, sign, is_norm in (("re", re, E_re, -1.0, np.abs(re) > np.abs(im)), ("im", im, E_im, 1.0, np.abs(im) > np.abs(re))):
        v = x / A
        delta = 127.0 * ((E_x + np.abs(v) * E_A) / (A - E_A) + np.abs(v) * ((1 + U32) ** 2 - 1))
        w = sign * 127.0 * v
        exact = clear & is_norm
        lo, hi = np.trunc(w - delta), np.trunc(w + delta)
        pm = np.rint(w)                                                  # +-127 exactly where the component is the norm
        lo, hi = np.where(exact, pm, lo), np.where(exact, pm, hi)
        parts[name] = [q[:, g.slot_of_symbol] for q in (lo, hi, exact, w, delta)]
    for i, key in enumerate(("lo", "hi", "exact", "w", "delta")):
        out[key] = np.concatenate([parts["re"][i], parts["im"][i]], axis=1).reshape(-1)
    out["lo"], out["hi"] = np.clip(out["lo"], -127, 127).astype(np.int64), np.clip(out["hi"], -127, 127).astype(np.int64)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# one stage each: assert, return the worst ratio to the bound
# ---------------------------------------------------------------------------------------------------------------------
AMBIGUOUS_CAP = 1e-3      # share of soft bits per frame whose interval may hold two integers (2 delta ~ 1.2e-4 of them for spread-out values)


def hold_fft(X32, ref, mode, f, what=""):
    """every symbol's spectrum within fft_symbol_bound of the model's"""
    g = Geometry(mode)
    got = np.asarray(X32).reshape(g.L + 1, g.N).astype(np.complex128)
    err = np.sqrt((np.abs(got - ref["X"]) ** 2).sum(axis=1)) / np.sqrt((np.abs(ref["X"]) ** 2).sum(axis=1))
    ratio = err / fft_symbol_bound(mode, f)
    assert (ratio <= 1.0).all(), (what, "spectrum of symbol", int(np.argmax(ratio)), float(ratio.max()))
    return float(ratio.max())


def hold_dqpsk(d32, iv, what=""):
    """the DQPSK view within the product bound, component by component"""
    got = np.asarray(d32).reshape(iv["d"].shape)
    ratio = max(float((np.abs(got.real - iv["d"].real) / iv["E_re"]).max()), float((np.abs(got.imag - iv["d"].imag) / iv["E_im"]).max()))
    assert ratio <= 1.0, (what, "DQPSK product", ratio)
    return ratio


def hold_soft_bits(bits, iv, what=""):
    """every soft bit in its interval, the norm's component exactly -+127, and an input that can tell: few intervals of two integers.
    -> (share of bits that differ from plain truncation of the float64 value, share of ambiguous bits)"""
    got = np.asarray(bits).reshape(-1).astype(np.int64)
    ambiguous = float(((iv["lo"] != iv["hi"]) & ~iv["exact"]).mean())
    assert ambiguous <= AMBIGUOUS_CAP, (what, f"{ambiguous:.2%} of the soft bits sit on a truncation boundary: the input carries no noise")
    assert 0.45 < iv["exact"].mean() <= 0.5, (what, "near-ties of |re| and |im|", float(iv["exact"].mean()))
    bad = (got < iv["lo"]) | (got > iv["hi"])
    assert not bad.any(), (what, int(bad.sum()), "soft bits outside their interval; first", int(np.argmax(bad)), int(got[np.argmax(bad)]),
                           float(iv["w"][np.argmax(bad)]), float(iv["delta"][np.argmax(bad)]))
    assert (np.abs(got[iv["exact"]]) == 127).all(), what
    return float((got != np.trunc(iv["w"])).mean()), ambiguous


def hold_cp(corr32, ref, mode, f, what=""):
    """every correlation within cp_corr_bound of the model's"""
    got = np.asarray(corr32).reshape(-1).astype(np.complex128)
    bound = cp_corr_bound(mode, f, ref["mass"])
    ratio = np.abs(got - ref["corr"]) / bound
    assert (ratio <= 1.0).all(), (what, "correlation of symbol", int(np.argmax(ratio)), float(ratio.max()))
    return float(ratio.max())


def angle_bounds_from_input(ref, mode, f):
    """[L] bound of a float32 angle against the model's: the correlation's own bound seen from the origin, plus atan2_bound"""
    sub = np.minimum(cp_corr_bound(mode, f, ref["mass"]) / np.abs(ref["corr"]), 1.0)
    return np.arcsin(sub) + atan2_bound()


def hold_angles(angle32, ref, bound, what=""):
    diff = np.abs(np.angle(np.exp(1j * (np.asarray(angle32, np.float64) - ref["angle"]))))       # (the branch cut at +-pi is one point)
    ratio = diff / bound
    assert (ratio <= 1.0).all(), (what, "angle of symbol", int(np.argmax(ratio)), float(ratio.max()))
    return float(ratio.max())


def hold_phase_tail(corr32, total32, fine_in, fine32, beta, mode, what=""):
    """the phase tail on float32 correlations taken as exact: total within total_phase_bound of the float64 sum of their angles (each
    within atan2_bound), the updated fine frequency within fine_freq_update's bound.  fine_in / fine32 may be None.
    -> (ratio of total, ratio of fine or None, excused as near the wrap point)"""
    c = np.asarray(corr32).reshape(-1).astype(np.complex128)
    angle = np.arctan2(c.imag, c.real)
    assert (np.abs(angle) < np.pi - 10 * atan2_bound()).all(), "an angle on the branch cut: the sum is not defined by the model"
    total = float(angle.sum())
    t_bound = total_phase_bound(angle, atan2_bound())
    r_total = abs(float(total32) - total) / t_bound
    assert r_total <= 1.0, (what, "total phase", float(total32), total, t_bound)
    if fine32 is None:
        return r_total, None, False
    exp, f_bound, near = fine_freq_update(mode, fine_in, total, t_bound, beta)
    if near:
        return r_total, None, True
    r_fine = abs(float(fine32) - exp) / f_bound
    assert r_fine <= 1.0, (what, "fine frequency", float(fine32), exp, f_bound)
    return r_total, r_fine, False
