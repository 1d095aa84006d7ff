"""The noise profile of mode I and the banded combiner, written from the definitions in include/dabgpu.h ("Noise profile", "Banded
receive diversity") and not from the library's code: a numpy float32 model in which every operation is one IEEE float32 operation
(softbit_model.fma32 is the exact fused multiply-add), a float64 model of the same steps with the bound the float32 one must keep to it,
the statistics of a band under white noise, and the float32 host model (the oracle's PLL and transform around
csrc/noise_profile_core.h compiled by g++), which the device is compared with bit for bit.

Statistics.  The transform is not normalised: under white noise of power s2 per complex sample a carrier power is 2048 s2 times a unit
exponential, the carriers independent (distinct bins of an orthogonal transform).  A band's m is the mean of `count` such draws over
2048: E[m] = s2, relative standard deviation 1 / sqrt(count) -- 1 / sqrt(12) for a whole band.  First-order smoothing
n_t = n_(t-1) + alpha (m_t - n_(t-1)) of independent frames has the variance alpha / (2 - alpha) of one frame's in the steady state.
The mean M of 128 independent bands has the relative deviation 1 / sqrt(1536) of one frame.

Float32 against float64 (derived as DESIGN 4.26 derives the estimator's): a carrier power is a product, a fused step and the
transform's own error, which both models share when they start from the same float32 spectrum; then one product and one fused
step, each within u = 2^-24 relative, of non-negative terms: (1 + u)^2.  The chain of at most 11 additions of non-negative terms is
within (1 + u)^11, R[count] within u of 1 / count, two more products (the second exact, a power of two): m within (1 + u)^15 - 1 <
16 u.  Smoothing adds a difference, a fused step: for alpha in (0, 1] and positive operands the result is a convex combination, and
the two roundings and both inputs' errors give at most 16 u + 3 u relative to max(m, p) (the difference m - p is not relative to the
result, so the bound is stated against the larger operand).  The mean adds 7 additions and an exact product: (1 + u)^7 - 1 < 8 u.  The
reciprocal is within 1 ulp = 2 u of the exact one."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import diversity_model as DM
import softbit_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
F32 = np.float32
NB_FFT, NB_PREFIX, NB_NULL = 2048, 608, 2656
N_BANDS, BAND, N_CARRIERS, EXCLUDE_WORDS = 128, 12, 1536, 48
WEIGHT_CAP = 2.0 ** -20
U = 2.0 ** -24
BOUND_M = 16 * U                           # m of a frame against float64, from the same float32 spectrum
BOUND_N = 19 * U                           # the smoothed value, relative to max(m, p)
BOUND_MEAN = 8 * U                         # the tree over 128 values beyond its inputs' errors: (1 + u)^7 - 1 < 8 u
R = np.array([0.0] + [F32(1.0) / F32(n) for n in range(1, 13)], F32)          # R[n]: float32 division is correctly rounded


def relative_deviation(alpha=1.0, count=BAND):
    """the relative standard deviation of a band's value under white noise (steady state for alpha < 1)"""
    return math.sqrt(alpha / (2.0 - alpha)) / math.sqrt(count)


def carrier_bins():
    """bin of carrier c in the order of d_dqpsk: carriers -768 .. -1, then 1 .. 768"""
    k = np.concatenate([np.arange(-768, 0), np.arange(1, 769)])
    return k % NB_FFT


def carrier_index(k):
    """carrier k of -768 .. 768 (not 0) -> its place in that order"""
    k = np.asarray(k)
    return np.where(k < 0, k + 768, k + 767)


def exclude_words(carriers):
    """48 words with bit (c mod 32) of word c / 32 set for every carrier index c"""
    w = np.zeros(EXCLUDE_WORDS, np.uint32)
    for c in np.asarray(carriers).reshape(-1):
        w[int(c) >> 5] |= np.uint32(1 << (int(c) & 31))
    return w


def excluded(words):
    """bool [1536] from the words (None: nothing excluded)"""
    if words is None:
        return np.zeros(N_CARRIERS, bool)
    w = np.asarray(words, np.uint32).reshape(EXCLUDE_WORDS)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)


def carrier_powers(spectrum):
    """C[1536] from a float32 spectrum of 2048 bins: fma(re, re, im * im)"""
    X = np.asarray(spectrum, np.complex64)[carrier_bins()]
    with np.errstate(all="ignore"):
        return SM.fma32(X.real, X.real, (X.imag * X.imag).astype(F32))


def tree_mean(v):
    """the mean of 128 float32 values: each half of 64 folded pairwise with partner distance 32 .. 1, the halves added, times 2^-7"""
    a = np.asarray(v, F32).reshape(2, 64).copy()
    with np.errstate(all="ignore"):
        h = 32
        while h >= 1:
            a[:, :h] = a[:, :h] + a[:, h:2 * h]
            h //= 2
        return F32(F32(a[0, 0] + a[1, 0]) * F32(2.0 ** -7))


def positive_finite(x):
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        return (x > 0) & (x <= SM.FLT_MAX)


def bands(C, exclude=None, profile_in=None, alpha=1.0):
    """steps 2 to 5 of one frame in float32 -> (profile_out [128], band_weight [128], mean_noise, valid)"""
    C = np.asarray(C, F32).reshape(N_CARRIERS)
    ex = excluded(exclude).reshape(N_BANDS, BAND)
    alpha = F32(alpha)
    n = np.zeros(N_BANDS, F32)
    with np.errstate(all="ignore"):
        for b in range(N_BANDS):
            keep = ~ex[b] if not ex[b].all() else np.ones(BAND, bool)
            s = None
            for p in C[BAND * b:BAND * b + BAND][keep]:
                s = F32(p) if s is None else F32(s + p)
            m = F32(F32(s * R[int(keep.sum())]) * F32(2.0 ** -11))
            if profile_in is not None and positive_finite(profile_in[b]):
                p = F32(profile_in[b])
                n[b] = SM.fma32(alpha, F32(m - p), p)
            else:
                n[b] = m
        M = tree_mean(n)
        prev = np.zeros(N_BANDS, F32) if profile_in is None else np.asarray(profile_in, F32).reshape(N_BANDS).copy()
        if not (M >= SM.FLT_MIN and M <= SM.FLT_MAX):
            return prev, np.zeros(N_BANDS, F32), F32(0), 0
        cap = F32(M * F32(WEIGHT_CAP))
        w = np.array([DM.reciprocal(x if x > cap else cap) for x in n], F32)
    return n, w, M, 1


def bands64(C, exclude=None, profile_in=None, alpha=1.0):
    """the same steps in float64 with true quotients -> (m [128], n [128], M, w [128]); a valid frame is assumed"""
    C = np.asarray(C, np.float64).reshape(N_BANDS, BAND)
    ex = excluded(exclude).reshape(N_BANDS, BAND)
    ex[ex.all(axis=1)] = False
    cnt = (~ex).sum(axis=1)
    m = np.where(ex, 0.0, C).sum(axis=1) / cnt / 2048.0
    n = m.copy()
    if profile_in is not None:
        p = np.asarray(profile_in, np.float64).reshape(N_BANDS)
        use = np.isfinite(p) & (p > 0)
        with np.errstate(all="ignore"):
            n = np.where(use, p + float(alpha) * (m - p), m)
    M = float(n.mean())
    return m, n, M, 1.0 / np.maximum(n, M * WEIGHT_CAP)


def spectrum64(samples, null_start, freq=0.0):
    """the window's spectrum in float64: 2048 samples from 608 behind the NULL's first, rotated, transformed"""
    w = np.asarray(samples[null_start + NB_PREFIX:null_start + NB_PREFIX + NB_FFT], np.complex128)
    return np.fft.fft(w * np.exp(2j * np.pi * float(freq) * np.arange(NB_FFT)))


def carrier_powers64(samples, null_start, freq=0.0):
    X = spectrum64(samples, null_start, freq)[carrier_bins()]
    return X.real * X.real + X.imag * X.imag


# ---- the banded combiner ----
def branch_weight(band_weight):
    """the weight of a branch with a band table: the tree mean of its band weights, one that is not positive and finite counting as 0"""
    bw = np.asarray(band_weight, F32).reshape(N_BANDS)
    return tree_mean(np.where(positive_finite(bw), bw, F32(0)))


def combine_frame(dq, k, mapper, w=None, valid=None, band=None, layout=DM.BITS_NATURAL):
    """one frame of the banded combiner: DM.combine_frame with band[b] = 128 band weights of branch b or None -> (bits, scale, mask)"""
    n = len(dq)
    band = [None] * n if band is None else list(band)
    if all(x is None for x in band):
        return DM.combine_frame(dq, k, mapper, w, valid, layout)
    ws = np.ones(n, F32) if w is None else np.asarray(w, F32).reshape(n).copy()
    for b in range(n):
        if band[b] is not None:
            ws[b] = branch_weight(band[b])
    kk, mask = DM.scale(k, ws, valid)
    shape = (DM.NB_DATA_SYMBOLS, DM.NB_CARRIERS)
    re = im = None
    with np.errstate(all="ignore"):
        if kk != 0:
            for b in range(n):
                if not (mask >> b) & 1:
                    continue
                d = np.asarray(dq[b], np.complex64).reshape(shape)
                if band[b] is None:
                    wc = np.full(N_CARRIERS, ws[b], F32)
                else:
                    bw = np.asarray(band[b], F32).reshape(N_BANDS)
                    wc = np.repeat(np.where(positive_finite(bw), bw, F32(0)), BAND).astype(F32)
                if re is None:
                    re, im = (wc[None, :] * d.real).astype(F32), (wc[None, :] * d.imag).astype(F32)
                else:
                    re, im = SM.fma32(np.broadcast_to(wc, shape), d.real, re), SM.fma32(np.broadcast_to(wc, shape), d.imag, im)
        if re is None:
            re, im = np.zeros(shape, F32), np.zeros(shape, F32)
        m = np.asarray(mapper)
        first, second = -(re[:, m] * kk), -((-im[:, m]) * kk)
    bits = np.concatenate([SM.quantise(first), SM.quantise(second)], axis=1).reshape(-1)
    return (DM.to_classed(bits) if layout == DM.BITS_MSC_CLASSED else bits), kk, mask


# ---- float32 host model: oracle.apply_pll + oracle.fft_n around noise_profile_core.h ----
_host = {}


def build_host_model(tmp):
    if "lib" in _host:
        return _host["lib"]
    so = os.path.join(str(tmp), "libnoise_profile_host_model.so")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                          "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "noise_profile_host_model.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"),
                          "-o", so], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    L = C.CDLL(so)
    L.npm_count_reciprocal.argtypes, L.npm_count_reciprocal.restype = [C.c_int], C.c_float
    L.npm_carrier_bin.argtypes = [C.c_int]
    L.npm_band_mask.argtypes, L.npm_band_mask.restype = [C.c_void_p, C.c_int], C.c_uint32
    L.npm_mean128.argtypes, L.npm_mean128.restype = [C.c_void_p], C.c_float
    L.npm_branch_weight.argtypes, L.npm_branch_weight.restype = [C.c_void_p], C.c_float
    L.npm_weight.argtypes, L.npm_weight.restype = [C.c_float, C.c_float], C.c_float
    L.npm_carrier_powers.argtypes = [C.c_void_p, C.c_void_p]
    L.npm_frame_bands.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.npm_combine_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dabgpu_noise_profile_bands_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dabgpu_noise_profile_exclude_tii.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.dabgpu_tii_carriers.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.dabgpu_diversity_band_mean_host.argtypes, L.dabgpu_diversity_band_mean_host.restype = [C.c_void_p], C.c_float
    L.dabgpu_get_carrier_mapper.argtypes = [C.c_int, C.c_void_p]
    _host["lib"] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data


def host_bands(lib, Cp, exclude=None, profile_in=None, alpha=1.0, entry="npm_frame_bands"):
    """the compiled header over one frame's carrier powers -> (profile_out, band_weight, mean_noise, valid)"""
    Cp = np.ascontiguousarray(Cp, F32).reshape(N_CARRIERS)
    ex = None if exclude is None else np.ascontiguousarray(exclude, np.uint32).reshape(EXCLUDE_WORDS)
    pin = None if profile_in is None else np.ascontiguousarray(profile_in, F32).reshape(N_BANDS)
    prof, bw, mean = np.full(N_BANDS, 99, F32), np.full(N_BANDS, 99, F32), C.c_float(99.0)
    ok = getattr(lib, entry)(_p(Cp), _p(ex), _p(pin), F32(alpha), _p(prof), _p(bw), C.byref(mean))
    return prof, bw, F32(mean.value), ok


def host_combine_frame(lib, dq, k, w=None, valid=None, band=None, layout=DM.BITS_NATURAL):
    """the compiled header over one frame of the banded combiner; a branch given as None is handed over as an address that must not be read"""
    n = len(dq)
    keep = [None if d is None else np.ascontiguousarray(d, dtype=np.complex64).reshape(-1) for d in dq]
    ptrs = (C.c_void_p * n)(*[_p(d) for d in keep])
    kb = [None if (band is None or x is None) else np.ascontiguousarray(x, F32).reshape(N_BANDS) for x in (band or [None] * n)]
    bptrs = (C.c_void_p * n)(*[_p(x) for x in kb])
    k = np.ascontiguousarray(k, dtype=F32).reshape(n)
    w = None if w is None else np.ascontiguousarray(w, F32).reshape(n)
    v = None if valid is None else np.ascontiguousarray(valid, np.int32).reshape(n)
    bits = np.full(DM.NB_FRAME_BITS, 99, np.int8)
    out_k, mask = C.c_float(0), C.c_uint32(0)
    st = lib.npm_combine_frame(ptrs, _p(k), _p(w), _p(v), bptrs, n, int(layout), _p(bits), C.byref(out_k), C.byref(mask))
    assert st == 0
    return bits, F32(out_k.value), mask.value


class HostModel:
    """one frame in the arithmetic of the device"""

    def __init__(self, lib, oracle):
        self.L, self.O = lib, oracle

    def powers(self, samples, null_start, freq=0.0):
        """C[1536] of the NULL that begins at null_start"""
        w = np.ascontiguousarray(samples[null_start + NB_PREFIX:null_start + NB_PREFIX + NB_FFT], np.complex64)
        X = np.ascontiguousarray(self.O.fft_n(self.O.apply_pll(w, F32(freq), 0.0)), np.complex64)
        Cp = np.zeros(N_CARRIERS, F32)
        self.L.npm_carrier_powers(X.ctypes.data, Cp.ctypes.data)
        return Cp

    def profile(self, samples, null_start, freq=0.0, exclude=None, profile_in=None, alpha=1.0):
        """-> dict(profile, band_weight, mean_noise, carrier_power, valid) as the device writes them"""
        Cp = self.powers(samples, null_start, freq)
        prof, bw, mean, ok = host_bands(self.L, Cp, exclude, profile_in, alpha)
        return dict(profile=prof, band_weight=bw, mean_noise=mean, carrier_power=Cp if ok else np.zeros_like(Cp), valid=np.uint32(ok))
