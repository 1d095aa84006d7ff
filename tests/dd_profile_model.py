"""The decision-directed noise profile of mode I, written from the definition in include/dabgpu.h ("Decision-directed noise profile") and
not from the library's code: a numpy float32 model of steps 1 and 2 in which every operation is one IEEE float32 operation
(softbit_model.fma32 is the exact fused multiply-add, numpy's float32 square root is correctly rounded), a float64 model with true roots
and quotients and the bound the float32 one must keep to it, a float64 Monte Carlo of one band, and the float32 host model
(csrc/dd_profile_core.h compiled by g++), which the device is compared with bit for bit.  Bands, smoothing, mean and weights are
tests/noise_profile_model.py's, with Q in the place of C.

Float32 against float64, from the same float32 products, u = 2^-24, no overflow and no result below the normal range.  A term of S2 is a
product and a fused step of non-negative parts: within (1 + u)^2.  The chain begins at 0 (the first addition is exact) and adds 74 times,
every partial sum non-negative: S2 within (1 + u)^76.  k75 is within u of 1 / 75 and the product rounds once: (1 + u)^78.  The root
halves a relative error and rounds once: R = sqrt(S2 k75) within (1 + u)^40 - 1 < 41 u.  A term of S1 rounds once, the chain 74 times, k1
is within u of 1 / (75 sqrt 2) and the product rounds once: A within (1 + u)^77 - 1 < 78 u.  The difference R - A rounds once more, and
its operands' errors are absolute, not relative to it (the cancellation): |Q32 - Q64| <= 41 u R + 78 u A + u |R - A|; clamping both
sides at 0 does not increase a difference.

Statistics.  With X_i = sqrt(a) s_i + n_i, n_i complex Gaussian of power q, the product rotated by its own phase step is
a + sqrt(a) (conj(u_i+1) + u_i) + u_i conj(u_i+1) with u_i = n_i conj(s_i): E|d|^2 = (a + q)^2 exactly, and while decisions are right
the projection (|re| + |im|) / sqrt(2) is the in-phase part, whose mean is a.  So the estimate is unbiased but for the root of a mean of
N = 75 products (Jensen): |X|^2 has mean a + q and relative variance v = q (2 a + q) / (a + q)^2, two consecutive products share one
symbol (relative covariance v), so the mean of |d|^2 has relative variance (4 v + v^2) / N to first order in 1 / N, and
E[rms] = (a + q) (1 - (4 v + v^2) / (8 N)) = a + q - (q / N) (1 + O((q / a)^2)): E[q^] / q = 1 - 1 / 75.  The deviation: to first order
q^ of a carrier is (sum (x - mean x)^2 + sum y^2) / (2 a N), x and y the in-phase and quadrature noise of the products, each of variance
a q: 2 N - 1 degrees of freedom if they were independent, relative deviation sqrt(2 / 149) = 0.116 for a carrier and 0.033 for a band of
12; neighbouring products share a symbol, which raises it somewhat (measured: 0.04).  The NULL's band mean has 1 / sqrt(12) = 0.29."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import noise_profile_model as PM
import softbit_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
F32 = np.float32
N_SYMBOLS, N_CARRIERS, N_BANDS, BAND = 75, 1536, 128, 12
U = 2.0 ** -24
K1 = F32(1.0 / (75.0 * math.sqrt(2.0)))                # 1 / (75 sqrt 2) in float64 lies far from a float32 tie: the nearest float
K75 = F32(1.0) / F32(75.0)                             # float32 division is correctly rounded
BOUND_R, BOUND_A = 41 * U, 78 * U
HIGH_SNR_RATIO = 1.0 - 1.0 / N_SYMBOLS                 # E[q^] / q while decisions are right
NULL_DEVIATION = 1.0 / math.sqrt(BAND)


def carriers(dq):
    """steps 1 and 2 of one frame in float32: dq [75][1536] complex64 -> (Q [1536], A [1536])"""
    d = np.asarray(dq, np.complex64).reshape(N_SYMBOLS, N_CARRIERS)
    s2, s1 = np.zeros(N_CARRIERS, F32), np.zeros(N_CARRIERS, F32)
    with np.errstate(all="ignore"):
        for s in range(N_SYMBOLS):
            re, im = d[s].real, d[s].imag
            s2 = (s2 + SM.fma32(re, re, (im * im).astype(F32))).astype(F32)
            s1 = (s1 + (np.abs(re) + np.abs(im)).astype(F32)).astype(F32)
        A = (s1 * K1).astype(F32)
        q = (np.sqrt((s2 * K75).astype(F32)).astype(F32) - A).astype(F32)
        Q = np.where(q > 0, q, F32(0)).astype(F32)                                    # (a NaN compares false)
    return Q, A


def carriers64(dq):
    """the same in float64 with true quotients -> (Q, A, R): R the root before the amplitude is taken off"""
    d = np.asarray(dq, np.complex64).reshape(N_SYMBOLS, N_CARRIERS).astype(np.complex128)
    R = np.sqrt((d.real ** 2 + d.imag ** 2).sum(axis=0) / 75.0)
    A = (np.abs(d.real) + np.abs(d.imag)).sum(axis=0) / (75.0 * math.sqrt(2.0))
    return np.maximum(R - A, 0.0), A, R


def frame(dq, sync_ok=True, exclude=None, profile_in=None, alpha=1.0):
    """one frame as the device writes it -> dict(profile, band_weight, mean_noise, carrier_noise, carrier_amplitude, valid)"""
    zeros = np.zeros(N_CARRIERS, F32)
    keep = np.zeros(N_BANDS, F32) if profile_in is None else np.asarray(profile_in, F32).reshape(N_BANDS).copy()
    skipped = dict(profile=keep, band_weight=np.zeros(N_BANDS, F32), mean_noise=F32(0), carrier_noise=zeros, carrier_amplitude=zeros.copy(),
                   valid=np.uint32(0))
    if not sync_ok:
        return skipped
    Q, A = carriers(dq)
    prof, w, M, ok = PM.bands(Q, exclude, profile_in, alpha)
    if not ok:
        return skipped
    return dict(profile=prof, band_weight=w, mean_noise=M, carrier_noise=Q, carrier_amplitude=A, valid=np.uint32(1))


# ---- float64 Monte Carlo of one band in one frame ----
def band_products(rng, snr_db, n_bands=1, a=1.0):
    """n_bands x 12 carriers, 76 symbols of unit-modulus pi/4 DQPSK at channel power a and noise power q = a / snr per bin ->
    (products [75][12 n_bands] complex128, q)"""
    q = a / 10.0 ** (snr_db / 10.0)
    n = BAND * n_bands
    phase = np.cumsum(rng.integers(0, 4, (N_SYMBOLS + 1, n)) * 0.5 + 0.25, axis=0) * math.pi
    X = math.sqrt(a) * np.exp(1j * phase) + math.sqrt(q / 2.0) * (rng.standard_normal((N_SYMBOLS + 1, n)) + 1j * rng.standard_normal((N_SYMBOLS + 1, n)))
    return X[:-1] * np.conj(X[1:]), q


def band_estimates(d):
    """q^ of every band of 12 carriers: the mean of the carriers' max(rms - mean projected amplitude, 0), float64"""
    R = np.sqrt((d.real ** 2 + d.imag ** 2).mean(axis=0))
    A = (np.abs(d.real) + np.abs(d.imag)).mean(axis=0) / math.sqrt(2.0)
    return np.maximum(R - A, 0.0).reshape(-1, BAND).mean(axis=1)


def monte_carlo(snr_db, seeds, n_bands=16):
    """-> (E[q^] / q, relative deviation of a band's q^ against its own mean, number of band draws)"""
    est = []
    for seed in seeds:
        d, q = band_products(np.random.Generator(np.random.PCG64(seed)), snr_db, n_bands)
        est.append(band_estimates(d) / q)
    est = np.concatenate(est)
    return float(est.mean()), float(est.std(ddof=1) / est.mean()), est.size


# ---- float32 host model: csrc/dd_profile_core.h ----
_host = {}


def build_host_model(tmp):
    if "lib" in _host:
        return _host["lib"]
    so = os.path.join(str(tmp), "libdd_profile_host_model.so")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                          "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "dd_profile_host_model.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"),
                          "-o", so], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    L = C.CDLL(so)
    L.ddm_k1.restype = L.ddm_k75.restype = C.c_float
    L.ddm_carriers.argtypes = [C.c_void_p] * 3
    L.ddm_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 5
    L.dabgpu_dd_profile_carriers_host.argtypes = [C.c_void_p] * 3
    L.dabgpu_noise_profile_bands_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    _host["lib"] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data


def host_carriers(lib, dq, entry="ddm_carriers"):
    d = np.ascontiguousarray(dq, np.complex64).reshape(N_SYMBOLS * N_CARRIERS)
    Q, A = np.full(N_CARRIERS, 99, F32), np.full(N_CARRIERS, 99, F32)
    getattr(lib, entry)(_p(d), _p(Q), _p(A))
    return Q, A


def host_frame(lib, dq, sync_ok=True, exclude=None, profile_in=None, alpha=1.0):
    """the compiled header over one frame -> the dict of frame(); dq may be None for a frame whose record is not valid"""
    d = None if dq is None else np.ascontiguousarray(dq, np.complex64).reshape(N_SYMBOLS * N_CARRIERS)
    ex = None if exclude is None else np.ascontiguousarray(exclude, np.uint32).reshape(PM.EXCLUDE_WORDS)
    pin = None if profile_in is None else np.ascontiguousarray(profile_in, F32).reshape(N_BANDS)
    prof, bw, mean = np.full(N_BANDS, 99, F32), np.full(N_BANDS, 99, F32), C.c_float(99.0)
    Q, A = np.full(N_CARRIERS, 99, F32), np.full(N_CARRIERS, 99, F32)
    ok = lib.ddm_frame(_p(d), int(bool(sync_ok)), _p(ex), _p(pin), F32(alpha), _p(prof), _p(bw), C.byref(mean), _p(Q), _p(A))
    return dict(profile=prof, band_weight=bw, mean_noise=F32(mean.value), carrier_noise=Q, carrier_amplitude=A, valid=np.uint32(ok))


class HostModel:
    """one frame in the arithmetic of the device, with the profile's interface of tests/noise_profile_model.py's HostModel"""

    def __init__(self, lib):
        self.L = lib

    def profile(self, dq, exclude=None, profile_in=None, alpha=1.0):
        return host_frame(self.L, dq, True, exclude, profile_in, alpha)
