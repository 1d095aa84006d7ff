"""The noise estimator of mode I, written from the definition in include/dabgpu.h ("Noise estimate"): a float64 model that shares no code
with the library, the derivation of the calibration constant and of the estimator's variance and TII bias, and the float32 host model
(the oracle's PLL and transform around csrc/noise_core.h compiled by g++), which the device is compared with bit for bit.

Under white noise of power s2 per complex sample a bin power of the unnormalised 2048-point transform is 2048 s2 times a unit
exponential, a group (8 bins) 2048 s2 times a Gamma(8, 1) draw, the groups independent (distinct bins of an orthogonal transform).
The floor F is the mean over 24 combs of the mean of each comb's four smallest groups, so E[F] = 2048 s2 mu with
    mu = E[mean of the four smallest of eight independent Gamma(8, 1) draws]
and N = F / (2048 mu) is unbiased.  Conditioning on the fifth smallest draw t (density 280 G(t)^4 (1 - G(t))^3 g(t), G and g the
Gamma(8, 1) distribution function and density): the four below it are independent draws of the distribution truncated at t, so with
m1(t) = E[x | x < t] = 8 G9(t) / G(t) and m2(t) = E[x^2 | x < t] = 72 G10(t) / G(t) (x g8(x) = 8 g9(x), x^2 g8(x) = 72 g10(x)):
    E[sum of four]   = E[4 m1(t)]
    E[(sum of four)^2] = E[4 m2(t) + 12 m1(t)^2]
Every G_k is closed-form (a finite Poisson sum), so one quadrature over t gives mu and the variance of a comb's share."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")

NB_FFT, NB_NULL, NB_PREFIX, NB_CP = 2048, 2656, 608, 504
N_SUB, N_GROUPS = 24, 8
BLOCKS = (-768, -384, 1, 385)
RATIO_CAP = 2.0 ** -40
RECORD_DTYPE = np.dtype([("noise_power", "<f4"), ("signal_power", "<f4"), ("weight", "<f4"), ("snr", "<f4"), ("valid", "<u4")])


# ---- the constant ----
def gamma_cdf(k, x):
    """P(Gamma(k, 1) <= x) for an integer k: 1 - exp(-x) sum_{j < k} x^j / j!"""
    x = np.asarray(x, np.float64)
    term, total = np.ones_like(x), np.ones_like(x)
    for j in range(1, k):
        term = term * x / j
        total = total + term
    upper = 1.0 - np.exp(-x) * total
    # below k the complement cancels: the series' own tail exp(-x) sum_{j >= k} x^j / j! there (terms fall faster than 2^-j past 2 k)
    term = term * x / k
    tail = np.zeros_like(x)
    for j in range(k, k + 80):
        tail = tail + term
        term = term * x / (j + 1)
    return np.where(x < k, np.exp(-x) * tail, upper)


def gamma_pdf(k, x):
    x = np.asarray(x, np.float64)
    return np.exp(-x) * x ** (k - 1) / math.factorial(k - 1)


def _simpson(y, h):
    return h / 3.0 * (y[0] + y[-1] + 4.0 * y[1:-1:2].sum() + 2.0 * y[2:-1:2].sum())


@functools.lru_cache(maxsize=None)
def low_four_moments(n=1 << 16, upper=80.0):
    """(E[S], E[S^2]) of S = the sum of the four smallest of eight Gamma(8, 1) draws, by Simpson's rule on n intervals over the
    fifth smallest draw (the integrand is smooth, of order t^39 at 0 and e^-4t beyond 20: the rule converges as n^-4)"""
    t = np.linspace(0.0, upper, n + 1)[1:]
    G, g = gamma_cdf(8, t), gamma_pdf(8, t)
    G9, G10 = 8.0 * gamma_cdf(9, t), 72.0 * gamma_cdf(10, t)              # m1 G and m2 G: no quotient is formed
    w = 280.0 * (1.0 - G) ** 3 * g
    h = upper / n
    z = np.zeros(1)
    e1 = _simpson(np.concatenate([z, w * 4.0 * G ** 3 * G9]), h)
    e2 = _simpson(np.concatenate([z, w * (4.0 * G ** 3 * G10 + 12.0 * G ** 2 * G9 * G9)]), h)
    return float(e1), float(e2)


@functools.lru_cache(maxsize=None)
def derive_mu():
    """(mu, its quadrature uncertainty): the difference between two grids, the finer one returned"""
    a = low_four_moments(1 << 14)[0] / 4.0
    b = low_four_moments(1 << 16)[0] / 4.0
    return b, abs(a - b)


def mu_monte_carlo(n=400000, seed=8101):
    """(mean, standard error) of the mean of the four smallest of eight Gamma(8, 1) draws"""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = np.sort(rng.gamma(8.0, 1.0, (n, 8)), axis=1)[:, :4].mean(axis=1)
    return float(m.mean()), float(m.std() / math.sqrt(n))


def unbias():
    """NOISE_UNBIAS = 8 / (mu * 8 * 2048)"""
    return 8.0 / (derive_mu()[0] * 8.0 * 2048.0)


def share_variance():
    """the variance of one comb's share (the mean of its four smallest), in units of (2048 s2)^2"""
    e1, e2 = low_four_moments()
    return (e2 - e1 * e1) / 16.0


def tii_factor(T):
    """E[N] / s2 with T strong transmitters on distinct combs: such a comb's four smallest groups are its four empty ones, four plain
    Gamma(8, 1) draws of mean 8 where a comb of noise alone has mu"""
    mu = derive_mu()[0]
    return (24.0 + T * (8.0 / mu - 1.0)) / 24.0


def relative_deviation(T=0):
    """the standard deviation of one frame's N / s2: 24 - T shares of the variance above, T means of four Gamma(8, 1) draws (8 / 4)"""
    mu = derive_mu()[0]
    return math.sqrt((24 - T) * share_variance() + T * 2.0) / (24.0 * mu)


# ---- the float64 model of steps 1 .. 5 ----
# bins of E[c][b]: four blocks, two carriers each
_BINS = np.array([[[[(B + 2 * c + 48 * b + i) % NB_FFT for i in (0, 1)] for B in BLOCKS] for b in range(N_GROUPS)] for c in range(N_SUB)])


def fold(power):
    """E[c][b] from the 2048 bin powers"""
    q = np.asarray(power, np.float64)[_BINS].sum(axis=3)                  # [24][8][4]
    return (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])


def group_energy(samples, null_start, freq):
    w = np.asarray(samples[null_start + NB_PREFIX:null_start + NB_PREFIX + NB_FFT], np.complex128)
    w = w * np.exp(2j * np.pi * float(freq) * np.arange(NB_FFT))
    X = np.fft.fft(w)
    return fold(X.real * X.real + X.imag * X.imag)


def floor_of(E):
    s = np.sort(np.asarray(E, np.float64).reshape(N_SUB, N_GROUPS), axis=1)
    return float(np.mean(np.mean(s[:, :4], axis=1)))


def signal_power(samples, null_start):
    a = null_start + NB_NULL + NB_CP
    x = np.asarray(samples[a:a + NB_FFT], np.complex128)
    return float(np.sum(x.real * x.real + x.imag * x.imag))


def finish(F, P):
    """steps 3 and 5 -> (noise_power, signal_power, weight, snr, valid)"""
    N = F * unbias()
    if not (math.isfinite(P) and math.isfinite(N) and P > 0.0):
        return (0.0, 0.0, 0.0, 0.0, 0)
    w = 1.0 / max(N, P * RATIO_CAP)
    return (N, P, w, max(P - N, 0.0) * w, 1)


def estimate(samples, null_start, freq=0.0):
    return finish(floor_of(group_energy(samples, null_start, freq)), signal_power(samples, null_start))


# ---- float32 host model: oracle.apply_pll + oracle.fft_n around noise_core.h ----
def build_host_model(tmp):
    so = os.path.join(str(tmp), "libnoise_host_model.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "noise_host_model.cpp"), "-o", so])
    L = C.CDLL(so)
    L.noise_host_fold.argtypes = [C.c_void_p, C.c_void_p]
    L.noise_host_floor.argtypes = [C.c_void_p]
    L.noise_host_floor.restype = C.c_float
    L.noise_host_frame_power.argtypes = [C.c_void_p]
    L.noise_host_frame_power.restype = C.c_float
    L.noise_host_finish.argtypes = [C.c_float, C.c_float, C.c_void_p]
    L.noise_host_finish.restype = C.c_int
    L.noise_host_unbias.restype = C.c_float
    L.noise_host_reciprocal.argtypes = [C.c_float]
    L.noise_host_reciprocal.restype = C.c_float
    L.noise_host_reciprocal_worst.argtypes = [C.c_void_p]
    L.noise_host_reciprocal_worst.restype = C.c_double
    L.noise_host_scale.argtypes = [C.c_float, C.c_float]
    L.noise_host_scale.restype = C.c_float
    return L


class HostModel:
    """one frame in the arithmetic of the device"""

    def __init__(self, lib, oracle):
        self.L, self.O = lib, oracle

    def energy(self, samples, null_start, freq):
        w = np.ascontiguousarray(samples[null_start + NB_PREFIX:null_start + NB_PREFIX + NB_FFT], np.complex64)
        X = np.ascontiguousarray(self.O.fft_n(self.O.apply_pll(w, np.float32(freq), 0.0)))
        E = np.zeros(N_SUB * N_GROUPS, np.float32)
        self.L.noise_host_fold(X.ctypes.data, E.ctypes.data)
        return E

    def power(self, samples, null_start):
        a = null_start + NB_NULL + NB_CP
        x = np.ascontiguousarray(samples[a:a + NB_FFT], np.complex64)
        return np.float32(self.L.noise_host_frame_power(x.ctypes.data))

    def finish(self, E, P):
        rec = np.zeros(1, RECORD_DTYPE)
        F = np.float32(self.L.noise_host_floor(np.ascontiguousarray(E, np.float32).ctypes.data))
        self.L.noise_host_finish(F, np.float32(P), rec.ctypes.data)
        return rec[0]

    def estimate(self, samples, null_start, freq=0.0):
        """(record, E[192]): a record with valid = 0 is all zeros, and the device then writes zeros for E as well"""
        E = self.energy(samples, null_start, freq)
        rec = self.finish(E, self.power(samples, null_start))
        return rec, (E if rec["valid"] else np.zeros_like(E))
