"""The sampling-clock tracker of mode I, written from the definition in include/dabgpu.h ("Sampling-clock tracker") and not from the
library's code: a numpy float64 model with the true arctangent, true quotients and the exact 64-bit ramp, the bounds the float32
arithmetic must keep to it, synthetic product frames, and the float32 host model (csrc/clock_core.h compiled by g++), which the device
is compared with bit for bit.

The products are the demodulator's, d = X[s] conj(X[s + 1]): a positive clock error leaves the ramp -theta k on them, the lag product
p = d[c] conj(d[c + L]) turns by +theta L, and the de-rotation multiplies by (cos, sin)(k slope).

Float32 against float64, from the same float32 products, u = 2^-24, no overflow and nothing below the normal range:
  lag     re = fma(lo.re, hi.re, fl(lo.im hi.im)): the inner product rounds (u |lo.im hi.im| <= u |p|), the fused step rounds (u |re|):
          2 u |p| a component, 2 sqrt(2) u |p| as a complex number.
  prior   (cos, sin) within eps_cs = 8.8e-8 + 8.8 u a component, the angle cut to 24 bits (at most 2^-24 cycle =
          2 pi 2^-24 rad), the product order of ch_finish 2 sqrt(2) u: |p| (sqrt(2) eps_cs + 2 sqrt(2) u + 2 pi 2^-24), on top of the
          lag error carried through a rotation of modulus <= 1 + eps.
  fold    exact (signs and swaps) -- as long as both sides choose the same sector, which a product nearer the 45 degree boundary than
          its own error need not: the bounded tests keep the folded angle inside +-40 degrees.
  sum     a component passes at most 450 chain links, 6 tree levels and 2 joins: 458 roundings, |error| <= 458 u (1 + 458 u) sum |p|.
  angle   an error E of the complex sum A turns it by at most asin(E / |A|).  t = im * fl(1 / re): the reciprocal is within 2 u, the
          product rounds: 3 u |t| <= 3 u, which moves atan by no more.  The polynomial: within ATAN_BOUND_CYCLES of atan / (2 pi)
          (approximation and Horner rounding; measured over every tested t, and split in test_clock_model.py).
  update  the residual times 2^59 is exact from 2^-36 cycles up and rounds by half a unit of 2^-64 below.
  ramp    de-rotation: |v32 - v64| <= |d| (sqrt(2) eps_cs + 2 sqrt(2) u + 2 pi 2^-24) (1 + 2 u) as a complex number.

Statistics.  arg p[c] = arg d[c] - arg d[c + L], so along a chain c, c + L, c + 2 L ... of one half (24 carriers, 23 pairs) the phase
noise of the inner products cancels in the sum and only the two ends remain: with carrier SNR g the phase variance of a product is about
1 / g, a row has 64 chains, and the mean angle over the 1472 x 75 pairs has variance about 128 / (g 1472^2 75) rad^2.  The larger term at
low SNR comes from the fold: a lag product's own phase deviates by about sqrt(2 / g), the fraction P = erfc((pi / 4) / (2 / sqrt g)) of
the pairs lies beyond 45 degrees and lands a quarter turn away, each a unit across the sum: another P / 110400 rad^2.  Together
(noise_floor_ppm) 2.2 ppm at 12 dB and 4.3 ppm at 9 dB.  The same wrongly folded pairs pull the sum towards zero: the estimate
under-reads, monotonely in the SNR (test_clock_model.py records the curve), and a loop that
carries the slope from frame to frame closes the rest."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
F32 = np.float32
N_SYMBOLS, N_CARRIERS, LAG, OWNERS = 75, 1536, 32, 256
N_ROW_PAIRS = 2 * (N_CARRIERS // 2 - LAG)                # 1472
N_PAIRS = N_SYMBOLS * N_ROW_PAIRS                        # 110400
U = 2.0 ** -24
Q64 = 1 << 64
CYCLES_PER_PPM = 1e-6 * 2552.0 / 2048.0                  # slope = ppm * 1e-6 * 2552 / 2048 cycles per carrier
MAX_SLOPE = (1000 * 2552 * (1 << 64) + 1024 * 10 ** 6) // (2048 * 10 ** 6)     # round(1000e-6 * 2552 / 2048 * 2^64) in integers
EPS_CS = 8.8e-8 + 8.8 * U
ROTATION_BOUND = math.sqrt(2.0) * EPS_CS + 2.0 * math.sqrt(2.0) * U + 2.0 * math.pi * 2.0 ** -24
LAG_BOUND = 2.0 * math.sqrt(2.0) * U
SUM_ROUNDINGS = 458
ATAN_LIMIT_RAD = 2.5e-5                                  # the equivalent of 0.1 ppm at lag 32: what the polynomial must stay below
ATAN_BOUND_CYCLES = 4.0e-7                               # what include/dabgpu.h states for it: 2.5e-6 rad
RAD_PER_PPM = 2.0 * math.pi * LAG * CYCLES_PER_PPM       # angle of A per ppm of residual
ATAN_COEFFS = (0.15915131568908691, -0.052938565611839294, 0.03080289624631405, -0.018529823049902916, 0.008379058912396431,
               -0.001865148195065558)


def carrier_numbers():
    c = np.arange(N_CARRIERS)
    return np.where(c < 768, c - 768, c - 767)


def slope_q64(ppm):
    return int(round(ppm * CYCLES_PER_PPM * 2.0 ** 64))


def ppm_of(slope):
    return int(slope) / 2.0 ** 64 / CYCLES_PER_PPM


def clamp(s):
    return max(-MAX_SLOPE, min(MAX_SLOPE, int(s)))


def ramp_cycles(slope, k):
    """the exact ramp k * slope mod 2^64 as cycles in [-1/2, 1/2), per Python integer"""
    out = np.empty(len(k), np.float64)
    for i, kk in enumerate(k):
        ph = (int(kk) * int(slope)) % Q64
        out[i] = (ph - Q64 if ph >= Q64 // 2 else ph) / 2.0 ** 64
    return out


def noise_floor_ppm(snr_db):
    """one standard deviation of a frame's estimate near lock at carrier SNR snr_db (module docstring): the end terms of the 64 chains of
    a row, and the pairs that noise folds into the wrong sector"""
    g = 10.0 ** (snr_db / 10.0)
    wrong = math.erfc((math.pi / 4.0) / (2.0 / math.sqrt(g)))             # P(|N(0, 2 / g)| > pi / 4)
    return math.sqrt(128.0 / (g * N_ROW_PAIRS ** 2 * N_SYMBOLS) + wrong / N_PAIRS) / RAD_PER_PPM


# ---- float64 model ----
def lag_products(d):
    """[75][1536] complex -> p [75][1472]: both carriers of a pair in one half"""
    d = np.asarray(d, np.complex128).reshape(N_SYMBOLS, N_CARRIERS)
    lo = np.concatenate([d[:, 0:768 - LAG], d[:, 768:1536 - LAG]], axis=1)
    hi = np.concatenate([d[:, LAG:768], d[:, 768 + LAG:1536]], axis=1)
    with np.errstate(all="ignore"):
        return lo * np.conj(hi)


def fold(p):
    """one of p, -p, -i p, i p with |im| <= re"""
    p = np.asarray(p, np.complex128)
    big = np.abs(p.real) >= np.abs(p.imag)
    return np.where(big, np.where(p.real >= 0, p, -p), np.where(p.imag > 0, -1j * p, 1j * p))


def estimate(d, slope_in=0, gain=1.0):
    """steps 1 to 6 in float64 -> dict(A, sum_abs, dropped, valid, residual_cycles, slope_out (a float), min_margin_rad)"""
    p32 = lag_products(np.asarray(d, np.complex64))
    s_in = clamp(slope_in)
    p = p32
    if s_in != 0:
        p = p * np.exp(-2j * np.pi * ramp_cycles(s_in, [LAG])[0])
    with np.errstate(all="ignore"):
        ok = np.isfinite(p.real) & np.isfinite(p.imag)
        f = fold(np.where(ok, p, 0))
        A = f.sum()
        dropped = int((~ok).sum())
        valid = bool(A.real > 0 and abs(A.imag) <= A.real and 2 * dropped < N_PAIRS and np.isfinite(A.real))
        ang = np.abs(np.angle(f[ok & (np.abs(f) > 0)]))
    res = math.atan2(A.imag, A.real) / (2.0 * math.pi) if valid else 0.0
    return dict(A=A, sum_abs=float(np.abs(np.where(ok, p, 0)).sum()), dropped=dropped, valid=valid, residual_cycles=res,
                slope_out=(s_in + gain * res * 2.0 ** 59) if valid else float(slope_in),
                min_margin_rad=float(math.pi / 4 - ang.max()) if ang.size else math.pi / 4)


def residual_bound_cycles(est, prior):
    """|float32 residual - float64 residual| in cycles, from the module docstring (same sectors on both sides)"""
    per_pair = LAG_BOUND * (1.0 + ROTATION_BOUND) + (ROTATION_BOUND if prior else 0.0)
    E = est["sum_abs"] * (per_pair + math.sqrt(2.0) * SUM_ROUNDINGS * U * (1.0 + SUM_ROUNDINGS * U))
    turn = math.asin(min(1.0, E / abs(est["A"])))
    return (turn + 3.0 * U) / (2.0 * math.pi) + ATAN_BOUND_CYCLES + 2.0 ** -60


def derotate(d, slope):
    """step 7 in float64 with the exact ramp"""
    d = np.asarray(d, np.complex64).astype(np.complex128).reshape(N_SYMBOLS, N_CARRIERS)
    return d * np.exp(2j * np.pi * ramp_cycles(slope, carrier_numbers()))[None, :]


# ---- synthetic frames ----
def qpsk_steps(rng, shape):
    return np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, shape)))


def products(rng, ppm, snr_db=None, second_path=0.5, amplitude=1.0):
    """one frame of DQPSK products [75][1536] complex64 of a two-path channel with the ramp of a clock error of ppm on them: the ramp
    sits on the products as a clock error leaves it there, d = X[s] conj(X[s + 1]) = |H|^2 step exp(-2 pi i theta k); noise (carrier SNR snr_db, None: none) is
    added to the symbols, not to the products, so that neighbouring products share it as on the air"""
    k = carrier_numbers()
    H = amplitude * (1.0 + second_path * np.exp(-2j * np.pi * k * 37.0 / 2048.0))
    theta = ppm * CYCLES_PER_PPM
    X = np.empty((N_SYMBOLS + 1, N_CARRIERS), np.complex128)
    X[0] = qpsk_steps(rng, N_CARRIERS)
    steps = qpsk_steps(rng, (N_SYMBOLS, N_CARRIERS))
    for s in range(N_SYMBOLS):
        X[s + 1] = X[s] * steps[s]
    X = X * H[None, :] * np.exp(2j * np.pi * theta * k[None, :] * np.arange(N_SYMBOLS + 1)[:, None])
    if snr_db is not None:
        q = np.mean(np.abs(H) ** 2) / 10.0 ** (snr_db / 10.0)
        X = X + math.sqrt(q / 2.0) * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    return (X[:-1] * np.conj(X[1:])).astype(np.complex64)


# ---- float32 host model: csrc/clock_core.h ----
_host = {}


def build_host_model(tmp):
    if "lib" in _host:
        return _host["lib"]
    so = os.path.join(str(tmp), "libclock_host_model.so")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                          "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "clock_host_model.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"),
                          "-o", so], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    L = C.CDLL(so)
    L.clkm_max_slope.restype = C.c_int64
    L.clkm_atan_cycles.restype = C.c_float
    L.clkm_atan_cycles.argtypes = [C.c_float]
    L.clkm_atan_cycles_many.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.clkm_fold.argtypes = [C.c_void_p, C.c_void_p]
    L.clkm_sum.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.clkm_estimate.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.clkm_derotate.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.dabgpu_clock_estimate_host.argtypes = [C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]
    L.dabgpu_clock_derotate_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.dabgpu_clock_slope_q64.restype = C.c_int64
    L.dabgpu_clock_slope_q64.argtypes = [C.c_double]
    L.dabgpu_clock_ppm.restype = C.c_double
    L.dabgpu_clock_ppm.argtypes = [C.c_int64]
    _host["lib"] = L
    return L


def _frame(dq):
    return np.ascontiguousarray(dq, np.complex64).reshape(N_SYMBOLS * N_CARRIERS)


def host_sum(lib, dq, slope_in=0):
    corr, n = np.full(2, 99, F32), C.c_uint32(99)
    lib.clkm_sum(_frame(dq).ctypes.data, int(slope_in), corr.ctypes.data, C.byref(n))
    return corr, n.value


def host_estimate(lib, dq, slope_in=0, gain=1.0, sync_ok=True):
    """the compiled header over one frame -> dict(slope, residual, corr, valid); dq may be None for a frame whose record is not valid"""
    s, r, corr = C.c_int64(99), C.c_int64(99), np.full(2, 99, F32)
    ok = lib.clkm_estimate(None if dq is None else _frame(dq).ctypes.data, int(bool(sync_ok)), int(slope_in), float(gain), C.byref(s), C.byref(r),
                           corr.ctypes.data)
    return dict(slope=s.value, residual=r.value, corr=corr, valid=np.uint32(ok))


def host_derotate(lib, dq, slope, in_place=False):
    x = _frame(dq).copy()
    out = x if in_place else np.full_like(x, 99)
    lib.clkm_derotate(x.ctypes.data, out.ctypes.data, int(slope))
    return out.reshape(N_SYMBOLS, N_CARRIERS)


def host_atan_cycles(lib, t):
    t = np.ascontiguousarray(t, F32)
    out = np.empty_like(t)
    lib.clkm_atan_cycles_many(t.ctypes.data, out.ctypes.data, t.size)
    return out


class HostModel:
    """the tracker in the arithmetic of the device: estimate, then de-rotate by the new slope; the state is carried"""

    def __init__(self, lib, gain=1.0):
        self.L, self.gain, self.slope = lib, gain, 0

    def track(self, dq):
        e = host_estimate(self.L, dq, self.slope, self.gain)
        self.slope = e["slope"]
        return host_derotate(self.L, dq, self.slope), e
