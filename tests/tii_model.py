"""Transmitter identification information (TII) of mode I, written from the definition in include/dabgpu.h ("TII"): a float64 generator and
detector that share no code with the library, the derivation of the default detection threshold, and the float32 host model (the
oracle's transform and PLL around csrc/tii_core.h compiled by g++), which the device is compared with bit for bit."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")

NB_FFT, NB_NULL, NB_PREFIX = 2048, 2656, 608
N_MAIN, N_SUB, N_GROUPS, MAX_TX = 70, 24, 8, 4
BLOCKS = (-768, -384, 1, 385)

# the 70 bytes with four bits set, ascending
TABLE = [v for v in range(256) if bin(v).count("1") == 4]


def pattern(p):
    return TABLE[p]


def a(p, b):
    return (TABLE[p] >> (7 - b)) & 1


def carriers(p, c):
    """the 32 carriers of (main id p, sub id c), in the order b ascending, block ascending, k0 then k0 + 1"""
    out = []
    for b in range(8):
        if a(p, b):
            for B in BLOCKS:
                k0 = B + 2 * c + 48 * b
                out += [k0, k0 + 1]
    return out


def null_spectrum(prs, txs):
    """z[k0] += amp PRS[k0], z[k0 + 1] += amp PRS[k0] for every pair of every transmitter (p, c, amp); float64"""
    z = np.zeros(NB_FFT, np.complex128)
    for p, c, amp in txs:
        ks = carriers(p, c)
        for k0, k1 in zip(ks[0::2], ks[1::2]):
            z[k0 % NB_FFT] += amp * complex(prs[k0 % NB_FFT])
            z[k1 % NB_FFT] += amp * complex(prs[k0 % NB_FFT])
    return z


def null_period(prs, txs):
    """the 2656 samples of the NULL period: unnormalised inverse transform of the spectrum behind its last 608 samples"""
    x = np.fft.ifft(null_spectrum(prs, txs)) * NB_FFT
    return np.concatenate([x[-NB_PREFIX:], x])


def fold(power):
    """E[c][b] from the 2048 bin powers"""
    E = np.zeros((N_SUB, N_GROUPS), np.float64)
    for c in range(N_SUB):
        for b in range(N_GROUPS):
            o = 2 * c + 48 * b
            q = [power[(B + o) % NB_FFT] + power[(B + o + 1) % NB_FFT] for B in BLOCKS]
            E[c, b] = (q[0] + q[1]) + (q[2] + q[3])
    return E


def window_energy(samples, null_start, freq):
    """steps 1-5 in float64: the window 608 samples into the NULL, rotated by `freq` cycles per sample from phase 0, transformed, folded"""
    w = np.asarray(samples[null_start + NB_PREFIX:null_start + NB_PREFIX + NB_FFT], np.complex128)
    w = w * np.exp(2j * np.pi * freq * np.arange(NB_FFT))
    X = np.fft.fft(w)
    return fold(X.real * X.real + X.imag * X.imag)


def decide(acc, threshold):
    """step 7 -> list of (sub_id, main_id, mask, strength), ascending sub id"""
    acc = np.asarray(acc, np.float64).reshape(N_SUB, N_GROUPS)
    s = np.sort(acc, axis=1)
    floor = float(np.mean(np.mean(s[:, :4], axis=1)))
    if not floor > 0.0:
        return []
    out = []
    for c in range(N_SUB):
        if s[c, 4] >= threshold * floor:
            on = acc[c] >= threshold * floor
            mask = sum(1 << (7 - b) for b in range(8) if on[b])
            p = TABLE.index(mask) if bin(mask).count("1") == 4 else -1
            out.append((c, p, mask, float(np.mean(acc[c][on])) / floor))
    return out


# ---- the default threshold ----
# Noise alone: a bin power is exponential, a group of a frame is the sum of 8 of them, an accumulated group after F frames a Gamma(8 F, 1)
# variable (any common scale cancels in the decision).  A comb is active when its fifth smallest value s4 reaches threshold x N, N the
# mean over the 24 combs of the mean of each comb's four smallest.  For one comb, splitting by which four of its eight groups are the
# smallest (70 choices, ties have probability 0) and calling them a_1..a_4:
#   P(active) = 70 E[ S(max(t, max a))^4 ],   t = threshold (23 N' + mean a) / 24,
# S the survival function of Gamma(8 F, 1), a_i independent Gamma(8 F, 1), N' the floor of the other 23 combs, independent of this one.
# The expectation is over smooth quantities and a plain seeded Monte Carlo resolves it (no rare event has to be drawn).  P(any comb active)
# lies between 24 P - (24 P)^2 / 2 and 24 P, so at 1e-6 the union bound is exact to 1e-12.
_NOISE = {}


def _noise_draws(frames, n, seed):
    """(floor of 23 other combs, the four smallest of the comb under test) x n, drawn once per (frames, n, seed)"""
    key = (frames, n, seed)
    if key not in _NOISE:
        k = 8 * frames
        rng = np.random.Generator(np.random.PCG64(seed))
        others = np.sort(rng.gamma(k, 1.0, (n, N_SUB - 1, N_GROUPS)), axis=2)[:, :, :4]
        low = rng.gamma(k, 1.0, (n, 4))
        _NOISE[key] = (others.mean(axis=(1, 2)), low.mean(axis=1), low.max(axis=1))
    return _NOISE[key]


def false_alarm_probability(threshold, frames=2, n=50000, seed=20241):
    """P(any comb active in one decision on noise alone) after `frames` accumulated frames"""
    from scipy.special import gammaincc
    n_other, low_mean, low_max = _noise_draws(frames, n, seed)
    t = float(threshold) * (23.0 * n_other + low_mean) / 24.0
    return 24.0 * 70.0 * float(np.mean(gammaincc(8 * frames, np.maximum(t, low_max)) ** 4))


def derive_threshold(frames=2, target=1e-6, step=0.01, seed=20241):
    """(the smallest multiple of `step` at which the false-alarm probability of one decision is below `target`, the root itself)"""
    lo, hi = 1.0, 8.0                                  # (1.0: far above the target; 8.0: far below)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if false_alarm_probability(mid, frames, seed=seed) < target:
            hi = mid
        else:
            lo = mid
    return round(math.ceil(hi / step - 1e-9) * step, 10), hi


# ---- float32 host model: oracle.apply_pll + oracle.fft_n around tii_core.h ----
RECORD_DTYPE = np.dtype([("sub_id", "<i4"), ("main_id", "<i4"), ("mask", "<u4"), ("strength", "<f4")])


def build_host_model(tmp):
    so = os.path.join(str(tmp), "libtii_host_model.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "tii_host_model.cpp"), "-o", so])
    L = C.CDLL(so)
    L.tii_host_fold.argtypes = [C.c_void_p, C.c_void_p]
    L.tii_host_decide.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
    L.tii_host_decide.restype = C.c_int
    L.tii_host_pattern.argtypes = [C.c_int]
    L.tii_host_sort8.argtypes = [C.c_void_p, C.c_void_p]
    L.tii_host_main_id.argtypes = [C.c_uint32]
    return L


class HostModel:
    """one receiver: accumulator and frame count, the steps in the arithmetic of the device"""

    def __init__(self, lib, oracle, threshold):
        self.L, self.O, self.threshold = lib, oracle, np.float32(threshold)
        self.reset()

    def reset(self):
        self.acc = np.zeros(N_SUB * N_GROUPS, np.float32)
        self.frames = 0

    def energy(self, samples, null_start, freq):
        w = np.ascontiguousarray(samples[null_start + NB_PREFIX:null_start + NB_PREFIX + NB_FFT], np.complex64)
        X = np.ascontiguousarray(self.O.fft_n(self.O.apply_pll(w, np.float32(freq), 0.0)))
        E = np.zeros(N_SUB * N_GROUPS, np.float32)
        self.L.tii_host_fold(X.ctypes.data, E.ctypes.data)
        return E

    def process(self, samples, null_start, freq):
        self.acc = (self.acc + self.energy(samples, null_start, freq)).astype(np.float32)
        self.frames += 1

    def decide(self):
        rec = np.zeros(N_SUB, RECORD_DTYPE)
        n = self.L.tii_host_decide(self.acc.ctypes.data, self.threshold, rec.ctypes.data)
        return rec[:n]


def records_as_tuples(rec):
    return [(int(r["sub_id"]), int(r["main_id"]), int(r["mask"])) for r in rec]
