"""The channel-state weighted soft bits (DABGPU_SOFT_CSI, dab-radio_amd/csrc/softbit_csi_core.h) in numpy float32, written from the
header's description and not from its code: the frame power of the phase reference symbol by the one fixed tree, the scale
k = level * 1536 / (2048 P) with its Newton quotient, the soft bit -(c k) with NaN -> 0, the clamp to +-127 and the truncation; and the
reference's normalised soft bits for comparison.  Every operation is one IEEE float32 operation; the fused multiply-add is made exact
below (the product of two floats is exact in a double; the sum is rounded to odd before it is rounded to float, which removes the double
rounding).  tests/test_softbit_model.py holds this file to the compiled header bit for bit; the GPU tests hold the device to both."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SOFT_NORMALISED, SOFT_CSI = 0, 1
NB_FFT, NB_CP, NB_CARRIERS, NB_SYM_BITS, NB_DATA_SYMBOLS = 2048, 504, 1536, 3072, 75
FLT_MAX, FLT_MIN = F32(3.40282347e+38), F32(1.17549435e-38)


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 operands, correctly rounded"""
    a, b, c = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                                  # exact: 48 significant bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                            # TwoSum: s + err = p + c exactly
        even = (s.view(np.int64) & 1) == 0
        fix = (err != 0) & even & np.isfinite(s) & np.isfinite(err)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)          # round to odd
        return s.astype(F32)


def lane_sample(lane, j):
    return 2 * lane + 512 * (j >> 1) + (j & 1)


def frame_power(prs):
    """P of the 2048 useful samples of the phase reference symbol: 256 lanes x 8 samples in the loader's order, each one chain
    re0 * re0, fma(im, im, .), fma(re, re, .), ...; lanes folded inside blocks of 64 at distances 32 .. 1; (w0 + w1) + (w2 + w3)"""
    x = np.ascontiguousarray(prs, dtype=np.complex64).reshape(NB_FFT)
    lanes = np.arange(256)
    with np.errstate(all="ignore"):
        s = x[lane_sample(lanes, 0)]
        acc = fma32(s.imag, s.imag, s.real * s.real)
        for j in range(1, 8):
            s = x[lane_sample(lanes, j)]
            acc = fma32(s.imag, s.imag, fma32(s.real, s.real, acc))
        a = acc.reshape(4, 64).copy()
        h = 32
        while h >= 1:
            a[:, :h] = a[:, :h] + a[:, h:2 * h]
            h >>= 1
        w = a[:, 0]
        return F32(F32(w[0] + w[1]) + F32(w[2] + w[3]))


def scale(level, P):
    """k = level * 1536 / (2048 P): the denominator m 2^e, 1 / m by three Newton steps from -8/17 m + 24/17, one residual correction
    of the quotient, the two powers of two; 0 where P is zero / NaN / infinite, the denominator is not a normal number, or k is not finite"""
    level, P = F32(level), F32(P)
    with np.errstate(all="ignore"):
        if not (P > 0) or not (P <= FLT_MAX):
            return F32(0)
        num = F32(level * F32(1536))
        den = F32(F32(2048) * P)
        if not (den <= FLT_MAX) or not (den >= FLT_MIN):
            return F32(0)
        b = int(den.view(np.uint32))
        e = (b >> 23) - 127
        m = np.uint32((b & 0x007FFFFF) | 0x3F800000).view(F32)
        r = fma32(F32(-0.470588235), m, F32(1.41176471))
        for _ in range(3):
            r = fma32(r, fma32(-m, r, F32(1)), r)
        q = F32(num * r)
        q = fma32(fma32(-m, q, num), r, q)
        a = int(e / 2)                                             # towards zero
        k = F32(F32(q * np.uint32((127 - a) << 23).view(F32)) * np.uint32((127 - (e - a)) << 23).view(F32))
        return F32(k) if k <= FLT_MAX else F32(0)


def soft_scale(prs, level=64.0):
    return scale(level, frame_power(prs))


def quantise(v):
    v = np.asarray(v, dtype=F32)
    with np.errstate(all="ignore"):
        w = np.where(np.isnan(v), F32(0), np.clip(v, F32(-127), F32(127)))
        return np.trunc(w).astype(np.int8)


def csi_bits(d, k):
    """(first, second) soft bits of the DQPSK products d: -(re d * k), -((-im d) * k)"""
    d = np.asarray(d, dtype=np.complex64)
    with np.errstate(all="ignore"):
        return quantise(-(d.real * F32(k))), quantise(-((-d.imag) * F32(k)))


def normalised_bits(d):
    """the reference's: to_vbit(re d / A), to_vbit(-(im d / A)), A = max(|re d|, |im d|), to_vbit(x) = trunc(-x * 127), NaN -> 0"""
    d = np.asarray(d, dtype=np.complex64)
    with np.errstate(all="ignore"):
        ar, ai = np.abs(d.real), np.abs(d.imag)
        A = np.where(ar < ai, ai, ar)

        def vbit(x):
            v = -x * F32(127)
            return np.trunc(np.where(np.isnan(v), F32(0), v)).astype(np.int8)
        return vbit(d.real / A), vbit(-(d.imag / A))


def dqpsk(x0, x1):
    """X_i conj(X_i+1) with the receiver's two fused operations: fma(b, d, a c), fma(b, c, -(a d))"""
    x0, x1 = np.asarray(x0, dtype=np.complex64), np.asarray(x1, dtype=np.complex64)
    a, b, c, d = x0.real, x0.imag, x1.real, x1.imag
    with np.errstate(all="ignore"):
        out = np.empty(x0.shape, np.complex64)
        out.real = fma32(b, d, a * c)
        out.imag = fma32(b, c, -(a * d))
        return out


def symbol_bits(d_sym, mapper, k=None):
    """the 3072 soft bits of one data symbol from its 1536 products in carrier order: bit i belongs to carrier mapper[i] (frequency
    de-interleave), the second bits follow the 1536 first ones; k = None: the normalised policy"""
    d = np.asarray(d_sym, dtype=np.complex64)[np.asarray(mapper)]
    first, second = normalised_bits(d) if k is None else csi_bits(d, k)
    return np.concatenate([first, second])


def frame_bits(dq, mapper, k=None):
    """[75][1536] products of a frame -> its 230400 soft bits in the natural layout"""
    dq = np.asarray(dq, dtype=np.complex64).reshape(NB_DATA_SYMBOLS, NB_CARRIERS)
    return np.concatenate([symbol_bits(dq[s], mapper, k) for s in range(NB_DATA_SYMBOLS)])


# ---- the compiled header ----
_host = {}


def build_host_model(out_dir):
    """g++ -ffp-contract=off over tests/cpp/softbit_host_model.cpp + the host half of the library -> a ctypes library (once per process)"""
    if "lib" in _host:
        return _host["lib"]
    so = os.path.join(str(out_dir), "libsoftbit_host_model.so")
    csrc = os.path.join(ROOT, "dab-radio_amd", "csrc")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                          "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "softbit_host_model.cpp"), os.path.join(csrc, "dabgpu_host_logic.cpp"),
                          "-o", so], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    lib = C.CDLL(so)
    lib.sbm_frame_power.argtypes, lib.sbm_frame_power.restype = [C.c_void_p], C.c_float
    lib.sbm_scale.argtypes, lib.sbm_scale.restype = [C.c_float, C.c_float], C.c_float
    lib.sbm_level_ok.argtypes = [C.c_float]
    lib.sbm_soft_bits.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]
    lib.dabgpu_soft_scale_host.argtypes, lib.dabgpu_soft_scale_host.restype = [C.c_void_p, C.c_float], C.c_float
    lib.dabgpu_soft_cfg_default.argtypes, lib.dabgpu_soft_cfg_default.restype = [C.c_void_p], None
    _host["lib"] = lib
    return lib


def host_frame_power(lib, prs):
    x = np.ascontiguousarray(prs, dtype=np.complex64).reshape(NB_FFT)
    return F32(lib.sbm_frame_power(x.ctypes.data))


def host_scale(lib, level, P):
    return F32(lib.sbm_scale(F32(level), F32(P)))


def host_soft_bits(lib, d, k):
    d = np.ascontiguousarray(d, dtype=np.complex64).reshape(-1)
    first, second = np.empty(d.size, np.int8), np.empty(d.size, np.int8)
    lib.sbm_soft_bits(d.ctypes.data, d.size, F32(k), first.ctypes.data, second.ctypes.data)
    return first, second
