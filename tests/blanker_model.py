"""The impulse blanker's models (include/dabgpu.h, "Impulse blanker"): an independent numpy model in float64 and in float32,
the ctypes binding of the host model (tests/cpp/blanker_host_model.cpp = dab-radio_amd/csrc/blanker_core.h under g++) and the false-alarm
probability of the detector.

THE FLOAT32 MODEL is bit for bit the definition: |x|^2 = fmaf(im, im, re * re) -- the fused step is emulated exactly (the product im * im is
exact in float64, the sum is rounded to odd there and then to float32, which is the correctly rounded float32 result because 53 >= 2 * 24 +
2) -- then five levels of neighbour sums, the product with 2^-5, the window sums in increasing k from 0 and the comparison
(float32)window * p > threshold * ref, every operation one float32 rounding.

THE FALSE-ALARM PROBABILITY.  For complex Gaussian samples of power s the 32 |x|^2 of a block are independent exponentials, so 32 p / s is
Gamma(32) and 32 (one side's sum of W blocks) / s is Gamma(32 W), independent of the block under test (gap >= 0 keeps them apart).  The block
is flagged against that side when W p > T ref, that is X > (T / W) Y with X ~ Gamma(32), Y ~ Gamma(32 W):
X / (X + Y) ~ Beta(32, 32 W) exceeds (T / W) / (1 + T / W).  The greater-of-two reference only lowers the probability (ref >= either side).
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEN, TILE = 32, 1024
DEFAULTS = dict(threshold=3.0, gap=8, window=16, guard=1, start=0, enabled=1)


def params(**kw):
    P = dict(DEFAULTS)
    P.update(kw)
    return P


def mask_words(n_out):
    return n_out // TILE + 2


def false_alarm(threshold, window=16):
    """per-block probability that W p > T (one side's sum) for complex Gaussian samples"""
    from scipy import stats
    c = threshold / window
    return float(stats.beta.sf(c / (1.0 + c), LEN, LEN * window))


def false_alarm_quad(threshold, window=16):
    """the same as the integral of the Gamma(32) tail over the Gamma(32 W) reference"""
    from scipy import integrate, stats
    k = LEN * window
    f = lambda y: stats.gamma.pdf(y, k) * stats.gamma.sf(threshold / window * y, LEN)
    # Gamma(k) beyond 4 k is below e^-700 for k >= 32; the integrand peaks below k, where the tail of X weighs most
    return float(integrate.quad(f, 0.0, 4.0 * k, epsabs=0.0, epsrel=1e-9, limit=400, points=[k * 0.25, k * 0.5, k * 0.75, k, k * 1.5])[0])


# ---- the numpy model ----
def _energy32(x):
    """fmaf(im, im, re * re) in float32, exactly"""
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        c = (re * re).astype(np.float64)                    # the float32 product
        a = im.astype(np.float64) * im.astype(np.float64)   # exact
        s = a + c
        bb = s - a
        err = (a - (s - bb)) + (c - bb)                     # TwoSum: a + c = s + err exactly
        fin = np.isfinite(s) & np.isfinite(err) & (err != 0)
        bits = s.view(np.int64).copy()
        lower = np.where(err < 0, bits - 1, bits)           # the float64 at or below the true sum (all values are >= 0)
        bits = np.where(fin, lower | 1, bits)               # round to odd
        return bits.view(np.float64).astype(np.float32)


def block_powers(x, n_in, start, b0, count, dtype=np.float32):
    """p of blocks [b0, b0 + count): x complex64 [>= n_in]"""
    m = np.arange(b0 * LEN, (b0 + count) * LEN, dtype=np.int64) - int(start)
    ok = (m >= 0) & (m < n_in)
    seg = np.zeros(count * LEN, np.complex64)
    seg[ok] = np.asarray(x)[m[ok]]
    with np.errstate(over="ignore", invalid="ignore"):
        if dtype == np.float32:
            e = _energy32(seg)
        else:
            e = seg.real.astype(np.float64) ** 2 + seg.imag.astype(np.float64) ** 2
        e = e.reshape(count, LEN)
        while e.shape[1] > 1:
            e = e[:, 0::2] + e[:, 1::2]
        return (e[:, 0] * dtype(1.0 / LEN)).astype(dtype)


def decide(P, x, n_in, b0, count, dtype=np.float32):
    """(p, flag, blank) of blocks [b0, b0 + count)"""
    G, W, g, T = P["gap"], P["window"], P["guard"], dtype(P["threshold"])
    r = G + W + g
    p = block_powers(x, n_in, P["start"], b0 - r, count + 2 * r, dtype)          # block b0 - r + j
    q = np.where(np.isfinite(p), p, dtype(0))
    nf = count + 2 * g                                                        # flags of blocks b0 - g + i
    c = np.arange(nf) + (r - g)
    before, after = np.zeros(nf, dtype), np.zeros(nf, dtype)
    for k in range(1, W + 1):
        before = before + q[c - G - k]
        after = after + q[c + G + k]
    ref = np.maximum(before, after)
    with np.errstate(over="ignore", invalid="ignore"):
        flag = ~np.isfinite(p[c]) | ((ref > 0) & (dtype(W) * p[c] > T * ref))
    blank = np.zeros(count, bool)
    for j in range(-g, g + 1):
        blank |= flag[np.arange(count) + g + j]
    return p[r:r + count], flag[g:g + count], blank


def apply(P, x, n_in, pos, n_out, dtype=np.float32):
    """one stream: (y complex64 [n_out], mask uint32 [mask_words(n_out)], blanked blocks among those whose first sample the call holds)"""
    x = np.asarray(x, np.complex64)
    words = np.zeros(mask_words(n_out), np.uint32)
    if n_out == 0:
        return np.zeros(0, np.complex64), words, 0
    m = np.arange(pos, pos + n_out, dtype=np.int64)
    i = m - int(P["start"])
    ok = (i >= 0) & (i < n_in)
    y = np.zeros(n_out, np.complex64)
    y[ok] = x[i[ok]]
    if not P["enabled"]:
        return y, words, 0
    b0, b1 = pos >> 5, (pos + n_out - 1) >> 5
    _, _, blank = decide(P, x, n_in, b0, b1 - b0 + 1, dtype)
    y[blank[(m >> 5) - b0]] = 0
    n = 0
    for b in np.nonzero(blank)[0] + b0:
        first = int(b) << 5
        if pos <= first < pos + n_out:
            words[(first >> 10) - (pos >> 10)] |= np.uint32(1 << (int(b) & 31))
            n += 1
    return y, words, n


# ---- the host model: blanker_core.h under g++ ----
class Stream(C.Structure):
    """dabgpu_blanker_stream (include/dabgpu.h)"""
    _fields_ = [("start", C.c_int64), ("threshold", C.c_float), ("gap", C.c_int32), ("window", C.c_int32), ("guard", C.c_int32),
                ("enabled", C.c_int32), ("reserved", C.c_int32)]


def to_struct(P, cls=Stream):
    T = cls()
    T.start, T.threshold, T.gap, T.window, T.guard, T.enabled = P["start"], P["threshold"], P["gap"], P["window"], P["guard"], P["enabled"]
    return T


_host = {}


def build_host_model(out_dir):
    """g++ -ffp-contract=off over tests/cpp/blanker_host_model.cpp -> a ctypes library (built once per process)"""
    if "lib" in _host:
        return _host["lib"]
    so = os.path.join(str(out_dir), "libblanker_host_model.so")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                          "-I" + os.path.join(ROOT, "dab-radio_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "blanker_host_model.cpp"), "-o", so],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    L = C.CDLL(so)
    L.blm_powers.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
    L.blm_decide.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.blm_apply.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p,
                            C.c_size_t]
    _host["lib"] = L
    return L


def host_powers(L, x, start, b0, count):
    x = np.ascontiguousarray(x, np.complex64)
    out = np.zeros(count, np.float32)
    L.blm_powers(x.ctypes.data, x.shape[-1], int(start), int(b0), int(count), out.ctypes.data)
    return out


def host_decide(L, P, x, b0, count):
    """(flag, blank) of blocks [b0, b0 + count) of one stream"""
    x = np.ascontiguousarray(x, np.complex64)
    flag, blank = np.zeros(count, np.uint8), np.zeros(count, np.uint8)
    L.blm_decide(C.byref(to_struct(P)), x.ctypes.data, x.shape[-1], int(b0), int(count), flag.ctypes.data, blank.ctypes.data)
    return flag.astype(bool), blank.astype(bool)


def host_apply(L, plist, x, pos, n_out, n_in=None):
    """the host model over every stream of plist: x [n_streams][n_in] complex64 or [n_in] shared -> (y [n_streams][n_out] complex64,
    mask [n_streams][mask_words(n_out)] uint32)"""
    x = np.ascontiguousarray(x, np.complex64)
    n_in = x.shape[-1] if n_in is None else n_in
    arr = (Stream * len(plist))(*[to_struct(P) for P in plist])
    y = np.zeros((len(plist), n_out), np.complex64)
    m = np.zeros((len(plist), mask_words(n_out)), np.uint32)
    L.blm_apply(arr, len(plist), x.ctypes.data, x.shape[-1] if x.ndim == 2 else 0, n_in, int(pos), int(n_out), y.ctypes.data, n_out * 8,
                m.ctypes.data, m.shape[1])
    return y, m


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8)).sum())
