"""The IQ balance bank's models (include/dabgpu.h, "IQ balance"): an independent numpy model in float64, a numpy float32
restatement of the tree, the fold and the solve that is bit for bit the definition, the ctypes binding of the host model
(tests/cpp/iqbal_host_model.cpp = dab-radio_amd/csrc/iqbal_core.h under g++), and the two-block test signal.

THE FRONT END.  y = K1 x + K2 conj(x) + c0 with K1 = (1 + g e^{-j phi}) / 2, K2 = (1 - g e^{j phi}) / 2.  For a proper x (E[x^2] = 0, which
a sum of OFDM blocks plus noise is) of power s: E[y] = c0, E|y - c0|^2 = (|K1|^2 + |K2|^2) s, E[(y - c0)^2] = 2 K1 K2 s, so
C = E[(y - c0)^2] / E|y - c0|^2 = 2 w / (1 + |w|^2) with w = K2 / conj(K1), whose root inside the unit circle is w = C / (1 + sqrt(1 - |C|^2)).
z = (y - c0) - w conj(y - c0) = K1 (1 - |w|^2) x: the image is gone, a complex gain stays.

THE FLOAT32 BOUNDS (u = 2^-24, inputs are float32 in both models).
  map      a component is four fmaf from c, each one rounding of a partial sum no larger than M = |c| + (|a_re| + |a_im| + |b_re| + |b_im|)
           max(|re|, |im|): |error| <= 4 u M (1 + 4 u).
  moments  the terms re, im are exact; |y|^2, re^2 - im^2 carry two roundings, 2 re im one, all bounded by u-multiples of re^2 + im^2.  The
           tree adds ten levels: |error of a tile sum| <= gamma(12) sum|term|, gamma(k) = k u / (1 - k u), sum|term| <= sum|re|, sum|im| or
           sum|y|^2.
  fold     T tiles with forget = 1 add T more roundings of the running sums: gamma(T + 12) A in all, A = sum|y|^2 over the whole input.
  solve    with e = gamma(T + 14) and A / N = P + |d|^2: |delta d| <= e sqrt(A / N), |delta P|, |delta Q| <= 3 e A / N, so
           |delta C| <= 6 e A / (N P) (1 + O(e)) and, w being (C / 2)(1 + |w|^2), |delta w| <= 3.2 e A / (N P) for |C| <= 0.2; the solve's own
           two dozen roundings add at most 32 u.  margin_w(T, A, N, P) below is that sum.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024
OFF, FIXED, TRACK = 0, 1, 2
MEASURE, APPLY = 1, 2
FMT_U8, FMT_F32 = 0, 10                                                       # DABGPU_IQ_RAW_U8, DABGPU_IQ_RAW_F32L
TREE_BITS = (0, 9, 1, 2, 3, 4, 5, 6, 7, 8)
U = 2.0 ** -24
DEFAULTS = dict(mode=TRACK, a=1 + 0j, b=0j, c=0j, forget=float(np.float32(np.exp(-1024.0 / (16 * 196608)))), min_weight=65536.0)
F32 = np.float32


def params(**kw):
    P = dict(DEFAULTS)
    P.update(kw)
    return P


def gamma(k):
    return k * U / (1.0 - k * U)


def margin_w(T, A, N, P):
    return 3.2 * gamma(T + 14) * A / (N * P) + 32 * U


# ---- the front end and the float64 model ----
def front_end(gain_db, phase_deg):
    """(K1, K2) in float64"""
    g, phi = 10.0 ** (gain_db / 20.0), np.deg2rad(phase_deg)
    return (1 + g * np.exp(-1j * phi)) / 2, (1 - g * np.exp(1j * phi)) / 2


def impair(x, gain_db, phase_deg, dc=0j):
    K1, K2 = front_end(gain_db, phase_deg)
    return K1 * x + K2 * np.conj(x) + dc


def irr_db(K1, K2):
    return 20 * np.log10(abs(K1) / max(abs(K2), 1e-300))


def residual(K1, K2, w):
    """(K1', K2') of z = y - w conj(y)"""
    return K1 - w * np.conj(K2), K2 - w * np.conj(K1)


def map64(a, b, c, y):
    y = np.asarray(y, np.complex128)
    return a * y + b * np.conj(y) + c


def moments64(y):
    """[tiles][5] float64: plain sums"""
    y = np.asarray(y, np.complex128).reshape(-1, TILE)
    return np.stack([y.real.sum(1), y.imag.sum(1), (abs(y) ** 2).sum(1), (y.real ** 2 - y.imag ** 2).sum(1), (2 * y.real * y.imag).sum(1)], axis=1)


def fold64(m, forget=1.0, N=0.0, S=None):
    S = np.zeros(5) if S is None else np.array(S, np.float64)
    for row in np.asarray(m, np.float64):
        if not np.all(np.isfinite(row)):
            continue
        N = forget * N + TILE
        S = forget * S + row
    return N, S


def solve64(N, S, min_weight=0.0):
    """dict(d, P, C, w, a, b, c, valid): the closed form w = C / (1 + sqrt(1 - |C|^2))"""
    ident = dict(d=0j, P=0.0, C=0j, w=0j, a=1 + 0j, b=0j, c=0j, valid=0)
    if not N >= max(min_weight, 1e-300):
        return ident
    d = complex(S[0], S[1]) / N
    P = S[2] / N - abs(d) ** 2
    if not (P > 0 and np.isfinite(P)):
        return dict(ident, d=d, P=P)
    Cq = (complex(S[3], S[4]) / N - d * d) / P
    if not abs(Cq) < 1:
        return dict(ident, d=d, P=P, C=Cq)
    w = Cq / (1 + np.sqrt(1 - abs(Cq) ** 2))
    return dict(d=d, P=P, C=Cq, w=w, a=1 + 0j, b=-w, c=-(d - w * np.conj(d)), valid=1)


# ---- the float32 restatement: every operation one float32 rounding, fmaf exact ----
def fma32(a, b, c):
    """fmaf(a, b, c) for float32 a, b, c, correctly rounded: the product is exact in float64, the sum is rounded to odd there (TwoSum), and
    53 >= 2 * 24 + 2 bits make the second rounding to float32 the correct one"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fin = np.isfinite(s) & np.isfinite(err) & (err != 0)
        bits = np.atleast_1d(s).view(np.uint64).copy()
        toward_zero = fin & (np.signbit(err) != np.signbit(s))
        bits = np.where(np.atleast_1d(toward_zero), bits - np.uint64(1), bits)
        bits = np.where(np.atleast_1d(fin), bits | np.uint64(1), bits)
        r = bits.view(np.float64).astype(np.float32)
    return r.reshape(np.shape(s)) if np.ndim(s) else r[0]


def terms32(y):
    """[5][n] float32 terms of float32 samples"""
    y = np.asarray(y, np.complex64)
    re, im = y.real.astype(F32), y.imag.astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        rr = re * re
        return np.stack([re, im, fma32(im, im, rr), fma32(-im, im, rr), (F32(2) * re) * im])


def tree32(v):
    """[..., 1024] float32 -> [...]: the ten levels in TREE_BITS order"""
    v = np.asarray(v, F32)
    idx = np.arange(TILE)
    done = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for bit in TREE_BITS:
            keep = idx[(idx & (done | (1 << bit))) == 0]
            out = v.copy()
            out[..., keep] = v[..., keep] + v[..., keep | (1 << bit)]
            v = out
            done |= 1 << bit
    return v[..., 0]


def moments32(y):
    """[tiles][5] float32, bit for bit the definition"""
    t = terms32(y).reshape(5, -1, TILE)
    return tree32(t).T.copy()


def reciprocal32(x):
    """dv_reciprocal (diversity_core.h) restated"""
    x = F32(x)
    if not x >= F32(1.17549435e-38):
        return F32(np.inf)
    b = int(np.array(x, F32).view(np.uint32))
    e = (b >> 23) - 127
    m = np.array((b & 0x007FFFFF) | 0x3F800000, np.uint32).view(F32)[()]
    r = fma32(F32(-0.470588235), m, F32(1.41176471))
    for _ in range(3):
        r = fma32(r, fma32(-m, r, F32(1)), r)
    q = fma32(fma32(-m, r, F32(1)), r, r)
    a = int(e / 2)                                                            # C division truncates toward zero
    p2 = lambda k: np.array((127 - k) << 23, np.uint32).view(F32)[()]
    with np.errstate(over="ignore", under="ignore"):
        return F32(F32(q * p2(a)) * p2(e - a))


def fold32(m, forget, N=0.0, S=None):
    """-> (N, S[5], used, skipped) in float32"""
    N, lam = F32(N), F32(forget)
    S = np.zeros(5, F32) if S is None else np.array(S, F32)
    used = skipped = 0
    for row in np.asarray(m, F32):
        if not np.all(np.isfinite(row)):
            skipped += 1
            continue
        N = fma32(lam, N, F32(TILE))
        S = fma32(lam, S, row)
        used += 1
    return N, S, used, skipped


def solve32(N, S, min_weight):
    """the record's solved fields as float32 scalars: dict(d_re, d_im, P, C_re, C_im, w_re, w_im, a_re .. c_im, valid)"""
    z = F32(0)
    R = dict(d_re=z, d_im=z, P=z, C_re=z, C_im=z, w_re=z, w_im=z, a_re=F32(1), a_im=z, b_re=z, b_im=z, c_re=z, c_im=z, valid=0)
    N, S = F32(N), np.asarray(S, F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if not (N >= F32(min_weight)) or not (N >= F32(1.17549435e-38)):
            return R
        r = reciprocal32(N)
        dr, di = F32(S[0] * r), F32(S[1] * r)
        R["d_re"], R["d_im"] = dr, di
        P = fma32(-di, di, fma32(-dr, dr, F32(S[2] * r)))
        R["P"] = P
        if not (P >= F32(1.17549435e-38) and P <= F32(3.40282347e+38)):
            return R
        qr = fma32(di, di, fma32(-dr, dr, F32(S[3] * r)))
        qi = fma32(F32(F32(-2) * dr), di, F32(S[4] * r))
        ip = reciprocal32(P)
        cr, ci = F32(qr * ip), F32(qi * ip)
        R["C_re"], R["C_im"] = cr, ci
        if not fma32(ci, ci, F32(cr * cr)) < F32(1):
            return R
        hr, hi = F32(F32(0.5) * cr), F32(F32(0.5) * ci)
        wr, wi = hr, hi
        for _ in range(3):
            t = fma32(wi, wi, fma32(wr, wr, F32(1)))
            wr, wi = F32(hr * t), F32(hi * t)
        R["w_re"], R["w_im"] = wr, wi
        ur, ui = fma32(wi, di, F32(wr * dr)), fma32(-wr, di, F32(wi * dr))
        R["b_re"], R["b_im"] = F32(-wr), F32(-wi)
        R["c_re"], R["c_im"] = F32(ur - dr), F32(ui - di)
        R["valid"] = 1
    return R


# ---- the test signal: two QPSK-OFDM blocks at +-856 kHz in an 8.192 MS/s stream, plus noise ----
D, NFFT, NCP, CARRIERS, OFFSET_BINS = 4, 2048 * 4, 504 * 4, 1536, 856
FRAME = 196608 * D                                                            # a mode-I frame at 8.192 MS/s: 768 tiles


def two_blocks(n_frames, neighbour_db, seed, snr_db=20.0):
    """complex128 [n_frames * FRAME]: the wanted block of unit power at +856 kHz, its neighbour at -856 kHz neighbour_db above it, white noise
    snr_db below the wanted block (in the whole 8.192 MHz)"""
    rng = np.random.default_rng(seed)
    n = n_frames * FRAME
    sym = NFFT + NCP
    n_sym = -(-n // sym)
    out = np.zeros(n_sym * sym, np.complex128)
    k = np.concatenate([np.arange(-CARRIERS // 2, 0), np.arange(1, CARRIERS // 2 + 1)])
    for centre, level_db in ((OFFSET_BINS, 0.0), (-OFFSET_BINS, neighbour_db)):
        X = np.zeros((n_sym, NFFT), np.complex128)
        q = (rng.integers(0, 2, (n_sym, CARRIERS)) * 2 - 1 + 1j * (rng.integers(0, 2, (n_sym, CARRIERS)) * 2 - 1)) / np.sqrt(2.0)
        X[:, (k + centre) % NFFT] = q
        t = np.fft.ifft(X, axis=1) * (NFFT / np.sqrt(CARRIERS)) * 10.0 ** (level_db / 20.0)
        out += np.concatenate([t[:, -NCP:], t], axis=1).reshape(-1)
    out = out[:n]
    sigma = 10.0 ** (-snr_db / 20.0)
    return out + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)


# ---- the host model: iqbal_core.h under g++ ----
class Stream(C.Structure):
    """dabgpu_iqbal_stream (include/dabgpu.h)"""
    _fields_ = [("mode", C.c_int32), ("reserved", C.c_int32), ("a_re", C.c_float), ("a_im", C.c_float), ("b_re", C.c_float), ("b_im", C.c_float),
                ("c_re", C.c_float), ("c_im", C.c_float), ("forget", C.c_float), ("min_weight", C.c_float)]


RECORD_DTYPE = np.dtype([("N", "<f4"), ("S", "<f4", (5,)), ("d_re", "<f4"), ("d_im", "<f4"), ("P", "<f4"), ("C_re", "<f4"), ("C_im", "<f4"),
                         ("w_re", "<f4"), ("w_im", "<f4"), ("a_re", "<f4"), ("a_im", "<f4"), ("b_re", "<f4"), ("b_im", "<f4"), ("c_re", "<f4"),
                         ("c_im", "<f4"), ("valid", "<u4"), ("tiles_used", "<u8"), ("tiles_skipped", "<u8"), ("calls_refused", "<u4"),
                         ("reserved", "<u4")])
SOLVED = ("d_re", "d_im", "P", "C_re", "C_im", "w_re", "w_im", "a_re", "a_im", "b_re", "b_im", "c_re", "c_im")


def to_struct(P, cls=Stream):
    T = cls()
    T.mode, T.forget, T.min_weight = P["mode"], P["forget"], P["min_weight"]
    for name in "abc":
        setattr(T, name + "_re", complex(P[name]).real)
        setattr(T, name + "_im", complex(P[name]).imag)
    return T


_host = {}


def build_host_model(out_dir):
    """g++ -ffp-contract=off over tests/cpp/iqbal_host_model.cpp -> a ctypes library (built once per process)"""
    if "lib" in _host:
        return _host["lib"]
    so = os.path.join(str(out_dir), "libiqbal_host_model.so")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                          "-I" + os.path.join(ROOT, "dab-radio_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "iqbal_host_model.cpp"), "-o", so],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    L = C.CDLL(so)
    L.iqm_map.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.iqm_moments.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.iqm_fold_and_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.iqm_reset.argtypes = [C.c_void_p, C.c_size_t]
    L.iqm_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int, C.c_size_t,
                            C.c_float, C.c_uint32, C.c_void_p]
    L.iqm_apply.restype = C.c_uint64
    _host["lib"] = L
    return L


def host_map(L, a, b, c, y):
    k = np.array([a.real, a.imag, b.real, b.imag, c.real, c.imag], F32)
    y = np.ascontiguousarray(y, np.complex64)
    out = np.zeros_like(y)
    L.iqm_map(k.ctypes.data, y.ctypes.data, y.size, out.ctypes.data)
    return out


def host_moments(L, y):
    y = np.ascontiguousarray(y, np.complex64)
    out = np.zeros((y.size // TILE, 5), F32)
    L.iqm_moments(y.ctypes.data, out.shape[0], out.ctypes.data)
    return out


def host_records(L, n):
    rec = np.zeros(n, RECORD_DTYPE)
    L.iqm_reset(rec.ctypes.data, n)
    return rec


def host_fold_and_solve(L, P, rec, m):
    """rec: a one-element RECORD_DTYPE array, updated in place"""
    m = np.ascontiguousarray(m, F32).reshape(-1, 5)
    L.iqm_fold_and_solve(C.byref(to_struct(P)), rec.ctypes.data, m.ctypes.data, m.shape[0])
    return rec


def host_apply(L, plist, rec, x, pos, n, flags, u8=False, scale=1.0):
    """the host model over every stream of plist on the records rec (updated in place): x [n_streams][>= n] complex64 or [>= n] shared ->
    (y [n_streams][n] complex64 or [n_streams][n][2] uint8 or None, moments [n_streams][n // 1024][5] or None, samples advanced)"""
    x = np.ascontiguousarray(x, np.complex64)
    arr = (Stream * len(plist))(*[to_struct(P) for P in plist])
    y = np.zeros((len(plist), n, 2), np.uint8) if u8 else np.zeros((len(plist), n), np.complex64)
    m = np.zeros((len(plist), n // TILE, 5), F32)
    adv = L.iqm_apply(arr, rec.ctypes.data, len(plist), x.ctypes.data, x.shape[-1] if x.ndim == 2 else 0, int(pos), int(n), y.ctypes.data,
                      FMT_U8 if u8 else FMT_F32, n * (2 if u8 else 8), float(scale), int(flags), m.ctypes.data)
    return (y if flags & APPLY else None), (m if flags & MEASURE and adv else None), int(adv)
