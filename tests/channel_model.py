"""An independent model of the channel (include/dabgpu.h, "Channel model"), written from the definition: integer parts exact (Philox in
uint64, the oscillator in 64-bit integers, the source indices), float parts in float64 with the library log / sin / cos.  Also the
builder and ctypes face of the host model (tests/cpp/channel_host_model.cpp = dab-radio_amd/csrc/channel_core.h under g++) and the
derived error bound of DESIGN.md 4.16 that ties the two together."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
U = 2.0 ** -24                      # unit roundoff of float
DELTA_SIN = 8.8e-8                  # max |Chebyshev form - sin(2 pi x)| on [-1/2, 1/2] in exact arithmetic (checked in test_channel_model.py)
G_MAX = 5.89                        # sqrt(-2 ln 2^-25)


def philox4x32_10(key, ctr):
    """key (k0, k1), ctr (c0..c3): arrays or ints -> four uint32 arrays; the published algorithm, every product in uint64"""
    k0, k1 = (np.asarray(v, np.uint64) & np.uint64(M32) for v in key)
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) & np.uint64(M32) for v in ctr)
    m32 = np.uint64(M32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & m32, p0 & m32
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def gauss(seed, s, m):
    """(g0, g1) float64 of absolute samples m (uint64 array) of stream s"""
    m = np.asarray(m, np.uint64)
    pair = m >> np.uint64(1)
    w = philox4x32_10((seed & M32, seed >> 32), (pair & np.uint64(M32), pair >> np.uint64(32), np.full(m.shape, s, np.uint64), np.zeros(m.shape, np.uint64)))
    odd = (m & np.uint64(1)).astype(bool)
    wa, wb = np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])
    u1 = ((wa >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = ((wb >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2 * np.pi * (u2 - 0.5)), r * np.sin(2 * np.pi * (u2 - 0.5))


def osc_cycles(phase0_q64, freq_q64, m):
    """top 24 bits of phase0 + m freq (mod 2^64) as cycles in [-1/2, 1/2), per Python integer"""
    out = np.empty(len(m), np.float64)
    for i, mm in enumerate(m):
        ph = (phase0_q64 + int(mm) * freq_q64) & M64
        top = ph >> 40
        out[i] = (top - (1 << 24) if top >= (1 << 23) else top) * 2.0 ** -24
    return out


def src_index(m, start, delay, n_in, wrap):
    """Python integers: the wrapped 64-bit difference as a signed number, then modulo n_in / -1 outside"""
    i = (int(m) - int(start) - int(delay)) & M64
    if i >= 1 << 63:
        i -= 1 << 64
    if wrap:
        return i % n_in
    return i if 0 <= i < n_in else -1


def apply(P, s, x, pos, n_out, wrap):
    """stream s with parameters P (a dict, see params_dict) over x (complex, float32 values): float64 complex y[n_out] from position pos"""
    x = np.asarray(x, np.complex128)
    n_in = x.size
    m = [(pos + i) & M64 for i in range(n_out)]
    z = np.zeros(n_out, np.complex128)
    for d, hr, hi in P["taps"]:
        idx = np.array([src_index(mm, P["start"], d, n_in, wrap) for mm in m])
        xs = np.where(idx >= 0, x[np.maximum(idx, 0)], 0)
        z += complex(np.float32(hr), np.float32(hi)) * xs
    y = float(np.float32(P["gain"])) * z * np.exp(2j * np.pi * osc_cycles(P["phase0_q64"], P["freq_q64"], m))
    sigma = float(np.float32(P["noise_sigma"]))
    if sigma != 0.0:
        g0, g1 = gauss(P["seed"], s, np.array(m, np.uint64))
        y = y + sigma * (g0 + 1j * g1)
    return y


def u8_pre(y, scale):
    """the quantiser's value before clamping and truncation, per component [n, 2]"""
    s = float(np.float32(scale))
    return np.stack([y.real * s + 127.5, y.imag * s + 127.5], -1)


def u8_of(pre):
    return np.floor(np.clip(np.nan_to_num(pre, nan=0.0), 0.0, 255.0)).astype(np.uint8)


def bound(P, x_max):
    """|host model - this model| per component, from DESIGN.md 4.16: float sums, sine, logarithm"""
    n = len(P["taps"])
    S = sum(abs(complex(np.float32(hr), np.float32(hi))) for _, hr, hi in P["taps"]) * x_max
    G = abs(float(np.float32(P["gain"])))
    sigma = float(np.float32(P["noise_sigma"]))
    eps_cs = DELTA_SIN + 8.8 * U
    sig = np.sqrt(2) * G * S * (np.sqrt(2) * (2 * n + 1) * U + eps_cs + 2 * U)
    noise = sigma * G_MAX * (eps_cs + 8 * U)
    return sig + noise + U * (np.sqrt(2) * G * S + G_MAX * sigma)


def params_dict(taps=((0, 1.0, 0.0),), freq_q64=0, phase0_q64=0, start=0, seed=0, gain=1.0, noise_sigma=0.0):
    return {"taps": [tuple(t) for t in taps], "freq_q64": int(freq_q64) & M64, "phase0_q64": int(phase0_q64) & M64, "start": int(start),
            "seed": int(seed) & M64, "gain": gain, "noise_sigma": noise_sigma}


# ---- the host model: channel_core.h under g++ ----
class ChannelStream(C.Structure):
    """dabgpu_channel_stream (include/dabgpu.h)"""
    _fields_ = [("freq_q64", C.c_uint64), ("phase0_q64", C.c_uint64), ("start", C.c_int64), ("seed", C.c_uint64),
                ("gain", C.c_float), ("noise_sigma", C.c_float), ("n_taps", C.c_int32), ("tap_delay", C.c_int32 * 8),
                ("tap_re", C.c_float * 8), ("tap_im", C.c_float * 8), ("reserved", C.c_int32)]


def to_struct(P, cls=ChannelStream):
    S = cls()
    S.freq_q64, S.phase0_q64, S.start, S.seed = P["freq_q64"], P["phase0_q64"], P["start"], P["seed"]
    S.gain, S.noise_sigma, S.n_taps = P["gain"], P["noise_sigma"], len(P["taps"])
    for k, (d, hr, hi) in enumerate(P["taps"]):
        S.tap_delay[k], S.tap_re[k], S.tap_im[k] = d, hr, hi
    return S


F32, U8 = 10, 0                     # DABGPU_IQ_RAW_F32L, DABGPU_IQ_RAW_U8
_host = {}


def build_host_model(out_dir):
    """g++ -ffp-contract=off over tests/cpp/channel_host_model.cpp -> a ctypes library (built once per process)"""
    if "lib" in _host:
        return _host["lib"]
    so = os.path.join(str(out_dir), "libchannel_host_model.so")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                          "-I" + os.path.join(ROOT, "dab-radio_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "channel_host_model.cpp"), "-o", so],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    L = C.CDLL(so)
    L.chm_philox.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.chm_log_n25.argtypes, L.chm_log_n25.restype = [C.c_uint32], C.c_float
    L.chm_sin_cycles.argtypes, L.chm_sin_cycles.restype = [C.c_float], C.c_float
    L.chm_sqrt.argtypes, L.chm_sqrt.restype = [C.c_float], C.c_float
    L.chm_osc_cycles.argtypes, L.chm_osc_cycles.restype = [C.c_uint64, C.c_uint64, C.c_uint64], C.c_float
    L.chm_src_index.argtypes, L.chm_src_index.restype = [C.c_uint64, C.c_int64, C.c_int32, C.c_int64, C.c_int], C.c_int64
    L.chm_gauss.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    L.chm_apply.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int, C.c_size_t,
                            C.c_float]
    _host["lib"] = L
    return L


def host_apply(L, plist, x, pos, n_out, wrap, fmt=F32, scale=1.0, in_stride=None):
    """the host model over every stream of plist: x [n_streams][n_in] complex64 (or [n_in] shared) -> [n_streams][n_out] complex64 / [..][n_out][2] u8"""
    x = np.ascontiguousarray(x, np.complex64)
    n_in = x.shape[-1]
    stride = (0 if x.ndim == 1 else n_in) if in_stride is None else in_stride
    arr = (ChannelStream * len(plist))(*[to_struct(P) for P in plist])
    sb = 8 if fmt == F32 else 2
    out = np.zeros((len(plist), n_out * sb), np.uint8)
    L.chm_apply(arr, len(plist), x.ctypes.data, stride, n_in, int(bool(wrap)), pos & M64, n_out, out.ctypes.data, fmt, n_out * sb, np.float32(scale))
    return out.view(np.complex64) if fmt == F32 else out.reshape(len(plist), n_out, 2)
