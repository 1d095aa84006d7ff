"""An independent model of the channeliser (include/dabgpu.h, "Channeliser"), written from the definition in numpy float64: the table
(np.i0 where the library sums the series), the oscillator from the exact 64-bit phase in Python integers (its top 24 bits, np.cos / np.sin),
split and combine as plain sums.  Also the builder and ctypes face of the host model (tests/cpp/channelise_host_model.cpp =
dab-radio_amd/csrc/channelise_core.h and the planner under g++) and the derived float32 bound of DESIGN.md 4.20 that ties the two together."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TPP, MAX_D, MAX_CH = 72, 8, 8
SPLIT_TILE, COMBINE_ROWS = 512, 128
BETA = 9.25
PASSBAND, STOPBAND = 0.375, 0.4609375
M64 = (1 << 64) - 1
U = 2.0 ** -24                      # unit roundoff of float
MAX_POSITION, MAX_START = 1 << 58, 1 << 61
F32, U8 = 10, 0                     # DABGPU_IQ_RAW_F32L, DABGPU_IQ_RAW_U8


def taps(D):
    return 1 if D == 1 else TPP * D


def peak(D):
    return 0 if D == 1 else taps(D) // 2 - 1


def channel(freq_q64=0, phase0_q64=0, gain=1.0, stream=0):
    return {"freq_q64": int(freq_q64) & M64, "phase0_q64": int(phase0_q64) & M64, "gain": gain, "stream": int(stream)}


def freq_q64(offset_hz, rate_hz):
    """the nearest Q64 word to offset / rate, two's complement"""
    return int(round(np.ldexp(offset_hz / rate_hz, 64))) & M64


# ---- the table ----
def design_table(D, passband=PASSBAND, stopband=STOPBAND):
    """[K] float32: 2 f_c / D sinc(2 f_c t / D) kaiser(2 t / K) at t = j - P, divided by its sum"""
    if D == 1:
        return np.ones(1, np.float32)
    K, fc = taps(D), 0.5 * (passband + stopband)
    t = np.arange(K, dtype=np.float64) - peak(D)
    u = 2.0 * t / K
    inside = np.abs(u) < 1.0
    win = np.where(inside, np.i0(BETA * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(BETA), 0.0)
    h = 2.0 * fc / D * np.sinc(2.0 * fc * t / D) * win
    return (h / h.sum()).astype(np.float32)


def response(table, D, f):
    """H(f) = sum_j h[j] e^(-2 pi i f (j - P)), f in cycles per wideband sample (array)"""
    t = np.arange(table.size, dtype=np.float64) - peak(D)
    return (table.astype(np.float64)[None, :] * np.exp(-2j * np.pi * np.asarray(f, np.float64)[:, None] * t[None, :])).sum(axis=1)


def design_error(table, D, passband=PASSBAND, stopband=STOPBAND):
    """(passband_error, stopband_level) as dabgpu_channeliser_design defines them, on its grid, with plain complex exponentials"""
    if D == 1:
        return 0.0, 0.0
    n_f = 16 * table.size + 1
    dev = np.abs(response(table, D, np.linspace(0.0, passband / D, n_f)) - 1.0).max()
    stop = np.abs(response(table, D, np.linspace(stopband / D, 0.5, n_f))).max()
    return float(dev), float(stop)


# ---- the oscillator ----
def osc(phase0, freq, n):
    """e^(2 pi i angle) for the absolute indices n (Python integers): the angle is the top 24 bits of (phase0 + n freq) mod 2^64, signed"""
    out = np.empty(len(n), np.complex128)
    for k, v in enumerate(n):
        ph = (phase0 + int(v) * freq) & M64
        top = ph >> 40
        top -= (1 << 24) if top >= (1 << 23) else 0
        out[k] = np.exp(2j * np.pi * top / float(1 << 24))
    return out


def fetch(x, idx, wrap):
    n_in = x.size
    if wrap:
        return x[np.array([int(v) % n_in for v in idx])]
    ok = np.array([0 <= int(v) < n_in for v in idx])
    return np.where(ok, x[np.array([min(max(int(v), 0), n_in - 1) for v in idx])], 0)


def split(ch, D, table, x, pos, start, n_out, wrap):
    """one channel over the wideband x: float64 complex y[n_out] from position pos"""
    x = np.asarray(x, np.complex128)
    H, K, P = table.astype(np.float64), taps(D), peak(D)
    g = float(np.float32(ch["gain"]))
    mixes = (ch["freq_q64"] | ch["phase0_q64"]) != 0
    y = np.zeros(n_out, np.complex128)
    for i in range(n_out):
        idx = [(pos + i) * D + start - P + j for j in range(K)]
        v = fetch(x, idx, wrap)
        if mixes:
            v = v * osc((-ch["phase0_q64"]) & M64, (-ch["freq_q64"]) & M64, idx)
        y[i] = g * (H * v).sum()
    return y


def combine(chs, D, table, xs, pos, start, n_out, wrap):
    """the channels chs (one stream) over their block rows xs: float64 complex wideband y[n_out] from position pos"""
    H, K, P = table.astype(np.float64), taps(D), peak(D)
    y = np.zeros(n_out, np.complex128)
    for ch, x in zip(chs, xs):
        x = np.asarray(x, np.complex128)
        g = float(np.float32(ch["gain"]))
        mixes = (ch["freq_q64"] | ch["phase0_q64"]) != 0
        u = np.zeros(n_out, np.complex128)
        for i in range(n_out):
            t = pos + i - start + P
            ms = [m for m in range((t - K) // D, t // D + 1) if 0 <= t - m * D < K]
            u[i] = D * (H[[t - m * D for m in ms]] * fetch(x, ms, wrap)).sum()
        term = g * u
        if mixes:
            term = term * osc(ch["phase0_q64"], ch["freq_q64"], [pos + i for i in range(n_out)])
        y += term
    return y


def tap_sum(table):
    """S = sum_j |h[j]|"""
    return float(np.abs(table.astype(np.float64)).sum())


EPS_CS = 8.8e-8 + 8.8 * U           # |(cos, sin) of ch_cos_sin - the exact pair| per component
ROT = np.sqrt(2.0) * EPS_CS + 2.0 * np.sqrt(2.0) * U     # a rotated sample against the exact rotation, relative to its modulus


def split_bound(table, x_max, gain=1.0, mixes=True):
    """|host model - this model| per component of a split output.  With u = 2^-24 and the modulus |x| <= x_max:
      rotation  the channel model's: |dv| <= ROT |x| per component (the angle is the same 24-bit number in both models), 0 when the
                rotation is skipped; it passes the filter weighted by |h|: ROT S x_max with S = sum_j |h[j]|
      chain     one product and K - 1 fmaf, each one rounding of a partial sum bounded by S x_max: K u S x_max to first order
      gain      one product: u S x_max
    together ((K + 1) u / (1 - (K + 1) u) + ROT) S x_max |gain|"""
    K, S = table.size, tap_sum(table)
    k = (K + 1) * U
    return (k / (1.0 - k) + (ROT if mixes else 0.0)) * S * x_max * abs(float(np.float32(gain)))


def combine_bound(table, D, x_max, gains, mixes=True):
    """the same for a wideband sample.  Per channel: a chain of K / D terms whose taps sum to S_rho = sum_k |h[rho + k D]| (the largest
    residue is taken), the product by D (one rounding), the gain (one), the rotation of a value of modulus <= A = D S_rho x_max |gain|:
    ((K / D + 2) u / (1 - ..) + ROT) A; then one addition per further channel, each one rounding of a partial sum bounded by the sum of
    the A"""
    H = np.abs(table.astype(np.float64))
    S = max(H[r::D].sum() for r in range(D)) * D
    k = (table.size // D + 2) * U
    amps = [S * x_max * abs(float(np.float32(g))) for g in gains]
    return sum((k / (1.0 - k) + (ROT if mixes else 0.0)) * a for a in amps) + (len(gains) - 1) * U * sum(amps)


def u8_pre(y, scale):
    s = float(np.float32(scale))
    return np.stack([y.real * s + 127.5, y.imag * s + 127.5], -1)


def u8_of(pre):
    return np.floor(np.clip(np.nan_to_num(pre, nan=0.0), 0.0, 255.0)).astype(np.uint8)


# ---- the host model: channelise_core.h and the planner under g++ ----
class Channel(C.Structure):
    """dabgpu_channeliser_channel (include/dabgpu.h)"""
    _fields_ = [("freq_q64", C.c_uint64), ("phase0_q64", C.c_uint64), ("gain", C.c_float), ("stream", C.c_uint32)]


class Filter(C.Structure):
    """dabgpu_channeliser_filter"""
    _fields_ = [("decim", C.c_int32), ("taps", C.c_int32), ("passband_cycles", C.c_double), ("stopband_cycles", C.c_double),
                ("cutoff_cycles", C.c_double), ("beta", C.c_double), ("passband_error", C.c_double), ("stopband_level", C.c_double),
                ("error", C.c_double), ("table", C.c_float * (TPP * MAX_D))]


def to_struct(ch, cls=Channel):
    S = cls()
    S.freq_q64, S.phase0_q64, S.gain, S.stream = ch["freq_q64"], ch["phase0_q64"], ch["gain"], ch["stream"]
    return S


_host = {}


def build_host_model(out_dir):
    """g++ -ffp-contract=off over tests/cpp/channelise_host_model.cpp + the planner -> a ctypes library (built once per process)"""
    if "lib" in _host:
        return _host["lib"]
    so = os.path.join(str(out_dir), "libchannelise_host_model.so")
    csrc = os.path.join(ROOT, "dab-radio_amd", "csrc")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                          "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "channelise_host_model.cpp"), os.path.join(csrc, "dabgpu_host_logic.cpp"),
                          "-o", so], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    lib = C.CDLL(so)
    lib.csm_split.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int, C.c_uint64, C.c_int64, C.c_uint64,
                              C.c_void_p, C.c_size_t]
    lib.csm_split_sample.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.c_int64, C.c_void_p]
    lib.csm_combine.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int, C.c_uint64, C.c_int64,
                                C.c_uint64, C.c_void_p, C.c_int, C.c_size_t, C.c_float]
    lib.dabgpu_channeliser_design.argtypes = [C.c_int, C.c_double, C.c_double, C.c_void_p]
    _host["lib"] = lib
    return lib


_designs = {}


def host_design(lib, D, passband=0.0, stopband=0.0):
    """dabgpu_channeliser_design of the host model's planner (one record per (D, edges), kept)"""
    key = (int(D), float(passband), float(stopband))
    if key not in _designs:
        F = Filter()
        assert lib.dabgpu_channeliser_design(key[0], key[1], key[2], C.byref(F)) == 0
        _designs[key] = F
    return _designs[key]


def table_of(F):
    return np.ctypeslib.as_array(F.table)[:F.taps].copy()


def host_split(lib, chs, F, x, pos, start, n_out, wrap, in_stride=None):
    """the host model over every channel of chs: x [n_streams][n_in] complex64 (or [n_in] shared) -> [n_channels][n_out] complex64"""
    x = np.ascontiguousarray(x, np.complex64)
    n_in = x.shape[-1]
    stride = (0 if x.ndim == 1 else n_in) if in_stride is None else in_stride
    arr = (Channel * len(chs))(*[to_struct(c) for c in chs])
    out = np.zeros((len(chs), n_out), np.complex64)
    lib.csm_split(arr, len(chs), F.decim, C.byref(F, Filter.table.offset), x.ctypes.data, stride, n_in, int(bool(wrap)), pos & M64, start, n_out,
                  out.ctypes.data, n_out * 8)
    return out


def host_split_sample(lib, ch, F, x, m, start, wrap):
    """one output through cs_split_sample, the definition's own loop (every tap rotates its sample itself)"""
    x = np.ascontiguousarray(x, np.complex64)
    out = np.zeros(1, np.complex64)
    S = to_struct(ch)
    lib.csm_split_sample(C.byref(S), F.decim, C.byref(F, Filter.table.offset), x.ctypes.data, x.size, int(bool(wrap)), m & M64, start, out.ctypes.data)
    return out[0]


def host_combine(lib, chs, n_streams, F, x, pos, start, n_out, wrap, fmt=F32, scale=1.0, in_stride=None):
    """the host model of a combine: x [n_channels][n_in] complex64 (or [n_in] shared) -> [n_streams][n_out] complex64 / [..][n_out][2] u8"""
    x = np.ascontiguousarray(x, np.complex64)
    n_in = x.shape[-1]
    stride = (0 if x.ndim == 1 else n_in) if in_stride is None else in_stride
    arr = (Channel * len(chs))(*[to_struct(c) for c in chs])
    sb = 8 if fmt == F32 else 2
    out = np.zeros((n_streams, n_out * sb), np.uint8)
    lib.csm_combine(arr, len(chs), n_streams, F.decim, C.byref(F, Filter.table.offset), x.ctypes.data, stride, n_in, int(bool(wrap)), pos & M64, start,
                    n_out, out.ctypes.data, fmt, n_out * sb, np.float32(scale))
    return out.view(np.complex64) if fmt == F32 else out.reshape(n_streams, n_out, 2)
