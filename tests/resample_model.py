"""An independent model of the resampler (include/dabgpu.h, "Resampler"), written from the definition: the time T(m) in Python integers
(exact at any width), the table recomputed here in numpy float64 (np.i0 where the library sums the series), the filter sum in float64.  Also
the builder and ctypes face of the host model (tests/cpp/resample_host_model.cpp = dab-radio_amd/csrc/resample_core.h and the planner under
g++) and the derived float32 bound of DESIGN.md 4.19 that ties the two together."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, LOG2L, TAPS, BLOCK = 256, 8, 48, 1024
BETA = 9.25
ONE = 1 << 62
M64 = (1 << 64) - 1
U = 2.0 ** -24                      # unit roundoff of float
MAX_POSITION = 1 << 62
F32, U8 = 10, 0                     # DABGPU_IQ_RAW_F32L, DABGPU_IQ_RAW_U8


def params_dict(step_q62=ONE, offset_samples=0, offset_frac_q62=0, gain=1.0):
    return {"step_q62": int(step_q62), "offset_samples": int(offset_samples), "offset_frac_q62": int(offset_frac_q62), "gain": gain}


def step_q62(in_rate, out_rate, ppm=0.0):
    """the nearest Q2.62 word to in / out * (1 + ppm 1e-6), the product taken in double as the library takes it"""
    return int(round(np.ldexp(in_rate / out_rate * (1.0 + ppm * 1e-6), 62)))


# ---- the table ----
def slower_rate_factor(max_step):
    return max(float(max_step), 1.0)


def design_table(max_step, passband=0.375):
    """[(L + 1), TAPS] float32: h(t) = sinc(t / M) / M * kaiser(t) at t = p / L + TAPS / 2 - 1 - j, rows below L normalised to sum 1, row L = row 0
    advanced by one input sample"""
    M = slower_rate_factor(max_step)
    p = np.arange(L, dtype=np.float64)[:, None]
    j = np.arange(TAPS, dtype=np.float64)[None, :]
    t = p / L + (TAPS // 2 - 1) - j
    u = 2.0 * t / TAPS
    inside = np.abs(u) < 1.0
    win = np.where(inside, np.i0(BETA * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(BETA), 0.0)
    h = np.sinc(t / M) / M * win
    h /= h.sum(axis=1, keepdims=True)
    out = np.zeros((L + 1, TAPS), np.float32)
    out[:L] = h.astype(np.float32)
    out[L, 1:] = out[0, :-1]
    return out


def response(table, f, weights=(0.0, 0.5, 32767.0 / 32768.0)):
    """sum_j c_j e^(2 pi i f (j - TAPS / 2 + 1 - frac)) for every phase row and the given weights: complex [len(weights), L]"""
    H = table.astype(np.float64)
    out = np.empty((len(weights), L), np.complex128)
    for k, w in enumerate(weights):
        c = H[:L] + w * (H[1:] - H[:L])
        frac = (np.arange(L) + w) / L
        tt = np.arange(TAPS)[None, :] - (TAPS // 2 - 1) - frac[:, None]
        out[k] = (c * np.exp(2j * np.pi * f * tt)).sum(axis=1)
    return out


def design_error(table, max_step, passband=0.375, n_f=65):
    """(passband_error, alias_leakage) as dabgpu_resample_design defines them, evaluated here with plain complex exponentials"""
    M = slower_rate_factor(max_step)
    f_pass, f_alias = passband / M, (1.0 - passband) / M
    dev = max(np.abs(response(table, f) - 1.0).max() for f in np.linspace(0.0, f_pass, n_f))
    leak = max(np.abs(response(table, f)).max() for f in np.linspace(f_alias, 0.5, n_f)) if f_alias < 0.5 else 0.0
    return dev, leak


# ---- the time ----
def time_of(P, m):
    """(n, frac): floor and remainder of T(m) / 2^62 as Python integers; n is the true signed index"""
    T = (P["offset_samples"] << 62) + P["offset_frac_q62"] + int(m) * P["step_q62"]
    return T >> 62, T & (ONE - 1)


def is_identity(P):
    return P["step_q62"] == ONE and P["offset_frac_q62"] == 0


def apply(P, table, x, pos, n_out, wrap):
    """one stream over x (complex, float32 values): float64 complex y[n_out] from position pos"""
    x = np.asarray(x, np.complex128)
    n_in = x.size
    H = table.astype(np.float64)
    g = float(np.float32(P["gain"]))
    y = np.zeros(n_out, np.complex128)
    jj = np.arange(TAPS)
    for i in range(n_out):
        n, frac = time_of(P, pos + i)
        if is_identity(P):
            idx, c = np.array([n]), np.ones(1)
        else:
            p = frac >> (62 - LOG2L)
            w = ((frac >> (62 - LOG2L - 15)) & 0x7FFF) / 32768.0
            c = H[p] + w * (H[p + 1] - H[p])
            idx = n - (TAPS // 2 - 1) + jj
        if wrap:
            xs = x[np.array([int(v) % n_in for v in idx])]
        else:
            ok = np.array([0 <= int(v) < n_in for v in idx])
            xs = np.where(ok, x[np.array([min(max(int(v), 0), n_in - 1) for v in idx])], 0)
        y[i] = g * (c * xs).sum()
    return y


def row_sum_max(table):
    """S = the largest sum_j |H[p][j]|; sum_j |c_j| of any interpolated row is a convex combination of two such sums"""
    return float(np.abs(table.astype(np.float64)).sum(axis=1).max())


def accumulation_bound(table, x_max, gain=1.0):
    """|host model - this model| per component.  With u = 2^-24 and |x_re|, |x_im| <= x_max:
      coefficients  h1 - h0 rounds once (u |h1 - h0| <= u (|h0| + |h1|), times w <= 1) and the fmaf once (u |c|): sum_j |dc_j| <= 3 u S
      the chain     one product and taps - 1 fmaf, each one rounding of a partial sum bounded by S x_max: taps u S x_max to first order
      the gain      one product: u |y| <= u S x_max
    together (taps + 4) u S x_max |gain|, taken with 1 / (1 - (taps + 4) u) for the higher orders"""
    k = (TAPS + 4) * U
    return k / (1.0 - k) * row_sum_max(table) * x_max * abs(float(np.float32(gain)))


def u8_pre(y, scale):
    s = float(np.float32(scale))
    return np.stack([y.real * s + 127.5, y.imag * s + 127.5], -1)


def u8_of(pre):
    return np.floor(np.clip(np.nan_to_num(pre, nan=0.0), 0.0, 255.0)).astype(np.uint8)


# ---- the host model: resample_core.h and the planner under g++ ----
class ResampleStream(C.Structure):
    """dabgpu_resample_stream (include/dabgpu.h)"""
    _fields_ = [("step_q62", C.c_uint64), ("offset_samples", C.c_int64), ("offset_frac_q62", C.c_uint64), ("gain", C.c_float), ("reserved", C.c_int32)]


class ResampleFilter(C.Structure):
    """dabgpu_resample_filter"""
    _fields_ = [("max_step", C.c_double), ("passband_cycles", C.c_double), ("beta", C.c_double),
                ("passband_error", C.c_double), ("alias_leakage", C.c_double), ("error", C.c_double), ("table", C.c_float * ((L + 1) * TAPS))]


def to_struct(P, cls=ResampleStream):
    S = cls()
    S.step_q62, S.offset_samples, S.offset_frac_q62, S.gain = P["step_q62"], P["offset_samples"], P["offset_frac_q62"], P["gain"]
    return S


_host = {}


def build_host_model(out_dir):
    """g++ -ffp-contract=off over tests/cpp/resample_host_model.cpp + the planner -> a ctypes library (built once per process)"""
    if "lib" in _host:
        return _host["lib"]
    so = os.path.join(str(out_dir), "libresample_host_model.so")
    csrc = os.path.join(ROOT, "dab-radio_amd", "csrc")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                          "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "resample_host_model.cpp"), os.path.join(csrc, "dabgpu_host_logic.cpp"),
                          "-o", so], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    lib = C.CDLL(so)
    lib.rsm_time.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                             C.POINTER(C.c_float)]
    lib.rsm_mod.argtypes, lib.rsm_mod.restype = [C.c_uint64, C.c_int, C.c_int64], C.c_int64
    lib.rsm_rows_needed.argtypes, lib.rsm_rows_needed.restype = [C.c_void_p], C.c_uint32
    lib.rsm_apply.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int,
                              C.c_size_t, C.c_float]
    lib.dabgpu_resample_design.argtypes = [C.c_double, C.c_double, C.c_void_p]
    _host["lib"] = lib
    return lib


_designs = {}


def host_design(lib, max_step, passband=0.0):
    """dabgpu_resample_design of the host model's planner (one record per (max_step, passband), kept)"""
    key = (float(max_step), float(passband))
    if key not in _designs:
        D = ResampleFilter()
        assert lib.dabgpu_resample_design(key[0], key[1], C.byref(D)) == 0
        _designs[key] = D
    return _designs[key]


def table_of(D):
    return np.ctypeslib.as_array(D.table).reshape(L + 1, TAPS).copy()


def host_time(lib, P, m):
    S = to_struct(P)
    n, neg, frac, row, w = C.c_uint64(), C.c_int32(), C.c_uint64(), C.c_int32(), C.c_float()
    lib.rsm_time(C.byref(S), m & M64, C.byref(n), C.byref(neg), C.byref(frac), C.byref(row), C.byref(w))
    return n.value, neg.value, frac.value, row.value, w.value


def host_apply(lib, plist, D, x, pos, n_out, wrap, fmt=F32, scale=1.0, in_stride=None):
    """the host model over every stream of plist: x [n_streams][n_in] complex64 (or [n_in] shared) -> [n_streams][n_out] complex64 / [..][n_out][2] u8"""
    x = np.ascontiguousarray(x, np.complex64)
    n_in = x.shape[-1]
    stride = (0 if x.ndim == 1 else n_in) if in_stride is None else in_stride
    arr = (ResampleStream * len(plist))(*[to_struct(P) for P in plist])
    sb = 8 if fmt == F32 else 2
    out = np.zeros((len(plist), n_out * sb), np.uint8)
    lib.rsm_apply(arr, len(plist), C.byref(D, ResampleFilter.table.offset), x.ctypes.data, stride, n_in, int(bool(wrap)), pos & M64, n_out, out.ctypes.data,
                  fmt, n_out * sb, np.float32(scale))
    return out.view(np.complex64) if fmt == F32 else out.reshape(len(plist), n_out, 2)


def design_max_step(step_word):
    """the max_step to design for a stream of this step: its value rounded up to a double, at least 1"""
    v = step_word * 2.0 ** -62
    return 1.0 if v <= 1.0 else min(float(np.nextafter(v, 4.0)), 2.0)
