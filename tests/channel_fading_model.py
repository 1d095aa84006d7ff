"""An independent model of the fading taps (include/dabgpu.h, "Channel model, fading taps"), written from the definition: the planner's
Philox words and oscillator phases in integers, the gains in float64 with the library cos / sin and this file's own interpolation.  Also the
builder and ctypes face of the host model (tests/cpp/channel_fading_host_model.cpp = dab-radio_amd/csrc/channel_core.h under g++) and the
derived error bounds of DESIGN.md 4.18 that tie the two together.  The static part is tests/channel_model.py's, imported."""
import ctypes as C
import os
import subprocess

import numpy as np

import channel_model as CM

ROOT = CM.ROOT
U = CM.U
EPS_CS = CM.DELTA_SIN + 8.8 * U       # one ch_cos_sin component against cos / sin of the same 24-bit angle
STATIC, FADING = 0, 1
N_OSC, GRID = 17, 64
MAX_DOPPLER = 2.0 ** -11


# ---- the planner, from the header's text ----
def freq_q64(cycles):
    """round(cycles 2^64) mod 2^64 in Python integers (cycles: a float64, |cycles| <= 0.5)"""
    num, den = float(cycles).as_integer_ratio()
    v = num * (1 << 64)
    q, r = divmod(v, den)                                      # floor; den is a power of two, so the half is exact
    if 2 * r > den or (2 * r == den and (q & 1)):
        q += 1
    return q & CM.M64


def plan_tap(doppler_cycles, seed, s, k, rice_k=0.0, los_cos=0.0):
    """one fading tap of stream s: {"freq": [17], "phase": [17], "amp_diffuse", "amp_los"} (amplitudes as the float32 values)"""
    freq, phase = [], []
    for n in range(N_OSC):
        w = [int(v) for v in CM.philox4x32_10((seed & CM.M32, seed >> 32), (n, k, s, 1))]
        c = np.cos(2 * np.pi * (n + (w[0] + 0.5) * 2.0 ** -32) / 16) if n < 16 else float(np.float32(los_cos))
        freq.append(freq_q64(doppler_cycles * c))
        phase.append((w[2] << 32) | w[3])
    K = float(np.float32(rice_k))
    return {"freq": freq, "phase": phase, "amp_diffuse": float(np.float32(np.float32(np.sqrt(1 / (K + 1))) * np.float32(0.25))),
            "amp_los": float(np.float32(np.sqrt(K / (K + 1))))}


def plan_stream(P, doppler_cycles, seed, s, kinds, rice_k=None, los_cos=None):
    """the table of stream s as a list per tap of P["taps"]: None (static) or plan_tap's dict"""
    n = len(P["taps"])
    rice_k = rice_k or [0.0] * n
    los_cos = los_cos or [0.0] * n
    return [plan_tap(doppler_cycles, seed, s, k, rice_k[k], los_cos[k]) if kinds[k] == FADING else None for k in range(n)]


# ---- the gains ----
def osc_angles(T, m):
    """[17][len(m)] angles in cycles: the top 24 bits of phase + m freq (mod 2^64, numpy's uint64 products wrap), in [-1/2, 1/2)"""
    m = np.asarray(m, np.uint64)
    out = np.empty((N_OSC, m.size), np.float64)
    with np.errstate(over="ignore"):
        for n in range(N_OSC):
            ph = np.uint64(T["phase"][n]) + m * np.uint64(T["freq"][n])
            out[n] = (ph >> np.uint64(40)).astype(np.int64).astype(np.float64)
    out[out >= 2.0 ** 23] -= 2.0 ** 24
    return out * 2.0 ** -24


def phasor_sum(T, m):
    """amp_diffuse sum_{n < 16} e^(j angle_n(m)) + amp_los e^(j angle_16(m)), float64 complex, no grid"""
    e = np.exp(2j * np.pi * osc_angles(T, m))
    return T["amp_diffuse"] * e[:16].sum(0) + T["amp_los"] * e[16]


def gain(T, m):
    """g(m), the definition: the phasor sums at the grid points 64 j and 64 (j + 1), a straight line between them"""
    m = np.asarray(m, np.uint64)
    j = m >> np.uint64(6)
    js = np.unique(np.concatenate([j, j + np.uint64(1)]))
    G = phasor_sum(T, js << np.uint64(6))
    i0 = np.searchsorted(js, j)
    g0, g1 = G[i0], G[np.searchsorted(js, j + np.uint64(1))]
    w = (m & np.uint64(63)).astype(np.float64) / 64.0
    return g0 + w * (g1 - g0)


def apply(P, table, s, x, pos, n_out, wrap):
    """stream s with parameters P and fading table (plan_stream) over x: float64 complex y[n_out] from position pos.  The statements of
    channel_model.apply with the tap replaced by h g(m) where the tap fades: an all-static table gives its result exactly."""
    x = np.asarray(x, np.complex128)
    n_in = x.size
    m = [(pos + i) & CM.M64 for i in range(n_out)]
    z = np.zeros(n_out, np.complex128)
    for (d, hr, hi), T in zip(P["taps"], table):
        idx = np.array([CM.src_index(mm, P["start"], d, n_in, wrap) for mm in m])
        xs = np.where(idx >= 0, x[np.maximum(idx, 0)], 0)
        h = complex(np.float32(hr), np.float32(hi))
        z += (h if T is None else h * gain(T, np.array(m, np.uint64))) * xs
    y = float(np.float32(P["gain"])) * z * np.exp(2j * np.pi * CM.osc_cycles(P["phase0_q64"], P["freq_q64"], m))
    sigma = float(np.float32(P["noise_sigma"]))
    if sigma != 0.0:
        g0, g1 = CM.gauss(P["seed"], s, np.array(m, np.uint64))
        y = y + sigma * (g0 + 1j * g1)
    return y


# ---- the derived bounds ----
def amp_max(T):
    """A = 16 amp_diffuse + amp_los >= |g| and >= each component of g"""
    return 16 * T["amp_diffuse"] + T["amp_los"]


def gain_bound(T):
    """|host g - model g| per component: 17 cos / sin errors, the tree (depth 4, partial sums up to 16), the two roundings of the
    combination, the three of the interpolation (the difference, at most 2 A; the fmaf, at most A)"""
    A = amp_max(T)
    grid = T["amp_diffuse"] * (16 * EPS_CS + 4 * U * 16) + T["amp_los"] * EPS_CS + 2 * U * A
    return grid + 3 * U * A


def bound(P, table, x_max):
    """|host model - this model| per component: DESIGN.md 4.16's B with |h_k| A_k for a fading tap, plus what the error of the effective
    tap (the gain's, and the product's two roundings) carries through the sum: 2 G x_max sum E_e"""
    n = len(P["taps"])
    S, extra = 0.0, 0.0
    for (_, hr, hi), T in zip(P["taps"], table):
        h = abs(complex(np.float32(hr), np.float32(hi)))
        S += h * (1.0 if T is None else amp_max(T))
        if T is not None:
            extra += np.sqrt(2) * h * (gain_bound(T) + 2 * U * amp_max(T))
    S *= x_max
    G = abs(float(np.float32(P["gain"])))
    sigma = float(np.float32(P["noise_sigma"]))
    sig = np.sqrt(2) * G * S * (np.sqrt(2) * (2 * n + 1) * U + EPS_CS + 2 * U)
    noise = sigma * CM.G_MAX * (EPS_CS + 8 * U)
    return sig + noise + U * (np.sqrt(2) * G * S + CM.G_MAX * sigma) + 2 * G * x_max * extra


def bessel_j0(x):
    """J0(x) = (1 / pi) int_0^pi cos(x cos t) dt by the midpoint rule (periodic integrand: converges geometrically)"""
    t = (np.arange(4096) + 0.5) * np.pi / 4096
    return np.cos(np.multiply.outer(np.asarray(x, np.float64), np.cos(t))).mean(-1)


# ---- the host model: channel_core.h under g++ ----
class FadingTap(C.Structure):
    """dabgpu_channel_fading_tap (include/dabgpu.h)"""
    _fields_ = [("freq_q64", C.c_uint64 * N_OSC), ("phase_q64", C.c_uint64 * N_OSC), ("amp_diffuse", C.c_float), ("amp_los", C.c_float)]


class FadingStream(C.Structure):
    """dabgpu_channel_fading_stream"""
    _fields_ = [("kind", C.c_int32 * 8), ("tap", FadingTap * 8)]


class FadingSpec(C.Structure):
    """dabgpu_channel_fading_spec"""
    _fields_ = [("doppler_cycles", C.c_double), ("seed", C.c_uint64), ("kind", C.c_int32 * 8), ("rice_k", C.c_float * 8), ("los_cos", C.c_float * 8)]


def to_struct(table, cls=FadingStream):
    F = cls()
    for k, T in enumerate(table):
        if T is None:
            continue
        F.kind[k] = FADING
        for n in range(N_OSC):
            F.tap[k].freq_q64[n], F.tap[k].phase_q64[n] = T["freq"][n], T["phase"][n]
        F.tap[k].amp_diffuse, F.tap[k].amp_los = T["amp_diffuse"], T["amp_los"]
    return F


def from_struct(F, n_taps):
    return [None if F.kind[k] != FADING else {"freq": list(F.tap[k].freq_q64), "phase": list(F.tap[k].phase_q64),
                                              "amp_diffuse": float(F.tap[k].amp_diffuse), "amp_los": float(F.tap[k].amp_los)} for k in range(n_taps)]


_host = {}


def build_host_model(out_dir):
    """g++ -ffp-contract=off over tests/cpp/channel_fading_host_model.cpp -> a ctypes library (built once per process)"""
    if "lib" in _host:
        return _host["lib"]
    so = os.path.join(str(out_dir), "libchannel_fading_host_model.so")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                          "-I" + os.path.join(ROOT, "dab-radio_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "channel_fading_host_model.cpp"), "-o", so],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    L = C.CDLL(so)
    L.chfm_grid_gain.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    L.chfm_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int,
                             C.c_size_t, C.c_float]
    _host["lib"] = L
    return L


def host_apply(L, plist, tables, x, pos, n_out, wrap, fmt=CM.F32, scale=1.0, in_stride=None):
    """the host model over every stream: plist dicts, tables = plan_stream lists or a ctypes array of dabgpu_channel_fading_stream; x as in
    channel_model.host_apply -> [n_streams][n_out] complex64 / [..][n_out][2] u8"""
    x = np.ascontiguousarray(x, np.complex64)
    n_in = x.shape[-1]
    stride = (0 if x.ndim == 1 else n_in) if in_stride is None else in_stride
    arr = (CM.ChannelStream * len(plist))(*[CM.to_struct(P) for P in plist])
    tab = tables if isinstance(tables, C.Array) else (FadingStream * len(plist))(*[to_struct(t) for t in tables])
    sb = 8 if fmt == CM.F32 else 2
    out = np.zeros((len(plist), n_out * sb), np.uint8)
    L.chfm_apply(arr, tab, len(plist), x.ctypes.data, stride, n_in, int(bool(wrap)), pos & CM.M64, n_out, out.ctypes.data, fmt, n_out * sb, np.float32(scale))
    return out.view(np.complex64) if fmt == CM.F32 else out.reshape(len(plist), n_out, 2)
