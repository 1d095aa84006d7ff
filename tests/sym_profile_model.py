"""The symbol noise profile of mode I, written from the definition in include/dabgpu.h ("Symbol noise profile") and not from the library's
code: a numpy float32 model in which every operation is one IEEE float32 operation (softbit_model.fma32 is the exact fused multiply-add,
numpy's float32 square root is correctly rounded, the reciprocal is tests/diversity_model.py's), a float64 model with true roots and
quotients and the bound the float32 one must keep to it, a float64 Monte Carlo of one product row, and the float32 host model
(csrc/sym_profile_core.h compiled by g++), which the device is compared with bit for bit.

Float32 against float64, from the same float32 products, u = 2^-24, no overflow and no result below the normal range.  Every sum is one
of non-negative terms, so relative errors carry through it.  An owner chains six terms from +0 (the first addition exact: five
roundings), the tree adds six levels, the join two: 13 roundings behind the terms.  A term of S1 rounds once: S1 within (1 + u)^14.  A
term of SD is a difference, its square: (1 + u)^3 on the term (the difference of two floats within a factor 2 of each other is exact,
otherwise it rounds once; the square doubles that and rounds): SD within (1 + u)^16.  A term of S2 is a product and a fused step of
non-negative parts: (1 + u)^2, S2 within (1 + u)^15.
  R   = sqrt(S2 k1536): k1536 within u of 1 / 1536, the product rounds, the root halves and rounds: (1 + u)^(17 / 2 + 1) - 1 < 10 u.
  P   = S1 r2: r2 within u of 1 / sqrt 2, one rounding: (1 + u)^16.  P^2 rounds once: (1 + u)^33.  The discriminant
        fma(1536, SD, P^2) is a sum of non-negative parts and rounds once: (1 + u)^34.  Its root: (1 + u)^18 - 1 < 19 u.
  qa  = (root - P) k1536.  THE CANCELLATION: at carrier SNR g the root is 1536 (a + q) and P is 1536 a, so the difference is the
        fraction 1 / (1 + g) of either, and the operands' errors are absolute, not relative to it:
        |qa32 - qa64| <= (19 u root + 16 u P + 3 u |root - P|) / 1536  (the difference, k1536 and the product round once each);
        clamping both sides at 0 does not increase a difference.  At 30 dB this is about 35 u * 1000 = 2e-3 of qa, at 12 dB 3e-5.
  med:  the k-th smallest of values that each moved by at most e moves by at most e, so a median carries the largest row bound.
  q   = max(qa, med(qa) + (R - med(R))): |q32 - q64| <= max(bound_qa) + (10 u (R + med R) + 2 u (|R - med R| + |lifted|)).
  v   = q_ref / q (q above q_ref): the reciprocal is within 1 ulp (2 u) of the true one, the product rounds:
        |v32 - v64| <= v64 (e(q_ref) / q_ref + e(q) / q + 4 u) to first order; rows at or below q_ref have v = 1 on both sides unless
        the comparison itself falls inside the two bounds, and then v64 is within that same distance of 1.

Statistics.  With X_i = sqrt(a) s_i + n_i, n_i complex Gaussian of power q, the product rotated by its own phase step is
a + sqrt(a) (conj(u_i+1) + u_i) + u_i conj(u_i+1): across the decision diagonal it has variance a q + q^2 / 2, and along it mean a.
Over the 1536 carriers of one row SD / 2 = sum (a_c q + q^2 / 2) chi^2_1: to first order qa = SD / (2 P) has relative variance
2 sum a_c^2 / (sum a_c)^2 = (2 / 1536) E[a^2] / E[a]^2 -- 0.036 for a flat channel, 0.041 for the two-path ripple with a second path at
half the amplitude.  Where decisions fail the folding into the first quadrant hides noise and qa under-reads, monotonely.
The power term has a jitter of its own, and it is the larger one at high SNR: |X|^2 has relative variance x = q (2 a + q) / (a + q)^2, a
product's |d|^2 has (1 + x)^2 - 1, the row's mean of 1536 of them that over 1536, and the root halves the relative deviation:
dev(R) = (a + q) sqrt(((1 + x)^2 - 1) / 1536) / 2 -- relative to q: 0.07 at 8 dB carrier SNR, 0.11 at 12 dB, 0.15 at 15 dB, 0.8 at 30 dB
(clean_row_floor below: what a clean row's weight stays above, five deviations of both terms out)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import diversity_model as DM
import softbit_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dab-radio_amd", "csrc")
F32 = np.float32
N_SYMBOLS, N_CARRIERS, OWNERS, MEDIAN_RANK = 75, 1536, 256, 37
U = 2.0 ** -24
K1536 = F32(1.0) / F32(1536.0)                         # float32 division is correctly rounded
RSQRT2 = F32(math.sqrt(0.5))                           # sqrt(1/2) in float64 lies far from a float32 tie: the nearest float
WEIGHT_CAP = F32(2.0 ** -20)
FLT_MAX, FLT_MIN = SM.FLT_MAX, SM.FLT_MIN
BOUND_R, BOUND_ROOT, BOUND_P = 10 * U, 19 * U, 16 * U
SECOND_PATH = 0.5                                      # the Monte Carlo's ripple: a second path at half the amplitude
FIRST_ORDER_DEVIATION = math.sqrt(2.0 / N_CARRIERS)


def power_term_deviation(snr_db, second=SECOND_PATH):
    """dev(R) / q of the head at mean carrier SNR snr_db (the ripple raises E[(a + q)^2 x'] over the flat channel's by at most
    E[a^2] / E[a]^2 = 1 + 2 s^2 / (1 + s^2)^2, taken in full)"""
    g = 10.0 ** (snr_db / 10.0)
    x = (2.0 * g + 1.0) / (g + 1.0) ** 2
    return (g + 1.0) * math.sqrt(((1.0 + x) ** 2 - 1.0) / N_CARRIERS * (1.0 + 2.0 * second ** 2 / (1.0 + second ** 2) ** 2)) / 2.0


def clean_row_floor(snr_db):
    """what the weight of a row without a burst stays above: its q five deviations of the power term and of qa above the reference"""
    return 1.0 / (1.0 + 5.0 * (power_term_deviation(snr_db) + FIRST_ORDER_DEVIATION * 1.15))


def owner_order():
    """[256][6]: the carriers owner t chains, in order"""
    t = np.arange(OWNERS)
    return np.stack([2 * (t + OWNERS * j) + h for j in range(3) for h in range(2)], axis=1)


def _tree64(a):
    """the wavefront tree over the last axis of 64: a[i] + a[i + h] for i < h, h = 32 .. 1"""
    a = a.astype(F32)
    h = 32
    while h >= 1:
        a = (a[..., :h] + a[..., h:2 * h]).astype(F32)
        h //= 2
    return a[..., 0]


def _row_sum(terms):
    """terms [75][1536] float32 -> [75]: owners' chains, four trees, the join"""
    x = terms[:, owner_order()]                                                        # [75][256][6]
    s = x[..., 0].astype(F32)                                                          # 0 + x is x (no term is -0)
    for i in range(1, 6):
        s = (s + x[..., i]).astype(F32)
    p = _tree64(s.reshape(N_SYMBOLS, 4, 64))                                           # [75][4]
    return ((p[:, 0] + p[:, 1]).astype(F32) + (p[:, 2] + p[:, 3]).astype(F32)).astype(F32)


def sums(dq):
    """step 1 of one frame in float32: dq [75][1536] complex64 -> (S1, SD, S2) [75]"""
    d = np.asarray(dq, np.complex64).reshape(N_SYMBOLS, N_CARRIERS)
    with np.errstate(all="ignore"):
        ar, ai = np.abs(d.real).astype(F32), np.abs(d.imag).astype(F32)
        diff = (ar - ai).astype(F32)
        return (_row_sum((ar + ai).astype(F32)), _row_sum((diff * diff).astype(F32)),
                _row_sum(SM.fma32(d.real, d.real, (d.imag * d.imag).astype(F32))))


def figures(S1, SD, S2):
    """steps 2 and 3a in float32 -> (qa, R) [75]; a row that is not finite: both +infinity"""
    with np.errstate(all="ignore"):
        P = (np.asarray(S1, F32) * RSQRT2).astype(F32)
        disc = SM.fma32(F32(1536), np.asarray(SD, F32), (P * P).astype(F32))
        m2 = (np.asarray(S2, F32) * K1536).astype(F32)
        bad = ~(disc <= FLT_MAX) | ~(m2 <= FLT_MAX)
        qa = ((np.sqrt(disc).astype(F32) - P).astype(F32) * K1536).astype(F32)
        qa = np.where(qa > 0, qa, F32(0)).astype(F32)
        R = np.sqrt(m2).astype(F32)
    return np.where(bad, F32(np.inf), qa).astype(F32), np.where(bad, F32(np.inf), R).astype(F32)


def median(x):
    """the 38th smallest of 75 values, ties by row index (a stable sort is exactly that)"""
    x = np.asarray(x).reshape(N_SYMBOLS)
    return x[np.argsort(x, kind="stable")[MEDIAN_RANK]]


def weight(q, q_ref):
    q, q_ref = F32(q), F32(q_ref)
    if not (q <= FLT_MAX):
        return F32(0)
    if q <= q_ref:
        return F32(1)
    with np.errstate(all="ignore"):
        cap = F32(q_ref * WEIGHT_CAP)
        v = F32(q_ref * DM.reciprocal(q if q > cap else cap))
    return v if v < 1 else F32(1)


def frame(dq, sync_ok=True):
    """one frame as the device writes it -> dict(symbol_weight [75], symbol_noise [75], ref_noise, valid)"""
    skipped = dict(symbol_weight=np.zeros(N_SYMBOLS, F32), symbol_noise=np.zeros(N_SYMBOLS, F32), ref_noise=F32(0), valid=np.uint32(0))
    if not sync_ok:
        return skipped
    qa, R = figures(*sums(dq))
    with np.errstate(all="ignore"):
        lifted = (median(qa) + (R - median(R)).astype(F32)).astype(F32)
        q = np.where(np.isinf(qa), qa, np.where(lifted > qa, lifted, qa)).astype(F32)
    q_ref = median(q)
    if not (q_ref >= FLT_MIN and q_ref <= FLT_MAX):
        return skipped
    return dict(symbol_weight=np.array([weight(x, q_ref) for x in q], F32), symbol_noise=q, ref_noise=F32(q_ref), valid=np.uint32(1))


# ---- float64 ----
def frame64(dq):
    """the definition in float64 with true roots and quotients, finite rows only -> dict(S1, SD, S2, P, root, qa, R, q, q_ref, v, lifted)"""
    d = np.asarray(dq, np.complex64).reshape(N_SYMBOLS, N_CARRIERS).astype(np.complex128)
    ar, ai = np.abs(d.real), np.abs(d.imag)
    S1, SD, S2 = (ar + ai).sum(axis=1), ((ar - ai) ** 2).sum(axis=1), (ar ** 2 + ai ** 2).sum(axis=1)
    P = S1 / math.sqrt(2.0)
    root = np.sqrt(P * P + 1536.0 * SD)
    qa = np.maximum(root - P, 0.0) / 1536.0
    R = np.sqrt(S2 / 1536.0)
    lifted = median(qa) + (R - median(R))
    q = np.maximum(qa, lifted)
    q_ref = median(q)
    v = np.where(q <= q_ref, 1.0, np.minimum(1.0, q_ref / np.maximum(q, q_ref * 2.0 ** -20)))
    return dict(S1=S1, SD=SD, S2=S2, P=P, root=root, qa=qa, R=R, q=q, q_ref=q_ref, v=v, lifted=lifted)


def bounds64(f):
    """the head's bounds from frame64's figures -> (bound_qa [75], bound_R [75], bound_q (one number for every row and the reference))"""
    b_qa = (BOUND_ROOT * f["root"] + BOUND_P * f["P"] + 3 * U * np.abs(f["root"] - f["P"])) / 1536.0
    b_R = BOUND_R * f["R"]
    med_R = median(f["R"])
    b_q = b_qa.max() + (BOUND_R * (f["R"] + med_R) + 2 * U * (np.abs(f["R"] - med_R) + np.abs(f["lifted"]))).max()
    return b_qa, b_R, float(b_q)


# ---- float64 Monte Carlo of one product row ----
def ripple(n=N_CARRIERS, second=SECOND_PATH, delay=37.0):
    """channel power |1 + second e^(-j 2 pi delay c / 2048)|^2 per carrier, mean normalised to 1"""
    a = np.abs(1.0 + second * np.exp(-2j * math.pi * delay * np.arange(n) / 2048.0)) ** 2
    return a / a.mean()


def row_products(rng, snr_db, rows=8, a=None):
    """rows + 1 symbols of unit-modulus pi/4 DQPSK over the ripple at mean carrier SNR snr_db -> (products [rows][1536] complex128, q)"""
    a = ripple() if a is None else a
    q = 1.0 / 10.0 ** (snr_db / 10.0)
    n = a.size
    phase = np.cumsum(rng.integers(0, 4, (rows + 1, n)) * 0.5 + 0.25, axis=0) * math.pi
    X = np.sqrt(a)[None, :] * np.exp(1j * phase) + math.sqrt(q / 2.0) * (rng.standard_normal((rows + 1, n)) + 1j * rng.standard_normal((rows + 1, n)))
    return X[:-1] * np.conj(X[1:]), q


def row_estimates(d):
    """qa of every row in float64"""
    ar, ai = np.abs(d.real), np.abs(d.imag)
    P = (ar + ai).sum(axis=1) / math.sqrt(2.0)
    return (np.sqrt(P * P + d.shape[1] * ((ar - ai) ** 2).sum(axis=1)) - P) / d.shape[1]


def monte_carlo(snr_db, seeds, rows=8):
    """-> (E[qa] / q, relative deviation of one row's qa against its own mean, number of row draws)"""
    est = []
    for seed in seeds:
        d, q = row_products(np.random.Generator(np.random.PCG64(seed)), snr_db, rows)
        est.append(row_estimates(d) / q)
    est = np.concatenate(est)
    return float(est.mean()), float(est.std(ddof=1) / est.mean()), est.size


def frame_products(rng, snr_db=15.0, amp=3.0e5, burst=None):
    """one frame's products in float32 at channel power amp x ripple; burst = (first symbol, symbols, I / S dB): white noise of that power
    on those OFDM symbols (0 .. 75) on top"""
    a = ripple() * amp
    q = amp / 10.0 ** (snr_db / 10.0)
    n = N_CARRIERS
    phase = np.cumsum(rng.integers(0, 4, (N_SYMBOLS + 1, n)) * 0.5 + 0.25, axis=0) * math.pi
    X = np.sqrt(a)[None, :] * np.exp(1j * phase) + math.sqrt(q / 2.0) * (rng.standard_normal((N_SYMBOLS + 1, n)) + 1j * rng.standard_normal((N_SYMBOLS + 1, n)))
    if burst is not None:
        s0, ns, is_db = burst
        p = amp * 10.0 ** (is_db / 10.0)
        X[s0:s0 + ns] += math.sqrt(p / 2.0) * (rng.standard_normal((ns, n)) + 1j * rng.standard_normal((ns, n)))
    return (X[:-1] * np.conj(X[1:])).astype(np.complex64)


# ---- float32 host model: csrc/sym_profile_core.h ----
_host = {}


def build_host_model(tmp):
    if "lib" in _host:
        return _host["lib"]
    so = os.path.join(str(tmp), "libsym_profile_host_model.so")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                          "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "sym_profile_host_model.cpp"), os.path.join(CSRC, "dabgpu_host_logic.cpp"),
                          "-o", so], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    L = C.CDLL(so)
    L.sypm_k1536.restype = L.sypm_rsqrt2.restype = L.sypm_median.restype = C.c_float
    L.sypm_median.argtypes = [C.c_void_p]
    L.sypm_sums.argtypes = [C.c_void_p] * 4
    L.sypm_figures.argtypes = [C.c_void_p] * 5
    L.sypm_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sypm_combine_frame.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_void_p] * 3
    L.dabgpu_sym_profile_rows_host.argtypes = [C.c_void_p] * 4
    L.dabgpu_get_carrier_mapper.argtypes = [C.c_int, C.c_void_p]
    _host["lib"] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data


def host_sums(lib, dq):
    d = np.ascontiguousarray(dq, np.complex64).reshape(N_SYMBOLS * N_CARRIERS)
    out = [np.full(N_SYMBOLS, 99, F32) for _ in range(3)]
    lib.sypm_sums(_p(d), *[_p(x) for x in out])
    return tuple(out)


def host_figures(lib, S1, SD, S2):
    a = [np.ascontiguousarray(x, F32).reshape(N_SYMBOLS) for x in (S1, SD, S2)]
    qa, R = np.full(N_SYMBOLS, 99, F32), np.full(N_SYMBOLS, 99, F32)
    lib.sypm_figures(*[_p(x) for x in a], _p(qa), _p(R))
    return qa, R


def host_median(lib, x):
    return F32(lib.sypm_median(_p(np.ascontiguousarray(x, F32).reshape(N_SYMBOLS))))


def host_frame(lib, dq, sync_ok=True, entry="sypm_frame"):
    """the compiled header over one frame -> the dict of frame(); dq may be None for a frame whose record is not valid"""
    d = None if dq is None else np.ascontiguousarray(dq, np.complex64).reshape(N_SYMBOLS * N_CARRIERS)
    v, q, ref = np.full(N_SYMBOLS, 99, F32), np.full(N_SYMBOLS, 99, F32), C.c_float(99.0)
    if entry == "sypm_frame":
        ok = lib.sypm_frame(_p(d), int(bool(sync_ok)), _p(v), _p(q), C.byref(ref))
    else:
        ok = getattr(lib, entry)(_p(d), _p(v), _p(q), C.byref(ref))
    return dict(symbol_weight=v, symbol_noise=q, ref_noise=F32(ref.value), valid=np.uint32(ok))


class HostModel:
    """one frame in the arithmetic of the device"""

    def __init__(self, lib):
        self.L = lib

    def profile(self, dq):
        return host_frame(self.L, dq, True)
