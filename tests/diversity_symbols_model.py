"""The symbol-weighted combiner (include/dabgpu.h, "Symbol-weighted receive diversity"), written from the definition: the banded rule of
tests/noise_profile_model.py with one more factor -- for a branch with a symbol table, carrier c of product row s enters the sum with
wband * clean(v[s]), the product rounded once to float32; symbol weights enter neither the live rule nor the scale -- and the compiled
host model of the same rule (tests/cpp/sym_profile_host_model.cpp over csrc/diversity_core.h and csrc/noise_profile_core.h), which the
device is compared with bit for bit."""
import ctypes as C

import numpy as np

import diversity_model as DM
import noise_profile_model as PM
import softbit_model as SM
import sym_profile_model as SP

F32 = np.float32
N_SYMBOLS, N_CARRIERS = SP.N_SYMBOLS, SP.N_CARRIERS
build_host_model = SP.build_host_model


def combine_frame(dq, k, mapper, w=None, valid=None, band=None, sym=None, layout=DM.BITS_NATURAL):
    """one frame: noise_profile_model's banded rule with sym[b] = 75 symbol weights of branch b or None -> (bits, scale, mask).  No symbol
    table at all: the banded rule itself"""
    n = len(dq)
    band = [None] * n if band is None else list(band)
    sym = [None] * n if sym is None else list(sym)
    if all(x is None for x in sym):
        return PM.combine_frame(dq, k, mapper, w, valid, band, layout)
    ws = np.ones(n, F32) if w is None else np.asarray(w, F32).reshape(n).copy()
    for b in range(n):
        if band[b] is not None:
            ws[b] = PM.branch_weight(band[b])
    kk, mask = DM.scale(k, ws, valid)                                                  # symbol weights have no say in the scale
    shape = (DM.NB_DATA_SYMBOLS, DM.NB_CARRIERS)
    re = im = None
    with np.errstate(all="ignore"):
        if kk != 0:
            for b in range(n):
                if not (mask >> b) & 1:
                    continue
                d = np.asarray(dq[b], np.complex64).reshape(shape)
                if band[b] is None:
                    wc = np.full(N_CARRIERS, ws[b], F32)
                else:
                    bw = np.asarray(band[b], F32).reshape(PM.N_BANDS)
                    wc = np.repeat(np.where(PM.positive_finite(bw), bw, F32(0)), PM.BAND).astype(F32)
                wc = np.broadcast_to(wc, shape)
                if sym[b] is not None:
                    v = np.asarray(sym[b], F32).reshape(N_SYMBOLS)
                    wc = (wc * np.where(PM.positive_finite(v), v, F32(0)).astype(F32)[:, None]).astype(F32)       # rounded once
                if re is None:
                    re, im = (wc * d.real).astype(F32), (wc * d.imag).astype(F32)
                else:
                    re, im = SM.fma32(wc, d.real, re), SM.fma32(wc, d.imag, im)
        if re is None:
            re, im = np.zeros(shape, F32), np.zeros(shape, F32)
        m = np.asarray(mapper)
        first, second = -(re[:, m] * kk), -((-im[:, m]) * kk)
    bits = np.concatenate([SM.quantise(first), SM.quantise(second)], axis=1).reshape(-1)
    return (DM.to_classed(bits) if layout == DM.BITS_MSC_CLASSED else bits), kk, mask


def _p(a):
    return None if a is None else a.ctypes.data


def host_combine_frame(lib, dq, k, w=None, valid=None, band=None, sym=None, layout=DM.BITS_NATURAL):
    """the compiled rule over one frame; a branch given as None is handed over as an address that must not be read; band / sym None: a
    null array"""
    n = len(dq)
    keep = [None if d is None else np.ascontiguousarray(d, dtype=np.complex64).reshape(-1) for d in dq]
    ptrs = (C.c_void_p * n)(*[_p(d) for d in keep])
    kb = [None if x is None else np.ascontiguousarray(x, F32).reshape(PM.N_BANDS) for x in (band or [None] * n)]
    ks = [None if x is None else np.ascontiguousarray(x, F32).reshape(N_SYMBOLS) for x in (sym or [None] * n)]
    bptrs = None if band is None else (C.c_void_p * n)(*[_p(x) for x in kb])
    sptrs = None if sym is None else (C.c_void_p * n)(*[_p(x) for x in ks])
    k = np.ascontiguousarray(k, dtype=F32).reshape(n)
    w = None if w is None else np.ascontiguousarray(w, F32).reshape(n)
    v = None if valid is None else np.ascontiguousarray(valid, np.int32).reshape(n)
    bits = np.full(DM.NB_FRAME_BITS, 99, np.int8)
    out_k, mask = C.c_float(0), C.c_uint32(0)
    st = lib.sypm_combine_frame(ptrs, _p(k), _p(w), _p(v), bptrs, sptrs, n, int(layout), _p(bits), C.byref(out_k), C.byref(mask))
    assert st == 0
    return bits, F32(out_k.value), mask.value


def host_mapper(lib):
    m = np.zeros(N_CARRIERS, np.int32)
    assert lib.dabgpu_get_carrier_mapper(1, m.ctypes.data) == 0
    return m
