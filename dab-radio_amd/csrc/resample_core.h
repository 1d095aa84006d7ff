// resample_core.h -- every arithmetic step of the resampler (include/dabgpu.h, "Resampler"), host and device: the kernel (resample.hip)
// and the host model of the tests (tests/cpp/resample_host_model.cpp) compile these same functions, so the device is checked bit for bit
// against a CPU run of this file, and this file against an independent numpy model (tests/resample_model.py).  The library's arithmetic
// contract holds: built with -ffp-contract=off, every fused operation an explicit fmaf, no library transcendental on the sample path (the
// filter table is designed on the host in double, dabgpu_resample_design, and only read here).  The time of an output sample is exact
// integer arithmetic, 128 bits wide, built from 32 x 32 -> 64 products in plain C++ so that both compilers see the same lines.
// Error bounds: DESIGN.md 4.19.
#pragma once
#include <stdint.h>

#include "channel_core.h"          // chf2, ch_u8 (the modulator's quantiser), DABGPU_HD

namespace dabgpu {

constexpr int RS_L = DABGPU_RESAMPLE_PHASES, RS_LOG2L = DABGPU_RESAMPLE_PHASE_BITS, RS_TAPS = DABGPU_RESAMPLE_TAPS;
constexpr int RS_BLK = DABGPU_RESAMPLE_BLOCK;
constexpr uint64_t RS_ONE = (uint64_t)1 << 62, RS_FRAC_MASK = RS_ONE - 1;
static_assert((1 << RS_LOG2L) == RS_L && RS_TAPS % 2 == 0, "table shape");

// a * b as (hi, lo), from four 32 x 32 -> 64 products
DABGPU_HD inline void rs_mul64(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;          // < 3 * 2^32
    lo = (mid << 32) | (uint32_t)p00;
    hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// T(m) = (offset_samples * 2^62 + offset_frac_q62) + m * step_q62, as an input index and a fraction:
//   n     floor(T / 2^62) modulo 2^64, and whether the true value is negative.  With |offset_samples| <= 2^62, m <= 2^62 + 2^31 and
//         step <= 2 the true value lies in [-2^62, 1.5 * 2^63 + 2^33]: 65 bits, of which `neg` is the sign (the word alone cannot tell
//         -2^62 from 1.5 * 2^63)
//   frac  T mod 2^62
struct RsIndex { uint64_t n; bool neg; };
struct RsTime { uint64_t n, frac; bool neg; };
DABGPU_HD inline RsTime rs_time(const dabgpu_resample_stream& P, uint64_t m) {
    uint64_t hi, lo;
    rs_mul64(m, P.step_q62, hi, lo);                                           // < 2^126: hi < 2^62
    const uint64_t sum = lo + P.offset_frac_q62;
    hi += (sum < lo) ? 1u : 0u;
    const uint64_t q = (hi << 2) | (sum >> 62), off = (uint64_t)P.offset_samples;
    return RsTime{off + q, sum & RS_FRAC_MASK, P.offset_samples < 0 && q < (uint64_t)0 - off};
}
DABGPU_HD inline RsIndex rs_index(const RsTime& t) { return RsIndex{t.n, t.neg}; }
// the index k samples earlier (k small) / j samples later
DABGPU_HD inline RsIndex rs_before(RsIndex a, uint64_t k) { return RsIndex{a.n - k, a.neg || a.n < k}; }
DABGPU_HD inline RsIndex rs_after(RsIndex a, uint64_t j) { const uint64_t n = a.n + j; return RsIndex{n, a.neg && !(n < j)}; }
// the index modulo n_in
DABGPU_HD inline int64_t rs_mod(RsIndex a, int64_t n_in) {
    if (a.neg) { const uint64_t r = ((uint64_t)0 - a.n) % (uint64_t)n_in; return r ? n_in - (int64_t)r : 0; }
    return (int64_t)(a.n % (uint64_t)n_in);
}
// the same index as a plain signed number, clamped to +-2^41: far enough outside any input (n_in <= 2^40) that index + a tile cannot overflow
DABGPU_HD inline int64_t rs_clamped(RsIndex a) {
    const int64_t far = (int64_t)1 << 41;
    if (a.neg) return (int64_t)a.n < -far ? -far : (int64_t)a.n;
    return a.n > (uint64_t)far ? far : (int64_t)a.n;
}
// x[n] of the definition: wrap takes the index modulo n_in, otherwise samples outside the input are zero
DABGPU_HD inline chf2 rs_fetch(const chf2* x, int64_t n_in, bool wrap, RsIndex a) {
    if (wrap) return x[rs_mod(a, n_in)];
    const int64_t i = rs_clamped(a);
    return (i >= 0 && i < n_in) ? x[i] : chf2{0.0f, 0.0f};
}

// phase row p = the top log2(L) bits of the fraction; w = the next 15 bits over 2^15 (exact in float)
DABGPU_HD inline int rs_row(uint64_t frac) { return (int)(frac >> (62 - RS_LOG2L)); }
DABGPU_HD inline float rs_weight(uint64_t frac) { return (float)(uint32_t)((frac >> (62 - RS_LOG2L - 15)) & 0x7FFFu) * 0x1p-15f; }

// step exactly 1 and no fractional offset: no filter, the output is the shifted input
DABGPU_HD inline bool rs_identity(const dabgpu_resample_stream& P) { return P.step_q62 == RS_ONE && P.offset_frac_q62 == 0; }

// Table rows one tile of RS_BLK outputs of a stream can touch: the phase moves by d = min(frac(step), 1 - frac(step)) per output, one way
// round the circle of L rows, so first and last output lie at most ceil(1023 d L) rows apart; + the row p + 1 of the interpolation, + row L
// beside row 0 where the tile passes the end of the circle, + 2 for the roundings here.  L + 1 (the whole table) where that is fewer.
DABGPU_HD inline bool rs_phase_rises(const dabgpu_resample_stream& P) { return (P.step_q62 & RS_FRAC_MASK) < (RS_ONE >> 1); }
DABGPU_HD inline uint32_t rs_rows_needed(const dabgpu_resample_stream& P) {
    const uint64_t sf = P.step_q62 & RS_FRAC_MASK, d = rs_phase_rises(P) ? sf : RS_ONE - sf;          // <= 2^61
    const uint64_t rows = ((((d >> 22) + 1) * (uint64_t)(RS_BLK - 1)) >> (62 - RS_LOG2L - 22)) + 1 + 4;
    return rows < (uint64_t)(RS_L + 1) ? (uint32_t)rows : (uint32_t)(RS_L + 1);
}
// where row p sits among the rows staged from row r0 on, in the order r0, r0 + 1, ..., L - 1, L, 0, 1, ... (row L, which is row 0 advanced
// by one input sample, keeps its place behind row L - 1: the pair (p, p + 1) is adjacent for every p)
DABGPU_HD inline int rs_slot(int p, int r0) { return p >= r0 ? p - r0 : p + (RS_L + 1) - r0; }
DABGPU_HD inline int rs_slot_row(int slot, int r0) { return r0 + slot <= RS_L ? r0 + slot : r0 + slot - (RS_L + 1); }

// c_j = fmaf(w, H[p + 1][j] - H[p][j], H[p][j]): the interpolated form IS the definition
DABGPU_HD inline float rs_coef(float w, float h0, float h1) { return __builtin_fmaf(w, h1 - h0, h0); }

// sum_j c_j * x[n - taps / 2 + 1 + j], re and im separate, ONE chain each in ascending j: the first term is the plain product c_0 * x,
// every later one fmaf(c_j, x, sum).  h0(j) = H[p][j], h1(j) = H[p + 1][j], x(j) = the input sample of tap j
template <class Row0, class Row1, class Fetch>
DABGPU_HD inline chf2 rs_filter(float w, Row0 h0, Row1 h1, Fetch x) {
    const float c0 = rs_coef(w, h0(0), h1(0));
    const chf2 x0 = x(0);
    float re = c0 * x0.re, im = c0 * x0.im;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 1; j < RS_TAPS; j++) {
        const float c = rs_coef(w, h0(j), h1(j));
        const chf2 v = x(j);
        re = __builtin_fmaf(c, v.re, re);
        im = __builtin_fmaf(c, v.im, im);
    }
    return chf2{re, im};
}

// the gain comes last
DABGPU_HD inline chf2 rs_finish(const dabgpu_resample_stream& P, chf2 z) { return chf2{P.gain * z.re, P.gain * z.im}; }

// one output sample from the input in memory and the table as dabgpu_resample_design holds it ([L + 1][taps]); the host model's loop, and
// what the kernel computes from LDS
DABGPU_HD inline chf2 rs_sample(const dabgpu_resample_stream& P, const float* table, const chf2* x, int64_t n_in, bool wrap, uint64_t m) {
    const RsTime t = rs_time(P, m);
    if (rs_identity(P)) return rs_finish(P, rs_fetch(x, n_in, wrap, rs_index(t)));
    const float* r0 = table + (size_t)rs_row(t.frac) * RS_TAPS;
    const RsIndex first = rs_before(rs_index(t), (uint64_t)(RS_TAPS / 2 - 1));
    const chf2 z = rs_filter(rs_weight(t.frac), [&](int j) { return r0[j]; }, [&](int j) { return r0[RS_TAPS + j]; },
                             [&](int j) { return rs_fetch(x, n_in, wrap, rs_after(first, (uint64_t)j)); });
    return rs_finish(P, z);
}

}  // namespace dabgpu
