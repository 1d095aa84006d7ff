// channelise_core.h -- every arithmetic step of the channeliser (include/dabgpu.h, "Channeliser"), host and device: the kernels
// (channelise.hip) and the host model of the tests (tests/cpp/channelise_host_model.cpp) compile these same functions, so the device is
// checked bit for bit against a CPU run of this file, and this file against an independent numpy model (tests/channelise_model.py).
// The library's arithmetic contract holds: built with -ffp-contract=off, every fused operation an explicit fmaf, no library
// transcendental on the sample path (the table is designed on the host in double, dabgpu_channeliser_design, and only read here; the
// oscillator is the channel model's: exact 64-bit phase, ch_osc_cycles, ch_cos_sin).  Error bound: DESIGN.md 4.20.
#pragma once
#include <stdint.h>

#include "channel_core.h"          // chf2, ch_osc_cycles, ch_cos_sin, ch_u8, DABGPU_HD

namespace dabgpu {

constexpr int CS_TPP = DABGPU_CHANNELISER_TAPS_PER_PHASE;
constexpr int CS_MAX_D = DABGPU_CHANNELISER_MAX_DECIM;
constexpr int CS_MAX_CH = DABGPU_CHANNELISER_MAX_CHANNELS;

// D = 1 is the mixer: one tap of 1 on the sample itself
DABGPU_HD constexpr int cs_phase_taps(int D) { return D == 1 ? 1 : CS_TPP; }           // K / D: taps per block-rate phase
DABGPU_HD constexpr int cs_taps(int D) { return cs_phase_taps(D) * D; }                // K
DABGPU_HD constexpr int cs_peak(int D) { return D == 1 ? 0 : cs_taps(D) / 2 - 1; }     // P

// y * (cos, sin)(phase0 + n * freq): the angle and the product order of the channel model's ch_finish
DABGPU_HD inline chf2 cs_rotate(chf2 y, uint64_t phase0_q64, uint64_t freq_q64, uint64_t n) {
    const chf2 cs = ch_cos_sin(ch_osc_cycles(phase0_q64, freq_q64, n));
    const float b0 = cs.im * y.im, b1 = cs.im * y.re;
    return chf2{__builtin_fmaf(cs.re, y.re, -b0), __builtin_fmaf(cs.re, y.im, b1)};
}
DABGPU_HD inline bool cs_mixes(const dabgpu_channeliser_channel& C) { return (C.freq_q64 | C.phase0_q64) != 0; }
// split: v_c[n], the sample rotated by -(phase0 + n * freq) = (-phase0) + n * (-freq) modulo 2^64
DABGPU_HD inline chf2 cs_mix_down(const dabgpu_channeliser_channel& C, chf2 x, uint64_t n) {
    return cs_mixes(C) ? cs_rotate(x, (uint64_t)0 - C.phase0_q64, (uint64_t)0 - C.freq_q64, n) : x;
}
// combine: the channel's term rotated by +(phase0 + n * freq)
DABGPU_HD inline chf2 cs_mix_up(const dabgpu_channeliser_channel& C, chf2 g, uint64_t n) {
    return cs_mixes(C) ? cs_rotate(g, C.phase0_q64, C.freq_q64, n) : g;
}

// The chain sum_j h[j] * v[j], re and im separate, ascending j: the first term is the plain product, every later one fmaf(h, v, sum).
// The chain starts from -0: fmaf(h, v, -0) IS the plain product h * v bit for bit (p + -0 = p for every p, both zeros included, and one
// rounding either way), so every term is the same instruction and a kernel may interleave the chains of several outputs.
DABGPU_HD inline chf2 cs_chain_start() { return chf2{-0.0f, -0.0f}; }
DABGPU_HD inline chf2 cs_tap(chf2 acc, float h, chf2 v) { return chf2{__builtin_fmaf(h, v.re, acc.re), __builtin_fmaf(h, v.im, acc.im)}; }
DABGPU_HD inline chf2 cs_scale(float g, chf2 z) { return chf2{g * z.re, g * z.im}; }
DABGPU_HD inline chf2 cs_add(chf2 y, chf2 t) { return chf2{y.re + t.re, y.im + t.im}; }

// x[i] of the definition: wrap takes the index modulo n_in, otherwise samples outside the input are zero
DABGPU_HD inline chf2 cs_fetch(const chf2* x, int64_t n_in, bool wrap, int64_t i) {
    if (wrap) { i %= n_in; return x[i < 0 ? i + n_in : i]; }
    return (i >= 0 && i < n_in) ? x[i] : chf2{0.0f, 0.0f};
}

// the wideband index under tap 0 of split output m (m = position + index in the call; m <= 2^58 + 2^31, |start| <= 2^61: no overflow)
DABGPU_HD inline int64_t cs_split_first(int D, uint64_t m, int64_t start) { return (int64_t)(m * (uint64_t)D) + start - cs_peak(D); }

// one split output: the host model's loop, and the kernel's D = 1 path; the kernel's filter runs the same cs_tap over the same j
DABGPU_HD inline chf2 cs_split_sample(const dabgpu_channeliser_channel& C, int D, const float* table, const chf2* x, int64_t n_in, bool wrap,
                                      uint64_t m, int64_t start) {
    const int64_t first = cs_split_first(D, m, start);
    const int K = cs_taps(D);
    chf2 acc = cs_chain_start();
    for (int j = 0; j < K; j++) acc = cs_tap(acc, table[j], cs_mix_down(C, cs_fetch(x, n_in, wrap, first + j), (uint64_t)(first + j)));
    return cs_scale(C.gain, acc);
}

DABGPU_HD inline int64_t cs_floor_div(int64_t a, int D) { const int64_t q = a / D; return (a % D < 0) ? q - 1 : q; }

// Combine, wideband sample n: t = n - start + P = q * D + rho.  The taps of x[m] are j = t - m * D in [0, K): m = q - (K / D - 1) .. q,
// ascending m = descending j.  cs_combine_row is the block-rate index q, cs_combine_tap the tap under x[q - (K / D - 1) + k] for residue rho.
DABGPU_HD inline int64_t cs_combine_t(int D, int64_t n, int64_t start) { return n - start + cs_peak(D); }
DABGPU_HD constexpr int cs_combine_tap(int D, int rho, int k) { return rho + (cs_phase_taps(D) - 1 - k) * D; }
// gain_c * (D * sum), rotated: the term of one channel from its chain
DABGPU_HD inline chf2 cs_combine_finish(const dabgpu_channeliser_channel& C, int D, chf2 acc, uint64_t n) {
    return cs_mix_up(C, cs_scale(C.gain, cs_scale((float)D, acc)), n);
}
DABGPU_HD inline chf2 cs_combine_term(const dabgpu_channeliser_channel& C, int D, const float* table, const chf2* x, int64_t n_in, bool wrap,
                                      int64_t n, int64_t start) {
    const int64_t t = cs_combine_t(D, n, start), q = cs_floor_div(t, D);
    const int rho = (int)(t - q * D), NT = cs_phase_taps(D);
    chf2 acc = cs_chain_start();
    for (int k = 0; k < NT; k++) acc = cs_tap(acc, table[cs_combine_tap(D, rho, k)], cs_fetch(x, n_in, wrap, q - (NT - 1) + k));
    return cs_combine_finish(C, D, acc, (uint64_t)n);
}
// one wideband sample from the channels [c0, c1) of its stream (none: zero)
DABGPU_HD inline chf2 cs_combine_sample(const dabgpu_channeliser_channel* ch, uint32_t c0, uint32_t c1, int D, const float* table, const chf2* in,
                                        size_t in_stride, int64_t n_in, bool wrap, int64_t n, int64_t start) {
    chf2 y = chf2{0.0f, 0.0f};
    for (uint32_t c = c0; c < c1; c++) {
        const chf2 term = cs_combine_term(ch[c], D, table, in + (size_t)c * in_stride, n_in, wrap, n, start);
        y = (c == c0) ? term : cs_add(y, term);
    }
    return y;
}

}  // namespace dabgpu
