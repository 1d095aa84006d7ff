// interferer_core.h -- every arithmetic step of the interferer (include/dabgpu.h, "Interferer"), host and device: the kernel
// (interferer.hip) and the host model of the tests (tests/cpp/interferer_host_model.cpp) compile these same functions, so the device is
// checked bit for bit against a CPU run of this file, and this file against an independent numpy model (tests/interferer_model.py).
// Philox, Box-Muller, the 64-bit oscillator and sine / cosine are channel_core.h's, unchanged, and so is the arithmetic contract:
// -ffp-contract=off, every fused operation an explicit fmaf, no library transcendental.  Error bounds: DESIGN.md 4.28.
#pragma once
#include <stdint.h>

#include "channel_core.h"

namespace dabgpu {

constexpr int ITF_TAPS = DABGPU_INTERFERER_TAPS;
constexpr float ITF_INV_SQRT2 = 0.70710678f;

// the four words shared by g[2 p] and g[2 p + 1] of source k of stream s (word 3: 0 is the channel's noise, 1 its fading tables)
DABGPU_HD inline void itf_noise_words(uint64_t seed, uint32_t s, uint32_t k, uint64_t pair, uint32_t w[4]) {
    ch_philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)pair, (uint32_t)(pair >> 32), s, 16u + k, w);
}
// g[n], n any unsigned 64-bit number
DABGPU_HD inline chf2 itf_gauss(uint64_t seed, uint32_t s, uint32_t k, uint64_t n) {
    uint32_t w[4];
    itf_noise_words(seed, s, k, n >> 1, w);
    const int h = (int)(n & 1u) * 2;
    return ch_gauss_pair(w[h], w[h + 1]);
}

DABGPU_HD inline int itf_log2(int interp) { return 31 - __builtin_clz((unsigned)interp); }

// a source that generates (kind TONE or BAND, amp != 0); shaped: it reads a shape of the bank
DABGPU_HD inline bool itf_live(const dabgpu_interferer_source& S) {
    return (S.kind == DABGPU_INTERFERER_TONE || S.kind == DABGPU_INTERFERER_BAND) && S.amp != 0.0f;
}
DABGPU_HD inline bool itf_shaped(const dabgpu_interferer_source& S) { return S.kind == DABGPU_INTERFERER_BAND && S.shape >= 0 && S.amp != 0.0f; }

// (m - offset) mod period, non-negative, for period > 0, m < 2^63 and |offset| < 2^62: every intermediate fits an unsigned 64-bit word
DABGPU_HD inline uint64_t itf_gate_rem(uint64_t m, int64_t offset, uint64_t period) {
    if (offset <= 0) return (m + (uint64_t)(-offset)) % period;
    const uint64_t o = (uint64_t)offset;
    if (m >= o) return (m - o) % period;
    return period - 1u - ((o - m - 1u) % period);
}
// the remainder k < 2048 samples behind one whose remainder is rem0 (the kernel divides once per tile and steps from there)
DABGPU_HD inline uint64_t itf_gate_step(uint64_t rem0, uint32_t k, uint64_t period) {
    if (period < 4096u) return (uint64_t)(((uint32_t)rem0 + k) % (uint32_t)period);
    const uint64_t r = rem0 + k;                                             // may wrap for a period near 2^64: then it is past the period too
    return (r >= period || r < rem0) ? r - period : r;
}
DABGPU_HD inline bool itf_gate_on(const dabgpu_interferer_source& S, uint64_t m) {
    return S.gate_period == 0 || itf_gate_rem(m, S.gate_offset, S.gate_period) < S.gate_on;
}

// b of a shaped BAND source: taps = the shape's table, r = m & (L - 1), g(t) = g[q - t]
template <class G>
DABGPU_HD inline chf2 itf_band_sum(const float* taps, int interp, int r, G g) {
    const chf2 g0 = g(0);
    const float h0 = taps[r];
    float re = h0 * g0.re, im = h0 * g0.im;
    for (int t = 1; t < ITF_TAPS; t++) {
        const chf2 gt = g(t);
        const float h = taps[r + interp * t];
        re = __builtin_fmaf(h, gt.re, re);
        im = __builtin_fmaf(h, gt.im, im);
    }
    return chf2{re, im};
}
DABGPU_HD inline chf2 itf_white(chf2 g) { return chf2{g.re * ITF_INV_SQRT2, g.im * ITF_INV_SQRT2}; }

// v of a BAND source from its b: the amplitude, then the rotation to the band's centre (the channel model's product)
DABGPU_HD inline chf2 itf_band_finish(const dabgpu_interferer_source& S, uint64_t m, chf2 b) {
    chf2 v = chf2{S.amp * b.re, S.amp * b.im};
    if ((S.freq_q64 | S.phase0_q64) != 0) {
        const chf2 cs = ch_cos_sin(ch_osc_cycles(S.phase0_q64, S.freq_q64, m));
        const float b0 = cs.im * v.im, b1 = cs.im * v.re;
        v = chf2{__builtin_fmaf(cs.re, v.re, -b0), __builtin_fmaf(cs.re, v.im, b1)};
    }
    return v;
}
DABGPU_HD inline chf2 itf_tone(const dabgpu_interferer_source& S, uint64_t m) {
    const chf2 cs = ch_cos_sin(ch_osc_cycles(S.phase0_q64, S.freq_q64, m));
    return chf2{S.amp * cs.re, S.amp * cs.im};
}
DABGPU_HD inline chf2 itf_add(chf2 y, chf2 v) { return chf2{y.re + v.re, y.im + v.im}; }

// one sample, one thread, straight from the definition (the host model; the kernel stages g and the taps in LDS and steps the gate)
DABGPU_HD inline chf2 itf_sample(const dabgpu_interferer_stream& P, const dabgpu_interferer_shape* shapes, uint32_t s, uint64_t m, chf2 x) {
    chf2 y = x;
    for (int k = 0; k < P.n_sources; k++) {
        const dabgpu_interferer_source& S = P.source[k];
        if (!itf_live(S) || !itf_gate_on(S, m)) continue;
        chf2 v;
        if (S.kind == DABGPU_INTERFERER_TONE) v = itf_tone(S, m);
        else if (S.shape < 0) v = itf_band_finish(S, m, itf_white(itf_gauss(P.seed, s, (uint32_t)k, m)));
        else {
            const dabgpu_interferer_shape& H = shapes[S.shape];
            const int l = itf_log2(H.interp);
            const uint64_t q = m >> l;
            const chf2 b = itf_band_sum(H.taps, H.interp, (int)(m & (uint64_t)(H.interp - 1)),
                                        [&](int t) { return itf_gauss(P.seed, s, (uint32_t)k, q - (uint64_t)t); });
            v = itf_band_finish(S, m, b);
        }
        y = itf_add(y, v);
    }
    return y;
}

// LDS of one shaped BAND source of interp L in a tile of DABGPU_INTERFERER_BLOCK samples: 16 L floats, then the tile's g from the even
// number at or below (first q) - 15 on -- 1024 / L + 1 values of q, 15 before them, one for the even start, rounded up to a pair
DABGPU_HD inline uint32_t itf_slot_g_count(int interp) { return (uint32_t)(DABGPU_INTERFERER_BLOCK / interp) + 18u; }
DABGPU_HD inline uint32_t itf_slot_bytes(int interp) { return (uint32_t)(ITF_TAPS * interp) * 4u + itf_slot_g_count(interp) * 8u; }

}  // namespace dabgpu
