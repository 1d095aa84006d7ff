// softbit_csi_core.h -- every arithmetic step of the channel-state weighted soft bits (include/dabgpu.h, DABGPU_SOFT_CSI), host and
// device: the demodulation kernel (ofdm_demod.hip), dabgpu_soft_scale_host and the host model of the tests
// (tests/cpp/softbit_host_model.cpp) compile these same functions, so the device is checked bit for bit against a CPU run of this file,
// and this file against an independent numpy model (tests/softbit_model.py).  The library's arithmetic contract holds: built with
// -ffp-contract=off, every fused operation an explicit fmaf.  The one quotient is a Newton iteration written out in fmaf: the `/` of the
// two compilers is not relied on (channel_core.h says why).  Error bounds: DESIGN.md 4.23.
//
// The normalised policy divides every DQPSK product d = X_i conj(X_{i+1}) by max(|re d|, |im d|): a carrier in a fade weighs as much as
// one at the channel's peak.  The weighted policy keeps |d| -- the channel state of the carrier -- and scales the whole frame by ONE
// factor k taken from the time-domain power P of the frame's phase reference symbol:
//     k = level * 1536 / (2048 * P)
// 2048 P / 1536 is, by Parseval, the mean carrier power of that symbol and so the mean of |d| to first order: a component of mean
// size lands at +-level.
#pragma once
#include <stdint.h>

#include "dabgpu_host_logic.h"

namespace dabgpu {

constexpr int SB_PRS_SAMPLES = 2048;         // the useful part of symbol 0: samples 504 .. 2551 of the frame
constexpr int SB_LANES = 256, SB_LANE_SAMPLES = 8, SB_WAVE = 64;

DABGPU_HD inline uint32_t sb_float_bits(float x) { uint32_t b; __builtin_memcpy(&b, &x, 4); return b; }
DABGPU_HD inline float sb_bits_float(uint32_t b) { float x; __builtin_memcpy(&x, &b, 4); return x; }

DABGPU_HD inline bool sb_level_ok(float level) { return level >= 1.0f && level <= 127.0f; }       // (false for NaN)

// ---- frame power: ONE tree, whatever the run length, the loader and the workgroup ----
// Lane l of 256 owns the eight samples the demodulator's loader hands that lane for a symbol: j = 0 .. 7 -> useful sample
// 2 l + 512 (j / 2) + (j mod 2).  Its partial sum is one chain in that order: re0 * re0, then fmaf(im, im, .), fmaf(re, re, .), ...
DABGPU_HD inline int sb_lane_sample(int lane, int j) { return 2 * lane + 512 * (j >> 1) + (j & 1); }
DABGPU_HD inline float sb_power_first(float re, float im) { return __builtin_fmaf(im, im, re * re); }
DABGPU_HD inline float sb_power_next(float acc, float re, float im) { return __builtin_fmaf(im, im, __builtin_fmaf(re, re, acc)); }
// Lanes 64 w .. 64 w + 63 (one wavefront) fold pairwise, partner distance 32, 16, 8, 4, 2, 1: a[i] + a[i + h] for i < h.  The four
// results w0 .. w3 end as (w0 + w1) + (w2 + w3).
DABGPU_HD inline float sb_power_join(float w0, float w1, float w2, float w3) { return (w0 + w1) + (w2 + w3); }

// the whole tree over 2048 complex samples in memory (re, im interleaved): the host's form, and the definition the kernel is tested against
inline float sb_frame_power(const float* prs) {
    float a[SB_LANES];
    for (int l = 0; l < SB_LANES; l++) {
        const float* s0 = prs + 2 * sb_lane_sample(l, 0);
        float acc = sb_power_first(s0[0], s0[1]);
        for (int j = 1; j < SB_LANE_SAMPLES; j++) { const float* s = prs + 2 * sb_lane_sample(l, j); acc = sb_power_next(acc, s[0], s[1]); }
        a[l] = acc;
    }
    for (int w = 0; w < SB_LANES; w += SB_WAVE)
        for (int h = SB_WAVE / 2; h >= 1; h >>= 1)
            for (int i = 0; i < h; i++) a[w + i] = a[w + i] + a[w + i + h];
    return sb_power_join(a[0], a[SB_WAVE], a[2 * SB_WAVE], a[3 * SB_WAVE]);
}

// ---- scale ----
// k = (level * 1536) / (2048 * P).  The denominator is split through its exponent field (exact) into m 2^e, m in [1, 2); 1 / m comes
// from a linear seed (within 1/17) by three Newton steps, the quotient q = num / m from one residual correction (within 1 ulp of the
// exact quotient); k = (q * 2^-a) * 2^-(e - a) with a = e / 2 -- the first product is exact, the second rounds once where it overflows.
// P zero, NaN or infinite, a denominator that is infinite or below the normal range (k would be beyond 2^136), k not finite: k = 0,
// the frame is erased.
DABGPU_HD inline float sb_scale(float level, float P) {
    if (!(P > 0.0f) || !(P <= 3.40282347e+38f)) return 0.0f;
    const float num = level * 1536.0f;
    const float den = 2048.0f * P;
    if (!(den <= 3.40282347e+38f) || !(den >= 1.17549435e-38f)) return 0.0f;
    const uint32_t b = sb_float_bits(den);
    const int e = (int)(b >> 23) - 127;                                            // -126 .. 127
    const float m = sb_bits_float((b & 0x007FFFFFu) | 0x3F800000u);
    float r = __builtin_fmaf(-0.470588235f, m, 1.41176471f);
    r = __builtin_fmaf(r, __builtin_fmaf(-m, r, 1.0f), r);
    r = __builtin_fmaf(r, __builtin_fmaf(-m, r, 1.0f), r);
    r = __builtin_fmaf(r, __builtin_fmaf(-m, r, 1.0f), r);
    float q = num * r;
    q = __builtin_fmaf(__builtin_fmaf(-m, q, num), r, q);
    const int a = e / 2;
    const float k = (q * sb_bits_float((uint32_t)(127 - a) << 23)) * sb_bits_float((uint32_t)(127 - (e - a)) << 23);
    return (k <= 3.40282347e+38f) ? k : 0.0f;
}

// ---- soft bit ----
// v = -(c * k), c = +re d for the first bit of a carrier and -im d for the second (the signs of to_vbit, ofdm_device.h); NaN -> 0,
// clamped to [-127, 127], truncated towards zero: -128 never leaves.  One body for host and device: the NaN is selected away and the
// value clamped BEFORE the conversion, so the conversion only ever sees a number in [-127, 127] and is defined C++ (an erased frame
// produces inf * 0 = NaN on purpose).
DABGPU_HD inline int sb_quantise(float v) {
    const float w = (v == v) ? v : 0.0f;
    const float c = w < -127.0f ? -127.0f : (w > 127.0f ? 127.0f : w);
    return (int)c;
}
DABGPU_HD inline int sb_soft_bit(float c, float k) { return sb_quantise(-(c * k)); }

}  // namespace dabgpu
