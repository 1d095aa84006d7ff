// noise_core.h -- the arithmetic of the noise estimator behind the transform (include/dabgpu.h, "Noise estimate"), host and device: the
// kernel (noise.hip), the host forms (dabgpu_noise_floor_host) and the host model of the tests (tests/cpp/noise_host_model.cpp) compile
// these same statements, so the device is checked bit for bit against a CPU run of this file, and this file against an independent
// float64 model (tests/noise_model.py).  The library's arithmetic contract holds: -ffp-contract=off, every fused step an explicit fmaf,
// sums in a written order, no `/`.  Power and fold are tii_core.h's, the frame power and its tree softbit_csi_core.h's; nothing of either
// is restated here.
#pragma once
#include <stdint.h>

#include "dabgpu_host_logic.h"
#include "softbit_csi_core.h"
#include "tii_core.h"

namespace dabgpu {

constexpr int NOISE_NULL = 2656;                     // the NULL period
constexpr int NOISE_PRS_USEFUL = NOISE_NULL + 504;   // the PRS's useful part behind the NULL's first sample: samples 504 .. 2551 of the frame
constexpr int NOISE_REACH = NOISE_NULL + 2552;       // what one frame's estimate may read from the NULL's first sample on

// N = F * NOISE_UNBIAS.  Under white noise of power s2 per complex sample a group is 2048 s2 times a Gamma(8, 1) draw and
// E[F] = 2048 s2 mu, mu = E[mean of the four smallest of eight such draws] = 5.982762381925 (tests/noise_model.py, by quadrature over
// the fifth order statistic; asserted there against this literal).  8 / (mu * 8 * 2048) = 8.161468211995e-05; the nearest float:
constexpr float NOISE_UNBIAS = 0x1.565118p-14f;      // 8.16146785e-05
constexpr float NOISE_RATIO_CAP = 0x1p-40f;          // weight = 1 / max(N, P * 2^-40): signal over noise is capped at 120 dB

DABGPU_HD inline bool noise_finite(float x) { return x >= -3.40282347e+38f && x <= 3.40282347e+38f; }       // (false for NaN)

// step 2: F from E[24][8], the detector's floor at one frame
DABGPU_HD inline float noise_floor(const float* E) {
    float share[TII_COMBS];
    for (int c = 0; c < TII_COMBS; c++) {
        float s[TII_GROUPS];
        tii_sort8(E + TII_GROUPS * c, s);
        share[c] = tii_comb_floor(s);
    }
    return tii_floor(share);
}

// 1 / x for a normal x > 0: x = m 2^e with m in [1, 2) through the exponent field (exact), 1 / m by tii_reciprocal (its seed and four
// Newton steps in fmaf), then (r 2^-a) 2^-(e - a) with a = e / 2 -- both products exact unless the result is below the normal range
// (x > 2^126), where the second rounds once.  Against the correctly rounded quotient: equal for all but one of the 2^23 mantissas, one
// unit in the last place off there (tests/test_noise_model.py walks all of them).
DABGPU_HD inline float noise_reciprocal(float x) {
    const uint32_t b = sb_float_bits(x);
    const int e = (int)(b >> 23) - 127;                                            // -126 .. 127
    const float r = tii_reciprocal(sb_bits_float((b & 0x007FFFFFu) | 0x3F800000u));
    const int a = e / 2;
    return (r * sb_bits_float((uint32_t)(127 - a) << 23)) * sb_bits_float((uint32_t)(127 - (e - a)) << 23);
}

// steps 3 and 5 from the floor F and the frame power P.  False: the frame is skipped and the record all zero -- P or N not finite, P not
// above 0, or max(N, P 2^-40) below the normal range (its reciprocal would not be a finite weight).
DABGPU_HD inline bool noise_finish(float F, float P, dabgpu_noise_record* out) {
    out->noise_power = 0.0f; out->signal_power = 0.0f; out->weight = 0.0f; out->snr = 0.0f; out->valid = 0u;
    const float N = F * NOISE_UNBIAS;
    if (!noise_finite(P) || !noise_finite(N) || !(P > 0.0f)) return false;
    const float cap = P * NOISE_RATIO_CAP;
    const float den = N > cap ? N : cap;
    if (!(den >= 1.17549435e-38f)) return false;
    const float w = noise_reciprocal(den);
    const float excess = P - N;
    out->noise_power = N;
    out->signal_power = P;
    out->weight = w;
    out->snr = (excess > 0.0f ? excess : 0.0f) * w;
    out->valid = 1u;
    return true;
}

}  // namespace dabgpu
