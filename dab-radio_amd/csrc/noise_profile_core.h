// noise_profile_core.h -- the arithmetic of the noise profile behind the transform (include/dabgpu.h, "Noise profile": bands, exclusion,
// smoothing, mean, weights) and of the band weights in the combiner, host and device: the kernels (noise_profile.hip, diversity.hip), the
// host forms (dabgpu_noise_profile_bands_host, dabgpu_diversity_band_mean_host) and the host model of the tests
// (tests/cpp/noise_profile_host_model.cpp) compile these same statements, so the device is checked bit for bit against a CPU run of this
// file, and this file against an independent numpy model (tests/noise_profile_model.py).  The library's arithmetic contract holds:
// -ffp-contract=off, the one fused step an explicit fmaf, sums in a written order, no `/` at run time (R[n] are constants).  The power
// is tii_core.h's, the reciprocal and the test of a weight diversity_core.h's; nothing of either is restated here.
#pragma once
#include <stdint.h>

#include "diversity_core.h"
#include "tii_core.h"

namespace dabgpu {

constexpr int NP_BANDS = DABGPU_NOISE_PROFILE_BANDS, NP_BAND_CARRIERS = DABGPU_NOISE_PROFILE_BAND_CARRIERS, NP_CARRIERS = 1536;
constexpr int NP_EXCLUDE_WORDS = DABGPU_NOISE_PROFILE_EXCLUDE_WORDS, NP_HALF = 64;
constexpr int NP_NULL = 2656;                        // what one frame's profile may read from the NULL's first sample on
static_assert(NP_BANDS * NP_BAND_CARRIERS == NP_CARRIERS && NP_EXCLUDE_WORDS * 32 == NP_CARRIERS && NP_BANDS == 2 * NP_HALF, "128 bands of 12");
constexpr float NP_WEIGHT_CAP = 0x1p-20f;            // w_b = 1 / max(n_b, M * 2^-20): a band weighs at most 60 dB above the mean

// step 1: the bin of carrier c in the order of d_dqpsk (c < 768: carriers -768 .. -1; c >= 768: carriers 1 .. 768)
DABGPU_HD inline int np_carrier_bin(int c) { return c < 768 ? 1280 + c : c - 767; }
// carrier k of -768 .. 768 (not 0) in that order
DABGPU_HD inline int np_carrier_index(int k) { return k < 0 ? k + 768 : k + 767; }

// R[n], n = 1 .. 12: the float nearest 1 / n (a constant of the compiler, correctly rounded; tests/test_noise_profile_model.py checks each)
DABGPU_HD inline float np_count_reciprocal(int n) {
    switch (n) {
        case 1: return 1.0f;
        case 2: return 0.5f;
        case 3: return 1.0f / 3.0f;
        case 4: return 0.25f;
        case 5: return 1.0f / 5.0f;
        case 6: return 1.0f / 6.0f;
        case 7: return 1.0f / 7.0f;
        case 8: return 0.125f;
        case 9: return 1.0f / 9.0f;
        case 10: return 1.0f / 10.0f;
        case 11: return 1.0f / 11.0f;
        default: return 1.0f / 12.0f;
    }
}

// step 3: bit i = carrier 12 b + i of band b is excluded (no table: none).  A band's twelve bits lie in at most two words.
DABGPU_HD inline uint32_t np_band_mask(const uint32_t* exclude, int b) {
    if (exclude == nullptr) return 0u;
    const int c0 = NP_BAND_CARRIERS * b, w = c0 >> 5, sh = c0 & 31;
    const uint64_t lo = exclude[w], hi = exclude[w + 1 < NP_EXCLUDE_WORDS ? w + 1 : w];
    return (uint32_t)(((hi << 32) | lo) >> sh) & 0xFFFu;
}

// step 2: m_b from the carrier powers, C(c) -> float.  All twelve excluded: the mask is ignored.
template <class Power>
DABGPU_HD inline float np_band_measure(Power C, int b, uint32_t mask) {
    if (mask == 0xFFFu) mask = 0u;
    float sum = 0.0f;
    int count = 0;
    for (int i = 0; i < NP_BAND_CARRIERS; i++) {
        if ((mask >> i) & 1u) continue;
        const float p = C(NP_BAND_CARRIERS * b + i);
        sum = count ? sum + p : p;
        count++;
    }
    return (sum * np_count_reciprocal(count)) * 0x1p-11f;
}

DABGPU_HD inline bool np_alpha_ok(float alpha) { return alpha > 0.0f && alpha <= 1.0f; }       // (false for NaN)
// step 4 (has_prev: a previous profile was given)
DABGPU_HD inline float np_smooth(float m, bool has_prev, float p, float alpha) {
    return (has_prev && dv_positive_finite(p)) ? __builtin_fmaf(alpha, m - p, p) : m;
}

// step 5 and the combiner's branch weight: the mean of 128 values from the sums of its halves (each half the wavefront tree)
DABGPU_HD inline float np_mean_join(float s0, float s1) { return (s0 + s1) * 0x1p-7f; }
// the wavefront tree over 64 values in memory: a[i] + a[i + h] for i < h, h = 32, 16, 8, 4, 2, 1 (softbit_csi_core.h's)
inline float np_half_tree(const float* v) {
    float a[NP_HALF];
    for (int i = 0; i < NP_HALF; i++) a[i] = v[i];
    for (int h = NP_HALF / 2; h >= 1; h >>= 1)
        for (int i = 0; i < h; i++) a[i] = a[i] + a[i + h];
    return a[0];
}
inline float np_mean128(const float* v) { return np_mean_join(np_half_tree(v), np_half_tree(v + NP_HALF)); }

// a normal positive finite mean (false for NaN): the frame is valid
DABGPU_HD inline bool np_mean_ok(float M) { return M >= 1.17549435e-38f && M <= 3.40282347e+38f; }
DABGPU_HD inline float np_weight(float n, float M) {
    const float cap = M * NP_WEIGHT_CAP;
    return dv_reciprocal(n > cap ? n : cap);
}

// the combiner: a band weight that is not positive and finite counts as 0, in the branch's mean and in the sum
DABGPU_HD inline float np_clean_weight(float w) { return dv_positive_finite(w) ? w : 0.0f; }
inline float np_branch_weight(const float* band_weight) {
    float c[NP_BANDS];
    for (int b = 0; b < NP_BANDS; b++) c[b] = np_clean_weight(band_weight[b]);
    return np_mean128(c);
}

// steps 2 to 5 of one frame on the host from its 1536 carrier powers; every output may be null, profile_out may be profile_in.
// False: the frame is skipped -- weights and mean 0, the profile unchanged (0 without a previous one).
inline bool np_frame_bands(const float* C, const uint32_t* exclude, const float* profile_in, float alpha, float* profile_out, float* band_weight,
                           float* mean_noise) {
    float n[NP_BANDS];
    for (int b = 0; b < NP_BANDS; b++) {
        const float m = np_band_measure([&](int c) { return C[c]; }, b, np_band_mask(exclude, b));
        n[b] = np_smooth(m, profile_in != nullptr, profile_in ? profile_in[b] : 0.0f, alpha);
    }
    const float M = np_mean128(n);
    const bool ok = np_mean_ok(M);
    for (int b = 0; b < NP_BANDS; b++) {
        const float keep = profile_in ? profile_in[b] : 0.0f;
        if (profile_out) profile_out[b] = ok ? n[b] : keep;
        if (band_weight) band_weight[b] = ok ? np_weight(n[b], M) : 0.0f;
    }
    if (mean_noise) *mean_noise = ok ? M : 0.0f;
    return ok;
}

}  // namespace dabgpu
