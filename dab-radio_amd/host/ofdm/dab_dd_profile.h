// ofdm/dab_dd_profile.h -- the decision-directed noise profile of one mode I receiver (include/dabgpu.h, "Decision-directed noise
// profile"): every frame's own DQPSK products become the noise power of 128 bands of 12 carriers, smoothed from frame to frame, and the
// bands' maximal-ratio weights, which is what DAB_Diversity_Combiner::Combine takes as a branch's band weights.  It stands where
// DAB_Noise_Profile stands and is shaped like it, for interferers that the NULL symbol does not show (gated, TDMA).  The reference has
// no such stage; the class follows the conventions of the other added classes: spans in, false for wrong sizes, exceptions for device
// failures.  The state (the smoothed profile) is the object's: one object per receiver.
#pragma once
#include <array>
#include <complex>
#include <cstdint>

#include "dabgpu.h"
#include "utility/span.h"

struct dabgpu_ctx;

class DAB_DD_Profile {
public:
    static constexpr size_t NB_PRODUCTS = 75 * 1536;        // one frame's products, symbol after symbol in carrier order
    static constexpr size_t NB_BANDS = DABGPU_NOISE_PROFILE_BANDS;
    DAB_DD_Profile();
    // products: the frame's NB_PRODUCTS products (OFDM_Demod's DQPSK view, a branch's d_dqpsk).  false for a span of another size.
    // true: out_weights holds the 128 band weights -- all zero, with IsValid() false and the state kept, for a frame without a usable
    // measurement.
    bool Update(tcb::span<const std::complex<float>> products, tcb::span<float> out_weights);
    // 48 words, bit c mod 32 of word c / 32 set: carrier c is left out of its band; an empty span: none.  false (and nothing changes)
    // for any other size
    bool SetExclude(tcb::span<const uint32_t> words);
    bool SetAlpha(float alpha);                             // (0, 1]; false (and nothing changes) for any other value
    void Reset();                                           // forget the profile: the next frame starts it again
    bool IsValid() const { return m_valid; }                // of the last Update
    float GetMeanNoise() const { return m_mean; }           // M of the last Update (0: skipped)
    tcb::span<const float> GetProfile() const { return {m_profile.data(), m_profile.size()}; }

private:
    dabgpu_ctx* m_ctx;
    std::array<float, NB_BANDS> m_profile{};
    std::array<uint32_t, DABGPU_NOISE_PROFILE_EXCLUDE_WORDS> m_exclude{};
    bool m_any_excluded = false, m_valid = false;
    float m_alpha = 1.0f, m_mean = 0.0f;
};
