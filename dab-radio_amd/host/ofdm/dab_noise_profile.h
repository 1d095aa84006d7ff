// ofdm/dab_noise_profile.h -- the noise profile of one mode I receiver (include/dabgpu.h, "Noise profile"): every frame's NULL symbol
// becomes the noise power of 128 bands of 12 carriers, smoothed from frame to frame, and the bands' maximal-ratio weights, which is what
// DAB_Diversity_Combiner::Combine takes as a branch's band weights.  The reference has no such stage; the class follows the conventions
// of the other added classes: spans in, false for wrong sizes, exceptions for device failures.  The state (the smoothed profile) is the
// object's: one object per receiver.
#pragma once
#include <array>
#include <complex>
#include <cstdint>

#include "dabgpu.h"
#include "utility/span.h"

struct dabgpu_ctx;

class DAB_Noise_Profile {
public:
    static constexpr size_t NB_SAMPLES = 2656;              // the NULL period
    static constexpr size_t NB_BANDS = DABGPU_NOISE_PROFILE_BANDS;
    DAB_Noise_Profile();
    // null_symbol: at least NB_SAMPLES + fine_time_offset samples, the NULL expected at its first sample and found fine_time_offset
    // (>= 0 here: nothing in front of the span can be read) samples later; freq_offset in cycles per sample, as the synchroniser reports
    // it.  false for a span that is too short or an offset outside [0, 1543].  true: out_weights holds the 128 band weights -- all zero,
    // with IsValid() false and the state kept, for a frame without a usable NULL.
    bool Update(tcb::span<const std::complex<float>> null_symbol, int fine_time_offset, float freq_offset, tcb::span<float> out_weights);
    // the carriers of these transmitters are left out of their bands; false (and nothing changes) for an id out of range
    bool SetExcluded(tcb::span<const uint8_t> main_ids, tcb::span<const uint8_t> sub_ids);
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
