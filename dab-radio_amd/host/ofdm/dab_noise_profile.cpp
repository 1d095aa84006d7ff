// ofdm/dab_noise_profile.cpp -- over dabgpu_noise_profile_host_sync
#include "./dab_noise_profile.h"

#include <stdexcept>
#include <string>

#include "../dab/dabgpu_shared_context.h"

DAB_Noise_Profile::DAB_Noise_Profile() : m_ctx(dabgpu_shared_context()) {}

bool DAB_Noise_Profile::Update(tcb::span<const std::complex<float>> null_symbol, int fine_time_offset, float freq_offset, tcb::span<float> out_weights) {
    if (fine_time_offset < 0 || fine_time_offset > 1543 || null_symbol.size() < NB_SAMPLES + (size_t)fine_time_offset || out_weights.size() != NB_BANDS)
        return false;
    uint32_t valid = 0;
    const int st = dabgpu_noise_profile_host_sync(m_ctx, reinterpret_cast<const float*>(null_symbol.data()), null_symbol.size(), 0, freq_offset,
                                                  fine_time_offset, m_any_excluded ? m_exclude.data() : nullptr, m_profile.data(), m_alpha,
                                                  out_weights.data(), &m_mean, nullptr, &valid);
    if (st != DABGPU_OK) throw std::runtime_error(std::string("DAB_Noise_Profile: ") + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
    m_valid = valid != 0;
    return true;
}

bool DAB_Noise_Profile::SetExcluded(tcb::span<const uint8_t> main_ids, tcb::span<const uint8_t> sub_ids) {
    if (main_ids.size() != sub_ids.size()) return false;
    std::array<uint32_t, DABGPU_NOISE_PROFILE_EXCLUDE_WORDS> words{};
    if (dabgpu_noise_profile_exclude_tii(main_ids.data(), sub_ids.data(), (int)main_ids.size(), words.data()) != DABGPU_OK) return false;
    m_exclude = words;
    m_any_excluded = !main_ids.empty();
    return true;
}

bool DAB_Noise_Profile::SetAlpha(float alpha) {
    if (!(alpha > 0.0f && alpha <= 1.0f)) return false;
    m_alpha = alpha;
    return true;
}

void DAB_Noise_Profile::Reset() {
    m_profile.fill(0.0f);
    m_valid = false;
    m_mean = 0.0f;
}
