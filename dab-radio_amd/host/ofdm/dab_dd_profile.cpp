// ofdm/dab_dd_profile.cpp -- over dabgpu_dd_profile_host_sync
#include "./dab_dd_profile.h"

#include <stdexcept>
#include <string>

#include "../dab/dabgpu_shared_context.h"

DAB_DD_Profile::DAB_DD_Profile() : m_ctx(dabgpu_shared_context()) {}

bool DAB_DD_Profile::Update(tcb::span<const std::complex<float>> products, tcb::span<float> out_weights) {
    if (products.size() != NB_PRODUCTS || out_weights.size() != NB_BANDS) return false;
    uint32_t valid = 0;
    const int st = dabgpu_dd_profile_host_sync(m_ctx, reinterpret_cast<const float*>(products.data()), m_any_excluded ? m_exclude.data() : nullptr,
                                               m_profile.data(), m_alpha, out_weights.data(), &m_mean, nullptr, nullptr, &valid);
    if (st != DABGPU_OK) throw std::runtime_error(std::string("DAB_DD_Profile: ") + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
    m_valid = valid != 0;
    return true;
}

bool DAB_DD_Profile::SetExclude(tcb::span<const uint32_t> words) {
    if (!words.empty() && words.size() != m_exclude.size()) return false;
    m_any_excluded = false;
    for (size_t i = 0; i < words.size(); i++) {
        m_exclude[i] = words[i];
        m_any_excluded = m_any_excluded || words[i] != 0u;
    }
    return true;
}

bool DAB_DD_Profile::SetAlpha(float alpha) {
    if (!(alpha > 0.0f && alpha <= 1.0f)) return false;
    m_alpha = alpha;
    return true;
}

void DAB_DD_Profile::Reset() {
    m_profile.fill(0.0f);
    m_valid = false;
    m_mean = 0.0f;
}
