// ofdm/dab_noise_estimator.cpp -- over dabgpu_noise_estimate_host_sync
#include "./dab_noise_estimator.h"

#include <stdexcept>
#include <string>

#include "../dab/dabgpu_shared_context.h"

DAB_Noise_Estimator::DAB_Noise_Estimator() : m_ctx(dabgpu_shared_context()) {}

bool DAB_Noise_Estimator::Estimate(tcb::span<const std::complex<float>> null_and_prs, float freq_offset, int fine_time_offset, dabgpu_noise_record& out) {
    out = dabgpu_noise_record{};
    if (fine_time_offset < 0 || fine_time_offset > 1543 || null_and_prs.size() < NB_SAMPLES + (size_t)fine_time_offset) return false;
    const int st = dabgpu_noise_estimate_host_sync(m_ctx, reinterpret_cast<const float*>(null_and_prs.data()), null_and_prs.size(), 0, freq_offset,
                                                   fine_time_offset, &out);
    if (st != DABGPU_OK) throw std::runtime_error(std::string("DAB_Noise_Estimator: ") + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
    return true;
}
