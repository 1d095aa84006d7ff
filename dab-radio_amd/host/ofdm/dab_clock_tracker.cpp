// ofdm/dab_clock_tracker.cpp -- over dabgpu_clock_track_host_sync
#include "./dab_clock_tracker.h"

#include <stdexcept>
#include <string>

#include "../dab/dabgpu_shared_context.h"

static bool gain_ok(float gain) { return gain > 0.0f && gain <= 1.0f; }

DAB_Clock_Tracker::DAB_Clock_Tracker(float gain) : m_ctx(dabgpu_shared_context()), m_gain(gain) {
    if (!gain_ok(gain)) throw std::invalid_argument("DAB_Clock_Tracker: gain outside (0, 1]");
}

bool DAB_Clock_Tracker::SetGain(float gain) {
    if (!gain_ok(gain)) return false;
    m_gain = gain;
    return true;
}

bool DAB_Clock_Tracker::Track(tcb::span<std::complex<float>> products) {
    if (products.size() != NB_PRODUCTS) return false;
    uint32_t valid = 0;
    float* const p = reinterpret_cast<float*>(products.data());
    const int st = dabgpu_clock_track_host_sync(m_ctx, p, p, &m_slope, m_gain, m_corr, &valid);
    if (st != DABGPU_OK) throw std::runtime_error(std::string("DAB_Clock_Tracker: ") + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
    m_valid = valid != 0;
    return m_valid;
}
