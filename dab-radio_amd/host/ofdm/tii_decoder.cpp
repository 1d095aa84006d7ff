// ofdm/tii_decoder.cpp -- see tii_decoder.h.
#include "./tii_decoder.h"

#include <stdexcept>
#include <string>

#include "dab/dabgpu_shared_context.h"

static void tii_fail(const char* what, int st) {
    throw std::runtime_error(std::string("TII_Decoder: ") + what + ": " + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
}

TII_Decoder::TII_Decoder(int transmission_mode, float threshold) : m_threshold(threshold) {
    if (transmission_mode != 1) throw std::runtime_error("TII_Decoder: TII is defined for transmission mode I only");
    Create();
}

void TII_Decoder::Create() {
    dabgpu_tii_cfg cfg;
    dabgpu_tii_cfg_default(&cfg);
    cfg.threshold = m_threshold;
    const int st = dabgpu_tii_bank_create(dabgpu_shared_context(), 1, &cfg, &m_bank);
    if (st != DABGPU_OK) tii_fail("dabgpu_tii_bank_create", st);
}

TII_Decoder::~TII_Decoder() { dabgpu_tii_bank_destroy(m_bank); }

// (a new bank: the host form owns the context's stream, so there is no stream of the caller's to clear the old one on)
void TII_Decoder::Reset() {
    dabgpu_tii_bank_destroy(m_bank);
    m_bank = nullptr;
    m_frames_since_reset = 0;
    m_total_frames = 0;
    m_records.clear();
    Create();
}

bool TII_Decoder::Process(tcb::span<const std::complex<float>> null_region, float net_freq_offset, int fine_time_offset, bool decide) {
    if (m_frames_since_reset < DABGPU_TII_SETTLE_FRAMES) { m_frames_since_reset++; return false; }
    dabgpu_tii_record rec[DABGPU_TII_COMBS];
    uint32_t count = 0;
    const int st = dabgpu_tii_bank_process_host_sync(m_bank, reinterpret_cast<const float*>(null_region.data()), null_region.size(), 0, net_freq_offset,
                                                     fine_time_offset, decide ? 1 : 0, rec, &count);
    if (st != DABGPU_OK) tii_fail("dabgpu_tii_bank_process_host_sync", st);
    m_frames_since_reset++;
    m_total_frames++;
    if (decide) {
        m_records.clear();
        for (uint32_t k = 0; k < count && k < DABGPU_TII_COMBS; k++) m_records.push_back({rec[k].main_id, rec[k].sub_id, rec[k].mask, rec[k].strength});
    }
    return true;
}
