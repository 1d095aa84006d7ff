// dab/tx/dabplus_superframe_encoder.cpp -- see dabplus_superframe_encoder.h
#include "./dabplus_superframe_encoder.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "dab/dabgpu_shared_context.h"
#include "./dabgpu_tx_check.h"

static void check(int st, const char* what) { dabgpu_tx_check("DABPlus_SuperFrame_Encoder", st, what); }

DABPlus_SuperFrame_Encoder::DABPlus_SuperFrame_Encoder(uint32_t frame_bytes) : m_frame_bytes(frame_bytes) {
    dabgpu_tx_check_abi("DABPlus_SuperFrame_Encoder");
    if (frame_bytes < 24 || frame_bytes > 1536 || frame_bytes % 24)
        throw std::invalid_argument("DABPlus_SuperFrame_Encoder: " + std::to_string(frame_bytes) + " bytes per logical frame (a multiple of 24 in 24..1536)");
    (void)dabgpu_shared_context();                  // throws where there is no device
}

bool DABPlus_SuperFrame_Encoder::Encode(uint8_t descriptor, tcb::span<const tcb::span<const uint8_t>> access_units, tcb::span<uint8_t> out) {
    m_status = 0;
    const int dac_rate = (descriptor >> 6) & 1, sbr = (descriptor >> 5) & 1;
    const size_t num_aus = dac_rate ? (sbr ? 3 : 6) : (sbr ? 2 : 4);
    if (access_units.size() != num_aus || out.size() != 5 * (size_t)m_frame_bytes) { std::fill(out.begin(), out.end(), (uint8_t)0); return false; }
    uint16_t au_len[6] = {};
    m_au_bytes.clear();
    for (size_t a = 0; a < num_aus; a++) {
        if (access_units[a].size() > 0xFFFF) { m_status = DABGPU_DABPLUS_TX_BAD_FILL; std::fill(out.begin(), out.end(), (uint8_t)0); return false; }
        au_len[a] = (uint16_t)access_units[a].size();
        m_au_bytes.insert(m_au_bytes.end(), access_units[a].begin(), access_units[a].end());
    }
    m_au_bytes.push_back(0);                        // (never read: keeps the pointer non-null for empty units)
    const uint64_t offset = 0;
    int32_t status = 0;
    check(dabgpu_dabplus_tx_encode_host_sync(dabgpu_shared_context(), 1, m_au_bytes.data(), &offset, au_len, &descriptor, m_frame_bytes, out.data(), &status),
          "dabgpu_dabplus_tx_encode_host_sync");
    m_status = status;
    return status == 0;
}
