// dab/tx/dab_packet_encoder.cpp -- see the header.
#include "./dab_packet_encoder.h"

#include <stdexcept>
#include <string>

#include "dab/dabgpu_shared_context.h"

DAB_Packet_Encoder::DAB_Packet_Encoder(uint32_t address, uint32_t packet_length, uint32_t frame_bytes)
    : m_address(address), m_packet_length(packet_length), m_frame_bytes(frame_bytes) {}

bool DAB_Packet_Encoder::EncodeBlock(tcb::span<const tcb::span<const uint8_t>> groups, int n_fec_frames, size_t* groups_consumed,
                                     std::vector<uint8_t>& frames) {
    if (groups_consumed) *groups_consumed = 0;
    if (n_fec_frames <= 0) { m_status = 0; return n_fec_frames == 0; }
    std::vector<uint32_t> lens(groups.size());
    std::vector<uint64_t> offs(groups.size() + 1, 0);
    std::vector<uint8_t> data;
    for (size_t g = 0; g < groups.size(); g++) {
        lens[g] = (uint32_t)groups[g].size();
        offs[g] = data.size();
        data.insert(data.end(), groups[g].begin(), groups[g].end());
    }
    const size_t K = (size_t)n_fec_frames;
    std::vector<dabgpu_packet_tx_entry> table(94 * K);
    std::vector<uint32_t> first(K + 1);
    size_t consumed = 0;
    uint64_t end_start = 0;
    uint32_t end_ci = 0;
    m_status = dabgpu_packet_tx_layout(lens.data(), lens.size(), m_address, m_packet_length, m_frame_bytes, m_start_byte, m_continuity_index, n_fec_frames,
                                       table.data(), table.size(), first.data(), &consumed, &end_start, &end_ci);
    if (m_status != 0) return false;
    const size_t lead = (size_t)(m_start_byte % m_frame_bytes);
    const size_t n_logical = (lead + K * 2472 + m_frame_bytes - 1) / m_frame_bytes;
    std::vector<uint8_t> out(n_logical * m_frame_bytes, 0);
    std::copy(m_partial.begin(), m_partial.end(), out.begin());                  // what the last block left of the first frame
    std::vector<int32_t> status(K, 0);
    data.push_back(0);
    const int st = dabgpu_packet_tx_encode_host_sync(dabgpu_shared_context(), n_fec_frames, data.data(), data.size() - 1, offs.data(), groups.size(),
                                                     table.data(), first.data(), m_address, m_frame_bytes, m_start_byte, out.data(), status.data());
    if (st != DABGPU_OK) throw std::runtime_error(std::string("DAB_Packet_Encoder: ") + dabgpu_strerror(st) + " -- " + dabgpu_last_error());
    for (int32_t s : status) if (s != 0) { m_status = s; return false; }
    const size_t filled = lead + K * 2472, whole = filled / m_frame_bytes;
    frames.insert(frames.end(), out.begin(), out.begin() + (ptrdiff_t)(whole * m_frame_bytes));
    m_partial.assign(out.begin() + (ptrdiff_t)(whole * m_frame_bytes), out.begin() + (ptrdiff_t)filled);
    m_start_byte = end_start;
    m_continuity_index = end_ci;
    if (groups_consumed) *groups_consumed = consumed;
    return true;
}

void DAB_Packet_Encoder::Flush(std::vector<uint8_t>& frames) {
    if (m_partial.empty()) return;
    const size_t rest = m_frame_bytes - m_partial.size();
    frames.insert(frames.end(), m_partial.begin(), m_partial.end());
    frames.insert(frames.end(), rest, (uint8_t)0);
    m_partial.clear();
    m_start_byte += rest;                                                       // (a multiple of 24: frame bytes and fill are)
}
