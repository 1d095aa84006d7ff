// dab/tx/dab_packet_encoder.h -- one packet-mode sub-channel's encoder with FEC on the device (include/dabgpu.h, "MSC packet mode"): data
// groups in, logical frames out, block by block.  The inverse of MSC_Reed_Solomon_Data_Packet_Processor + MSC_Data_Packet_Processor; the
// reference has no encoder, the class follows DABPlus_SuperFrame_Encoder beside it.  It keeps the stream position and the continuity index
// between blocks, and the bytes of a logical frame a block left unfinished.  A convenience over dabgpu_packet_tx_layout +
// dabgpu_packet_tx_encode_host_sync, no throughput path.
#pragma once
#include <cstdint>
#include <vector>

#include "dabgpu.h"
#include "utility/span.h"

class DAB_Packet_Encoder {
public:
    // address 1..1021, packet_length 24/48/72/96, frame_bytes = the sub-channel's bytes per CIF (a multiple of 24, >= packet_length)
    DAB_Packet_Encoder(uint32_t address, uint32_t packet_length, uint32_t frame_bytes);
    // why the last EncodeBlock returned false: DABGPU_PACKET_TX_* (0 after a success)
    int GetLastStatus() const { return m_status; }
    // n_fec_frames FEC frames from as many whole groups as fit (the rest of the block is padding packets): *groups_consumed of them are in;
    // the whole logical frames the stream now holds are APPENDED to `frames` (a trailing partial frame waits for the next block)
    bool EncodeBlock(tcb::span<const tcb::span<const uint8_t>> groups, int n_fec_frames, size_t* groups_consumed, std::vector<uint8_t>& frames);
    // the unfinished logical frame, zero padded: appends it to `frames` and starts the next block on a frame boundary
    void Flush(std::vector<uint8_t>& frames);
private:
    uint32_t m_address, m_packet_length, m_frame_bytes;
    uint64_t m_start_byte = 0;
    uint32_t m_continuity_index = 0;
    int m_status = 0;
    std::vector<uint8_t> m_partial;      // the bytes of the logical frame that holds m_start_byte
};
