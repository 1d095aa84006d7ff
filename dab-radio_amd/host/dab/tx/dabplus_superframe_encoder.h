// dab/tx/dabplus_superframe_encoder.h -- one DAB+ sub-channel's super-frame encoder on the device (include/dabgpu.h, "DAB+ super-frame
// encoder"): the access units of a super frame -> its five logical frames, ETSI TS 102 563 clauses 5.2 and 6.  The inverse of
// AAC_Frame_Processor (dab/audio/aac_frame_processor.h); the reference has no encoder, the class follows the conventions of
// DAB_Channel_Encoder beside it: spans in, false where nothing could be encoded, exceptions for device failures.  Stateless between calls.
// A convenience over dabgpu_dabplus_tx_encode_host_sync -- one staged copy up, one launch, copies down and a synchronise per super frame --
// and no throughput path: many streams or super frames per call are what dabgpu_dabplus_tx_encode is for.
#pragma once
#include <cstdint>
#include <vector>

#include "dabgpu.h"
#include "utility/span.h"

class DABPlus_SuperFrame_Encoder {
public:
    // bytes per logical frame = the sub-channel's bytes per CIF: a multiple of 24 in 24..1536
    explicit DABPlus_SuperFrame_Encoder(uint32_t frame_bytes);
    uint32_t GetFrameBytes() const { return m_frame_bytes; }
    // why the last Encode returned false: DABGPU_DABPLUS_TX_BAD_* (0 after a success or a wrong buffer size)
    int GetLastStatus() const { return m_status; }
    // descriptor = byte 2 of the super frame; access_units = the payloads without CRCs, as many as (dac_rate, sbr_flag) announce;
    // out [5 * GetFrameBytes()].  false, with `out` (whatever its size) zeroed: wrong number of units or wrong size of `out` (GetLastStatus()
    // = 0, no device call), or lengths the super frame cannot hold (GetLastStatus() = the DABGPU_DABPLUS_TX_BAD_* code)
    bool Encode(uint8_t descriptor, tcb::span<const tcb::span<const uint8_t>> access_units, tcb::span<uint8_t> out);
private:
    uint32_t m_frame_bytes;
    int m_status = 0;
    std::vector<uint8_t> m_au_bytes;
};
