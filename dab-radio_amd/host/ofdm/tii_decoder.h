// ofdm/tii_decoder.h -- TII_Decoder: the transmitter identification of mode I (include/dabgpu.h, "TII") for one receiver, over the
// MI355X C ABI (dabgpu_tii_bank_process_host_sync).  The reference has no such class; its GUI stops at plotting the NULL spectrum.
//   Process   null_region = samples that hold a NULL period: it begins at sample fine_time_offset of the span, and the 2048 samples from
//             608 samples into it must lie inside the span.  net_freq_offset = OFDM_Demod::GetNetFrequencyOffset() (cycles per sample).
//             Inside an On_OFDM_Frame observer OFDM_Demod::GetCorrelationTimeBuffer() begins with the NULL period that follows the
//             delivered frame, cut with that frame's timing already applied: there fine_time_offset is 0, whatever GetFineTimeOffset()
//             says about where the frame's PRS was found in ITS window.
//             The first DABGPU_TII_SETTLE_FRAMES calls after construction or Reset() are not accumulated (false is returned): the
//             synchroniser's record is up to half a carrier spacing off in the first frame after an acquisition.  So call Reset() whenever
//             the demodulator lost synchronisation (GetTotalFramesDesync() changed) or was retuned.
//             decide = true ends the call with a decision; GetRecords() then holds it (ascending sub id).
// A device failure or a span that does not hold the window throws std::runtime_error.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <complex>
#include <vector>
#include "utility/span.h"
#include "dabgpu.h"

class TII_Decoder
{
public:
    struct Record { int main_id; int sub_id; uint32_t mask; float strength; };   // main_id -1: `mask` is no pattern (two main ids on one comb)
private:
    dabgpu_tii_bank* m_bank = nullptr;
    float m_threshold;
    int m_frames_since_reset = 0;
    int m_total_frames = 0;
    std::vector<Record> m_records;
    void Create();
public:
    explicit TII_Decoder(int transmission_mode = 1, float threshold = DABGPU_TII_DEFAULT_THRESHOLD);
    ~TII_Decoder();
    TII_Decoder(const TII_Decoder&) = delete;
    TII_Decoder& operator=(const TII_Decoder&) = delete;
    bool Process(tcb::span<const std::complex<float>> null_region, float net_freq_offset, int fine_time_offset, bool decide);
    void Reset();
    int GetTotalFrames() const { return m_total_frames; }                          // accumulated since the last Reset()
    tcb::span<const Record> GetRecords() const { return m_records; }               // of the last decision
};
