// dab/quality/dab_channel_ber.h -- the channel ("pre-Viterbi") bit error rate of decoded code words (include/dabgpu.h, "Channel BER"):
// the decoded bytes are encoded again on the device and compared with the hard decisions of the soft bits the decoder consumed.  The
// reference reports no signal quality; the class follows the conventions of the other added classes: spans in, false for wrong buffer
// sizes, exceptions for device failures.  It sits BESIDE the decoder classes, which stay as they are: hand it what FIC_Decoder /
// MSC_Decoder were given (a FIB group's soft bits, a sub-channel's de-interleaved CIF) and what they delivered.
#pragma once
#include <cstdint>

#include "dabgpu.h"
#include "utility/span.h"
#include "viterbi_config.h"

struct dabgpu_ctx;

class DAB_Channel_BER {
public:
    DAB_Channel_BER();
    // one FIB group: 2304 soft bits, the 96 decoded bytes (3 x (30 + the received CRC)) as FIC_Decoder holds them
    bool MeasureFIBGroup(tcb::span<const viterbi_bit_t> encoded_bits, tcb::span<const uint8_t> decoded_bytes, dabgpu_ber_result& out);
    // one CIF of a sub-channel: its length x 64 de-interleaved soft bits (CIF_Deinterleaver's output) and the bytes MSC_Decoder returned
    bool MeasureSubchannel(const dabgpu_subchannel& subchannel, tcb::span<const viterbi_bit_t> deinterleaved_bits,
                           tcb::span<const uint8_t> decoded_bytes, dabgpu_ber_result& out);
    // running totals over every code word measured since the last Reset
    uint64_t GetTotalBits() const { return m_bits; }
    uint64_t GetTotalErrors() const { return m_errors; }
    double GetBitErrorRate() const { return m_bits ? (double)m_errors / (double)m_bits : 0.0; }
    void Reset() { m_bits = m_errors = 0; }

private:
    void Add(int status, const dabgpu_ber_result& r);
    dabgpu_ctx* m_ctx;
    uint64_t m_bits = 0, m_errors = 0;
};
