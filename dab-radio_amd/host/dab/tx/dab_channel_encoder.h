// dab/tx/dab_channel_encoder.h -- one ensemble's channel encoder on the device (include/dabgpu.h, "Channel encoder"): FIB bodies and
// the CIFs' sub-channel bytes of a transmission frame (mode I) -> the frame's bits, or NULL-first IQ.  ETSI EN 300 401 5.2.1, 10, 11, 12.
// The reference has no channel encoder; the class follows the conventions of its OFDM_Modulator mirror (ofdm/ofdm_modulator.h): spans
// in, false for wrong buffer sizes, exceptions for device failures.  The time interleaver's state lives in the object: frames are
// encoded in the order they are handed over, Reset() starts a new sequence.
#pragma once
#include <complex>
#include <cstdint>
#include <vector>

#include "dabgpu.h"
#include "utility/span.h"

class DAB_Channel_Encoder {
public:
    static constexpr size_t FIB_DATA_BYTES = 4 * 3 * 30;            // 12 FIB bodies per transmission frame
    static constexpr size_t FRAME_BITS_BYTES = DABGPU_NB_FRAME_BITS / 8;
    explicit DAB_Channel_Encoder(tcb::span<const dabgpu_subchannel> subchannels);
    ~DAB_Channel_Encoder();
    DAB_Channel_Encoder(const DAB_Channel_Encoder&) = delete;
    DAB_Channel_Encoder& operator=(const DAB_Channel_Encoder&) = delete;
    // bytes of one CIF's input record (the sub-channels' bytes back to back in list order); a frame takes four
    size_t GetCifInputBytes() const { return m_cif_in_bytes; }
    void Reset();
    // fib_data [4][3][30], cif_bytes [4][GetCifInputBytes()] -> frame_bits [28800] (DABGPU_TX_PAYLOAD_FRAME_BITS)
    bool EncodeFrame(tcb::span<uint8_t> frame_bits, tcb::span<const uint8_t> fib_data, tcb::span<const uint8_t> cif_bytes);
    // ... -> NULL period + 76 symbols, 196608 samples
    bool TransmitFrame(tcb::span<std::complex<float>> frame_out, tcb::span<const uint8_t> fib_data, tcb::span<const uint8_t> cif_bytes,
                       float freq_norm = 0.0f);
private:
    dabgpu_tx_bank* m_bank = nullptr;
    size_t m_cif_in_bytes = 0;
};
