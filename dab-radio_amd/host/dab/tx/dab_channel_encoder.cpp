// dab/tx/dab_channel_encoder.cpp -- see dab_channel_encoder.h
#include "./dab_channel_encoder.h"

#include <stdexcept>
#include <string>

#include "dab/dabgpu_shared_context.h"
#include "./dabgpu_tx_check.h"

static void check(int st, const char* what) { dabgpu_tx_check("DAB_Channel_Encoder", st, what); }

DAB_Channel_Encoder::DAB_Channel_Encoder(tcb::span<const dabgpu_subchannel> subchannels) {
    dabgpu_tx_check_abi("DAB_Channel_Encoder");
    const int n = (int)subchannels.size();
    std::vector<dabgpu_tx_sub_plan> plans((size_t)n + 1);
    uint32_t cif_in = 0;
    check(dabgpu_tx_encode_plan(n ? subchannels.data() : nullptr, n, plans.data(), &cif_in, nullptr, 0, nullptr, nullptr), "dabgpu_tx_encode_plan");
    m_cif_in_bytes = cif_in;
    check(dabgpu_tx_bank_create(dabgpu_shared_context(), 1, n ? subchannels.data() : nullptr, n, &m_bank), "dabgpu_tx_bank_create");
}

DAB_Channel_Encoder::~DAB_Channel_Encoder() { dabgpu_tx_bank_destroy(m_bank); }

void DAB_Channel_Encoder::Reset() {
    check(dabgpu_tx_bank_reset(m_bank, nullptr), "dabgpu_tx_bank_reset");
    check(dabgpu_synchronize(dabgpu_shared_context(), nullptr), "dabgpu_synchronize");
}

bool DAB_Channel_Encoder::EncodeFrame(tcb::span<uint8_t> frame_bits, tcb::span<const uint8_t> fib_data, tcb::span<const uint8_t> cif_bytes) {
    if (frame_bits.size() != FRAME_BITS_BYTES || fib_data.size() != FIB_DATA_BYTES || cif_bytes.size() != 4 * m_cif_in_bytes) return false;
    check(dabgpu_tx_bank_encode_frames_host_sync(m_bank, fib_data.data(), cif_bytes.data(), 1, frame_bits.data()), "dabgpu_tx_bank_encode_frames_host_sync");
    return true;
}

bool DAB_Channel_Encoder::TransmitFrame(tcb::span<std::complex<float>> frame_out, tcb::span<const uint8_t> fib_data, tcb::span<const uint8_t> cif_bytes,
                                        float freq_norm) {
    if (frame_out.size() != DABGPU_NB_FRAME_SAMPLES || fib_data.size() != FIB_DATA_BYTES || cif_bytes.size() != 4 * m_cif_in_bytes) return false;
    check(dabgpu_tx_bank_transmit_frames_host_sync(m_bank, fib_data.data(), cif_bytes.data(), 1, freq_norm, frame_out.data(), DABGPU_IQ_RAW_F32L),
          "dabgpu_tx_bank_transmit_frames_host_sync");
    return true;
}
